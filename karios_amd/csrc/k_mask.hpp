// k_mask.hip: vector masks on the device - the polygon burn of rasterize_vector_mask (karios/core/image.py:104-191: GDAL's fill at
// pixel centres OR its all-touched line pass, BURN=1) and the AND of _load_mask with its three counts (karios/api/core.py:593-612).
// The arithmetic is mask_math.hpp's; tests/rasterize_restatement.py is the definition.
// A compiler that is not hipcc (the host sanitizer build of the API files, the stand-alone program of tests/test_mask_host.py) gets the
// launchers defined here, as plain loops over the same header: device memory is host memory there, `c` is not touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/karios_hip.h"
#include "mask_math.hpp"

// one feature: its edges [e0, e1) of the call's edge list and the rows its fill visits (miny > maxy: none)
struct kmk_feature {
    int e0, e1, miny, maxy;
};
struct kmk_polygons {
    const mk::edge *edges;
    int n_edges;
    const kmk_feature *features;
    int n_features;
    int H, W;                  // H * W < 2^32 - 1
    uint8_t *out;
    ptrdiff_t stride;
};
#define KMK_EDGE_CHUNK 896     // edges of a feature staged in LDS at a time (32 bytes each)

// The edge list and the feature table of km_rasterize_polygons' three host tables; nullptr, or what is wrong with them.
inline const char *kmk_tables(const double *xy, int n_vertices, const int32_t *ring_sizes, int n_rings, const int32_t *feature_rings, int n_features,
                              int H, std::vector<mk::edge> &edges, std::vector<kmk_feature> &features)
{
    if (n_vertices < 0 || n_rings < 0 || n_features < 0) return "negative count";
    if (n_vertices > mk::MAX_VERTICES) return "more than 2^20 vertices";
    if ((n_vertices && !xy) || (n_rings && !ring_sizes) || (n_features && !feature_rings)) return "null table";
    for (int i = 0; i < 2 * n_vertices; i++)
        if (!(fabs(xy[i]) <= mk::MAX_COORD)) return "a coordinate is not finite or lies beyond 2^30";      // (NaN fails the comparison)
    edges.clear(); features.clear();
    long long ring = 0, vertex = 0;
    for (int f = 0; f < n_features; f++) {
        if (feature_rings[f] < 0 || ring + feature_rings[f] > n_rings) return "the features own more rings than there are";
        kmk_feature F = {(int)edges.size(), 0, 0, -1};
        double lo = 0.0, hi = 0.0;
        bool any = false;
        for (int r = 0; r < feature_rings[f]; r++, ring++) {
            const int n = ring_sizes[ring];
            if (n < 2) return "a ring of fewer than 2 vertices";
            if (vertex + n > n_vertices) return "the rings own more vertices than there are";
            const double *v = xy + 2 * vertex;
            if (v[0] != v[2 * (n - 1)] || v[1] != v[2 * (n - 1) + 1]) return "a ring is not closed";
            for (int i = 0; i < n; i++) {
                if (!any || v[2 * i + 1] < lo) lo = v[2 * i + 1];
                if (!any || v[2 * i + 1] > hi) hi = v[2 * i + 1];
                any = true;
                if (i) edges.push_back(mk::edge{v[2 * i - 2], v[2 * i - 1], v[2 * i], v[2 * i + 1]});
            }
            vertex += n;
        }
        F.e1 = (int)edges.size();
        if (any) mk::row_range(lo, hi, H, F.miny, F.maxy);
        features.push_back(F);
    }
    if (ring != n_rings || vertex != n_vertices) return "rings or vertices no feature owns";
    return nullptr;
}

// every byte of the H x W window becomes the OR of the features' fills, zeros included: stored exactly once, nothing is read
int kmk_fill(km_ctx *c, const kmk_polygons &p, int edge_chunk);
// the all-touched line pass of every edge, stream-ordered behind the fill: ones only.  *d_flag |= 1 when a walk exceeded mk::walk_cap
int kmk_lines(km_ctx *c, const kmk_polygons &p, int32_t *d_flag);
// out = (a > 0) & (b > 0); d_counts[3] = pixels with a > 0, with b > 0, with both
int kmk_mask_and(km_ctx *c, const uint8_t *d_a, ptrdiff_t sa, const uint8_t *d_b, ptrdiff_t sb, int H, int W, uint8_t *d_out, ptrdiff_t so,
                 unsigned long long *d_counts);

#if !defined(__HIPCC__)
#include <algorithm>

inline int kmk_fill(km_ctx *, const kmk_polygons &p, int)
{
    std::vector<int> xs;
    for (int y = 0; y < p.H; y++) {
        uint8_t *row = p.out + (ptrdiff_t)y * p.stride;
        for (int x = 0; x < p.W; x++) row[x] = 0;
        auto burn = [&](long long first, long long last) {
            if (first < 0) first = 0;
            if (last > p.W - 1) last = p.W - 1;
            for (long long x = first; x <= last; x++) row[x] = 1;
        };
        for (int f = 0; f < p.n_features; f++) {
            const kmk_feature &F = p.features[f];
            if (y < F.miny || y > F.maxy) continue;
            xs.clear();
            for (int e = F.e0; e < F.e1; e++) {
                int a, b;
                const int kind = mk::crossing(p.edges[e], y + 0.5, a, b);
                if (kind == mk::CROSS) xs.push_back(a);
                else if (kind == mk::SPAN) burn(a, b);
            }
            std::sort(xs.begin(), xs.end());
            for (size_t i = 0; i + 1 < xs.size(); i += 2) burn(xs[i], (long long)xs[i + 1] - 1);
        }
    }
    return KM_OK;
}

inline int kmk_lines(km_ctx *, const kmk_polygons &p, int32_t *d_flag)
{
    for (int e = 0; e < p.n_edges; e++) {
        mk::line_plan L;
        mk::plan_line(p.edges[e], p.H, p.W, L);
        if (L.kind == mk::L_COLUMN)
            for (int y = L.lo; y <= L.hi; y++) p.out[(ptrdiff_t)y * p.stride + L.fixed] = 1;
        else if (L.kind == mk::L_ROW)
            for (int x = L.lo; x <= L.hi; x++) p.out[(ptrdiff_t)L.fixed * p.stride + x] = 1;
        else if (L.kind == mk::L_WALK) {
            const long long cap = mk::walk_cap(p.H, p.W);
            long long steps = 0;
            int ix, iy;
            bool burn;
            while (mk::walk_step(L, p.H, p.W, ix, iy, burn)) {
                if (++steps > cap) { *d_flag |= 1; break; }
                if (burn) p.out[(ptrdiff_t)iy * p.stride + ix] = 1;
            }
        }
    }
    return KM_OK;
}

inline int kmk_mask_and(km_ctx *, const uint8_t *d_a, ptrdiff_t sa, const uint8_t *d_b, ptrdiff_t sb, int H, int W, uint8_t *d_out, ptrdiff_t so,
                        unsigned long long *d_counts)
{
    d_counts[0] = d_counts[1] = d_counts[2] = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const bool a = d_a[(ptrdiff_t)y * sa + x] > 0, b = d_b[(ptrdiff_t)y * sb + x] > 0;
            d_out[(ptrdiff_t)y * so + x] = a && b;
            d_counts[0] += a; d_counts[1] += b; d_counts[2] += a && b;
        }
    return KM_OK;
}
#endif
