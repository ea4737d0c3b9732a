// k_products.hip: the report's products and the altitude figure's numbers on resident data - the key-point mask and the dx / dy raster
// of ProductGenerator (karios/report/product_generator.py:138-218), the altitude column (karios/api/core.py:1049-1053) and the
// statistics `boxplot` takes of the altitude groups (karios/report/shift_by_alt_plot.py:127-171).  The arithmetic is
// products_math.hpp's; tests/products_restatement.py is the definition.
// A compiler that is not hipcc (the host sanitizer build of the API files, the stand-alone program of tests/test_products_host.py)
// gets the launchers defined here, as plain loops over the same header: device memory is host memory there, `c` is not touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/karios_hip.h"
#include "products_math.hpp"

// ---- point rasters: n rows (0 .. 2^20) onto an H x W grid (H * W < 2^32 - 1)
struct kpd_rasters {
    const float *x0, *y0, *dx, *dy;   // dx / dy are read only when there is a delta raster
    int n, H, W;
    uint8_t *mask;                    // null: none
    ptrdiff_t mask_stride;
    float *delta;                     // null: none; band b, row y at delta + b * band_stride + y * row_stride
    ptrdiff_t band_stride, row_stride;
};
struct kpd_rasters_ws {
    unsigned long long *keys_a, *keys_b;   // n each; read only when there is a delta raster
};
// fills the planes (0; NaN 0x7FC00000), then scatters; *d_out_of_range = the rows that landed nowhere
int kpd_point_rasters(km_ctx *c, const kpd_rasters &r, const kpd_rasters_ws &ws, int32_t *d_out_of_range);

// ---- sampling: out[i] = raster[y_index, x_index] under numpy's wrap, 0 for a row that is out of range
int kpd_sample_points(km_ctx *c, const void *d_raster, int dtype, int H, int W, ptrdiff_t stride, int n, const float *d_x0, const float *d_y0,
                      void *d_out, int32_t *d_out_of_range);

// ---- box statistics of n rows (0 .. 2^20); outputs of capacity n, stats as pm::N_STATS columns of n
struct kpd_box {
    const float *values, *positions;
    int bin;
    float *key;
    int32_t *count;
    float *mean;
    double *stats;
    int8_t *cls;
};
struct kpd_box_ws {
    unsigned long long *keys_a, *keys_b;   // n each
    unsigned *flags;                       // n
    uint32_t *misc;                        // KPD_BOX_MISC_WORDS(n)
};
#define KPD_BOX_MISC_WORDS(n) (5 * (size_t)(n) + 4)
enum { KPD_GROUPS = 0, KPD_KEPT = 1, KPD_COUNTS = 4 };
// d_counts[KPD_COUNTS]: groups, rows with a key
int kpd_box_stats(km_ctx *c, const kpd_box &b, int n, const kpd_box_ws &ws, int32_t *d_counts);

#if !defined(__HIPCC__)
#include <algorithm>
#include <vector>

inline int kpd_point_rasters(km_ctx *, const kpd_rasters &r, const kpd_rasters_ws &, int32_t *d_out_of_range)
{
    for (int y = 0; y < r.H && r.mask; y++)
        for (int x = 0; x < r.W; x++) r.mask[(ptrdiff_t)y * r.mask_stride + x] = 0;
    for (int b = 0; b < 2 && r.delta; b++)
        for (int y = 0; y < r.H; y++)
            for (int x = 0; x < r.W; x++) r.delta[b * r.band_stride + (ptrdiff_t)y * r.row_stride + x] = ac::bits_f32(pm::NAN_FILL);
    int32_t out = 0;
    for (int i = 0; i < r.n; i++) {
        const uint32_t px = pm::raster_pixel(r.x0[i], r.y0[i], r.H, r.W);
        if (px == pm::NO_PIXEL) { out++; continue; }
        const ptrdiff_t y = (ptrdiff_t)(px / (uint32_t)r.W), x = (ptrdiff_t)(px % (uint32_t)r.W);
        if (r.mask) r.mask[y * r.mask_stride + x] = 1;
        if (r.delta) { r.delta[y * r.row_stride + x] = r.dx[i]; r.delta[r.band_stride + y * r.row_stride + x] = r.dy[i]; }   // (row order: the last wins)
    }
    *d_out_of_range = out;
    return KM_OK;
}

template <typename T>
static inline int32_t kpd_sample_host(const T *src, int H, int W, ptrdiff_t stride, int n, const float *x0, const float *y0, T *out)
{
    int32_t bad = 0;
    for (int i = 0; i < n; i++) {
        int x, y;
        const bool ok = pm::wrapped(x0[i], W, x) && pm::wrapped(y0[i], H, y);
        out[i] = ok ? src[(ptrdiff_t)y * stride + x] : T(0);
        bad += !ok;
    }
    return bad;
}
inline int kpd_sample_points(km_ctx *, const void *d_raster, int dtype, int H, int W, ptrdiff_t stride, int n, const float *d_x0, const float *d_y0,
                             void *d_out, int32_t *d_out_of_range)
{
    switch (dtype) {
    case KM_U8: *d_out_of_range = kpd_sample_host<uint8_t>((const uint8_t *)d_raster, H, W, stride, n, d_x0, d_y0, (uint8_t *)d_out); return KM_OK;
    case KM_U16: *d_out_of_range = kpd_sample_host<uint16_t>((const uint16_t *)d_raster, H, W, stride, n, d_x0, d_y0, (uint16_t *)d_out); return KM_OK;
    case KM_I16: *d_out_of_range = kpd_sample_host<int16_t>((const int16_t *)d_raster, H, W, stride, n, d_x0, d_y0, (int16_t *)d_out); return KM_OK;
    case KM_F32: *d_out_of_range = kpd_sample_host<float>((const float *)d_raster, H, W, stride, n, d_x0, d_y0, (float *)d_out); return KM_OK;
    default: return KM_E_ARG;
    }
}

inline int kpd_box_stats(km_ctx *, const kpd_box &b, int n, const kpd_box_ws &ws, int32_t *d_counts)
{
    const float bin = (float)b.bin;
    int kept = 0;
    for (int i = 0; i < n; i++) {
        const uint32_t k = rp::group_key(b.positions[i], bin);
        b.cls[i] = -1;
        if (k != rp::DROPPED) ws.keys_a[kept++] = ((unsigned long long)k << 32) | (uint32_t)i;
    }
    std::sort(ws.keys_a, ws.keys_a + kept);
    std::vector<float> x;
    std::vector<uint32_t> keys;
    int groups = 0;
    for (int at = 0; at < kept;) {
        const uint32_t k = (uint32_t)(ws.keys_a[at] >> 32);
        const int start = at;
        x.clear(); keys.clear();
        for (; at < kept && (uint32_t)(ws.keys_a[at] >> 32) == k; at++) {
            x.push_back(b.values[(uint32_t)ws.keys_a[at]]);
            keys.push_back(pm::value_key(x.back()));
        }
        const int m = at - start;
        std::sort(keys.begin(), keys.end());
        std::vector<float> bsum;
        for (int o = 0; o < m; o += ac::BLOCK) bsum.push_back(ac::block_sum(x.data() + o, std::min<int>(ac::BLOCK, m - o)));
        double st[pm::N_STATS];
        pm::box_of_sorted([&](int i) { return keys[(size_t)i]; }, m, st);
        b.key[groups] = rp::key_value(k); b.count[groups] = m;
        b.mean[groups] = ac::mean_of(ac::fold_blocks(bsum.data(), (int)bsum.size()), m);
        for (int s = 0; s < pm::N_STATS; s++) b.stats[(size_t)s * n + groups] = st[s];
        for (int j = 0; j < m; j++) b.cls[(uint32_t)ws.keys_a[start + j]] = pm::flier_class(x[(size_t)j], st[pm::WHISLO], st[pm::WHISHI]);
        groups++;
    }
    d_counts[KPD_GROUPS] = groups; d_counts[KPD_KEPT] = kept; d_counts[2] = d_counts[3] = 0;
    return KM_OK;
}
#endif
