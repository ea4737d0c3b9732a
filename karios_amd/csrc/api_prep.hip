// The dense front half of the global align step (karios/matcher/global_align.py:87-108, _to_uint8 and _preprocess) and the
// percentiles of the quality check (karios/api/core.py:491-506): exact order statistics of a raster, the percentile stretch to uint8
// and CLAHE.  The kernels live in k_prep.hip.  The interpolation between the two order statistics of a percentile is numpy's and stays
// with the caller (karios_amd/ops/prep.py): it is arithmetic of the SOURCE dtype there, wrap-around of int16 included.
// Also the display range of the report's overview figure (karios/report/overview_plot.py:134-194): the same select under the
// reference's invalid-pixel rule; kernels in k_report.hip.
// And the masks a pair is matched under (karios/api/core.py:538-620 _load_mask): a vector mask burnt on the monitored raster's grid
// (karios/core/image.py:104-191) and its AND with a raster mask; kernels in k_mask.hip.
#include "api_internal.hpp"
#include "k_mask.hpp"
#include "k_prep.hpp"
#include "k_report.hpp"

#include <stddef.h>
#include <string.h>

#include <vector>

namespace {

bool prep_dtype(int dtype) { return dtype == KM_U8 || dtype == KM_U16 || dtype == KM_I16 || dtype == KM_F32; }

int stats_args(km_ctx *c, const void *img, int dtype, int H, int W, ptrdiff_t stride, int exclude, int n_q, const double *q, const int64_t *n_out,
               const double *v0, const double *v1, const double *vi)
{
    int rc;
    if ((rc = check_image(c, img, H, W, stride, "order_statistics"))) return rc;
    if (!prep_dtype(dtype)) return km_fail(c, KM_E_ARG, "order_statistics: dtype %d (uint8, uint16, int16 and float32 only)", dtype);
    if (exclude != 0 && exclude != 1) return km_fail(c, KM_E_ARG, "order_statistics: exclude %d (0: NaN, 1: every non-finite value)", exclude);
    if (n_q < 0 || !n_out || (n_q && (!q || !v0 || !v1 || !vi))) return km_fail(c, KM_E_ARG, "order_statistics: bad arguments");
    for (int j = 0; j < n_q; j++)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return km_fail(c, KM_E_ARG, "order_statistics: quantile %d = %g outside [0, 1]", j, q[j]);
    if ((unsigned long long)H * (unsigned long long)W >= (1ull << 42))   // (a workgroup's 32-bit LDS counters hold its share of the raster)
        return km_fail(c, KM_E_ARG, "order_statistics: %d x %d raster", H, W);
    return KM_OK;
}

// The quantiles go through the select KP_MAX_Q at a time: three passes per group, no host synchronisation inside a group, one copy of
// its results at the end.
int stats_dev(km_ctx *c, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, int exclude, int n_q, const double *q, int64_t *n_out,
              double *v0, double *v1, double *vi)
{
    kp_state *st = (kp_state *)km_ws(c, WS_PR_STATE, sizeof(kp_state));
    if (!st) return KM_E_NOMEM;
    struct { long long n; double vi[KP_MAX_Q], v0[KP_MAX_Q], v1[KP_MAX_Q]; } res;
    static_assert(sizeof(res) == sizeof(kp_state) - offsetof(kp_state, n), "results are the tail of kp_state");
    bool plain = false;
#ifdef KM_DEV
    plain = c->opt_prep_plain;
#endif
    int j0 = 0;
    do {
        const int m = n_q - j0 < KP_MAX_Q ? n_q - j0 : KP_MAX_Q;
        int rc;
        if ((rc = kp_order_statistics(c, d_img, dtype, H, W, stride, exclude, m, q + j0, st, plain))) return rc;
        KM_D2H(c, &res, &st->n, sizeof(res));
        KM_FLUSH(c);
        *n_out = (int64_t)res.n;
        if (res.n > 0)
            for (int j = 0; j < m; j++) { vi[j0 + j] = res.vi[j]; v0[j0 + j] = res.v0[j]; v1[j0 + j] = res.v1[j]; }
        j0 += m;
    } while (j0 < n_q);
    return KM_OK;
}

// ---- the display range of the report's overview (karios/report/overview_plot.py:134-194)
struct range_args {
    const void *img;
    int dtype, H, W;
    ptrdiff_t stride;
    const uint8_t *mask;
    ptrdiff_t mask_stride;
    const double *nodata, *no_values;
    int n_no_values, n_q;
    const double *q;
    km_display_range_result *out;
    double *v0, *v1, *vi;
};

int range_check(km_ctx *c, const range_args &a)
{
    int rc;
    if ((rc = check_image(c, a.img, a.H, a.W, a.stride, "display_range"))) return rc;
    if (!prep_dtype(a.dtype)) return km_fail(c, KM_E_ARG, "display_range: dtype %d (uint8, uint16, int16 and float32 only)", a.dtype);
    if (a.mask && a.mask_stride < a.W) return km_fail(c, KM_E_ARG, "display_range: mask stride %td < width %d", a.mask_stride, a.W);
    if (a.n_no_values < 0 || (a.n_no_values > 0 && !a.no_values)) return km_fail(c, KM_E_ARG, "display_range: bad DN value list");
    if (a.n_no_values > KM_DISPLAY_MAX_NO_VALUES)
        return km_fail(c, KM_E_ARG, "display_range: %d DN values (at most %d)", a.n_no_values, KM_DISPLAY_MAX_NO_VALUES);
    if (a.n_q < 0 || !a.out || (a.n_q && (!a.q || !a.v0 || !a.v1 || !a.vi))) return km_fail(c, KM_E_ARG, "display_range: bad arguments");
    for (int j = 0; j < a.n_q; j++)
        if (!(a.q[j] >= 0.0 && a.q[j] <= 1.0)) return km_fail(c, KM_E_ARG, "display_range: quantile %d = %g outside [0, 1]", j, a.q[j]);
    if ((unsigned long long)a.H * (unsigned long long)a.W >= (1ull << 42))
        return km_fail(c, KM_E_ARG, "display_range: %d x %d raster", a.H, a.W);
    return KM_OK;
}

// the DN values and the no-data value as pixels of the raster's type: what no pixel can equal is left out
rp::tests range_tests(const range_args &a)
{
    rp::tests t = kr_no_tests();
    for (int k = 0; k < a.n_no_values; k++) kr_add_test(t, a.dtype, a.no_values[k]);
    if (a.nodata) kr_add_test(t, a.dtype, *a.nodata);
    return t;
}

// the quantiles go through the select KR_MAX_Q at a time, like stats_dev; the counts and the extremes come with every group
int range_dev(km_ctx *c, const range_args &a, const void *d_img, ptrdiff_t stride, const uint8_t *d_mask, ptrdiff_t mask_stride)
{
    const size_t ws_bytes = up256(kr_range_ws_bytes());
    char *ws = (char *)km_ws(c, WS_RP_STATE, ws_bytes + sizeof(kr_range_result));
    if (!ws) return KM_E_NOMEM;
    kr_range_result *d_res = (kr_range_result *)(ws + ws_bytes);
    const rp::tests t = range_tests(a);
    kr_range_result res;
    int j0 = 0;
    do {
        const int m = a.n_q - j0 < KR_MAX_Q ? a.n_q - j0 : KR_MAX_Q;
        int rc;
        if ((rc = kr_display_range(c, d_img, a.dtype, a.H, a.W, stride, d_mask, mask_stride, t, m, a.q + j0, ws, d_res))) return rc;
        KM_D2H(c, &res, d_res, sizeof res);
        KM_FLUSH(c);
        a.out->n_valid = (int64_t)res.n_valid; a.out->n_invalid = (int64_t)res.n_invalid;
        a.out->raster_min = res.raster_min; a.out->raster_max = res.raster_max;
        if (res.n_valid > 0)
            for (int j = 0; j < m; j++) { a.vi[j0 + j] = res.vi[j]; a.v0[j0 + j] = res.v0[j]; a.v1[j0 + j] = res.v1[j]; }
        j0 += m;
    } while (j0 < a.n_q);
    return KM_OK;
}

int stretch_args(km_ctx *c, const void *img, int dtype, int H, int W, ptrdiff_t stride, const void *out, ptrdiff_t ostride)
{
    int rc;
    if ((rc = check_image(c, img, H, W, stride, "stretch_percentile_u8")) || (rc = check_image(c, out, H, W, ostride, "stretch_percentile_u8 output")))
        return rc;
    if (!prep_dtype(dtype)) return km_fail(c, KM_E_ARG, "stretch_percentile_u8: dtype %d (uint8, uint16, int16 and float32 only)", dtype);
    return KM_OK;
}

int clahe_args(km_ctx *c, const void *img, int H, int W, ptrdiff_t stride, double clip_limit, int tiles_x, int tiles_y, const void *out,
               ptrdiff_t ostride, kp_clahe_geom *g)
{
    int rc;
    if ((rc = check_image(c, img, H, W, stride, "clahe")) || (rc = check_image(c, out, H, W, ostride, "clahe output"))) return rc;
    if (clip_limit != clip_limit) return km_fail(c, KM_E_ARG, "clahe: clip limit is NaN");
    return kp_clahe_geometry(c, H, W, clip_limit, tiles_x, tiles_y, g);
}

int clahe_dev(km_ctx *c, const uint8_t *d_img, int H, int W, ptrdiff_t stride, const kp_clahe_geom &g, uint8_t *d_out, ptrdiff_t ostride)
{
    const size_t tiles = (size_t)g.tiles_x * g.tiles_y;
    unsigned *d_hist = (unsigned *)km_ws(c, WS_PR_CLAHE, tiles * 256 * (sizeof(unsigned) + 1));
    if (!d_hist) return KM_E_NOMEM;
    return kp_clahe(c, d_img, H, W, stride, g, d_hist, (uint8_t *)(d_hist + tiles * 256), d_out, ostride);
}

// ---- vector masks (k_mask.hip)
struct polygon_tables {
    std::vector<mk::edge> edges;
    std::vector<kmk_feature> features;
};

int polygons_args(km_ctx *c, const double *xy, int n_vertices, const int32_t *ring_sizes, int n_rings, const int32_t *feature_rings, int n_features, int H,
                  int W, const uint8_t *out, ptrdiff_t stride, polygon_tables &t)
{
    if (H < 1 || W < 1 || (unsigned long long)H * (unsigned long long)W >= 0xFFFFFFFFull)
        return km_fail(c, KM_E_ARG, "rasterize_polygons: a raster of %d x %d (at least 1 x 1, fewer than 2^32 - 1 pixels)", H, W);
    if (!out || stride < W) return km_fail(c, KM_E_ARG, "rasterize_polygons: null output or row stride %td < width %d", stride, W);
    const char *why = kmk_tables(xy, n_vertices, ring_sizes, n_rings, feature_rings, n_features, H, t.edges, t.features);
    if (why) return km_fail(c, KM_E_ARG, "rasterize_polygons: %s", why);
    return KM_OK;
}

// the tables to the device, then the fill and the line pass into d_out; *d_flag: raised by a walk that exceeded its cap
int polygons_enqueue(km_ctx *c, const polygon_tables &t, int H, int W, uint8_t *d_out, ptrdiff_t stride, int32_t **d_flag)
{
    const size_t eb = t.edges.size() * sizeof(mk::edge), fb = t.features.size() * sizeof(kmk_feature);
    char *d_tab = (char *)km_ws(c, WS_MK_EDGES, up256(eb) + up256(fb) + 256);
    *d_flag = (int32_t *)km_ws(c, WS_MK_STATE, 256);
    if (!d_tab || !*d_flag) return KM_E_NOMEM;
    int rc;
    if (eb && (rc = km_h2d_small(c, d_tab, t.edges.data(), eb))) return rc;
    if (fb && (rc = km_h2d_small(c, d_tab + up256(eb), t.features.data(), fb))) return rc;
    KM_HIP(c, hipMemsetAsync(*d_flag, 0, sizeof(int32_t), c->stream));
    const kmk_polygons p = {(const mk::edge *)d_tab, (int)t.edges.size(), (const kmk_feature *)(d_tab + up256(eb)), (int)t.features.size(), H, W, d_out, stride};
    c->mask_timed = false;
    const bool timed = c->profiling;
    if (timed) {
        for (auto &e : c->ev_mask) KM_HIP(c, e.create(0));      // (flags 0: timing events)
        KM_HIP(c, hipEventRecord(c->ev_mask[0], c->stream));
    }
    if ((rc = kmk_fill(c, p, c->opt_mask_edge_chunk))) return rc;
    if (timed) KM_HIP(c, hipEventRecord(c->ev_mask[1], c->stream));
    if ((rc = kmk_lines(c, p, *d_flag))) return rc;
    if (timed) KM_HIP(c, hipEventRecord(c->ev_mask[2], c->stream));
    c->mask_timed = timed;
    return KM_OK;
}

int polygons_flag(km_ctx *c, int32_t flag)
{
    return flag ? km_fail(c, KM_E_INTERNAL, "rasterize_polygons: a line walk exceeded 4 (H + W) + 64 steps") : (int)KM_OK;
}

int mask_and_args(km_ctx *c, const uint8_t *a, ptrdiff_t sa, const uint8_t *b, ptrdiff_t sb, int H, int W, const uint8_t *out, ptrdiff_t so,
                  const int64_t *counts)
{
    int rc;
    if ((rc = check_image(c, a, H, W, sa, "mask_and")) || (rc = check_image(c, b, H, W, sb, "mask_and")) || (rc = check_image(c, out, H, W, so, "mask_and output")))
        return rc;
    if (!counts) return km_fail(c, KM_E_ARG, "mask_and: null counts");
    return KM_OK;
}

int mask_and_dev(km_ctx *c, const uint8_t *d_a, ptrdiff_t sa, const uint8_t *d_b, ptrdiff_t sb, int H, int W, uint8_t *d_out, ptrdiff_t so,
                 unsigned long long **d_counts)
{
    *d_counts = (unsigned long long *)km_ws(c, WS_MK_STATE, 256);
    if (!*d_counts) return KM_E_NOMEM;
    return kmk_mask_and(c, d_a, sa, d_b, sb, H, W, d_out, so, *d_counts);
}

// a dense device plane back into the caller's rows: one copy where they are dense, else row by row
int plane_out(km_ctx *c, uint8_t *out, ptrdiff_t stride, const uint8_t *d_plane, int H, int W)
{
    if (stride == W || H == 1) KM_D2H(c, out, d_plane, (size_t)H * W);
    else for (int y = 0; y < H; y++) KM_D2H(c, out + (ptrdiff_t)y * stride, d_plane + (size_t)y * W, (size_t)W);
    return KM_OK;
}

}  // namespace

extern "C" {

int km_rasterize_polygons_dev(km_ctx *c, const double *xy, int n_vertices, const int32_t *ring_sizes, int n_rings, const int32_t *feature_rings,
                              int n_features, int H, int W, uint8_t *d_out, ptrdiff_t out_stride)
{
    int rc;
    polygon_tables t;
    if ((rc = begin_call(c)) || (rc = polygons_args(c, xy, n_vertices, ring_sizes, n_rings, feature_rings, n_features, H, W, d_out, out_stride, t)))
        return rc;
    int32_t *d_flag, flag = 0;
    if ((rc = polygons_enqueue(c, t, H, W, d_out, out_stride, &d_flag))) return rc;
    KM_D2H(c, &flag, d_flag, sizeof flag);
    KM_FLUSH(c);
    return polygons_flag(c, flag);
}

int km_rasterize_polygons(km_ctx *c, const double *xy, int n_vertices, const int32_t *ring_sizes, int n_rings, const int32_t *feature_rings,
                          int n_features, int H, int W, uint8_t *out, ptrdiff_t out_stride)
{
    int rc;
    polygon_tables t;
    if ((rc = begin_call(c)) || (rc = polygons_args(c, xy, n_vertices, ring_sizes, n_rings, feature_rings, n_features, H, W, out, out_stride, t)))
        return rc;
    uint8_t *d_out = (uint8_t *)km_ws(c, WS_MK_IO, (size_t)H * W);
    if (!d_out) return KM_E_NOMEM;
    int32_t *d_flag, flag = 0;
    if ((rc = polygons_enqueue(c, t, H, W, d_out, W, &d_flag)) || (rc = plane_out(c, out, out_stride, d_out, H, W))) return rc;
    KM_D2H(c, &flag, d_flag, sizeof flag);
    KM_FLUSH(c);
    return polygons_flag(c, flag);
}

int km_mask_pass_ms(km_ctx *c, float *fill_ms, float *lines_ms)
{
    if (!c || !fill_ms || !lines_ms) return km_fail(c, KM_E_ARG, "km_mask_pass_ms: null argument");
    if (!c->mask_timed) return km_fail(c, KM_E_ARG, "km_mask_pass_ms: the last km_rasterize_polygons* call did not run under km_set_profiling(1)");
    KM_HIP(c, hipEventElapsedTime(fill_ms, c->ev_mask[0], c->ev_mask[1]));
    KM_HIP(c, hipEventElapsedTime(lines_ms, c->ev_mask[1], c->ev_mask[2]));
    return KM_OK;
}

int km_mask_and_dev(km_ctx *c, const uint8_t *d_a, ptrdiff_t a_stride, const uint8_t *d_b, ptrdiff_t b_stride, int H, int W, uint8_t *d_out,
                    ptrdiff_t out_stride, int64_t *counts)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = mask_and_args(c, d_a, a_stride, d_b, b_stride, H, W, d_out, out_stride, counts))) return rc;
    unsigned long long *d_counts;
    if ((rc = mask_and_dev(c, d_a, a_stride, d_b, b_stride, H, W, d_out, out_stride, &d_counts))) return rc;
    KM_D2H(c, counts, d_counts, 3 * sizeof(int64_t));
    KM_FLUSH(c);
    return KM_OK;
}

int km_mask_and(km_ctx *c, const uint8_t *a, ptrdiff_t a_stride, const uint8_t *b, ptrdiff_t b_stride, int H, int W, uint8_t *out,
                ptrdiff_t out_stride, int64_t *counts)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = mask_and_args(c, a, a_stride, b, b_stride, H, W, out, out_stride, counts))) return rc;
    void *d_a, *d_b;
    uint8_t *d_out = (uint8_t *)km_ws(c, WS_MK_IO, (size_t)H * W);
    if (!d_out) return KM_E_NOMEM;
    if ((rc = upload_image(c, WS_RAW_A, a, 1, H, W, a_stride, &d_a)) || (rc = upload_image(c, WS_RAW_B, b, 1, H, W, b_stride, &d_b))) return rc;
    unsigned long long *d_counts;
    if ((rc = mask_and_dev(c, (const uint8_t *)d_a, W, (const uint8_t *)d_b, W, H, W, d_out, W, &d_counts)) || (rc = plane_out(c, out, out_stride, d_out, H, W)))
        return rc;
    KM_D2H(c, counts, d_counts, 3 * sizeof(int64_t));
    KM_FLUSH(c);
    return KM_OK;
}

int km_order_statistics_dev(km_ctx *c, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, int exclude, int n_q, const double *q,
                            int64_t *n_out, double *v0, double *v1, double *vi)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = stats_args(c, d_img, dtype, H, W, stride, exclude, n_q, q, n_out, v0, v1, vi))) return rc;
    return stats_dev(c, d_img, dtype, H, W, stride, exclude, n_q, q, n_out, v0, v1, vi);
}

int km_order_statistics(km_ctx *c, const void *img, int dtype, int H, int W, ptrdiff_t stride, int exclude, int n_q, const double *q,
                        int64_t *n_out, double *v0, double *v1, double *vi)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = stats_args(c, img, dtype, H, W, stride, exclude, n_q, q, n_out, v0, v1, vi))) return rc;
    void *d_img;
    if ((rc = upload_image(c, WS_RAW_A, img, km_dtype_size(dtype), H, W, stride, &d_img))) return rc;
    return stats_dev(c, d_img, dtype, H, W, W, exclude, n_q, q, n_out, v0, v1, vi);
}

int km_display_range_dev(km_ctx *c, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *d_mask, ptrdiff_t mask_stride,
                         const double *nodata, const double *no_values, int n_no_values, int n_q, const double *q, km_display_range_result *out,
                         double *v0, double *v1, double *vi)
{
    const range_args a = {d_img, dtype, H, W, stride, d_mask, mask_stride, nodata, no_values, n_no_values, n_q, q, out, v0, v1, vi};
    int rc;
    if ((rc = begin_call(c)) || (rc = range_check(c, a))) return rc;
    return range_dev(c, a, d_img, stride, d_mask, mask_stride);
}

int km_display_range(km_ctx *c, const void *img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *mask, ptrdiff_t mask_stride,
                     const double *nodata, const double *no_values, int n_no_values, int n_q, const double *q, km_display_range_result *out,
                     double *v0, double *v1, double *vi)
{
    const range_args a = {img, dtype, H, W, stride, mask, mask_stride, nodata, no_values, n_no_values, n_q, q, out, v0, v1, vi};
    int rc;
    if ((rc = begin_call(c)) || (rc = range_check(c, a))) return rc;
    void *d_img, *d_mask = nullptr;
    if ((rc = upload_image(c, WS_RAW_A, img, km_dtype_size(dtype), H, W, stride, &d_img))) return rc;
    if (mask && (rc = upload_image(c, WS_MASK_IN, mask, 1, H, W, mask_stride, &d_mask))) return rc;
    return range_dev(c, a, d_img, W, (const uint8_t *)d_mask, W);
}

int km_stretch_percentile_u8_dev(km_ctx *c, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, double lo, double hi, uint8_t *d_out,
                                 ptrdiff_t out_stride)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = stretch_args(c, d_img, dtype, H, W, stride, d_out, out_stride))) return rc;
    return kp_stretch(c, d_img, dtype, H, W, stride, lo, hi, d_out, out_stride);
}

int km_stretch_percentile_u8(km_ctx *c, const void *img, int dtype, int H, int W, ptrdiff_t stride, double lo, double hi, uint8_t *out)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = stretch_args(c, img, dtype, H, W, stride, out, W))) return rc;
    void *d_img;
    uint8_t *d_out = (uint8_t *)km_ws(c, WS_PR_OUT, (size_t)H * W);
    if (!d_out) return KM_E_NOMEM;
    if ((rc = upload_image(c, WS_RAW_A, img, km_dtype_size(dtype), H, W, stride, &d_img))) return rc;
    if ((rc = kp_stretch(c, d_img, dtype, H, W, W, lo, hi, d_out, W))) return rc;
    KM_D2H(c, out, d_out, (size_t)H * W);
    KM_FLUSH(c);
    return KM_OK;
}

int km_clahe_dev(km_ctx *c, const uint8_t *d_img, int H, int W, ptrdiff_t stride, double clip_limit, int tiles_x, int tiles_y, uint8_t *d_out,
                 ptrdiff_t out_stride)
{
    int rc;
    kp_clahe_geom g;
    if ((rc = begin_call(c)) || (rc = clahe_args(c, d_img, H, W, stride, clip_limit, tiles_x, tiles_y, d_out, out_stride, &g))) return rc;
    return clahe_dev(c, d_img, H, W, stride, g, d_out, out_stride);
}

int km_clahe(km_ctx *c, const uint8_t *img, int H, int W, ptrdiff_t stride, double clip_limit, int tiles_x, int tiles_y, uint8_t *out)
{
    int rc;
    kp_clahe_geom g;
    if ((rc = begin_call(c)) || (rc = clahe_args(c, img, H, W, stride, clip_limit, tiles_x, tiles_y, out, W, &g))) return rc;
    void *d_img;
    uint8_t *d_out = (uint8_t *)km_ws(c, WS_PR_OUT, (size_t)H * W);
    if (!d_out) return KM_E_NOMEM;
    if ((rc = upload_image(c, WS_RAW_A, img, 1, H, W, stride, &d_img))) return rc;
    if ((rc = clahe_dev(c, (const uint8_t *)d_img, H, W, W, g, d_out, W))) return rc;
    KM_D2H(c, out, d_out, (size_t)H * W);
    KM_FLUSH(c);
    return KM_OK;
}

}  // extern "C"
