// Scoring entry points: ZNCCService.compute_zncc / _zncc2 (zncc_service.py:45-238), the mutual-information scores
// (mutual_info_service.py:73-130, zncc_service.py:240-287), the DN-value filter of the key points (core.py:650-737) and
// KariosAPI.analyze_accuracy (core.py:268-328): the valid-pixel count and GeometricStat (accuracy_statistics.py); the tracker's outlier clip
// (klt.py:52-71) on resident columns; ChipService.generate_chips (report/chip_service.py): the key-point selection and the chips;
// mean_profile of the report's figures (report/commons.py:49-71); the report's products (report/product_generator.py:138-218), the altitude
// column (core.py:1049-1053) and the box statistics of the altitude figure (report/shift_by_alt_plot.py:127-171).
#include "api_internal.hpp"
#include "k_accuracy.hpp"
#include "k_chips.hpp"
#include "k_clip.hpp"
#include "k_products.hpp"
#include "k_report.hpp"

#include <cstring>
#include <vector>

extern "C" {

int km_zncc_batch_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref,
                      ptrdiff_t smon, const float *d_x0, const float *d_y0, const float *d_dx, const float *d_dy, int n, double *d_out)
{
    int rc;
    if ((rc = begin_call(c, RESET_ZNCC)) || (rc = check_image(c, d_ref, Href, Wref, sref, "zncc")) || (rc = check_image(c, d_mon, Hmon, Wmon, smon, "zncc")))
        return rc;
    if (n < 0 || (n > 0 && (!d_x0 || !d_y0 || !d_dx || !d_dy || !d_out))) return km_fail(c, KM_E_ARG, "zncc: bad keypoint arrays");
    km_stage_timer t(c, ST_ZNCC);
    return kz_zncc(c, d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, d_x0, d_y0, d_dx, d_dy, n, d_out);
}

int km_zncc_batch(km_ctx *c, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref,
                  ptrdiff_t smon, const float *x0, const float *y0, const float *dx, const float *dy, int n, double *out)
{
    int rc;
    if ((rc = begin_call(c, RESET_ZNCC)) || (rc = check_image(c, ref, Href, Wref, sref, "zncc")) || (rc = check_image(c, mon, Hmon, Wmon, smon, "zncc")))
        return rc;
    const size_t es = km_dtype_size(dtype);
    if (!es) return km_fail(c, KM_E_ARG, "zncc: bad dtype %d", dtype);
    if (n < 0 || (n > 0 && (!x0 || !y0 || !dx || !dy || !out))) return km_fail(c, KM_E_ARG, "zncc: bad keypoint arrays");
    if (n == 0) return KM_OK;
    void *d_ref, *d_mon;
    if ((rc = upload_image(c, WS_RAW_A, ref, es, Href, Wref, sref, &d_ref)) || (rc = upload_image(c, WS_RAW_B, mon, es, Hmon, Wmon, smon, &d_mon)))
        return rc;
    float *kp = (float *)km_ws(c, WS_MISC0, (size_t)n * 4 * sizeof(float));
    double *d_out = (double *)km_ws(c, WS_MISC1, (size_t)n * sizeof(double));
    if (!kp || !d_out) return KM_E_NOMEM;
    const float *src[4] = {x0, y0, dx, dy};
    for (int i = 0; i < 4; i++) { const int rch = h2d_now(c, kp + (size_t)i * n, src[i], (size_t)n * sizeof(float)); if (rch) return rch; }
    {
        km_stage_timer t(c, ST_ZNCC);
        if ((rc = kz_zncc(c, d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, Wref, Wmon, kp, kp + n, kp + 2 * (size_t)n, kp + 3 * (size_t)n, n, d_out)))
            return rc;
    }
    KM_D2H(c, out, d_out, (size_t)n * sizeof(double));
    KM_FLUSH(c);
    return KM_OK;
}

int km_zncc_windows(km_ctx *c, const void *img1, const void *img2, int dtype1, int dtype2, int H1, int W1, int H2, int W2, ptrdiff_t stride1,
                    ptrdiff_t stride2, const int32_t *uv, int half_size, int count, double *out, uint8_t *out_outside)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, img1, H1, W1, stride1, "zncc_windows")) || (rc = check_image(c, img2, H2, W2, stride2, "zncc_windows")))
        return rc;
    const size_t e1 = km_any_dtype_size(dtype1), e2 = km_any_dtype_size(dtype2);
    if (!e1 || !e2) return km_fail(c, KM_E_ARG, "zncc_windows: bad dtypes %d / %d", dtype1, dtype2);
    if (half_size < 0) return km_fail(c, KM_E_ARG, "zncc_windows: window half-size must be non-negative");
    if (count < 0 || (count > 0 && (!uv || !out))) return km_fail(c, KM_E_ARG, "zncc_windows: bad window arrays");
    if (count == 0) return KM_OK;
    void *d1, *d2;
    if ((rc = upload_image(c, WS_RAW_A, img1, e1, H1, W1, stride1, &d1)) || (rc = upload_image(c, WS_RAW_B, img2, e2, H2, W2, stride2, &d2))) return rc;
    int *d_uv = (int *)km_ws(c, WS_MISC0, (size_t)count * 4 * sizeof(int));
    double *d_out = (double *)km_ws(c, WS_MISC1, (size_t)count * sizeof(double));
    uint8_t *d_fl = (uint8_t *)km_ws(c, WS_MISC2, (size_t)count);
    if (!d_uv || !d_out || !d_fl) return KM_E_NOMEM;
    { const int rch = h2d_now(c, d_uv, uv, (size_t)count * 4 * sizeof(int)); if (rch) return rch; }
    if ((rc = kz_zncc_windows(c, d1, d2, dtype1, dtype2, H1, W1, H2, W2, W1, W2, d_uv, half_size, count, d_out, d_fl))) return rc;
    KM_D2H(c, out, d_out, (size_t)count * sizeof(double));
    if (out_outside) KM_D2H(c, out_outside, d_fl, (size_t)count);
    KM_FLUSH(c);
    return KM_OK;
}

int km_mi_batch_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref,
                    ptrdiff_t smon, const float *d_x0, const float *d_y0, const float *d_dx, const float *d_dy, int n, double *d_st,
                    double *d_nmi)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, d_ref, Href, Wref, sref, "mi")) || (rc = check_image(c, d_mon, Hmon, Wmon, smon, "mi")))
        return rc;
    if (n < 0 || (n > 0 && (!d_x0 || !d_y0 || !d_dx || !d_dy || (!d_st && !d_nmi)))) return km_fail(c, KM_E_ARG, "mi: bad keypoint arrays");
    c->evs_used[c->ev_cur][ST_MI] = false;
    km_stage_timer t(c, ST_MI);
    return kmi_batch(c, d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, d_x0, d_y0, d_dx, d_dy, n, nullptr, nullptr, 0.f, d_st, d_nmi);
}

int km_mi_batch(km_ctx *c, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref,
                ptrdiff_t smon, const float *x0, const float *y0, const float *dx, const float *dy, int n, double *out_st, double *out_nmi)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, ref, Href, Wref, sref, "mi")) || (rc = check_image(c, mon, Hmon, Wmon, smon, "mi")))
        return rc;
    const size_t es = km_dtype_size(dtype);
    if (!es) return km_fail(c, KM_E_ARG, "mi: bad dtype %d", dtype);
    if (n < 0 || (n > 0 && (!x0 || !y0 || !dx || !dy || (!out_st && !out_nmi)))) return km_fail(c, KM_E_ARG, "mi: bad keypoint arrays");
    if (n == 0) return KM_OK;
    void *d_ref, *d_mon;
    if ((rc = upload_image(c, WS_RAW_A, ref, es, Href, Wref, sref, &d_ref)) || (rc = upload_image(c, WS_RAW_B, mon, es, Hmon, Wmon, smon, &d_mon)))
        return rc;
    float *kp = (float *)km_ws(c, WS_MISC0, (size_t)n * 4 * sizeof(float));
    double *d_out = (double *)km_ws(c, WS_MISC1, (size_t)n * 2 * sizeof(double));
    if (!kp || !d_out) return KM_E_NOMEM;
    const float *src[4] = {x0, y0, dx, dy};
    for (int i = 0; i < 4; i++) { const int rch = h2d_now(c, kp + (size_t)i * n, src[i], (size_t)n * sizeof(float)); if (rch) return rch; }
    if ((rc = kmi_batch(c, d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, Wref, Wmon, kp, kp + n, kp + 2 * (size_t)n, kp + 3 * (size_t)n, n, nullptr,
                        nullptr, 0.f, out_st ? d_out : nullptr, out_nmi ? d_out + n : nullptr)))
        return rc;
    if (out_st) KM_D2H(c, out_st, d_out, (size_t)n * sizeof(double));
    if (out_nmi) KM_D2H(c, out_nmi, d_out + n, (size_t)n * sizeof(double));
    KM_FLUSH(c);
    return KM_OK;
}

// KariosAPI._filter_by_dn_values (core.py:650-737) on resident images: x0 / y0 / no_values / keep are HOST arrays
// (n key points, n_no values), the images stay on the device.  keep[i] = 1 keep, 0 drop; a key point outside the image
// is an error (numpy's fancy indexing would raise or wrap).
int km_dn_keep_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon, const float *x0,
                   const float *y0, int n, const double *no_values, int n_no, const double *nodata_ref, const double *nodata_mon, uint8_t *keep)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, d_ref, H, W, sref, "dn_keep")) || (rc = check_image(c, d_mon, H, W, smon, "dn_keep"))) return rc;
    if (!km_dtype_size(dtype)) return km_fail(c, KM_E_ARG, "dn_keep: bad dtype %d", dtype);
    if (n < 0 || n_no < 0 || (n > 0 && (!x0 || !y0 || !keep)) || (n_no > 0 && !no_values)) return km_fail(c, KM_E_ARG, "dn_keep: bad arrays");
    if (n == 0) return KM_OK;
    float *d_xy = (float *)km_ws(c, WS_MISC0, (size_t)n * 2 * sizeof(float));
    double *d_nv = (double *)km_ws(c, WS_MISC1, (size_t)(n_no > 0 ? n_no : 1) * sizeof(double));
    uint8_t *d_keep = (uint8_t *)km_ws(c, WS_MISC2, (size_t)n);
    if (!d_xy || !d_nv || !d_keep) return KM_E_NOMEM;
    { const int rch = h2d_now(c, d_xy, x0, (size_t)n * sizeof(float)); if (rch) return rch; }
    { const int rch = h2d_now(c, d_xy + n, y0, (size_t)n * sizeof(float)); if (rch) return rch; }
    if (n_no > 0) { const int rch = h2d_now(c, d_nv, no_values, (size_t)n_no * sizeof(double)); if (rch) return rch; }
    if ((rc = kf_dn_keep(c, d_ref, d_mon, dtype, H, W, sref, smon, d_xy, d_xy + n, n, d_nv, n_no, nodata_ref, nodata_mon, d_keep))) return rc;
    KM_D2H(c, keep, d_keep, (size_t)n);
    KM_FLUSH(c);
    for (int i = 0; i < n; i++)
        if (keep[i] > 1) return km_fail(c, KM_E_ARG, "dn_keep: key point %d (%g, %g) lies outside the %dx%d image", i, (double)x0[i], (double)y0[i], W, H);
    return KM_OK;
}

// ---- KariosAPI.analyze_accuracy (core.py:268-328)
}  // extern "C"

namespace {

// WS_AC_STATE: the statistics' state, their result block, the pixel count
struct ac_block {
    ka_state st;
    km_accuracy_result res;
    unsigned long long count;
};

int count_valid_dev(km_ctx *c, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *d_mask, ptrdiff_t mask_stride, int64_t *count)
{
    ac_block *blk = (ac_block *)km_ws(c, WS_AC_STATE, sizeof(ac_block));
    if (!blk) return KM_E_NOMEM;
    int rc;
    if ((rc = ka_count_valid(c, d_img, dtype, H, W, stride, d_mask, mask_stride, &blk->count))) return rc;
    unsigned long long got = 0;
    KM_D2H(c, &got, &blk->count, sizeof got);
    KM_FLUSH(c);
    *count = (int64_t)got;
    return KM_OK;
}

int check_count_args(km_ctx *c, const void *img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *mask, ptrdiff_t mask_stride, int64_t *count)
{
    int rc;
    if ((rc = check_image(c, img, H, W, stride, "count_valid_pixels"))) return rc;
    if (!km_dtype_size(dtype)) return km_fail(c, KM_E_ARG, "count_valid_pixels: bad dtype %d", dtype);
    if (mask && mask_stride < W) return km_fail(c, KM_E_ARG, "count_valid_pixels: mask stride %td < width %d", mask_stride, W);
    if (!count) return km_fail(c, KM_E_ARG, "count_valid_pixels: null result");
    return KM_OK;
}

int check_stats_args(km_ctx *c, const float *dx, const float *dy, const float *score, int n, double thr, int n_percent, const double *percents,
                     km_accuracy_result *out)
{
    if (n < 0 || n > (1 << 24)) return km_fail(c, KM_E_ARG, "accuracy_stats: %d rows (0 .. 2^24)", n);
    if (n > 0 && (!dx || !dy || !score)) return km_fail(c, KM_E_ARG, "accuracy_stats: null column");
    if (thr != thr) return km_fail(c, KM_E_ARG, "accuracy_stats: the threshold is NaN");
    if (n_percent < 0 || n_percent > KM_ACC_MAX_PERCENTS || (n_percent > 0 && !percents))
        return km_fail(c, KM_E_ARG, "accuracy_stats: %d percents (0 .. %d)", n_percent, KM_ACC_MAX_PERCENTS);
    for (int k = 0; k < n_percent; k++)
        if (!(percents[k] >= 0.0)) return km_fail(c, KM_E_ARG, "accuracy_stats: percent %d is negative or NaN", k);
    if (!out) return km_fail(c, KM_E_ARG, "accuracy_stats: null result");
    return KM_OK;
}

int accuracy_stats_dev(km_ctx *c, const float *d_dx, const float *d_dy, const float *d_score, int n, double thr, int carto, double factor,
                       int n_percent, const double *percents, km_accuracy_result *out)
{
    const int cap = n > 0 ? n : 1;
    ac_block *blk = (ac_block *)km_ws(c, WS_AC_STATE, sizeof(ac_block));
    float *cols = (float *)km_ws(c, WS_AC_COLS, (size_t)cap * 3 * sizeof(float));
    float *bsum = (float *)km_ws(c, WS_AC_BSUM, (size_t)ka_nblocks(cap) * 3 * sizeof(float));
    if (!blk || !cols || !bsum) return KM_E_NOMEM;
    ka_percents pc;
    pc.n = n_percent;
    for (int k = 0; k < KM_ACC_MAX_PERCENTS; k++) pc.q[k] = k < n_percent ? percents[k] : 0.0;
    int rc;
    if ((rc = ka_compact(c, d_dx, d_dy, d_score, n, thr, carto, cols, &blk->st)) || (rc = ka_block_sums(c, cols, n, &blk->st, 0, bsum)) ||
        (rc = ka_finish(c, bsum, n, &blk->st, 0)) || (rc = ka_block_sums(c, cols, n, &blk->st, 1, bsum)) || (rc = ka_finish(c, bsum, n, &blk->st, 1)) ||
        (rc = ka_order(c, cols, n, (float)factor, pc, &blk->st, &blk->res)))
        return rc;
    KM_D2H(c, out, &blk->res, sizeof *out);
    KM_FLUSH(c);
    return KM_OK;
}

}  // namespace

extern "C" {

int km_count_valid_pixels_dev(km_ctx *c, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *d_mask, ptrdiff_t mask_stride,
                              int64_t *count)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_count_args(c, d_img, dtype, H, W, stride, d_mask, mask_stride, count))) return rc;
    return count_valid_dev(c, d_img, dtype, H, W, stride, d_mask, mask_stride, count);
}

int km_count_valid_pixels(km_ctx *c, const void *img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *mask, ptrdiff_t mask_stride,
                          int64_t *count)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_count_args(c, img, dtype, H, W, stride, mask, mask_stride, count))) return rc;
    void *d_img, *d_mask = nullptr;
    if ((rc = upload_image(c, WS_RAW_A, img, km_dtype_size(dtype), H, W, stride, &d_img))) return rc;
    if (mask && (rc = upload_image(c, WS_MASK_IN, mask, 1, H, W, mask_stride, &d_mask))) return rc;
    return count_valid_dev(c, d_img, dtype, H, W, W, (const uint8_t *)d_mask, W, count);
}

int km_accuracy_stats_dev(km_ctx *c, const float *d_dx, const float *d_dy, const float *d_score, int n, double thr, int carto, double factor,
                          int n_percent, const double *percents, km_accuracy_result *out)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_stats_args(c, d_dx, d_dy, d_score, n, thr, n_percent, percents, out))) return rc;
    return accuracy_stats_dev(c, d_dx, d_dy, d_score, n, thr, carto, factor, n_percent, percents, out);
}

int km_accuracy_stats(km_ctx *c, const float *dx, const float *dy, const float *score, int n, double thr, int carto, double factor, int n_percent,
                      const double *percents, km_accuracy_result *out)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_stats_args(c, dx, dy, score, n, thr, n_percent, percents, out))) return rc;
    const int cap = n > 0 ? n : 1;
    float *in = (float *)km_ws(c, WS_AC_IN, (size_t)cap * 3 * sizeof(float));
    if (!in) return KM_E_NOMEM;
    const float *src[3] = {dx, dy, score};
    for (int i = 0; i < 3 && n > 0; i++) { const int rch = h2d_now(c, in + (size_t)i * cap, src[i], (size_t)n * sizeof(float)); if (rch) return rch; }
    return accuracy_stats_dev(c, in, in + cap, in + 2 * (size_t)cap, n, thr, carto, factor, n_percent, percents, out);
}

// the tracker's outlier clip on resident columns (include/karios_hip.h): every check in front of the launch, a refused call queues nothing
int km_sigma_clip_dev(km_ctx *c, const float *const *d_dx, const float *const *d_dy, const int *n, int n_units, int32_t *const *d_keep_index,
                      km_clip_result *d_result)
{
    int rc;
    if ((rc = begin_call(c))) return rc;
    if (!d_dx || !d_dy || !n || !d_keep_index || !d_result) return km_fail(c, KM_E_ARG, "sigma_clip: null argument");
    if (n_units < 1 || n_units > KC_UNITS_MAX) return km_fail(c, KM_E_ARG, "sigma_clip: %d units (1 .. %d per call)", n_units, KC_UNITS_MAX);
    int n_max = 0;
    for (int k = 0; k < n_units; k++) {
        if (n[k] < 0 || (n[k] > 0 && (!d_dx[k] || !d_dy[k] || !d_keep_index[k]))) return km_fail(c, KM_E_ARG, "sigma_clip: bad columns of unit %d", k);
        if (n[k] > cl::MAX_ROWS) return km_fail(c, KM_E_UNSUPPORTED, "sigma_clip: unit %d has %d rows (at most %d)", k, n[k], (int)cl::MAX_ROWS);
        n_max = n[k] > n_max ? n[k] : n_max;
    }
    const size_t rows = kc_ws_rows(n_max);
    float *ws = (float *)km_ws(c, WS_CL_COLS, rows * 4 * sizeof(float) * (size_t)n_units);
    if (!ws) return KM_E_NOMEM;
    kc_units A;
    for (int k = 0; k < n_units; k++) {
        kc_unit &u = A.u[k];
        u = kc_unit();
        float *base = ws + rows * 4 * (size_t)k;
        u.dx = d_dx[k]; u.dy = d_dy[k]; u.n = n[k]; u.keep_index = d_keep_index[k];
        u.u = base; u.v = base + rows; u.idx = (int32_t *)(base + 2 * rows); u.lab = (int32_t *)(base + 3 * rows);
        u.rec = d_result + k;
    }
    return kc_clip_units(c, A, n_units);
}

}  // extern "C"

// ---- ChipService.generate_chips (include/karios_hip.h): every check in front of the first launch or copy
namespace {

int check_select_args(km_ctx *c, const float *x0, const float *y0, const float *score, int n, int width, int height, double threshold, int grid_rows,
                      int grid_cols, const int32_t *out_index, const int32_t *out_count)
{
    if (n < 0 || n > ch::MAX_SELECT_ROWS) return km_fail(c, KM_E_ARG, "chip_select: %d rows (0 .. 2^24)", n);
    if (n > 0 && (!x0 || !y0 || !score)) return km_fail(c, KM_E_ARG, "chip_select: null column");
    if (threshold != threshold) return km_fail(c, KM_E_ARG, "chip_select: the threshold is NaN");
    if (width < 1 || height < 1) return km_fail(c, KM_E_ARG, "chip_select: image of %d x %d", width, height);
    if (grid_rows < 1 || grid_rows > ch::MAX_GRID || grid_cols < 1 || grid_cols > ch::MAX_GRID)
        return km_fail(c, KM_E_ARG, "chip_select: grid of %d x %d cells (1 .. %d each)", grid_rows, grid_cols, (int)ch::MAX_GRID);
    if (!out_index || !out_count) return km_fail(c, KM_E_ARG, "chip_select: null result");
    return KM_OK;
}

ch::grid select_grid(int width, int height, double threshold, int threshold_f64, int grid_rows, int grid_cols)
{
    ch::grid g;
    g.rows = grid_rows; g.cols = grid_cols;
    g.width = (double)width; g.height = (double)height;
    g.thr = threshold_f64 ? threshold : (double)(float)threshold;
    return g;
}

// WS_MISC2: the slots of every cell, the packed indices (unless the caller's own device memory takes them), the count
int chip_select_dev(km_ctx *c, const float *d_x0, const float *d_y0, const float *d_score, int n, const ch::grid &g, int32_t *d_out_index,
                    int32_t *host_index, int32_t *out_count)
{
    const size_t ns = kch_slots(g);
    int32_t *ws = (int32_t *)km_ws(c, WS_MISC2, (2 * ns + 1) * sizeof(int32_t));
    if (!ws) return KM_E_NOMEM;
    int32_t *d_index = d_out_index ? d_out_index : ws + ns, *d_count = ws + 2 * ns;
    int rc;
    if ((rc = kch_select(c, d_x0, d_y0, d_score, n, g, ws, d_index, d_count))) return rc;
    int32_t got = 0;
    KM_D2H(c, &got, d_count, sizeof got);
    KM_FLUSH(c);
    if (host_index && got > 0) {
        KM_D2H(c, host_index, d_index, (size_t)got * sizeof(int32_t));
        KM_FLUSH(c);
    }
    *out_count = got;
    return KM_OK;
}

int check_chips_args(km_ctx *c, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref, ptrdiff_t smon,
                     const float *x0, const float *y0, const float *dx, const float *dy, int n, int ksize_ref, int ksize_mon, const km_chip_outputs *out)
{
    int rc;
    if ((rc = check_image(c, ref, Href, Wref, sref, "chips")) || (rc = check_image(c, mon, Hmon, Wmon, smon, "chips"))) return rc;
    if (!km_dtype_size(dtype)) return km_fail(c, KM_E_ARG, "chips: bad dtype %d", dtype);
    if (Href < ch::CHIP || Wref < ch::CHIP || Hmon < ch::CHIP || Wmon < ch::CHIP)
        return km_fail(c, KM_E_ARG, "chips: rasters of %d x %d and %d x %d (at least %d x %d)", Wref, Href, Wmon, Hmon, (int)ch::CHIP, (int)ch::CHIP);
    if (n < 0 || n > ch::MAX_CHIP_ROWS) return km_fail(c, KM_E_ARG, "chips: %d rows (0 .. 2^20)", n);
    if (n > 0 && (!x0 || !y0 || !dx || !dy)) return km_fail(c, KM_E_ARG, "chips: null column");
    if (!ch::ksize_ok(ksize_ref) || !ch::ksize_ok(ksize_mon))
        return km_fail(c, KM_E_ARG, "chips: Laplacian ksize ref=%d mon=%d (0, 1, 3, 5, 7, 9, 11)", ksize_ref, ksize_mon);
    if (!out) return km_fail(c, KM_E_ARG, "chips: null outputs");
    if (n > 0 && (!out->ref_raw || !out->mon_raw || !out->ref_u8 || !out->mon_u8 || !out->ok || !out->windows || (ksize_ref && !out->ref_lap) ||
                  (ksize_mon && !out->mon_lap)))
        return km_fail(c, KM_E_ARG, "chips: null output buffer");
    return KM_OK;
}

}  // namespace

extern "C" {

int km_chip_select_dev(km_ctx *c, const float *d_x0, const float *d_y0, const float *d_score, int n, int width, int height, double threshold,
                       int threshold_f64, int grid_rows, int grid_cols, int32_t *d_out_index, int32_t *out_count)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_select_args(c, d_x0, d_y0, d_score, n, width, height, threshold, grid_rows, grid_cols, d_out_index, out_count)))
        return rc;
    return chip_select_dev(c, d_x0, d_y0, d_score, n, select_grid(width, height, threshold, threshold_f64, grid_rows, grid_cols), d_out_index, nullptr,
                           out_count);
}

int km_chip_select(km_ctx *c, const float *x0, const float *y0, const float *score, int n, int width, int height, double threshold, int threshold_f64,
                   int grid_rows, int grid_cols, int32_t *out_index, int32_t *out_count)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_select_args(c, x0, y0, score, n, width, height, threshold, grid_rows, grid_cols, out_index, out_count)))
        return rc;
    const int cap = n > 0 ? n : 1;
    float *in = (float *)km_ws(c, WS_MISC0, (size_t)cap * 3 * sizeof(float));
    if (!in) return KM_E_NOMEM;
    const float *src[3] = {x0, y0, score};
    for (int i = 0; i < 3 && n > 0; i++) { const int rch = h2d_now(c, in + (size_t)i * cap, src[i], (size_t)n * sizeof(float)); if (rch) return rch; }
    return chip_select_dev(c, in, in + cap, in + 2 * (size_t)cap, n, select_grid(width, height, threshold, threshold_f64, grid_rows, grid_cols), nullptr,
                           out_index, out_count);
}

int km_chips_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref, ptrdiff_t smon,
                 const float *d_x0, const float *d_y0, const float *d_dx, const float *d_dy, int n, int ksize_ref, int ksize_mon, const km_chip_outputs *d_out)
{
    int rc;
    if ((rc = begin_call(c)) ||
        (rc = check_chips_args(c, d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, d_x0, d_y0, d_dx, d_dy, n, ksize_ref, ksize_mon, d_out)))
        return rc;
    if (n == 0) return KM_OK;
    const kch_images I = {d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, sref, smon};
    const kch_rows R = {d_x0, d_y0, d_dx, d_dy, n};
    return kch_chips(c, I, R, ksize_ref, ksize_mon, *d_out);
}

int km_chips(km_ctx *c, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref, ptrdiff_t smon,
             const float *x0, const float *y0, const float *dx, const float *dy, int n, int ksize_ref, int ksize_mon, const km_chip_outputs *out)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_chips_args(c, ref, mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, x0, y0, dx, dy, n, ksize_ref, ksize_mon, out)))
        return rc;
    if (n == 0) return KM_OK;
    const size_t es = km_dtype_size(dtype), px = (size_t)n * ch::PIXELS;
    void *d_ref, *d_mon;
    if ((rc = upload_image(c, WS_RAW_A, ref, es, Href, Wref, sref, &d_ref)) || (rc = upload_image(c, WS_RAW_B, mon, es, Hmon, Wmon, smon, &d_mon)))
        return rc;
    float *kp = (float *)km_ws(c, WS_MISC0, (size_t)n * 4 * sizeof(float));
    // WS_MISC1: ref_raw | mon_raw | ref_u8 | mon_u8 | ref_lap | mon_lap | windows | ok (the raw chips first: their type's alignment)
    const size_t lap_r = ksize_ref ? px : 0, lap_m = ksize_mon ? px : 0;
    const size_t off_u8 = up256(2 * px * es), off_win = up256(off_u8 + 2 * px + lap_r + lap_m), total = off_win + (size_t)n * 4 * sizeof(int32_t) + (size_t)n;
    char *buf = (char *)km_ws(c, WS_MISC1, total);
    if (!kp || !buf) return KM_E_NOMEM;
    const float *src[4] = {x0, y0, dx, dy};
    for (int i = 0; i < 4; i++) { const int rch = h2d_now(c, kp + (size_t)i * n, src[i], (size_t)n * sizeof(float)); if (rch) return rch; }
    km_chip_outputs d;
    d.ref_raw = buf; d.mon_raw = buf + px * es;
    d.ref_u8 = (uint8_t *)buf + off_u8; d.mon_u8 = d.ref_u8 + px;
    d.ref_lap = ksize_ref ? d.mon_u8 + px : nullptr;
    d.mon_lap = ksize_mon ? d.mon_u8 + px + lap_r : nullptr;
    d.windows = (int32_t *)(buf + off_win);
    d.ok = (uint8_t *)(d.windows + (size_t)n * 4);
    const kch_images I = {d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, (ptrdiff_t)Wref, (ptrdiff_t)Wmon};
    const kch_rows R = {kp, kp + n, kp + 2 * (size_t)n, kp + 3 * (size_t)n, n};
    if ((rc = kch_chips(c, I, R, ksize_ref, ksize_mon, d))) return rc;
    KM_D2H(c, out->ref_raw, d.ref_raw, px * es);
    KM_D2H(c, out->mon_raw, d.mon_raw, px * es);
    KM_D2H(c, out->ref_u8, d.ref_u8, px);
    KM_D2H(c, out->mon_u8, d.mon_u8, px);
    if (ksize_ref) KM_D2H(c, out->ref_lap, d.ref_lap, px);
    if (ksize_mon) KM_D2H(c, out->mon_lap, d.mon_lap, px);
    KM_D2H(c, out->windows, d.windows, (size_t)n * 4 * sizeof(int32_t));
    KM_D2H(c, out->ok, d.ok, (size_t)n);
    KM_FLUSH(c);
    return KM_OK;
}

}  // extern "C"

// ---- mean_profile of the report's figures (karios/report/commons.py:49-71): every check in front of the first launch or copy
namespace {

int check_profiles_args(km_ctx *c, int n, int n_prof, const km_profile *prof, const int32_t *n_groups, const int32_t *n_out_of_range)
{
    if (n < 0 || n > rp::MAX_ROWS) return km_fail(c, KM_E_ARG, "mean_profiles: %d rows (0 .. 2^20)", n);
    if (n_prof < 1 || n_prof > KM_PROFILE_MAX) return km_fail(c, KM_E_ARG, "mean_profiles: %d profiles (1 .. %d per call)", n_prof, KM_PROFILE_MAX);
    if (!prof || !n_groups || !n_out_of_range) return km_fail(c, KM_E_ARG, "mean_profiles: null argument");
    for (int k = 0; k < n_prof; k++) {
        const km_profile &p = prof[k];
        if (p.bin_size < 1 || p.bin_size > rp::MAX_BIN) return km_fail(c, KM_E_ARG, "mean_profiles: bin size %d of profile %d (1 .. 2^24)", p.bin_size, k);
        if (n > 0 && (!p.values || !p.positions || !p.key || !p.position || !p.count || !p.mean || !p.std))
            return km_fail(c, KM_E_ARG, "mean_profiles: null column or output of profile %d", k);
    }
    return KM_OK;
}

// the profiles one after the other on the context stream; their counts come back in one copy
int mean_profiles_dev(km_ctx *c, int n, int n_prof, const km_profile *d_prof, int32_t *n_groups, int32_t *n_out_of_range)
{
    const size_t cap = n > 0 ? (size_t)n : 1;
    kr_profile_ws ws;
    ws.keys_a = (unsigned long long *)km_ws(c, WS_RP_KEYS0, cap * sizeof(unsigned long long));
    ws.keys_b = (unsigned long long *)km_ws(c, WS_RP_KEYS1, cap * sizeof(unsigned long long));
    char *fl = (char *)km_ws(c, WS_RP_FLAG, up256(cap * sizeof(unsigned)) + KM_PROFILE_MAX * KR_COUNTS * sizeof(int32_t));
    if (!ws.keys_a || !ws.keys_b || !fl) return KM_E_NOMEM;
    ws.flags = (unsigned *)fl;
    int32_t *d_counts = (int32_t *)(fl + up256(cap * sizeof(unsigned)));
    for (int k = 0; k < n_prof; k++) {
        const km_profile &q = d_prof[k];
        const kr_profile p = {q.values, q.positions, q.bin_size, q.key, q.position, q.count, q.mean, q.std};
        const int rc = kr_mean_profile(c, p, n, ws, d_counts + (size_t)k * KR_COUNTS);
        if (rc) return rc;
    }
    int32_t counts[KM_PROFILE_MAX * KR_COUNTS];
    KM_D2H(c, counts, d_counts, (size_t)n_prof * KR_COUNTS * sizeof(int32_t));
    KM_FLUSH(c);
    for (int k = 0; k < n_prof; k++) { n_groups[k] = counts[k * KR_COUNTS + KR_GROUPS]; n_out_of_range[k] = counts[k * KR_COUNTS + KR_OUT_OF_RANGE]; }
    return KM_OK;
}

}  // namespace

extern "C" {

int km_mean_profiles_dev(km_ctx *c, int n, int n_prof, const km_profile *d_prof, int32_t *n_groups, int32_t *n_out_of_range)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_profiles_args(c, n, n_prof, d_prof, n_groups, n_out_of_range))) return rc;
    return mean_profiles_dev(c, n, n_prof, d_prof, n_groups, n_out_of_range);
}

int km_mean_profiles(km_ctx *c, int n, int n_prof, const km_profile *prof, int32_t *n_groups, int32_t *n_out_of_range)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_profiles_args(c, n, n_prof, prof, n_groups, n_out_of_range))) return rc;
    // WS_RP_IO: per profile values | positions | key | position | count | mean | std, n words each
    const size_t cap = n > 0 ? (size_t)n : 1;
    uint32_t *io = (uint32_t *)km_ws(c, WS_RP_IO, (size_t)n_prof * 7 * cap * sizeof(uint32_t));
    if (!io) return KM_E_NOMEM;
    km_profile d[KM_PROFILE_MAX];
    for (int k = 0; k < n_prof; k++) {
        uint32_t *b = io + (size_t)k * 7 * cap;
        d[k].values = (const float *)b; d[k].positions = (const float *)(b + cap);
        d[k].key = (float *)(b + 2 * cap); d[k].position = (int32_t *)(b + 3 * cap); d[k].count = (int32_t *)(b + 4 * cap);
        d[k].mean = (float *)(b + 5 * cap); d[k].std = (float *)(b + 6 * cap);
        d[k].bin_size = prof[k].bin_size;
        if (n > 0) {
            int rch;
            if ((rch = h2d_now(c, b, prof[k].values, (size_t)n * sizeof(float))) || (rch = h2d_now(c, b + cap, prof[k].positions, (size_t)n * sizeof(float))))
                return rch;
        }
    }
    if ((rc = mean_profiles_dev(c, n, n_prof, d, n_groups, n_out_of_range))) return rc;
    bool any = false;
    for (int k = 0; k < n_prof; k++) {
        const size_t bytes = (size_t)n_groups[k] * sizeof(uint32_t);
        if (!bytes) continue;
        KM_D2H(c, prof[k].key, d[k].key, bytes);
        KM_D2H(c, prof[k].position, d[k].position, bytes);
        KM_D2H(c, prof[k].count, d[k].count, bytes);
        KM_D2H(c, prof[k].mean, d[k].mean, bytes);
        KM_D2H(c, prof[k].std, d[k].std, bytes);
        any = true;
    }
    if (any) KM_FLUSH(c);
    return KM_OK;
}

}  // extern "C"

// ---- the report's products and the altitude figure's numbers (karios/report/product_generator.py:138-218, karios/api/core.py:1049-1053,
// karios/report/shift_by_alt_plot.py:127-171): every check in front of the first launch or copy
namespace {

int check_rasters_args(km_ctx *c, int n, const float *x0, const float *y0, const float *dx, const float *dy, int H, int W, const uint8_t *mask,
                       ptrdiff_t mask_stride, const float *delta, ptrdiff_t band_stride, ptrdiff_t row_stride, const int32_t *n_out_of_range)
{
    if (n < 0 || n > pm::MAX_ROWS) return km_fail(c, KM_E_ARG, "point_rasters: %d rows (0 .. 2^20)", n);
    if (H < 1 || W < 1 || (unsigned long long)H * (unsigned long long)W >= pm::NO_PIXEL)
        return km_fail(c, KM_E_ARG, "point_rasters: a raster of %d x %d (at least 1 x 1, fewer than 2^32 - 1 pixels)", H, W);
    if (!n_out_of_range) return km_fail(c, KM_E_ARG, "point_rasters: null count");
    if (n > 0 && (!x0 || !y0)) return km_fail(c, KM_E_ARG, "point_rasters: null coordinates");
    if (mask && mask_stride < W) return km_fail(c, KM_E_ARG, "point_rasters: mask stride %td < width %d", mask_stride, W);
    if (delta) {
        if (n > 0 && (!dx || !dy)) return km_fail(c, KM_E_ARG, "point_rasters: a delta raster needs dx and dy");
        if (row_stride < W) return km_fail(c, KM_E_ARG, "point_rasters: delta row stride %td < width %d", row_stride, W);
        if (band_stride < (ptrdiff_t)(H - 1) * row_stride + W) return km_fail(c, KM_E_ARG, "point_rasters: delta band stride %td: the bands overlap", band_stride);
        if ((uintptr_t)delta & 3u) return km_fail(c, KM_E_ARG, "point_rasters: delta raster off the float grid");
    }
    return KM_OK;
}

int point_rasters_dev(km_ctx *c, const kpd_rasters &r, int32_t *n_out_of_range)
{
    const size_t cap = r.n > 0 ? (size_t)r.n : 1;
    kpd_rasters_ws ws = {nullptr, nullptr};
    if (r.delta) {
        ws.keys_a = (unsigned long long *)km_ws(c, WS_RP_KEYS0, cap * sizeof(unsigned long long));
        ws.keys_b = (unsigned long long *)km_ws(c, WS_RP_KEYS1, cap * sizeof(unsigned long long));
        if (!ws.keys_a || !ws.keys_b) return KM_E_NOMEM;
    }
    int32_t *d_count = (int32_t *)km_ws(c, WS_RP_FLAG, 256);
    if (!d_count) return KM_E_NOMEM;
    const int rc = kpd_point_rasters(c, r, ws, d_count);
    if (rc) return rc;
    KM_D2H(c, n_out_of_range, d_count, sizeof(int32_t));
    KM_FLUSH(c);
    return KM_OK;
}

int check_sample_args(km_ctx *c, const void *raster, int dtype, int H, int W, ptrdiff_t stride, int n, const float *x0, const float *y0, const void *out,
                      const int32_t *n_out_of_range)
{
    int rc;
    if ((rc = check_image(c, raster, H, W, stride, "sample_points"))) return rc;
    if (!km_dtype_size(dtype)) return km_fail(c, KM_E_ARG, "sample_points: dtype %d (uint8, uint16, int16 and float32 only)", dtype);
    if (n < 0 || n > pm::MAX_ROWS) return km_fail(c, KM_E_ARG, "sample_points: %d rows (0 .. 2^20)", n);
    if (!n_out_of_range || (n > 0 && (!x0 || !y0 || !out))) return km_fail(c, KM_E_ARG, "sample_points: null argument");
    return KM_OK;
}

int check_box_args(km_ctx *c, int n, const float *values, const float *positions, int bin_size, const float *key, const int32_t *count, const float *mean,
                   const double *stats, const int8_t *cls, const int32_t *n_groups)
{
    if (n < 0 || n > pm::MAX_ROWS) return km_fail(c, KM_E_ARG, "box_stats: %d rows (0 .. 2^20)", n);
    if (bin_size < 1 || bin_size > pm::MAX_BIN) return km_fail(c, KM_E_ARG, "box_stats: bin size %d (1 .. 2^24)", bin_size);
    if (!n_groups || (n > 0 && (!values || !positions || !key || !count || !mean || !stats || !cls))) return km_fail(c, KM_E_ARG, "box_stats: null argument");
    return KM_OK;
}

int box_stats_dev(km_ctx *c, const kpd_box &b, int n, int32_t *n_groups)
{
    const size_t cap = n > 0 ? (size_t)n : 1;
    kpd_box_ws ws;
    ws.keys_a = (unsigned long long *)km_ws(c, WS_RP_KEYS0, cap * sizeof(unsigned long long));
    ws.keys_b = (unsigned long long *)km_ws(c, WS_RP_KEYS1, cap * sizeof(unsigned long long));
    char *fl = (char *)km_ws(c, WS_RP_FLAG, up256(cap * sizeof(unsigned)) + KPD_COUNTS * sizeof(int32_t));
    ws.misc = (uint32_t *)km_ws(c, WS_PD_MISC, KPD_BOX_MISC_WORDS(cap) * sizeof(uint32_t));
    if (!ws.keys_a || !ws.keys_b || !fl || !ws.misc) return KM_E_NOMEM;
    ws.flags = (unsigned *)fl;
    int32_t *d_counts = (int32_t *)(fl + up256(cap * sizeof(unsigned)));
    const int rc = kpd_box_stats(c, b, n, ws, d_counts);
    if (rc) return rc;
    int32_t counts[KPD_COUNTS];
    KM_D2H(c, counts, d_counts, sizeof counts);
    KM_FLUSH(c);
    *n_groups = counts[KPD_GROUPS];
    return KM_OK;
}

}  // namespace

extern "C" {

int km_point_rasters_dev(km_ctx *c, int n, const float *d_x0, const float *d_y0, const float *d_dx, const float *d_dy, int H, int W, uint8_t *d_mask,
                         ptrdiff_t mask_stride, float *d_delta, ptrdiff_t band_stride, ptrdiff_t row_stride, int32_t *n_out_of_range)
{
    int rc;
    if ((rc = begin_call(c)) ||
        (rc = check_rasters_args(c, n, d_x0, d_y0, d_dx, d_dy, H, W, d_mask, mask_stride, d_delta, band_stride, row_stride, n_out_of_range)))
        return rc;
    const kpd_rasters r = {d_x0, d_y0, d_dx, d_dy, n, H, W, d_mask, mask_stride, d_delta, band_stride, row_stride};
    return point_rasters_dev(c, r, n_out_of_range);
}

int km_point_rasters(km_ctx *c, int n, const float *x0, const float *y0, const float *dx, const float *dy, int H, int W, uint8_t *mask,
                     ptrdiff_t mask_stride, float *delta, ptrdiff_t band_stride, ptrdiff_t row_stride, int32_t *n_out_of_range)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_rasters_args(c, n, x0, y0, dx, dy, H, W, mask, mask_stride, delta, band_stride, row_stride, n_out_of_range)))
        return rc;
    // WS_MISC0: x0 | y0 | dx | dy; WS_RP_IO: the mask, then the two bands, all dense
    const size_t cap = n > 0 ? (size_t)n : 1, px = (size_t)H * W, off_delta = up256(mask ? px : 0);
    float *kp = (float *)km_ws(c, WS_MISC0, cap * 4 * sizeof(float));
    char *io = (char *)km_ws(c, WS_RP_IO, off_delta + (delta ? 2 * px * sizeof(float) : 0));
    if (!kp || !io) return KM_E_NOMEM;
    const float *src[4] = {x0, y0, delta ? dx : nullptr, delta ? dy : nullptr};
    for (int i = 0; i < 4 && n > 0; i++)
        if (src[i]) { const int rch = h2d_now(c, kp + (size_t)i * cap, src[i], (size_t)n * sizeof(float)); if (rch) return rch; }
    kpd_rasters r = {kp, kp + cap, kp + 2 * cap, kp + 3 * cap, n, H, W, mask ? (uint8_t *)io : nullptr, (ptrdiff_t)W,
                     delta ? (float *)(io + off_delta) : nullptr, (ptrdiff_t)px, (ptrdiff_t)W};
    if ((rc = point_rasters_dev(c, r, n_out_of_range))) return rc;
    // the planes back: one copy where the caller's rows are dense, else row by row
    if (mask) {
        if (mask_stride == W) KM_D2H(c, mask, r.mask, px);
        else for (int y = 0; y < H; y++) KM_D2H(c, mask + (ptrdiff_t)y * mask_stride, r.mask + (size_t)y * W, (size_t)W);
    }
    for (int b = 0; b < 2 && delta; b++) {
        if (row_stride == W) KM_D2H(c, delta + b * band_stride, r.delta + b * px, px * sizeof(float));
        else for (int y = 0; y < H; y++) KM_D2H(c, delta + b * band_stride + (ptrdiff_t)y * row_stride, r.delta + b * px + (size_t)y * W, (size_t)W * sizeof(float));
    }
    if (mask || delta) KM_FLUSH(c);
    return KM_OK;
}

int km_sample_points_dev(km_ctx *c, const void *d_raster, int dtype, int H, int W, ptrdiff_t stride, int n, const float *d_x0, const float *d_y0, void *d_out,
                         int32_t *n_out_of_range)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_sample_args(c, d_raster, dtype, H, W, stride, n, d_x0, d_y0, d_out, n_out_of_range))) return rc;
    int32_t *d_count = (int32_t *)km_ws(c, WS_RP_FLAG, 256);
    if (!d_count) return KM_E_NOMEM;
    if ((rc = kpd_sample_points(c, d_raster, dtype, H, W, stride, n, d_x0, d_y0, d_out, d_count))) return rc;
    KM_D2H(c, n_out_of_range, d_count, sizeof(int32_t));
    KM_FLUSH(c);
    return KM_OK;
}

int km_sample_points(km_ctx *c, const void *raster, int dtype, int H, int W, ptrdiff_t stride, int n, const float *x0, const float *y0, void *out,
                     int32_t *n_out_of_range)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_sample_args(c, raster, dtype, H, W, stride, n, x0, y0, out, n_out_of_range))) return rc;
    const size_t es = km_dtype_size(dtype), cap = n > 0 ? (size_t)n : 1;
    void *d_raster;
    if ((rc = upload_image(c, WS_RAW_A, raster, es, H, W, stride, &d_raster))) return rc;
    float *kp = (float *)km_ws(c, WS_MISC0, cap * 2 * sizeof(float));
    char *d_out = (char *)km_ws(c, WS_MISC1, up256(cap * es) + 256);
    if (!kp || !d_out) return KM_E_NOMEM;
    if (n > 0) {
        int rch;
        if ((rch = h2d_now(c, kp, x0, (size_t)n * sizeof(float))) || (rch = h2d_now(c, kp + cap, y0, (size_t)n * sizeof(float)))) return rch;
    }
    int32_t *d_count = (int32_t *)(d_out + up256(cap * es));
    if ((rc = kpd_sample_points(c, d_raster, dtype, H, W, (ptrdiff_t)W, n, kp, kp + cap, d_out, d_count))) return rc;
    if (n > 0) KM_D2H(c, out, d_out, (size_t)n * es);
    KM_D2H(c, n_out_of_range, d_count, sizeof(int32_t));
    KM_FLUSH(c);
    return KM_OK;
}

int km_box_stats_dev(km_ctx *c, int n, const float *d_values, const float *d_positions, int bin_size, float *d_key, int32_t *d_count, float *d_mean,
                     double *d_stats, int8_t *d_cls, int32_t *n_groups)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_box_args(c, n, d_values, d_positions, bin_size, d_key, d_count, d_mean, d_stats, d_cls, n_groups))) return rc;
    const kpd_box b = {d_values, d_positions, bin_size, d_key, d_count, d_mean, d_stats, d_cls};
    return box_stats_dev(c, b, n, n_groups);
}

int km_box_stats(km_ctx *c, int n, const float *values, const float *positions, int bin_size, float *key, int32_t *count, float *mean, double *stats,
                 int8_t *cls, int32_t *n_groups)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_box_args(c, n, values, positions, bin_size, key, count, mean, stats, cls, n_groups))) return rc;
    // WS_RP_IO: stats (8 n doubles) | values | positions | key | count | mean (n words each) | cls (n bytes)
    const size_t cap = n > 0 ? (size_t)n : 1;
    char *io = (char *)km_ws(c, WS_RP_IO, cap * (pm::N_STATS * sizeof(double) + 5 * sizeof(uint32_t) + 1));
    if (!io) return KM_E_NOMEM;
    double *d_stats = (double *)io;
    uint32_t *w = (uint32_t *)(io + cap * pm::N_STATS * sizeof(double));
    const kpd_box b = {(const float *)w, (const float *)(w + cap), bin_size, (float *)(w + 2 * cap), (int32_t *)(w + 3 * cap), (float *)(w + 4 * cap), d_stats,
                       (int8_t *)(w + 5 * cap)};
    if (n > 0) {
        int rch;
        if ((rch = h2d_now(c, w, values, (size_t)n * sizeof(float))) || (rch = h2d_now(c, w + cap, positions, (size_t)n * sizeof(float)))) return rch;
    }
    if ((rc = box_stats_dev(c, b, n, n_groups))) return rc;
    if (n == 0) return KM_OK;
    const size_t g = (size_t)*n_groups;
    if (g) {
        KM_D2H(c, key, b.key, g * sizeof(float));
        KM_D2H(c, count, b.count, g * sizeof(int32_t));
        KM_D2H(c, mean, b.mean, g * sizeof(float));
        for (int s = 0; s < pm::N_STATS; s++) KM_D2H(c, stats + (size_t)s * n, d_stats + (size_t)s * n, g * sizeof(double));
    }
    KM_D2H(c, cls, b.cls, (size_t)n);
    KM_FLUSH(c);
    return KM_OK;
}

}  // extern "C"
