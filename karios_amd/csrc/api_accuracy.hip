// KariosAPI.analyze_accuracy (core.py:268-328): the valid-pixel count and GeometricStat (accuracy_statistics.py); the tracker's outlier clip
// (klt.py:52-71) on resident columns.
#include "api_internal.hpp"
#include "k_accuracy.hpp"
#include "k_clip.hpp"

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
    const size_t cap = n > 0 ? (size_t)n : 1;
    const float *src[3] = {dx, dy, score};
    float *in;
    if ((rc = upload_columns(c, WS_AC_IN, src, 3, n, &in))) return rc;
    return accuracy_stats_dev(c, in, in + cap, in + 2 * cap, n, thr, carto, factor, n_percent, percents, out);
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
