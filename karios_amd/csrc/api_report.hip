// mean_profile of the report's figures (report/commons.py:49-71); the report's products (report/product_generator.py:138-218), the altitude
// column (core.py:1049-1053) and the box statistics of the altitude figure (report/shift_by_alt_plot.py:127-171): every check in front of
// the first launch or copy.  The numbers of the circular-error figure (report/circular_error_plot.py), in three stages.
#include "api_internal.hpp"
#include "k_ce.hpp"
#include "k_products.hpp"
#include "k_report.hpp"

#include <math.h>
#include <string.h>
#include <vector>

// ---- mean_profile of the report's figures
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

// ---- the report's products and the altitude figure's numbers
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
    char *io = (char *)km_ws(c, WS_RP_IO, off_delta + (delta ? 2 * px * sizeof(float) : 0));
    if (!io) return KM_E_NOMEM;
    const float *src[4] = {x0, y0, delta ? dx : nullptr, delta ? dy : nullptr};
    float *kp;
    if ((rc = upload_columns(c, WS_MISC0, src, 4, n, &kp))) return rc;
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
    char *d_out = (char *)km_ws(c, WS_MISC1, up256(cap * es) + 256);
    if (!d_out) return KM_E_NOMEM;
    const float *src[2] = {x0, y0};
    float *kp;
    if ((rc = upload_columns(c, WS_MISC0, src, 2, n, &kp))) return rc;
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

// ---- the circular-error figure's numbers (karios/report/circular_error_plot.py): three stages on one sample, which the context keeps
namespace {

int check_ce_args(km_ctx *c, const km_ce_job *j)
{
    if (!j) return km_fail(c, KM_E_ARG, "ce_figure: null job");
    if (j->n < 0 || j->n > (1 << 24)) return km_fail(c, KM_E_ARG, "ce_figure: %d rows (0 .. 2^24)", j->n);
    if (j->n > 0 && (!j->dx || !j->dy || !j->score)) return km_fail(c, KM_E_ARG, "ce_figure: null column");
    switch (j->stage) {
    case KM_CE_SAMPLE:
        if (j->thr != j->thr) return km_fail(c, KM_E_ARG, "ce_figure: the threshold is NaN");
        if (!isfinite((float)j->res)) return km_fail(c, KM_E_ARG, "ce_figure: the resolution is not a finite float32");
        if (!j->block) return km_fail(c, KM_E_ARG, "ce_figure: null block");
        return KM_OK;
    case KM_CE_COUNTS:
        if (j->bins_x < 0 || j->bins_x > KM_CE_MAX_BINS || j->bins_y < 0 || j->bins_y > KM_CE_MAX_BINS)
            return km_fail(c, KM_E_ARG, "ce_figure: %d and %d bins (0 .. %d each)", j->bins_x, j->bins_y, KM_CE_MAX_BINS);
        if ((j->bins_x && (!j->edges_x || !j->hist_x)) || (j->bins_y && (!j->edges_y || !j->hist_y)) || !j->edges_grid || !j->counts_grid)
            return km_fail(c, KM_E_ARG, "ce_figure: null edges or counts");
        break;
    case KM_CE_CURVES:
        if (!j->tx || !j->ty || !j->coef || !j->box || !j->scatter_x || !j->scatter_y || !j->scatter_z || !j->radial || !j->tail)
            return km_fail(c, KM_E_ARG, "ce_figure: null spline or output");
        break;
    default: return km_fail(c, KM_E_ARG, "ce_figure: stage %d", j->stage);
    }
    if (j->n == 0 || c->ce_rows != j->n || c->ce_cols != j->dx || c->ce_sample < 1)
        return km_fail(c, KM_E_ARG, "ce_figure: stage %d needs KM_CE_SAMPLE of the same columns first, with a sample that is not empty", j->stage);
    return KM_OK;
}

int ce_sample_stage(km_ctx *c, const km_ce_job *j, const float *d_dx, const float *d_dy, const float *d_score)
{
    c->ce_rows = -1;
    *j->block = km_ce_block();
    if (j->n == 0) return KM_OK;
    const size_t cap = (size_t)j->n;
    kce_state *s = (kce_state *)km_ws(c, WS_CE_STATE, sizeof(kce_state));
    float *cols = (float *)km_ws(c, WS_AC_COLS, cap * 3 * sizeof(float));
    float *scaled = (float *)km_ws(c, WS_CE_COLS, cap * 4 * sizeof(float));
    float *bsum = (float *)km_ws(c, WS_AC_BSUM, (size_t)ka_nblocks(j->n) * 3 * sizeof(float));
    if (!s || !cols || !scaled || !bsum) return KM_E_NOMEM;
    int rc;
    if ((rc = ka_compact(c, d_dx, d_dy, d_score, j->n, j->thr, j->carto, cols, &s->st)) || (rc = kce_scale(c, cols, j->n, (float)j->res, scaled, s)) ||
        (rc = ka_block_sums(c, scaled, j->n, &s->scaled, 0, bsum)) || (rc = ka_finish(c, bsum, j->n, &s->scaled, 0)) ||
        (rc = ka_block_sums(c, scaled, j->n, &s->scaled, 1, bsum)) || (rc = ka_finish(c, bsum, j->n, &s->scaled, 1)) || (rc = kce_block(c, s)))
        return rc;
    KM_D2H(c, j->block, &s->block, sizeof(km_ce_block));
    KM_FLUSH(c);
    c->ce_rows = j->n; c->ce_sample = j->block->sample; c->ce_cols = j->dx;
    return KM_OK;
}

int ce_counts_stage(km_ctx *c, const km_ce_job *j)
{
    kce_state *s = (kce_state *)km_ws_peek(c, WS_CE_STATE);
    const float *scaled = (const float *)km_ws_peek(c, WS_CE_COLS);
    // WS_CE_TAB: edges of x (bins_x + 1) | of y (bins_y + 1) | of the grid (22) | counters of x | of y | of the grid (100), zero
    const size_t bx = (size_t)j->bins_x, by = (size_t)j->bins_y, ng = 2 * (ce::GRID + 1), nc = ce::GRID * ce::GRID;
    const size_t off_y = bx + 1, off_g = off_y + by + 1, off_cx = off_g + ng, off_cy = off_cx + bx, off_cg = off_cy + by, words = off_cg + nc;
    uint32_t *tab = (uint32_t *)km_ws(c, WS_CE_TAB, words * sizeof(uint32_t));
    if (!s || !scaled || !tab) return s && scaled ? KM_E_NOMEM : km_fail(c, KM_E_ARG, "ce_figure: the sample has left the context");
    std::vector<uint32_t> host(words, 0u);
    if (bx) memcpy(host.data(), j->edges_x, (bx + 1) * sizeof(float));
    if (by) memcpy(host.data() + off_y, j->edges_y, (by + 1) * sizeof(float));
    memcpy(host.data() + off_g, j->edges_grid, ng * sizeof(float));
    int rc;
    if ((rc = h2d_now(c, tab, host.data(), words * sizeof(uint32_t)))) return rc;
    const kce_axis ax = {(const float *)tab, tab + off_cx, j->bins_x}, ay = {(const float *)(tab + off_y), tab + off_cy, j->bins_y};
    if ((rc = kce_axis_hist(c, scaled, j->n, s, ax, ay)) || (rc = kce_grid_hist(c, scaled, j->n, s, (const float *)(tab + off_g), tab + off_cg))) return rc;
    if (bx) KM_D2H(c, j->hist_x, tab + off_cx, bx * sizeof(uint32_t));
    if (by) KM_D2H(c, j->hist_y, tab + off_cy, by * sizeof(uint32_t));
    KM_D2H(c, j->counts_grid, tab + off_cg, nc * sizeof(uint32_t));
    KM_FLUSH(c);
    return KM_OK;
}

int ce_curves_stage(km_ctx *c, const km_ce_job *j, bool dev)
{
    const size_t cap = (size_t)j->n, got = (size_t)c->ce_sample;
    kce_state *s = (kce_state *)km_ws_peek(c, WS_CE_STATE);
    float *scaled = (float *)km_ws_peek(c, WS_CE_COLS);
    kce_spline *d_sp = (kce_spline *)km_ws(c, WS_CE_TAB, sizeof(kce_spline));
    unsigned long long *k0 = (unsigned long long *)km_ws(c, WS_AC_KEYS0, 2 * cap * sizeof(unsigned long long));
    unsigned long long *k1 = (unsigned long long *)km_ws(c, WS_AC_KEYS1, 2 * cap * sizeof(unsigned long long));
    float *io = dev ? nullptr : (float *)km_ws(c, WS_CE_IO, 4 * cap * sizeof(float));
    if (!s || !scaled) return km_fail(c, KM_E_ARG, "ce_figure: the sample has left the context");
    if (!d_sp || !k0 || !k1 || (!dev && !io)) return KM_E_NOMEM;
    kce_spline sp;
    memcpy(sp.tx, j->tx, sizeof sp.tx); memcpy(sp.ty, j->ty, sizeof sp.ty); memcpy(sp.c, j->coef, sizeof sp.c); memcpy(sp.box, j->box, sizeof sp.box);
    int rc;
    if ((rc = h2d_now(c, d_sp, &sp, sizeof sp))) return rc;
    float *out[4] = {dev ? j->scatter_x : io, dev ? j->scatter_y : io + cap, dev ? j->scatter_z : io + 2 * cap, dev ? j->radial : io + 3 * cap};
    if ((rc = kce_density_keys(c, scaled, j->n, s, d_sp, scaled + 3 * cap, k0)) ||
        (rc = kce_sort_gather(c, scaled, scaled + 3 * cap, k0, k1, j->n, s, out[0], out[1], out[2], out[3])))
        return rc;
    KM_D2H(c, j->tail, &s->tail, sizeof(km_ce_tail));
    if (!dev) {
        float *dst[4] = {j->scatter_x, j->scatter_y, j->scatter_z, j->radial};
        for (int k = 0; k < 4; k++) KM_D2H(c, dst[k], out[k], got * sizeof(float));
    }
    KM_FLUSH(c);
    return KM_OK;
}

}  // namespace

extern "C" {

int km_ce_figure_dev(km_ctx *c, const km_ce_job *job)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_ce_args(c, job))) return rc;
    if (job->stage == KM_CE_SAMPLE) return ce_sample_stage(c, job, job->dx, job->dy, job->score);
    return job->stage == KM_CE_COUNTS ? ce_counts_stage(c, job) : ce_curves_stage(c, job, true);
}

int km_ce_figure(km_ctx *c, const km_ce_job *job)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_ce_args(c, job))) return rc;
    if (job->stage == KM_CE_COUNTS) return ce_counts_stage(c, job);
    if (job->stage == KM_CE_CURVES) return ce_curves_stage(c, job, false);
    const size_t cap = job->n > 0 ? (size_t)job->n : 1;
    const float *src[3] = {job->dx, job->dy, job->score};
    float *in;
    if ((rc = upload_columns(c, WS_AC_IN, src, 3, job->n, &in))) return rc;
    return ce_sample_stage(c, job, in, in + cap, in + 2 * cap);
}

}  // extern "C"
