// ChipService.generate_chips (report/chip_service.py): the key-point selection and the chips (include/karios_hip.h): every check in front of
// the first launch or copy.
#include "api_internal.hpp"
#include "k_chips.hpp"

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
    const size_t cap = n > 0 ? (size_t)n : 1;
    const float *src[3] = {x0, y0, score};
    float *in;
    if ((rc = upload_columns(c, WS_MISC0, src, 3, n, &in))) return rc;
    return chip_select_dev(c, in, in + cap, in + 2 * cap, n, select_grid(width, height, threshold, threshold_f64, grid_rows, grid_cols), nullptr,
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
    // WS_MISC1: ref_raw | mon_raw | ref_u8 | mon_u8 | ref_lap | mon_lap | windows | ok (the raw chips first: their type's alignment)
    const size_t lap_r = ksize_ref ? px : 0, lap_m = ksize_mon ? px : 0;
    const size_t off_u8 = up256(2 * px * es), off_win = up256(off_u8 + 2 * px + lap_r + lap_m), total = off_win + (size_t)n * 4 * sizeof(int32_t) + (size_t)n;
    char *buf = (char *)km_ws(c, WS_MISC1, total);
    if (!buf) return KM_E_NOMEM;
    const float *src[4] = {x0, y0, dx, dy};
    float *kp;
    if ((rc = upload_columns(c, WS_MISC0, src, 4, n, &kp))) return rc;
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
