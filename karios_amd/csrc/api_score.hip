// Scoring entry points: ZNCCService.compute_zncc / _zncc2 (zncc_service.py:45-238), the ZNCC search around each key point
// (k_zncc_search.hip; no counterpart in the reference's call graph), the mutual-information scores
// (mutual_info_service.py:73-130, zncc_service.py:240-287) and their search (k_mi_search.hip), the DN-value filter of the key points (core.py:650-737).
#include "api_internal.hpp"
#include "k_mi_search.hpp"
#include "k_zncc_search.hpp"

namespace {

// what km_zncc_search, km_mi_search and their device forms refuse alike; n == 0 passes (nothing is launched then)
int search_args(km_ctx *c, const char *what, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref, ptrdiff_t smon,
                const float *x0, const float *y0, const float *dx, const float *dy, int n, int radius, const int32_t *offset, const double *peak,
                const double *shift, const uint8_t *status)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, ref, Href, Wref, sref, what)) || (rc = check_image(c, mon, Hmon, Wmon, smon, what)))
        return rc;
    if (!km_dtype_size(dtype)) return km_fail(c, KM_E_ARG, "%s: bad dtype %d", what, dtype);
    if (radius < 1 || radius > zs::MAX_RADIUS) return km_fail(c, KM_E_ARG, "%s: radius %d (1 .. %d)", what, radius, zs::MAX_RADIUS);
    if (n < 0 || n > zs::MAX_ROWS) return km_fail(c, KM_E_ARG, "%s: %d rows (0 .. 2^20)", what, n);
    if (n > 0 && (!x0 || !y0 || !dx || !dy || !offset || !peak || !shift || !status)) return km_fail(c, KM_E_ARG, "%s: null keypoint or output array", what);
    if (c->window.H) return km_fail(c, KM_E_UNSUPPORTED, "%s: an image window is set (km_set_image_window); the search reads whole rasters", what);
    return KM_OK;
}

}  // namespace

extern "C" {

int km_zncc_search_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref,
                       ptrdiff_t smon, const float *d_x0, const float *d_y0, const float *d_dx, const float *d_dy, int n, int radius,
                       int32_t *d_offset, double *d_peak, double *d_shift, uint8_t *d_status, double *d_surface)
{
    int rc;
    if ((rc = search_args(c, "zncc_search", d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, d_x0, d_y0, d_dx, d_dy, n, radius, d_offset, d_peak, d_shift, d_status)))
        return rc;
    if (n == 0) return KM_OK;
    const kzs_args a = {d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, d_x0, d_y0, d_dx, d_dy, n, radius, d_offset, d_peak, d_shift, d_status, d_surface};
    c->evs_used[c->ev_cur][ST_ZNCC] = false;
    km_stage_timer t(c, ST_ZNCC);
    return kzs_search(c, a);
}

int km_zncc_search(km_ctx *c, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref,
                   ptrdiff_t smon, const float *x0, const float *y0, const float *dx, const float *dy, int n, int radius, int32_t *out_offset,
                   double *out_peak, double *out_shift, uint8_t *out_status, double *out_surface)
{
    int rc;
    if ((rc = search_args(c, "zncc_search", ref, mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, x0, y0, dx, dy, n, radius, out_offset, out_peak, out_shift, out_status)))
        return rc;
    if (n == 0) return KM_OK;
    const size_t es = km_dtype_size(dtype), N = (size_t)n, SS = (size_t)(2 * radius + 1) * (2 * radius + 1);
    void *d_ref, *d_mon;
    if ((rc = upload_image(c, WS_RAW_A, ref, es, Href, Wref, sref, &d_ref)) || (rc = upload_image(c, WS_RAW_B, mon, es, Hmon, Wmon, smon, &d_mon)))
        return rc;
    // peak | shift | offset | status in one slot (each part a multiple of 256 bytes apart); the surface in one of its own
    const size_t o_shift = up256(N * sizeof(double)), o_offset = o_shift + up256(2 * N * sizeof(double)), o_status = o_offset + up256(2 * N * sizeof(int32_t));
    char *d_out = (char *)km_ws(c, WS_MISC1, o_status + up256(N));
    double *d_surface = out_surface ? (double *)km_ws(c, WS_MISC2, N * SS * sizeof(double)) : nullptr;
    if (!d_out || (out_surface && !d_surface)) return KM_E_NOMEM;
    const float *src[4] = {x0, y0, dx, dy};
    float *kp;
    if ((rc = upload_columns(c, WS_MISC0, src, 4, n, &kp))) return rc;
    const kzs_args a = {d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, Wref, Wmon, kp, kp + N, kp + 2 * N, kp + 3 * N, n, radius,
                        (int32_t *)(d_out + o_offset), (double *)d_out, (double *)(d_out + o_shift), (uint8_t *)(d_out + o_status), d_surface};
    {
        c->evs_used[c->ev_cur][ST_ZNCC] = false;
        km_stage_timer t(c, ST_ZNCC);
        if ((rc = kzs_search(c, a))) return rc;
    }
    KM_D2H(c, out_peak, a.peak, N * sizeof(double));
    KM_D2H(c, out_shift, a.shift, 2 * N * sizeof(double));
    KM_D2H(c, out_offset, a.offset, 2 * N * sizeof(int32_t));
    KM_D2H(c, out_status, a.status, N);
    if (out_surface) KM_D2H(c, out_surface, d_surface, N * SS * sizeof(double));
    KM_FLUSH(c);
    return KM_OK;
}

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
    double *d_out = (double *)km_ws(c, WS_MISC1, (size_t)n * sizeof(double));
    if (!d_out) return KM_E_NOMEM;
    const float *src[4] = {x0, y0, dx, dy};
    float *kp;
    if ((rc = upload_columns(c, WS_MISC0, src, 4, n, &kp))) return rc;
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
    {
        c->evs_used[c->ev_cur][ST_ZNCC] = false;      // (timed like the other ZNCC kernels: tools/ubench/zncc_search.py reads it)
        km_stage_timer t(c, ST_ZNCC);
        if ((rc = kz_zncc_windows(c, d1, d2, dtype1, dtype2, H1, W1, H2, W2, W1, W2, d_uv, half_size, count, d_out, d_fl))) return rc;
    }
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
    double *d_out = (double *)km_ws(c, WS_MISC1, (size_t)n * 2 * sizeof(double));
    if (!d_out) return KM_E_NOMEM;
    const float *src[4] = {x0, y0, dx, dy};
    float *kp;
    if ((rc = upload_columns(c, WS_MISC0, src, 4, n, &kp))) return rc;
    if ((rc = kmi_batch(c, d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, Wref, Wmon, kp, kp + n, kp + 2 * (size_t)n, kp + 3 * (size_t)n, n, nullptr,
                        nullptr, 0.f, out_st ? d_out : nullptr, out_nmi ? d_out + n : nullptr)))
        return rc;
    if (out_st) KM_D2H(c, out_st, d_out, (size_t)n * sizeof(double));
    if (out_nmi) KM_D2H(c, out_nmi, d_out + n, (size_t)n * sizeof(double));
    KM_FLUSH(c);
    return KM_OK;
}

int km_mi_search_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref,
                     ptrdiff_t smon, const float *d_x0, const float *d_y0, const float *d_dx, const float *d_dy, int n, int radius,
                     int32_t *d_offset, double *d_peak, double *d_peak_mi, double *d_shift, uint8_t *d_status, double *d_surface)
{
    int rc;
    if ((rc = search_args(c, "mi_search", d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, d_x0, d_y0, d_dx, d_dy, n, radius, d_offset, d_peak, d_shift, d_status)))
        return rc;
    if (n > 0 && !d_peak_mi) return km_fail(c, KM_E_ARG, "mi_search: null keypoint or output array");
    if (n == 0) return KM_OK;
    const kms_args a = {d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, d_x0, d_y0, d_dx, d_dy, n, radius, d_offset, d_peak, d_peak_mi, d_shift, d_status, d_surface};
    c->evs_used[c->ev_cur][ST_MI] = false;
    km_stage_timer t(c, ST_MI);
    return kms_search(c, a);
}

int km_mi_search(km_ctx *c, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref,
                 ptrdiff_t smon, const float *x0, const float *y0, const float *dx, const float *dy, int n, int radius, int32_t *out_offset,
                 double *out_peak, double *out_peak_mi, double *out_shift, uint8_t *out_status, double *out_surface)
{
    int rc;
    if ((rc = search_args(c, "mi_search", ref, mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, x0, y0, dx, dy, n, radius, out_offset, out_peak, out_shift, out_status)))
        return rc;
    if (n > 0 && !out_peak_mi) return km_fail(c, KM_E_ARG, "mi_search: null keypoint or output array");
    if (n == 0) return KM_OK;
    const size_t es = km_dtype_size(dtype), N = (size_t)n, SS = (size_t)(2 * radius + 1) * (2 * radius + 1);
    void *d_ref, *d_mon;
    if ((rc = upload_image(c, WS_RAW_A, ref, es, Href, Wref, sref, &d_ref)) || (rc = upload_image(c, WS_RAW_B, mon, es, Hmon, Wmon, smon, &d_mon)))
        return rc;
    // peak | peak_mi | shift | offset | status in one slot (each part a multiple of 256 bytes apart); the surface in one of its own
    const size_t o_mi = up256(N * sizeof(double)), o_shift = o_mi + up256(N * sizeof(double)), o_offset = o_shift + up256(2 * N * sizeof(double)),
                 o_status = o_offset + up256(2 * N * sizeof(int32_t));
    char *d_out = (char *)km_ws(c, WS_MISC1, o_status + up256(N));
    double *d_surface = out_surface ? (double *)km_ws(c, WS_MISC2, N * SS * sizeof(double)) : nullptr;
    if (!d_out || (out_surface && !d_surface)) return KM_E_NOMEM;
    const float *src[4] = {x0, y0, dx, dy};
    float *kp;
    if ((rc = upload_columns(c, WS_MISC0, src, 4, n, &kp))) return rc;
    const kms_args a = {d_ref, d_mon, dtype, Href, Wref, Hmon, Wmon, Wref, Wmon, kp, kp + N, kp + 2 * N, kp + 3 * N, n, radius,
                        (int32_t *)(d_out + o_offset), (double *)d_out, (double *)(d_out + o_mi), (double *)(d_out + o_shift), (uint8_t *)(d_out + o_status), d_surface};
    {
        c->evs_used[c->ev_cur][ST_MI] = false;
        km_stage_timer t(c, ST_MI);
        if ((rc = kms_search(c, a))) return rc;
    }
    KM_D2H(c, out_peak, a.peak, N * sizeof(double));
    KM_D2H(c, out_peak_mi, a.peak_mi, N * sizeof(double));
    KM_D2H(c, out_shift, a.shift, 2 * N * sizeof(double));
    KM_D2H(c, out_offset, a.offset, 2 * N * sizeof(int32_t));
    KM_D2H(c, out_status, a.status, N);
    if (out_surface) KM_D2H(c, out_surface, d_surface, N * SS * sizeof(double));
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
    double *d_nv = (double *)km_ws(c, WS_MISC1, (size_t)(n_no > 0 ? n_no : 1) * sizeof(double));
    uint8_t *d_keep = (uint8_t *)km_ws(c, WS_MISC2, (size_t)n);
    if (!d_nv || !d_keep) return KM_E_NOMEM;
    const float *src[2] = {x0, y0};
    float *d_xy;
    if ((rc = upload_columns(c, WS_MISC0, src, 2, n, &d_xy))) return rc;
    if (n_no > 0) { const int rch = h2d_now(c, d_nv, no_values, (size_t)n_no * sizeof(double)); if (rch) return rch; }
    if ((rc = kf_dn_keep(c, d_ref, d_mon, dtype, H, W, sref, smon, d_xy, d_xy + n, n, d_nv, n_no, nodata_ref, nodata_mon, d_keep))) return rc;
    KM_D2H(c, keep, d_keep, (size_t)n);
    KM_FLUSH(c);
    for (int i = 0; i < n; i++)
        if (keep[i] > 1) return km_fail(c, KM_E_ARG, "dn_keep: key point %d (%g, %g) lies outside the %dx%d image", i, (double)x0[i], (double)y0[i], W, H);
    return KM_OK;
}

}  // extern "C"
