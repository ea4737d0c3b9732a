// Global align step (karios/matcher/global_align.py): warpPerspective, _sobel_magnitude, findTransformECC(MOTION_HOMOGRAPHY) and
// _refine_with_ecc.  The kernels live in k_align.hip; the small algebra of an ECC iteration (8 x 8 float32 LU inverse, lambda, the
// parameter update) runs here on the host, on the 66 fp64 sums one small copy brings back per iteration.
#include "api_internal.hpp"
#include "k_align.hpp"

#include <math.h>
#include <string.h>

namespace {

// cv::invert(DECOMP_LU) of a 3 x 3 double matrix: cofactors over det3 times 1 / det, zeros when singular
void invert3x3(const double *m, double *t)
{
#define A(r, c) m[(r) * 3 + (c)]
    double d = A(0, 0) * (A(1, 1) * A(2, 2) - A(1, 2) * A(2, 1)) - A(0, 1) * (A(1, 0) * A(2, 2) - A(1, 2) * A(2, 0)) +
               A(0, 2) * (A(1, 0) * A(2, 1) - A(1, 1) * A(2, 0));
    if (d == 0.0) {
        for (int i = 0; i < 9; i++) t[i] = 0.0;
        return;
    }
    d = 1.0 / d;
    t[0] = (A(1, 1) * A(2, 2) - A(1, 2) * A(2, 1)) * d;
    t[1] = (A(0, 2) * A(2, 1) - A(0, 1) * A(2, 2)) * d;
    t[2] = (A(0, 1) * A(1, 2) - A(0, 2) * A(1, 1)) * d;
    t[3] = (A(1, 2) * A(2, 0) - A(1, 0) * A(2, 2)) * d;
    t[4] = (A(0, 0) * A(2, 2) - A(0, 2) * A(2, 0)) * d;
    t[5] = (A(0, 2) * A(1, 0) - A(0, 0) * A(1, 2)) * d;
    t[6] = (A(1, 0) * A(2, 1) - A(1, 1) * A(2, 0)) * d;
    t[7] = (A(0, 1) * A(2, 0) - A(0, 0) * A(2, 1)) * d;
    t[8] = (A(0, 0) * A(1, 1) - A(0, 1) * A(1, 0)) * d;
#undef A
}

// Mat::inv() of a float32 8 x 8 matrix: hal::LU32f on [A | I] (partial pivoting, eps = 10 FLT_EPSILON); zeros when singular
void lu_inv_f32(float a[8][8], float b[8][8])
{
    const int n = 8;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) b[i][j] = i == j ? 1.0f : 0.0f;
    const float eps = 1.1920929e-07f * 10;
    for (int i = 0; i < n; i++) {
        int k = i;
        for (int j = i + 1; j < n; j++)
            if (fabsf(a[j][i]) > fabsf(a[k][i])) k = j;
        if (fabsf(a[k][i]) < eps) {
            for (int r = 0; r < n; r++)
                for (int q = 0; q < n; q++) b[r][q] = 0.0f;
            return;
        }
        if (k != i) {
            for (int j = i; j < n; j++) { const float t = a[i][j]; a[i][j] = a[k][j]; a[k][j] = t; }
            for (int j = 0; j < n; j++) { const float t = b[i][j]; b[i][j] = b[k][j]; b[k][j] = t; }
        }
        const float d = -1.0f / a[i][i];
        for (int j = i + 1; j < n; j++) {
            const float alpha = a[j][i] * d;
            for (int q = i + 1; q < n; q++) a[j][q] = a[j][q] + alpha * a[i][q];
            for (int q = 0; q < n; q++) b[j][q] = b[j][q] + alpha * b[i][q];
        }
    }
    for (int i = n - 1; i >= 0; i--)
        for (int j = 0; j < n; j++) {
            float s = b[i][j];
            for (int q = i + 1; q < n; q++) s = s - a[i][q] * b[q][j];
            b[i][j] = s / a[i][i];
        }
}

// float32 matrix x vector with the products summed in double (GEMM of small float32 matrices)
void matvec_f32(const float A[8][8], const float *v, float *out)
{
    for (int i = 0; i < 8; i++) {
        double acc = 0.0;
        for (int j = 0; j < 8; j++) acc += (double)A[i][j] * (double)v[j];
        out[i] = (float)acc;
    }
}

// One iteration's algebra on the KA_NSUM sums (order: k_align.hip ecc_iter_kernel): rho, then the update of the float32 map.
// Returns false where findTransformECC raises StsNoConv.
bool ecc_step(const double *s, float map[9], double *rho_out, const char **why)
{
    const double N = s[0], SmI = s[1], SmI2 = s[2], SmT = s[3], SmT2 = s[4], SmTI = s[5];
    float H[8][8];
    int q = 6;
    for (int k = 0; k < 8; k++)
        for (int l = k; l < 8; l++) { H[k][l] = H[l][k] = (float)s[q]; q++; }
    const double *SJI = s + 42, *SJm = s + 50, *SJmT = s + 58;
    const double inv_n = N != 0.0 ? 1.0 / N : 0.0;   // meanStdDev: scale = nz ? 1 / nz : 0
    const double mi = SmI * inv_n, mt = SmT * inv_n;
    const double si = sqrt(fmax(SmI2 * inv_n - mi * mi, 0.0)), st = sqrt(fmax(SmT2 * inv_n - mt * mt, 0.0));
    const double tmp_norm = sqrt(N * st * st), img_norm = sqrt(N * si * si);
    const double corr = SmTI - mi * SmT - mt * SmI + N * mt * mi;
    float hinv[8][8];
    lu_inv_f32(H, hinv);
    const double rho = corr / (img_norm * tmp_norm);
    *rho_out = rho;
    if (rho != rho) { *why = "NaN encountered"; return false; }
    double IP[8], TP[8];
    float ip[8], tp[8], iph[8];
    for (int k = 0; k < 8; k++) {
        IP[k] = SJI[k] - mi * SJm[k];     // image projection: ecc.cpp's in-place masked subtract leaves the raw value outside the mask
        TP[k] = SJmT[k] - mt * SJm[k];    // template projection
        ip[k] = (float)IP[k];
        tp[k] = (float)TP[k];
    }
    matvec_f32(hinv, ip, iph);
    double d_ip = 0.0, d_tp = 0.0;
    for (int k = 0; k < 8; k++) d_ip += (double)ip[k] * (double)iph[k];
    for (int k = 0; k < 8; k++) d_tp += (double)tp[k] * (double)iph[k];
    const double lam_n = img_norm * img_norm - d_ip, lam_d = corr - d_tp;
    if (lam_d <= 0.0) { *why = "the correlation is going to be minimized (images uncorrelated or not overlapping)"; return false; }
    const double lam = lam_n / lam_d;
    float ep[8], dp[8];
    for (int k = 0; k < 8; k++) ep[k] = (float)(lam * TP[k] - IP[k]);   // projection of lambda templateZM - imageWarped
    matvec_f32(hinv, ep, dp);
    const int slot[8] = {0, 3, 6, 1, 4, 7, 2, 5};   // update_warping_matrix_ECC, MOTION_HOMOGRAPHY
    for (int k = 0; k < 8; k++) map[slot[k]] = map[slot[k]] + dp[k];
    return true;
}

// findTransformECC's loop on prepared planes: the |rho - last_rho| >= eps check at the top, one more map update after the last rho
int ecc_loop(km_ctx *c, const float *d_t, int hs, int ws, const float4 *d_plane, int hd, int wd, float map[9], int max_iter, double eps,
             double *cc, int *iters)
{
    double *d_part = (double *)km_ws(c, WS_AL_PART, ((size_t)KA_ECC_MAX_BLOCKS + 1) * KA_NSUM * sizeof(double));
    if (!d_part) return KM_E_NOMEM;
    double *d_sums = d_part + (size_t)KA_ECC_MAX_BLOCKS * KA_NSUM;
    double rho = -1.0, last = -eps, s[KA_NSUM];
    int it = 0, rc;
    while (it + 1 <= max_iter && fabs(rho - last) >= eps) {
        it++;
        if ((rc = ka_ecc_sums(c, d_t, hs, ws, d_plane, hd, wd, map, d_part, d_sums))) return rc;
        KM_D2H(c, s, d_sums, sizeof(s));
        KM_FLUSH(c);
        last = rho;
        const char *why = "";
        if (!ecc_step(s, map, &rho, &why)) {
            *cc = rho;
            *iters = it;
            return km_fail(c, KM_E_NO_CONVERGENCE, "find_transform_ecc: iteration %d: %s", it, why);
        }
    }
    *cc = rho;
    *iters = it;
    return KM_OK;
}

// blurred template (float32)
int ecc_prepare_template(km_ctx *c, const void *d_tmpl, int dtype, int hs, int ws, ptrdiff_t st, float **d_t_out)
{
    float *d_tmp = (float *)km_ws(c, WS_AL_TMP, (size_t)hs * ws * sizeof(float));
    float *d_t = (float *)km_ws(c, WS_AL_T, (size_t)hs * ws * sizeof(float));
    if (!d_tmp || !d_t) return KM_E_NOMEM;
    int rc;
    if ((rc = ka_gauss5(c, d_tmpl, dtype, hs, ws, st, d_tmp, d_t))) return rc;
    *d_t_out = d_t;
    return KM_OK;
}

// blurred input, pre-mask and the {image, gx, gy, pre-mask} plane
int ecc_prepare_input(km_ctx *c, const void *d_in, int dtype, int hd, int wd, ptrdiff_t si, const uint8_t *d_mask, ptrdiff_t sm,
                      float4 **d_plane_out)
{
    const size_t ni = (size_t)hd * wd;
    float *d_tmp = (float *)km_ws(c, WS_AL_TMP, ni * sizeof(float));
    float *d_i = (float *)km_ws(c, WS_AL_I, ni * sizeof(float));
    float4 *d_plane = (float4 *)km_ws(c, WS_AL_PLANE, ni * sizeof(float4));
    float *d_pm = d_mask ? (float *)km_ws(c, WS_AL_PM, ni * sizeof(float)) : nullptr;
    if (!d_tmp || !d_i || !d_plane || (d_mask && !d_pm)) return KM_E_NOMEM;
    int rc;
    if ((rc = ka_gauss5(c, d_in, dtype, hd, wd, si, d_tmp, d_i))) return rc;
    if (d_mask && (rc = ka_gauss5(c, d_mask, KA_MASK, hd, wd, sm, d_tmp, d_pm))) return rc;
    if ((rc = ka_ecc_plane(c, d_i, d_pm, hd, wd, d_plane))) return rc;
    *d_plane_out = d_plane;
    return KM_OK;
}

int ecc_prepare(km_ctx *c, const void *d_tmpl, const void *d_in, int dtype, int hs, int ws, ptrdiff_t st, int hd, int wd, ptrdiff_t si,
                const uint8_t *d_mask, ptrdiff_t sm, float **d_t_out, float4 **d_plane_out)
{
    int rc;
    if ((rc = ecc_prepare_template(c, d_tmpl, dtype, hs, ws, st, d_t_out))) return rc;
    return ecc_prepare_input(c, d_in, dtype, hd, wd, si, d_mask, sm, d_plane_out);
}

int warp_args(km_ctx *c, int dtype, int dH, int dW, int interpolation, const double *M)
{
    if (dtype != KM_U8 && dtype != KM_F32) return km_fail(c, KM_E_UNSUPPORTED, "warp_perspective: dtype %d (uint8 and float32 only)", dtype);
    if (dH <= 0 || dW <= 0 || !M) return km_fail(c, KM_E_ARG, "warp_perspective: empty destination or null matrix");
    if (interpolation != 0 && interpolation != 1) return km_fail(c, KM_E_UNSUPPORTED, "warp_perspective: interpolation %d", interpolation);
    return KM_OK;
}

int warp_dev(km_ctx *c, const void *d_src, int dtype, int sH, int sW, ptrdiff_t ss, void *d_dst, int dH, int dW, ptrdiff_t ds,
             int interpolation, int inverse, double border, const double M[9])
{
    double Mi[9];
    if (inverse) memcpy(Mi, M, sizeof(Mi));
    else invert3x3(M, Mi);
    return ka_warp(c, d_src, dtype, sH, sW, ss, d_dst, dH, dW, ds, interpolation, Mi, border);
}

int ecc_args(km_ctx *c, int dtype, int hs, int ws, int hd, int wd, int max_iter, int gauss, const float *map, const double *cc, const int *iters)
{
    if (gauss != 5) return km_fail(c, KM_E_UNSUPPORTED, "find_transform_ecc: gaussFiltSize %d (5 only)", gauss);
    if (dtype != KM_U8 && dtype != KM_F32) return km_fail(c, KM_E_UNSUPPORTED, "find_transform_ecc: dtype %d (uint8 and float32 only)", dtype);
    if (!map || !cc || !iters || max_iter < 0 || hs <= 0 || ws <= 0 || hd <= 0 || wd <= 0)
        return km_fail(c, KM_E_ARG, "find_transform_ecc: bad arguments");
    return KM_OK;
}

int refine_candidates(km_ctx *c, const uint8_t *d_mon, int hm, int wm, ptrdiff_t smon, const uint8_t *d_ref, int hr, int wr,
                                 ptrdiff_t sref, int n, const double *inits, int max_iter, double eps, double *final_out, float *residual_out,
                                 double *cc_out, int *iters_out, int64_t *valid_out, int *status_out)
{
    int rc;
    if (n < 0 || (n && (!inits || !final_out || !residual_out || !cc_out || !iters_out || !valid_out || !status_out)) || max_iter < 0)
        return km_fail(c, KM_E_ARG, "refine_ecc_candidates: bad arguments");
    const size_t nr = (size_t)hr * wr;
    uint8_t *d_warp = (uint8_t *)km_ws(c, WS_AL_WARP, nr);
    float *d_tsob = (float *)km_ws(c, WS_AL_TSOB, nr * sizeof(float));
    float *d_sob = (float *)km_ws(c, WS_AL_SOB, nr * sizeof(float));
    unsigned long long *d_scal = (unsigned long long *)km_ws(c, WS_AL_SCAL, 64);
    if (!d_warp || !d_tsob || !d_sob || !d_scal) return KM_E_NOMEM;
    float *d_t = nullptr;   // the template's Sobel magnitude and blur: once for all candidates
    for (int k = 0; k < n; k++) {
        const double *init = inits + 9 * (size_t)k;
        double M[9], Mi[9];
        for (int i = 0; i < 9; i++) M[i] = (double)(float)init[i];   // warpPerspective(mon, init.astype(np.float32), ...)
        invert3x3(M, Mi);
        if ((rc = ka_warp(c, d_mon, KM_U8, hm, wm, smon, d_warp, hr, wr, wr, 1, Mi, 0.0))) return rc;
        if ((rc = ka_count_nonzero(c, d_warp, nr, d_scal))) return rc;
        unsigned long long valid = 0;
        KM_D2H(c, &valid, d_scal, sizeof(valid));
        KM_FLUSH(c);
        valid_out[k] = (int64_t)valid;
        cc_out[k] = NAN;
        iters_out[k] = 0;
        for (int i = 0; i < 9; i++) { final_out[9 * k + i] = NAN; residual_out[9 * k + i] = NAN; }
        if (valid < 1000) { status_out[k] = KM_ECC_SKIPPED; continue; }
        if (!d_t) {
            if ((rc = ka_sobel_magnitude(c, d_ref, hr, wr, sref, d_tsob, (unsigned *)(d_scal + 1))) ||
                (rc = ecc_prepare_template(c, d_tsob, KM_F32, hr, wr, wr, &d_t)))
                return rc;
        }
        if ((rc = ka_sobel_magnitude(c, d_warp, hr, wr, wr, d_sob, (unsigned *)(d_scal + 1)))) return rc;
        float4 *d_plane;
        if ((rc = ecc_prepare_input(c, d_sob, KM_F32, hr, wr, wr, d_warp, wr, &d_plane))) return rc;
        float map[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        double cc = NAN;
        int it = 0;
        rc = ecc_loop(c, d_t, hr, wr, d_plane, hr, wr, map, max_iter, eps, &cc, &it);
        if (rc == KM_E_NO_CONVERGENCE) { status_out[k] = KM_ECC_NO_CONVERGENCE; continue; }
        if (rc) return rc;
        status_out[k] = KM_ECC_CONVERGED;
        cc_out[k] = cc;
        iters_out[k] = it;
        for (int i = 0; i < 9; i++) residual_out[9 * k + i] = map[i];
        for (int r = 0; r < 3; r++)   // residual.astype(float64) @ init.astype(float64)
            for (int q = 0; q < 3; q++) {
                double s = 0.0;
                for (int j = 0; j < 3; j++) s += (double)map[3 * r + j] * init[3 * j + q];
                final_out[9 * k + 3 * r + q] = s;
            }
    }
    c->err.clear();
    return KM_OK;
}

}  // namespace

extern "C" {

int km_warp_perspective_dev(km_ctx *c, const void *d_src, int dtype, int sH, int sW, ptrdiff_t ss, void *d_dst, int dH, int dW, ptrdiff_t ds,
                            int interpolation, int inverse, double border, const double M[9])
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, d_src, sH, sW, ss, "warp_perspective")) ||
        (rc = check_image(c, d_dst, dH, dW, ds, "warp_perspective")) || (rc = warp_args(c, dtype, dH, dW, interpolation, M)))
        return rc;
    return warp_dev(c, d_src, dtype, sH, sW, ss, d_dst, dH, dW, ds, interpolation, inverse, border, M);
}

int km_warp_perspective(km_ctx *c, const void *src, int dtype, int sH, int sW, ptrdiff_t ss, void *dst, int dH, int dW, int interpolation,
                        int inverse, double border, const double M[9])
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, src, sH, sW, ss, "warp_perspective")) ||
        (rc = check_image(c, dst, dH, dW, dW, "warp_perspective")) || (rc = warp_args(c, dtype, dH, dW, interpolation, M)))
        return rc;
    const size_t es = km_dtype_size(dtype);
    void *d_src, *d_dst = km_ws(c, WS_AL_OUT, (size_t)dH * dW * es);
    if (!d_dst) return KM_E_NOMEM;
    if ((rc = upload_image(c, WS_RAW_A, src, es, sH, sW, ss, &d_src))) return rc;
    if ((rc = warp_dev(c, d_src, dtype, sH, sW, sW, d_dst, dH, dW, dW, interpolation, inverse, border, M))) return rc;
    KM_D2H(c, dst, d_dst, (size_t)dH * dW * es);
    KM_FLUSH(c);
    return KM_OK;
}

int km_sobel_magnitude_dev(km_ctx *c, const uint8_t *d_img, int H, int W, ptrdiff_t stride, float *d_out)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, d_img, H, W, stride, "sobel_magnitude"))) return rc;
    if (!d_out) return km_fail(c, KM_E_ARG, "sobel_magnitude: null output");
    unsigned *d_max = (unsigned *)km_ws(c, WS_AL_SCAL, 64);
    if (!d_max) return KM_E_NOMEM;
    return ka_sobel_magnitude(c, d_img, H, W, stride, d_out, d_max);
}

int km_sobel_magnitude(km_ctx *c, const uint8_t *img, int H, int W, ptrdiff_t stride, float *out)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, img, H, W, stride, "sobel_magnitude"))) return rc;
    if (!out) return km_fail(c, KM_E_ARG, "sobel_magnitude: null output");
    void *d_img;
    float *d_out = (float *)km_ws(c, WS_AL_OUT, (size_t)H * W * sizeof(float));
    unsigned *d_max = (unsigned *)km_ws(c, WS_AL_SCAL, 64);
    if (!d_out || !d_max) return KM_E_NOMEM;
    if ((rc = upload_image(c, WS_RAW_A, img, 1, H, W, stride, &d_img))) return rc;
    if ((rc = ka_sobel_magnitude(c, (const uint8_t *)d_img, H, W, W, d_out, d_max))) return rc;
    KM_D2H(c, out, d_out, (size_t)H * W * sizeof(float));
    KM_FLUSH(c);
    return KM_OK;
}

int km_find_transform_ecc_dev(km_ctx *c, const void *d_tmpl, const void *d_in, int dtype, int hs, int ws, ptrdiff_t st, int hd, int wd,
                              ptrdiff_t si, const uint8_t *d_mask, ptrdiff_t sm, float map[9], int max_iter, double eps, int gauss,
                              double *cc, int *iters)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = ecc_args(c, dtype, hs, ws, hd, wd, max_iter, gauss, map, cc, iters)) ||
        (rc = check_image(c, d_tmpl, hs, ws, st, "find_transform_ecc")) || (rc = check_image(c, d_in, hd, wd, si, "find_transform_ecc")) ||
        (d_mask && (rc = check_image(c, d_mask, hd, wd, sm, "find_transform_ecc mask"))))
        return rc;
    float *d_t;
    float4 *d_plane;
    if ((rc = ecc_prepare(c, d_tmpl, d_in, dtype, hs, ws, st, hd, wd, si, d_mask, sm, &d_t, &d_plane))) return rc;
    return ecc_loop(c, d_t, hs, ws, d_plane, hd, wd, map, max_iter, eps, cc, iters);
}

int km_find_transform_ecc(km_ctx *c, const void *tmpl, const void *in, int dtype, int hs, int ws, ptrdiff_t st, int hd, int wd, ptrdiff_t si,
                          const uint8_t *mask, ptrdiff_t sm, float map[9], int max_iter, double eps, int gauss, double *cc, int *iters)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = ecc_args(c, dtype, hs, ws, hd, wd, max_iter, gauss, map, cc, iters)) ||
        (rc = check_image(c, tmpl, hs, ws, st, "find_transform_ecc")) || (rc = check_image(c, in, hd, wd, si, "find_transform_ecc")) ||
        (mask && (rc = check_image(c, mask, hd, wd, sm, "find_transform_ecc mask"))))
        return rc;
    const size_t es = km_dtype_size(dtype);
    void *d_t_raw, *d_i_raw, *d_m = nullptr;
    if ((rc = upload_image(c, WS_RAW_A, tmpl, es, hs, ws, st, &d_t_raw)) || (rc = upload_image(c, WS_RAW_B, in, es, hd, wd, si, &d_i_raw)) ||
        (mask && (rc = upload_image(c, WS_MASK_IN, mask, 1, hd, wd, sm, &d_m))))
        return rc;
    float *d_t;
    float4 *d_plane;
    if ((rc = ecc_prepare(c, d_t_raw, d_i_raw, dtype, hs, ws, ws, hd, wd, wd, (const uint8_t *)d_m, wd, &d_t, &d_plane))) return rc;
    return ecc_loop(c, d_t, hs, ws, d_plane, hd, wd, map, max_iter, eps, cc, iters);
}

// For tests: what km_find_transform_ecc's first iteration at `map` works on.  The same ecc_prepare, one ka_ecc_sums, three copies out.
int km_ecc_stages(km_ctx *c, const void *tmpl, const void *in, int dtype, int hs, int ws, ptrdiff_t st, int hd, int wd, ptrdiff_t si,
                  const uint8_t *mask, ptrdiff_t sm, const float map[9], float *t_blur, float *plane, double *sums)
{
    int rc, no_iters = 0;
    double no_cc = 0.0;
    if ((rc = begin_call(c)) || (rc = ecc_args(c, dtype, hs, ws, hd, wd, 0, 5, map, &no_cc, &no_iters)) ||
        (rc = check_image(c, tmpl, hs, ws, st, "ecc_stages")) || (rc = check_image(c, in, hd, wd, si, "ecc_stages")) ||
        (mask && (rc = check_image(c, mask, hd, wd, sm, "ecc_stages mask"))))
        return rc;
    if (!t_blur || !plane || !sums) return km_fail(c, KM_E_ARG, "ecc_stages: null output");
    const size_t es = km_dtype_size(dtype);
    void *d_t_raw, *d_i_raw, *d_m = nullptr;
    if ((rc = upload_image(c, WS_RAW_A, tmpl, es, hs, ws, st, &d_t_raw)) || (rc = upload_image(c, WS_RAW_B, in, es, hd, wd, si, &d_i_raw)) ||
        (mask && (rc = upload_image(c, WS_MASK_IN, mask, 1, hd, wd, sm, &d_m))))
        return rc;
    float *d_t;
    float4 *d_plane;
    if ((rc = ecc_prepare(c, d_t_raw, d_i_raw, dtype, hs, ws, ws, hd, wd, wd, (const uint8_t *)d_m, wd, &d_t, &d_plane))) return rc;
    double *d_part = (double *)km_ws(c, WS_AL_PART, ((size_t)KA_ECC_MAX_BLOCKS + 1) * KA_NSUM * sizeof(double));
    if (!d_part) return KM_E_NOMEM;
    double *d_sums = d_part + (size_t)KA_ECC_MAX_BLOCKS * KA_NSUM;
    if ((rc = ka_ecc_sums(c, d_t, hs, ws, d_plane, hd, wd, map, d_part, d_sums))) return rc;
    KM_D2H(c, t_blur, d_t, (size_t)hs * ws * sizeof(float));
    KM_D2H(c, plane, d_plane, (size_t)hd * wd * sizeof(float4));
    KM_D2H(c, sums, d_sums, KA_NSUM * sizeof(double));
    KM_FLUSH(c);
    return KM_OK;
}

int km_refine_ecc_candidates_dev(km_ctx *c, const uint8_t *d_mon, int hm, int wm, ptrdiff_t smon, const uint8_t *d_ref, int hr, int wr,
                                 ptrdiff_t sref, int n, const double *inits, int max_iter, double eps, double *final_out, float *residual_out,
                                 double *cc_out, int *iters_out, int64_t *valid_out, int *status_out)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, d_mon, hm, wm, smon, "refine_ecc_candidates")) ||
        (rc = check_image(c, d_ref, hr, wr, sref, "refine_ecc_candidates")))
        return rc;
    return refine_candidates(c, d_mon, hm, wm, smon, d_ref, hr, wr, sref, n, inits, max_iter, eps, final_out, residual_out, cc_out,
                             iters_out, valid_out, status_out);
}

int km_refine_ecc_candidates(km_ctx *c, const uint8_t *mon, int hm, int wm, ptrdiff_t smon, const uint8_t *ref, int hr, int wr, ptrdiff_t sref,
                             int n, const double *inits, int max_iter, double eps, double *final_out, float *residual_out, double *cc_out,
                             int *iters_out, int64_t *valid_out, int *status_out)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, mon, hm, wm, smon, "refine_ecc_candidates")) ||
        (rc = check_image(c, ref, hr, wr, sref, "refine_ecc_candidates")))
        return rc;
    void *d_mon, *d_ref;
    if ((rc = upload_image(c, WS_RAW_B, mon, 1, hm, wm, smon, &d_mon)) || (rc = upload_image(c, WS_RAW_A, ref, 1, hr, wr, sref, &d_ref))) return rc;
    return refine_candidates(c, (const uint8_t *)d_mon, hm, wm, wm, (const uint8_t *)d_ref, hr, wr, wr, n, inits, max_iter, eps, final_out,
                             residual_out, cc_out, iters_out, valid_out, status_out);
}

}  // extern "C"
