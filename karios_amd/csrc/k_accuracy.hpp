// k_accuracy.hip: the device half of KariosAPI.analyze_accuracy (karios/api/core.py:268-328): the valid-pixel count of the monitored
// raster under the mask, and GeometricStat's sample, statistics and CE order statistics (accuracy_statistics.py:82-238).  The
// arithmetic is accuracy_math.hpp's; tests/accuracy_restatement.py is the definition.
// A compiler that is not hipcc (the host sanitizer build of the API files, the stand-alone program of tests/test_accuracy_host.py)
// gets the launchers defined here, as plain loops over the same header: device memory is host memory there, `c` is not touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/karios_hip.h"
#include "accuracy_math.hpp"

// device-side state of one statistics call
struct ka_state {
    int n;                 // rows of the sample
    int n_nan;             // ... with a NaN in dx or dy
    float sum[3];          // x, y, c: the float32 sum, then the sum of the squared deviations
    float mean[3];
    float std[3];
    int pad;
};
struct ka_percents {
    int n;
    double q[KM_ACC_MAX_PERCENTS];
};
AC_HD static inline int ka_nblocks(int n) { return (n + ac::BLOCK - 1) / ac::BLOCK; }

#if defined(__HIPCC__)
// pixels that are non-zero (float32: by their bits) and whose mask byte, if a mask is given, is non-zero -> *d_count
int ka_count_valid(km_ctx *c, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *d_mask, ptrdiff_t mask_stride,
                   unsigned long long *d_count);
// rows with (double)score > thr, in row order -> d_cols = x[n_max] | y[n_max] | c[n_max] (y negated with carto), st->n, st->n_nan
int ka_compact(km_ctx *c, const float *d_dx, const float *d_dy, const float *d_score, int n_max, double thr, int carto, float *d_cols, ka_state *st);
// sums of the 8192-blocks of the three columns (dev_sq: of (a - st->mean)^2) -> d_bsum[3][ka_nblocks(n_max)]
int ka_block_sums(km_ctx *c, const float *d_cols, int n_max, const ka_state *st, int dev_sq, float *d_bsum);
// block sums -> st->sum, and st->mean (dev_sq 0) or st->std (dev_sq 1)
int ka_finish(km_ctx *c, const float *d_bsum, int n_max, ka_state *st, int dev_sq);
// the four columns (x, y, c, radial) in ascending order; minimum, maximum, median and the two order statistics of every percent -> d_out
int ka_order(km_ctx *c, const float *d_cols, int n_max, float factor, ka_percents pc, const ka_state *st, km_accuracy_result *d_out);
#else
#include <algorithm>
#include <vector>

template <typename T> static inline bool ka_nonzero(T v) { return v != 0; }
template <> inline bool ka_nonzero<float>(float v) { return ac::nonzero_f32_bits(ac::f32_bits(v)); }
template <typename T>
static inline unsigned long long ka_count_rows(const T *img, int H, int W, ptrdiff_t stride, const uint8_t *mask, ptrdiff_t ms)
{
    unsigned long long n = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) n += ka_nonzero(img[(ptrdiff_t)y * stride + x]) && (!mask || mask[(ptrdiff_t)y * ms + x]) ? 1u : 0u;
    return n;
}
static inline int ka_count_valid(km_ctx *, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *d_mask,
                                 ptrdiff_t mask_stride, unsigned long long *d_count)
{
    switch (dtype) {
    case KM_U8: *d_count = ka_count_rows((const uint8_t *)d_img, H, W, stride, d_mask, mask_stride); return KM_OK;
    case KM_U16: *d_count = ka_count_rows((const uint16_t *)d_img, H, W, stride, d_mask, mask_stride); return KM_OK;
    case KM_I16: *d_count = ka_count_rows((const int16_t *)d_img, H, W, stride, d_mask, mask_stride); return KM_OK;
    case KM_F32: *d_count = ka_count_rows((const float *)d_img, H, W, stride, d_mask, mask_stride); return KM_OK;
    default: return KM_E_ARG;
    }
}
static inline int ka_compact(km_ctx *, const float *d_dx, const float *d_dy, const float *d_score, int n_max, double thr, int carto, float *d_cols,
                             ka_state *st)
{
    int n = 0, nan = 0;
    for (int i = 0; i < n_max; i++) {
        if (!ac::above(d_score[i], thr)) continue;
        d_cols[n] = d_dx[i];
        d_cols[(size_t)n_max + n] = carto ? -d_dy[i] : d_dy[i];
        d_cols[2 * (size_t)n_max + n] = d_score[i];
        nan += ac::is_nan(d_dx[i]) || ac::is_nan(d_dy[i]) ? 1 : 0;
        n++;
    }
    *st = ka_state();
    st->n = n; st->n_nan = nan;
    return KM_OK;
}
static inline int ka_block_sums(km_ctx *, const float *d_cols, int n_max, const ka_state *st, int dev_sq, float *d_bsum)
{
    const int nb = ka_nblocks(n_max);
    std::vector<float> tmp(ac::BLOCK);
    for (int col = 0; col < 3; col++)
        for (int b = 0; b < ka_nblocks(st->n); b++) {
            const int len = std::min<int>(ac::BLOCK, st->n - b * ac::BLOCK);
            const float *a = d_cols + (size_t)col * n_max + (size_t)b * ac::BLOCK;
            for (int i = 0; i < len; i++) tmp[i] = dev_sq ? ac::dev_sq(a[i], st->mean[col]) : a[i];
            d_bsum[(size_t)col * nb + b] = ac::block_sum(tmp.data(), len);
        }
    return KM_OK;
}
static inline int ka_finish(km_ctx *, const float *d_bsum, int n_max, ka_state *st, int dev_sq)
{
    const int nb = ka_nblocks(n_max);
    for (int col = 0; col < 3; col++) {
        st->sum[col] = ac::fold_blocks(d_bsum + (size_t)col * nb, ka_nblocks(st->n));
        if (dev_sq) st->std[col] = ac::std_of(st->sum[col], st->n);
        else st->mean[col] = ac::mean_of(st->sum[col], st->n);
    }
    return KM_OK;
}
static inline int ka_order(km_ctx *, const float *d_cols, int n_max, float factor, ka_percents pc, const ka_state *st, km_accuracy_result *d_out)
{
    const int n = st->n;
    km_accuracy_result r = km_accuracy_result();
    r.sample = n; r.n_nan = st->n_nan;
    const float nanv = ac::bits_f32(0x7fc00000u);
    for (int i = 0; i < 15; i++) r.stats[i] = nanv;
    for (int i = 0; i < 2 * KM_ACC_MAX_PERCENTS; i++) r.order[i] = nanv;
    std::vector<uint32_t> key((size_t)(n > 0 ? n : 1));
    for (int col = 0; col < 4 && n > 0; col++) {
        for (int i = 0; i < n; i++)
            key[i] = ac::order_key(col < 3 ? d_cols[(size_t)col * n_max + i] : ac::radial(d_cols[i], d_cols[(size_t)n_max + i], factor));
        std::sort(key.begin(), key.begin() + n);
        if (col < 3) {
            float *s = r.stats + 5 * col;
            s[0] = ac::order_value(key[0]);
            s[1] = ac::order_value(key[n - 1]);
            s[2] = (n & 1) ? ac::order_value(key[n / 2]) : ac::median_even(ac::order_value(key[n / 2 - 1]), ac::order_value(key[n / 2]));
            s[3] = st->mean[col];
            s[4] = st->std[col];
        } else {
            for (int k = 0; k < pc.n; k++) {
                long long lo, hi;
                if (!ac::ce_ranks(pc.q[k], n, lo, hi)) continue;
                r.order[2 * k] = ac::order_value(key[lo]);
                r.order[2 * k + 1] = ac::order_value(key[hi]);
            }
        }
    }
    *d_out = r;
    return KM_OK;
}
#endif
