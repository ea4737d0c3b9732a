// k_report.hip: the numbers of the report step on resident data - the display range of OverviewPlot._plot_image
// (karios/report/overview_plot.py:134-194) and the mean profiles of karios/report/commons.py:49-71.  The arithmetic is
// report_math.hpp's; tests/report_restatement.py is the definition.
// A compiler that is not hipcc (the host sanitizer build of the API files, the stand-alone program of tests/test_report_host.py) gets
// the launchers defined here, as plain loops over the same header: device memory is host memory there, `c` is not touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/karios_hip.h"
#include "report_math.hpp"

#define KR_MAX_Q 4   // quantiles of one selection (KP_MAX_Q of the radix select; api_prep.hip runs longer lists in groups)

// ---- display range: device-side results of one selection
struct kr_range_result {
    long long n_valid, n_invalid;
    double vi[KR_MAX_Q], v0[KR_MAX_Q], v1[KR_MAX_Q];   // as km_order_statistics gives them; untouched when n_valid is 0
    double raster_min, raster_max;                     // of every pixel that is not NaN (a zero as +0.0); NaN when there is none
};
// one more value the pixels are compared with: a DN value or the no-data value as a pixel of the raster's type (what no pixel can
// equal - out of the type's range, not an integer, NaN - is left out).  t.n < rp::MAX_TESTS
static inline void kr_add_test(rp::tests &t, int dtype, double v)
{
    bool ok;
    if (dtype == KM_F32) ok = rp::as_float_pixel(v, t.f[t.n]);
    else ok = rp::as_integer_pixel(v, dtype == KM_I16 ? -32768.0 : 0.0, dtype == KM_U8 ? 255.0 : dtype == KM_U16 ? 65535.0 : 32767.0, t.i[t.n]);
    t.n += ok;
}
static inline rp::tests kr_no_tests()
{
    rp::tests t;
    t.n = 0;
    for (int k = 0; k < rp::MAX_TESTS; k++) t.i[k] = 0;
    return t;
}
size_t kr_range_ws_bytes();   // the select's device state
// the pixels a predicate keeps - finite, not zero, mask byte (if any) not zero, not among t's values - through the three-pass radix
// select; n_invalid, the minimum and the maximum out of its first pass.  n_q <= KR_MAX_Q
int kr_display_range(km_ctx *c, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, const uint8_t *d_mask, ptrdiff_t ms, const rp::tests &t,
                     int n_q, const double *q, void *d_ws, kr_range_result *d_res);

// ---- mean profiles: one profile of n rows; outputs of capacity n
struct kr_profile {
    const float *values, *positions;
    int bin;
    float *key;
    int32_t *position, *count;
    float *mean, *std;
};
struct kr_profile_ws {
    unsigned long long *keys_a, *keys_b;   // n each (keys_b holds the gathered values and the group heads after the sort)
    unsigned *flags;                       // n
};
enum { KR_GROUPS = 0, KR_OUT_OF_RANGE = 1, KR_KEPT = 2, KR_COUNTS = 4 };
// d_counts[KR_COUNTS]: groups, groups whose position int32 cannot hold, rows with a key
int kr_mean_profile(km_ctx *c, const kr_profile &p, int n, const kr_profile_ws &ws, int32_t *d_counts);

#if !defined(__HIPCC__)
#include <algorithm>
#include <vector>

inline size_t kr_range_ws_bytes() { return 16; }

template <typename T>
static inline void kr_range_host(const T *src, int H, int W, ptrdiff_t ss, const uint8_t *mask, ptrdiff_t ms, const rp::tests &t, int n_q, const double *q,
                                 kr_range_result *res)
{
    std::vector<uint32_t> keys;
    long long n_invalid = 0;
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const T raw = src[(ptrdiff_t)y * ss + x];
            const bool invalid = (mask && mask[(ptrdiff_t)y * ms + x] == 0) || rp::listed<T>(raw, t);
            n_invalid += invalid;
            if (!rp::is_nan<T>(raw)) {
                const uint32_t k = rp::order_key((float)raw);
                lo = k < lo ? k : lo; hi = k > hi ? k : hi;
            }
            if (!invalid && rp::countable<T>(raw)) keys.push_back(rp::order_key((float)raw));
        }
    std::sort(keys.begin(), keys.end());
    const unsigned long long n = keys.size();
    res->n_valid = (long long)n; res->n_invalid = n_invalid;
    const float mn = rp::key_value(lo), mx = rp::key_value(hi);
    res->raster_min = lo > hi ? (double)NAN : mn == 0.0f ? 0.0 : (double)mn;
    res->raster_max = lo > hi ? (double)NAN : mx == 0.0f ? 0.0 : (double)mx;
    for (int j = 0; j < n_q && n > 0; j++) {
        const double vi = sizeof(T) == 4 ? (double)((float)(n - 1) * (float)q[j]) : (double)(n - 1) * q[j];   // float32: numpy's float32 index
        double f = floor(vi);
        f = f < 0.0 ? 0.0 : f;
        unsigned long long r0 = (unsigned long long)f;
        if (r0 > n - 1) r0 = n - 1;
        const unsigned long long r1 = r0 + 1 < n ? r0 + 1 : n - 1;
        res->vi[j] = vi; res->v0[j] = (double)rp::key_value(keys[r0]); res->v1[j] = (double)rp::key_value(keys[r1]);
    }
}

inline int kr_display_range(km_ctx *, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, const uint8_t *d_mask, ptrdiff_t ms, const rp::tests &t,
                            int n_q, const double *q, void *, kr_range_result *d_res)
{
    switch (dtype) {
    case KM_U8: kr_range_host<uint8_t>((const uint8_t *)d_src, H, W, ss, d_mask, ms, t, n_q, q, d_res); return KM_OK;
    case KM_U16: kr_range_host<uint16_t>((const uint16_t *)d_src, H, W, ss, d_mask, ms, t, n_q, q, d_res); return KM_OK;
    case KM_I16: kr_range_host<int16_t>((const int16_t *)d_src, H, W, ss, d_mask, ms, t, n_q, q, d_res); return KM_OK;
    case KM_F32: kr_range_host<float>((const float *)d_src, H, W, ss, d_mask, ms, t, n_q, q, d_res); return KM_OK;
    default: return KM_E_ARG;
    }
}

inline int kr_mean_profile(km_ctx *, const kr_profile &p, int n, const kr_profile_ws &ws, int32_t *d_counts)
{
    const float bin = (float)p.bin;
    int kept = 0;
    for (int i = 0; i < n; i++) {
        const uint32_t k = rp::group_key(p.positions[i], bin);
        if (k != rp::DROPPED) ws.keys_a[kept++] = ((unsigned long long)k << 32) | (uint32_t)i;
    }
    std::sort(ws.keys_a, ws.keys_a + kept);
    int groups = 0, out_of_range = 0;
    for (int at = 0; at < kept;) {
        const uint32_t k = (uint32_t)(ws.keys_a[at] >> 32);
        rp::accum a = rp::accum_zero();
        for (; at < kept && (uint32_t)(ws.keys_a[at] >> 32) == k; at++) rp::accum_add(a, p.values[(uint32_t)ws.keys_a[at]]);
        const float key = rp::key_value(k);
        p.key[groups] = key;
        out_of_range += !rp::group_position(key, p.bin, p.position[groups]);
        p.count[groups] = a.n; p.mean[groups] = rp::accum_mean(a); p.std[groups] = rp::accum_std(a);
        groups++;
    }
    d_counts[KR_GROUPS] = groups; d_counts[KR_OUT_OF_RANGE] = out_of_range; d_counts[KR_KEPT] = kept; d_counts[3] = 0;
    return KM_OK;
}
#endif
