// k_mi_search.hip: the mutual-information search around each key point - the (2R+1)^2 surface of MutualInfoService._mutual_info
// (karios/matcher/mutual_info_service.py:32-63) on the 57 x 57 chips at the offsets around the centre _compute_mutual_info scores
// (:99-130), its peak, the peak's sub-pixel position, and ZNCCService._mutual_information (zncc_service.py:129-151) at the peak.  The
// reference's call graph has no such search; its two formulas and np.histogram2d define every value.  The arithmetic is
// mi_search_math.hpp's; tests/mi_search_restatement.py is the definition.
// A compiler that is not hipcc (the host sanitizer build of the API files, the stand-alone program of tests/test_mi_search_host.py) gets
// the launcher defined here, as plain loops over the same header: device memory is host memory there, `c` is not touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/karios_hip.h"
#include "mi_search_math.hpp"

struct kms_args {
    const void *ref, *mon;
    int dtype;                         // KM_U8 / KM_U16 / KM_I16 / KM_F32, the same for both rasters
    int Href, Wref, Hmon, Wmon;
    ptrdiff_t sref, smon;              // row strides in pixels
    const float *x0, *y0, *dx, *dy;
    int n, radius;                     // 0 < n <= zs::MAX_ROWS, 1 <= radius <= zs::MAX_RADIUS
    int32_t *offset;                   // n x 2
    double *peak;                      // n: Studholme's NMI at the peak
    double *peak_mi;                   // n: the mi_score formula at the same offset
    double *shift;                     // n x 2
    uint8_t *status;                   // n
    double *surface;                   // nullptr, or n x S x S (Studholme)
};

// every output of every row is written exactly once; KM_E_ARG: a pixel type the search does not read
int kms_search(km_ctx *c, const kms_args &a);

#if !defined(__HIPCC__)
#include <vector>

namespace ms {
static const int64_t host_table[TABLE] = {
#include "mi_clogc_q36.inc"
};
}

// the bins of one chip (first pixel p, row stride s) -> b[NPX]; false: a non-finite float32 sample
template <typename T>
inline bool kms_chip_bins(const T *p, ptrdiff_t s, int dtype, uint8_t *b)
{
    if (dtype == KM_F32) {
        double lo = (double)p[0], hi = lo;
        for (int r = 0; r < ms::CHIP; r++)
            for (int cx = 0; cx < ms::CHIP; cx++) {
                const double v = (double)p[r * s + cx];
                if (!(fabs(v) <= 3.5e38)) return false;         // NaN or an infinity (every finite float32 is below)
                lo = v < lo ? v : lo; hi = v > hi ? v : hi;
            }
        const ms::float_rule rule = ms::float_bins(lo, hi);
        double edges[ms::BINS + 1];
        for (int i = 0; i <= ms::BINS; i++) edges[i] = ms::float_edge(i, rule);
        for (int r = 0; r < ms::CHIP; r++)
            for (int cx = 0; cx < ms::CHIP; cx++) b[r * ms::CHIP + cx] = (uint8_t)ms::float_bin((double)p[r * s + cx], rule, edges);
        return true;
    }
    const int bias = dtype == KM_I16 ? 32768 : 0;             // int16 biased by 2^15: the bias cancels in v - lo
    unsigned lo = 65535u, hi = 0u;
    for (int r = 0; r < ms::CHIP; r++)
        for (int cx = 0; cx < ms::CHIP; cx++) {
            const unsigned v = (unsigned)((int)p[r * s + cx] + bias);
            lo = v < lo ? v : lo; hi = v > hi ? v : hi;
        }
    const ms::int_rule rule = ms::int_bins(lo, hi);
    for (int r = 0; r < ms::CHIP; r++)
        for (int cx = 0; cx < ms::CHIP; cx++) b[r * ms::CHIP + cx] = (uint8_t)ms::int_bin((unsigned)((int)p[r * s + cx] + bias), rule);
    return true;
}

template <typename T>
inline void kms_search_host(const kms_args &a)
{
    const int R = a.radius, S = 2 * R + 1;
    const T *ref = (const T *)a.ref, *mon = (const T *)a.mon;
    const int64_t *tab = ms::host_table, L = tab[ms::NPX];
    std::vector<double> z((size_t)S * S), zmi((size_t)S * S);
    std::vector<uint8_t> b1(ms::NPX), b2(ms::NPX);
    std::vector<int> hist(ms::CELLS), marg(ms::BINS);
    for (int k = 0; k < a.n; k++) {
        int X0, Y0, X1, Y1;
        double *zk = a.surface ? a.surface + (size_t)k * S * S : z.data();
        if (!zs::centres(a.x0[k], a.y0[k], a.dx[k], a.dy[k], a.Href, a.Wref, a.Hmon, a.Wmon, X0, Y0, X1, Y1)) {
            for (int i = 0; i < S * S; i++) zk[i] = zs::quiet_nan();
            ms::skipped(a.offset + 2 * k, a.peak + k, a.peak_mi + k, a.shift + 2 * k, a.status + k);
            continue;
        }
        // the reference chip: its bins and the sum over its marginal, once per row
        const bool ref_ok = kms_chip_bins(ref + (ptrdiff_t)(Y0 - ms::MARGIN) * a.sref + (X0 - ms::MARGIN), a.sref, a.dtype, b1.data());
        int64_t Sx = 0;
        if (ref_ok) {
            for (int i = 0; i < ms::BINS; i++) marg[i] = 0;
            for (int i = 0; i < ms::NPX; i++) marg[b1[i]]++;
            for (int i = 0; i < ms::BINS; i++) Sx += tab[marg[i]];
        }
        for (int oy = -R; oy <= R; oy++)
            for (int ox = -R; ox <= R; ox++) {
                const int i = (oy + R) * S + (ox + R), x = X1 + ox, y = Y1 + oy;
                zk[i] = zmi[i] = zs::quiet_nan();
                if (!ref_ok || !ms::chip_inside(x, y, a.Wmon, a.Hmon)) continue;
                if (!kms_chip_bins(mon + (ptrdiff_t)(y - ms::MARGIN) * a.smon + (x - ms::MARGIN), a.smon, a.dtype, b2.data())) continue;
                for (int j = 0; j < ms::CELLS; j++) hist[j] = 0;
                for (int j = 0; j < ms::BINS; j++) marg[j] = 0;
                for (int j = 0; j < ms::NPX; j++) { hist[b1[j] * ms::BINS + b2[j]]++; marg[b2[j]]++; }
                int64_t Sy = 0, Sxy = 0;
                for (int j = 0; j < ms::BINS; j++) Sy += tab[marg[j]];
                for (int j = 0; j < ms::CELLS; j++) Sxy += tab[hist[j]];
                const int64_t num = ms::numerator(L, Sx, Sy), den = ms::denominator(L, Sxy);
                zk[i] = ms::studholme(num, den);
                zmi[i] = ms::mi_score(num, den);
            }
        ms::finish(zk, zmi.data(), R, zs::argmax(zk, S), X0, Y0, X1, Y1, a.offset + 2 * k, a.peak + k, a.peak_mi + k, a.shift + 2 * k, a.status + k);
    }
}

inline int kms_search(km_ctx *, const kms_args &a)
{
    switch (a.dtype) {
    case KM_U8: kms_search_host<uint8_t>(a); return KM_OK;
    case KM_U16: kms_search_host<uint16_t>(a); return KM_OK;
    case KM_I16: kms_search_host<int16_t>(a); return KM_OK;
    case KM_F32: kms_search_host<float>(a); return KM_OK;
    default: return KM_E_ARG;
    }
}
#endif
