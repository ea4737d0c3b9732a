// k_zncc_search.hip: the ZNCC search around each key point - the (2R+1)^2 surface of _zncc2 (karios/matcher/zncc_service.py:45-126) at
// the offsets around the centre ZNCCService._compute_zncc scores (:186-238), its peak and the peak's sub-pixel position.  The
// reference's call graph has no such search; its _zncc2 defines every value.  The arithmetic is zncc_math.hpp's;
// tests/zncc_search_restatement.py is the definition.
// A compiler that is not hipcc (the host sanitizer build of the API files, the stand-alone program of tests/test_zncc_search_host.py) gets
// the launcher defined here, as plain loops over the same header: device memory is host memory there, `c` is not touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/karios_hip.h"
#include "zncc_math.hpp"

struct kzs_args {
    const void *ref, *mon;
    int dtype;                         // KM_U8 / KM_U16 / KM_I16 / KM_F32, the same for both rasters
    int Href, Wref, Hmon, Wmon;
    ptrdiff_t sref, smon;              // row strides in pixels
    const float *x0, *y0, *dx, *dy;
    int n, radius;                     // 0 < n <= zs::MAX_ROWS, 1 <= radius <= zs::MAX_RADIUS
    int32_t *offset;                   // n x 2
    double *peak;                      // n
    double *shift;                     // n x 2
    uint8_t *status;                   // n
    double *surface;                   // nullptr, or n x S x S
};

// every output of every row is written exactly once; KM_E_ARG: a pixel type the search does not read
int kzs_search(km_ctx *c, const kzs_args &a);

#if !defined(__HIPCC__)
#include <vector>

template <typename T>
inline void kzs_search_host(const kzs_args &a)
{
    const int R = a.radius, S = 2 * R + 1;
    const T *ref = (const T *)a.ref, *mon = (const T *)a.mon;
    std::vector<double> z((size_t)S * S);
    const int64_t bias = a.dtype == KM_I16 ? 32768 : 0;      // int16 biased by 2^15: a constant does not change the value
    for (int k = 0; k < a.n; k++) {
        int X0, Y0, X1, Y1;
        double *zk = a.surface ? a.surface + (size_t)k * S * S : z.data();
        if (!zs::centres(a.x0[k], a.y0[k], a.dx[k], a.dy[k], a.Href, a.Wref, a.Hmon, a.Wmon, X0, Y0, X1, Y1)) {
            for (int i = 0; i < S * S; i++) zk[i] = zs::quiet_nan();
            zs::skipped(a.offset + 2 * k, a.peak + k, a.shift + 2 * k, a.status + k);
            continue;
        }
        const T *pa = ref + (ptrdiff_t)(Y0 - zs::HW) * a.sref + (X0 - zs::HW);
        // the template's moments: once per row
        int64_t sa = 0, saa = 0;
        double m1 = 0.0, q1 = 0.0;
        for (int r = 0; r < zs::SIDE; r++)
            for (int cx = 0; cx < zs::SIDE; cx++) {
                if (a.dtype == KM_F32) m1 += (double)pa[r * a.sref + cx];
                else { const int64_t v = (int64_t)pa[r * a.sref + cx] + bias; sa += v; saa += v * v; }
            }
        if (a.dtype == KM_F32) {
            m1 = m1 / (double)zs::NPX;
            for (int r = 0; r < zs::SIDE; r++)
                for (int cx = 0; cx < zs::SIDE; cx++) { const double d = (double)pa[r * a.sref + cx] - m1; q1 += d * d; }
        }
        for (int oy = -R; oy <= R; oy++)
            for (int ox = -R; ox <= R; ox++) {
                double &out = zk[(oy + R) * S + (ox + R)];
                const int x = X1 + ox, y = Y1 + oy;
                if (!zs::window_inside(x, y, a.Wmon, a.Hmon)) { out = zs::quiet_nan(); continue; }
                const T *pb = mon + (ptrdiff_t)(y - zs::HW) * a.smon + (x - zs::HW);
                if (a.dtype == KM_F32) {
                    double m2 = 0.0, q2 = 0.0, cc = 0.0;
                    for (int r = 0; r < zs::SIDE; r++)
                        for (int cx = 0; cx < zs::SIDE; cx++) m2 += (double)pb[r * a.smon + cx];
                    m2 = m2 / (double)zs::NPX;
                    for (int r = 0; r < zs::SIDE; r++)
                        for (int cx = 0; cx < zs::SIDE; cx++) {
                            const double d1 = (double)pa[r * a.sref + cx] - m1, d2 = (double)pb[r * a.smon + cx] - m2;
                            q2 += d2 * d2; cc += d1 * d2;
                        }
                    const double sd1 = sqrt(q1 / (double)zs::NPX), sd2 = sqrt(q2 / (double)zs::NPX);
                    out = (sd1 == 0.0 || sd2 == 0.0) ? zs::quiet_nan() : cc / (sd1 * sd2) / (double)zs::NPX;
                } else {
                    int64_t sb = 0, sbb = 0, sab = 0;
                    for (int r = 0; r < zs::SIDE; r++)
                        for (int cx = 0; cx < zs::SIDE; cx++) {
                            const int64_t va = (int64_t)pa[r * a.sref + cx] + bias, vb = (int64_t)pb[r * a.smon + cx] + bias;
                            sb += vb; sbb += vb * vb; sab += va * vb;
                        }
                    out = zs::int_value(zs::covariance_n2(sa, sb, sab), zs::variance_n2(sa, saa), zs::variance_n2(sb, sbb));
                }
            }
        zs::finish(zk, R, zs::argmax(zk, S), X0, Y0, X1, Y1, a.offset + 2 * k, a.peak + k, a.shift + 2 * k, a.status + k);
    }
}

inline int kzs_search(km_ctx *, const kzs_args &a)
{
    switch (a.dtype) {
    case KM_U8: kzs_search_host<uint8_t>(a); return KM_OK;
    case KM_U16: kzs_search_host<uint16_t>(a); return KM_OK;
    case KM_I16: kzs_search_host<int16_t>(a); return KM_OK;
    case KM_F32: kzs_search_host<float>(a); return KM_OK;
    default: return KM_E_ARG;
    }
}
#endif
