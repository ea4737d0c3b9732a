// The arithmetic of the ZNCC search around a key point (k_zncc_search.hip, the host launcher of k_zncc_search.hpp):
// the window centres and the skip rule of ZNCCService._compute_zncc (zncc_service.py:186-238), the value of _zncc2
// (zncc_service.py:45-126) from exact integer moments, the peak of a (2R+1)^2 surface and its per-axis parabola.
// tests/zncc_search_restatement.py is the definition; this text is compiled by hipcc for the device and by any C++ compiler for the host,
// always with -ffp-contract=off: every float64 operation below rounds on its own, in the order written.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZS_HD __host__ __device__ __forceinline__
#else
#define ZS_HD inline
#endif

namespace zs {

constexpr int HW = 21;                  // the correlated window: 43 x 43
constexpr int SIDE = 2 * HW + 1;
constexpr int NPX = SIDE * SIDE;        // 1849
constexpr int MARGIN = 28;              // the bounds rule is stated on the 57 x 57 chip
constexpr int MAX_RADIUS = 8;
constexpr int MAX_ROWS = 1 << 20;
enum : uint8_t { SKIPPED = 1, NO_VALUE = 2, RIM_X = 4, RIM_Y = 8 };

ZS_HD double quiet_nan()
{
    union { uint64_t u; double d; } v = {0x7ff8000000000000ull};
    return v.d;
}

// X0 = int(x0), X1 = round(x0 + dx) on the float32 sum, half to even; false: the row is skipped
ZS_HD bool centres(float x0, float y0, float dx, float dy, int Href, int Wref, int Hmon, int Wmon, int &X0, int &Y0, int &X1, int &Y1)
{
    X0 = Y0 = X1 = Y1 = 0;
    const float sx = x0 + dx, sy = y0 + dy;
    // (a coordinate beyond 1e9 lies outside every raster: refused before the conversions, which are then defined)
    if (!(fabsf(x0) < 1e9f) || !(fabsf(y0) < 1e9f) || !(fabsf(sx) < 1e9f) || !(fabsf(sy) < 1e9f)) return false;
    X0 = (int)x0; Y0 = (int)y0;
    X1 = (int)rintf(sx); Y1 = (int)rintf(sy);
    return !(X0 - MARGIN < 0 || Y0 - MARGIN < 0 || X1 - MARGIN < 0 || Y1 - MARGIN < 0) &&
           !(X0 >= Wref - MARGIN || Y0 >= Href - MARGIN || X1 >= Wmon - MARGIN || Y1 >= Hmon - MARGIN);
}

// the 43 x 43 window centred at column x, row y lies in a W x H raster
ZS_HD bool window_inside(int x, int y, int W, int H) { return x - HW >= 0 && y - HW >= 0 && x + HW < W && y + HW < H; }

// exact moments of NPX pixel pairs (a, b < 2^16): sums S_a, S_b < 2^27, S_aa, S_bb, S_ab < 2^43
ZS_HD int64_t variance_n2(int64_t s, int64_t ss) { return (int64_t)NPX * ss - s * s; }
ZS_HD int64_t covariance_n2(int64_t sa, int64_t sb, int64_t sab) { return (int64_t)NPX * sab - sa * sb; }
ZS_HD double int_value(int64_t cv, int64_t v1, int64_t v2)
{
    return (v1 == 0 || v2 == 0) ? quiet_nan() : (double)cv / (sqrt((double)v1) * sqrt((double)v2));
}

// Is (v, i) a better peak than (bv, bi)?  bi < 0: no peak yet.  NaN never wins; ties go to the smaller raster index.
ZS_HD bool better(double v, int i, double bv, int bi) { return v == v && i >= 0 && (bi < 0 || v > bv || (v == bv && i < bi)); }

// index of the largest value of z[0 .. S * S), the first among equals; -1: none has a value
ZS_HD int argmax(const double *z, int S)
{
    int bi = -1;
    double bv = 0.0;
    for (int i = 0; i < S * S; i++)
        if (better(z[i], i, bv, bi)) { bv = z[i]; bi = i; }
    return bi;
}

// the vertex of the parabola through (zl, zc, zr) at -1, 0, 1 when it is a maximum; *rim: the step was refused by the rim or a missing neighbour
ZS_HD double axis_step(const double *z, int stride, int pos, int S, bool *rim)
{
    *rim = true;
    if (pos == 0 || pos == S - 1) return 0.0;
    const double zl = z[-stride], zc = z[0], zr = z[stride];
    if (zl != zl || zr != zr) return 0.0;
    *rim = false;
    const double den = (zl - 2.0 * zc) + zr;
    if (!(den < 0.0)) return 0.0;
    return 0.5 * (zl - zr) / den;
}

// the outputs of one row from its surface (S x S, raster order) and its peak's index (argmax)
ZS_HD void finish(const double *z, int R, int best, int X0, int Y0, int X1, int Y1, int32_t *offset, double *peak, double *shift, uint8_t *status)
{
    const int S = 2 * R + 1;
    if (best < 0) {
        offset[0] = offset[1] = 0;
        *peak = shift[0] = shift[1] = quiet_nan();
        *status = NO_VALUE;
        return;
    }
    const int iy = best / S, ix = best - iy * S;
    bool rim_x, rim_y;
    const double sx = axis_step(z + best, 1, ix, S, &rim_x), sy = axis_step(z + best, S, iy, S, &rim_y);
    offset[0] = ix - R; offset[1] = iy - R;
    *peak = z[best];
    shift[0] = (double)(X1 + (ix - R) - X0) + sx;
    shift[1] = (double)(Y1 + (iy - R) - Y0) + sy;
    *status = (uint8_t)((rim_x ? RIM_X : 0) | (rim_y ? RIM_Y : 0));
}

ZS_HD void skipped(int32_t *offset, double *peak, double *shift, uint8_t *status)
{
    offset[0] = offset[1] = 0;
    *peak = shift[0] = shift[1] = quiet_nan();
    *status = SKIPPED;
}

}  // namespace zs
