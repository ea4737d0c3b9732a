// chips_math.hpp: the arithmetic of the key-point chips (karios/report/chip_service.py) as plain C++, shared by the kernels
// (k_chips.hip), the host build of the launchers (k_chips.hpp) and the CPU test (tests/test_chips_host.py compiles this file with
// g++): CenterAndQuarterCellPointSelector's cells, bounds, distances and picks (:46-306) in float32, and the chip windows of
// _to_chips_gdal_dataset (:567-593) in float64.
// tests/chips_restatement.py is the definition; every function here is held to it bit for bit, which needs -ffp-contract=off and
// correctly rounded float32 division / square root on every compiler that reads this text.
#pragma once
#include <math.h>
#include <stdint.h>

#include "accuracy_math.hpp"

// one float32 rounding per operation: the device intrinsics, plain operators on the host.  The square root is sqrtf on both sides:
// HIP's __fsqrt_rn is the hardware's approximate square root unless the headers are built with OCML_BASIC_ROUNDED_OPERATIONS, sqrtf
// is correctly rounded under the library's -fhip-fp32-correctly-rounded-divide-sqrt (as accuracy_math.hpp's radial error relies on)
#if defined(__HIP_DEVICE_COMPILE__)
#define CH_SUB(a, b) __fsub_rn((a), (b))
#define CH_ADD(a, b) __fadd_rn((a), (b))
#define CH_MUL(a, b) __fmul_rn((a), (b))
#define CH_DIV(a, b) __fdiv_rn((a), (b))
#else
#define CH_SUB(a, b) ((a) - (b))
#define CH_ADD(a, b) ((a) + (b))
#define CH_MUL(a, b) ((a) * (b))
#define CH_DIV(a, b) ((a) / (b))
#endif
#define CH_SQRT(a) sqrtf(a)

namespace ch {

enum {
    CHIP = 57, MARGIN = 28, PIXELS = CHIP * CHIP,
    MAX_GRID = 16,                 // cells per axis
    PICKS = 5,                     // per cell: the centre and one per quarter
    MAX_SELECT_ROWS = 1 << 24,
    MAX_CHIP_ROWS = 1 << 20,
};

// ---- selection --------------------------------------------------------------------------------------------------------------------
struct grid {
    int rows, cols;
    double width, height;
    double thr;                    // (double)score >= thr: the caller's threshold, through float32 first unless it compares in float64
};

AC_HD inline bool passes(float score, double thr) { return (double)score >= thr; }

// clip(floor(v / float32(extent / count)), 0, count - 1); a NaN goes to cell 0
AC_HD inline int axis_cell(float v, double extent, int count)
{
    const float size = (float)(extent / (double)count);
    const float q = floorf(CH_DIV(v, size));
    if (!(q >= 0.0f)) return 0;
    return q >= (float)(count - 1) ? count - 1 : (int)q;
}
AC_HD inline int cell_of(float x, float y, const grid &g) { return axis_cell(y, g.height, g.rows) * g.cols + axis_cell(x, g.width, g.cols); }

// the float64 bounds of a cell as the reference computes them, rounded to the float32 the columns are compared with
struct cell_box {
    float xs, xm, xe, ys, ym, ye;  // start, middle, end
    float cx, cy;                  // centre
};
AC_HD inline void axis_bounds(int k, int count, double extent, float &s, float &m, float &e, float &c)
{
    const double size = extent / (double)count;
    const double start = (double)k * size;
    const double end = k < count - 1 ? (double)(k + 1) * size : extent;
    const double half = (end - start) / 2.0;
    s = (float)start; e = (float)end;
    m = (float)(start + half);
    c = (float)((start + end) / 2.0);
}
AC_HD inline cell_box make_box(const grid &g, int cell)
{
    cell_box b;
    axis_bounds(cell % g.cols, g.cols, g.width, b.xs, b.xm, b.xe, b.cx);
    axis_bounds(cell / g.cols, g.rows, g.height, b.ys, b.ym, b.ye, b.cy);
    return b;
}

AC_HD inline float dist(float x, float y, const cell_box &b)
{
    const float ddx = CH_SUB(x, b.cx), ddy = CH_SUB(y, b.cy);
    return CH_SQRT(CH_ADD(CH_MUL(ddx, ddx), CH_MUL(ddy, ddy)));
}
AC_HD inline float dev(float d, float med) { return fabsf(CH_SUB(d, med)); }

// bit q: the row belongs to quarter q (0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right).  The right quarters also take every row
// ON x_end, the bottom ones every row ON y_end - whatever its other coordinate, as the reference's masks do
AC_HD inline unsigned quarters(float x, float y, const cell_box &b)
{
    const bool left = x >= b.xs && x < b.xm, right = x >= b.xm && x < b.xe;
    const bool top = y >= b.ys && y < b.ym, bottom = y >= b.ym && y < b.ye;
    const bool on_x = x == b.xe, on_y = y == b.ye;
    return (left && top ? 1u : 0u) | ((right && top) || on_x ? 2u : 0u) | ((left && bottom) || on_y ? 4u : 0u) |
           ((right && bottom) || on_x || on_y ? 8u : 0u);
}

// lexicographic pick: the smallest key, then the largest score, then the first row
struct pick {
    unsigned long long hi;         // order key of the distance (or deviation) << 32 | ~order key of the score
    uint32_t row;                  // 0xffffffff: none
};
AC_HD inline pick no_pick() { pick p; p.hi = ~0ull; p.row = 0xffffffffu; return p; }
AC_HD inline pick make_pick(float key, float score, uint32_t row)
{
    pick p;
    p.hi = ((unsigned long long)ac::order_key(key) << 32) | (uint32_t)~ac::order_key(CH_ADD(score, 0.0f));     // (-0 and +0 are one score)
    p.row = row;
    return p;
}
AC_HD inline bool better(const pick &a, const pick &b) { return a.hi < b.hi || (a.hi == b.hi && a.row < b.row); }

// np.median from the two middle order statistics (equal for an odd count)
AC_HD inline float median_of(uint32_t key_lo, uint32_t key_hi, int count)
{
    return (count & 1) ? ac::order_value(key_hi) : ac::median_even(ac::order_value(key_lo), ac::order_value(key_hi));
}

// ---- windows ----------------------------------------------------------------------------------------------------------------------
struct window {
    int X0, Y0, X1, Y1;            // centres: int(x0), int(y0), round(x0 + dx), round(y0 + dy) (float64 sums, half to even)
    int ok;
};
// a centre that is not finite or beyond 2^30 is reported as 0 and makes the row not ok (the reference raises there)
AC_HD inline bool centre(double v, bool nearest, int &out)
{
    if (!(fabs(v) <= 1073741824.0)) { out = 0; return false; }
    out = (int)(nearest ? rint(v) : trunc(v));
    return true;
}
AC_HD inline bool inside(int X, int Y, int H, int W) { return X - MARGIN >= 0 && Y - MARGIN >= 0 && X - MARGIN + CHIP <= W && Y - MARGIN + CHIP <= H; }
AC_HD inline window make_window(float x0, float y0, float dx, float dy, int Href, int Wref, int Hmon, int Wmon)
{
    window w;
    bool ok = centre((double)x0, false, w.X0);
    ok = centre((double)y0, false, w.Y0) && ok;
    ok = centre((double)x0 + (double)dx, true, w.X1) && ok;
    ok = centre((double)y0 + (double)dy, true, w.Y1) && ok;
    w.ok = ok && inside(w.X0, w.Y0, Href, Wref) && inside(w.X1, w.Y1, Hmon, Wmon) ? 1 : 0;
    return w;
}

// BORDER_REFLECT_101 at the chip's own edge (radius <= 5)
AC_HD inline int reflect(int i) { i = i < 0 ? -i : i; return i > CHIP - 1 ? 2 * (CHIP - 1) - i : i; }
AC_HD inline bool ksize_ok(int k) { return k == 0 || (k >= 1 && k <= 11 && (k & 1)); }

}  // namespace ch
