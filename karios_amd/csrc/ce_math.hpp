// ce_math.hpp: every operation of the circular-error figure's numbers (karios/report/circular_error_plot.py:181-228, 254-303, 359-368) that
// decides a bit, as plain C++ shared by the kernels (k_ce.hip), the host build of the launchers (k_ce.hpp) and the CPU test
// (tests/test_ce_figure_host.py compiles this file with g++): the float32 bin index of np.histogram's uniform path with its three
// corrections, the right-side search of np.histogramdd on 11 edges, and FITPACK's fpbspl / bispeu for a bicubic spline in float64.
// tests/ce_figure_restatement.py is the definition; every function here is held to it bit for bit, which needs -ffp-contract=off and
// correctly rounded float32 division on every compiler that reads this text.
#pragma once
#include "accuracy_math.hpp"

namespace ce {

enum {
    LDS_BINS = 4095,        // bins of one axis histogram whose edges and counters a workgroup keeps in LDS ((2 * 4095 + 1) words)
    MAX_BINS = 65536,       // bins of one axis histogram the device form takes; beyond it numpy on a host copy
    GRID = 10,              // bins per axis of the scatter's density (np.histogram2d(bins=10))
    KNOTS = GRID + 4,       // knots per axis of the interpolating bicubic spline on GRID centres
    ROW_BITS = 24           // a row index inside a sort key (the sample has at most 2^24 rows)
};

// double arithmetic with one rounding per operation, whatever the compiler's contraction setting
#if defined(__HIP_DEVICE_COMPILE__)
AC_HD inline double dadd(double a, double b) { return __dadd_rn(a, b); }
AC_HD inline double dsub(double a, double b) { return __dadd_rn(a, -b); }
AC_HD inline double dmul(double a, double b) { return __dmul_rn(a, b); }
AC_HD inline double ddiv(double a, double b) { return __ddiv_rn(a, b); }
#else
AC_HD inline double dadd(double a, double b) { return a + b; }
AC_HD inline double dsub(double a, double b) { return a - b; }
AC_HD inline double dmul(double a, double b) { return a * b; }
AC_HD inline double ddiv(double a, double b) { return a / b; }
#endif

// ---- np.histogram, uniform bins (numpy/lib/_histograms_impl.py): first <= v <= last, edges[0] == first, edges[nb] == last ------------
// f = ((v - first) / (last - first)) * nb in float32, truncated; the value on the last edge belongs to the last bin; then numpy's two
// corrections against the edges themselves.  The clamps cannot act for a value inside the range; they keep every read inside the table.
AC_HD inline int axis_bin(float v, float first, float denom, int nb, const float *edges)
{
    const float d = v - first;
    const float q = d / denom;
    const float f = q * (float)nb;
    int i = (int)f;
    if (i >= nb) i = nb - 1;
    if (i < 0) i = 0;
    if (v < edges[i] && i > 0) i--;
    if (v >= edges[i + 1] && i != nb - 1) i++;
    return i;
}

// ---- np.histogramdd: searchsorted(edges, v, side="right") on GRID + 1 edges, the value on the last edge pulled into the last bin ------
// -> bin 0 .. GRID - 1, or -1 / GRID for a value outside the edges (an outlier numpy drops)
AC_HD inline int grid_bin(float v, const float *e)
{
    int k = 0;
    for (int j = 0; j <= GRID; j++) k += e[j] <= v ? 1 : 0;
    if (v == e[GRID]) k--;
    return k - 1;
}

// ---- FITPACK (scipy.interpolate.dfitpack.bispeu) for kx = ky = 3 on KNOTS knots per axis ------------------------------------------------
// fpbisp's clamp and interval search, then fpbspl: the four non-zero cubic B-splines at t[l - 1] <= x < t[l] (l one-based as in
// FITPACK) by de Boor's recurrence, operand order as the Fortran text has it -> h[0 .. 3]; returns l - 4, the first coefficient row
AC_HD inline int bspline4(const double *t, double x, double *h)
{
    const int k = 3, k1 = 4, nk1 = KNOTS - k1;
    const double tb = t[k1 - 1], te = t[nk1];
    double arg = x;
    if (arg < tb) arg = tb;
    if (arg > te) arg = te;
    int l = k1;
    while (!(arg < t[l] || l == nk1)) l++;
    double hh[3];
    h[0] = 1.0;
    for (int j = 1; j <= k; j++) {
        for (int i = 0; i < j; i++) hh[i] = h[i];
        h[0] = 0.0;
        for (int i = 1; i <= j; i++) {
            const int li = l + i, lj = li - j;            // one-based knot numbers
            const double tli = t[li - 1], tlj = t[lj - 1];
            if (tli == tlj) { h[i] = 0.0; continue; }
            const double f = ddiv(hh[i - 1], dsub(tli, tlj));
            h[i - 1] = dadd(h[i - 1], dmul(f, dsub(tli, arg)));
            h[i] = dmul(f, dsub(arg, tlj));
        }
    }
    return l - k1;
}

// fpbisp's double sum for one point: sp = sp + c * wx[i] * wy[j], i outer, j inner, from 0
AC_HD inline double bispeu(const double *tx, const double *ty, const double *c, double x, double y)
{
    double wx[4], wy[4];
    const int lx = bspline4(tx, x, wx), ly = bspline4(ty, y, wy);
    double sp = 0.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) sp = dadd(sp, dmul(dmul(c[(lx + i) * GRID + ly + j], wx[i]), wy[j]));
    return sp;
}

// interpn(method="splinef2d", bounds_error=False): the spline where the point lies inside the grid of centres (float32 comparisons, a NaN
// fails them), NaN elsewhere; the float64 value rounded into the float32 result
AC_HD inline float density(const double *tx, const double *ty, const double *c, const float *box /* cx[0], cx[-1], cy[0], cy[-1] */, float x, float y)
{
    if (!(box[0] <= x && x <= box[1] && box[2] <= y && y <= box[3])) return ac::bits_f32(0x7fc00000u);
    return (float)bispeu(tx, ty, c, (double)x, (double)y);
}

// ---- the drawing order: np.argsort(z, kind="stable") - ascending, equal values (-0 == +0) in row order, NaN last ------------------------
AC_HD inline uint32_t z_key(float z)
{
    if (ac::is_nan(z)) return 0xffffffffu;
    return ac::order_key(z == 0.0f ? 0.0f : z);
}
// sort keys of one launch: column `col` (0: the density, 1: the radial error) in bit 57, the rows beyond the sample behind the column's
// own in bit 56, the value's order key above the row
AC_HD inline unsigned long long sort_key(int col, uint32_t key, uint32_t row) { return ((unsigned long long)col << 57) | ((unsigned long long)key << ROW_BITS) | row; }
AC_HD inline unsigned long long pad_key(int col, uint32_t row) { return ((unsigned long long)col << 57) | (1ull << 56) | row; }
AC_HD inline uint32_t key_row(unsigned long long k) { return (uint32_t)k & ((1u << ROW_BITS) - 1u); }
AC_HD inline uint32_t key_value(unsigned long long k) { return (uint32_t)(k >> ROW_BITS); }

}  // namespace ce
