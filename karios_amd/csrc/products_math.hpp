// products_math.hpp: the arithmetic of the report's products (karios/report/product_generator.py:138-218), the altitude column
// (karios/api/core.py:1049-1053) and the altitude figure's box statistics (karios/report/shift_by_alt_plot.py:127-171, which is
// matplotlib.cbook.boxplot_stats) as plain C++, shared by the kernels (k_products.hip), the host build of the launchers
// (k_products.hpp) and the CPU test (tests/test_products_host.py compiles this file with g++).
// tests/products_restatement.py is the definition; every function here is held to it bit for bit, which needs -ffp-contract=off and
// correctly rounded division / square root on every compiler that reads this text.
#pragma once
#include <math.h>
#include <stdint.h>

#include "report_math.hpp"

namespace pm {

enum { MAX_ROWS = rp::MAX_ROWS, MAX_BIN = rp::MAX_BIN };
constexpr uint32_t NAN_FILL = 0x7FC00000u;       // float(np.float32(np.nan)) stored into a float32 row
constexpr uint32_t NO_PIXEL = 0xFFFFFFFFu;       // pixel index of a row that is out of range (H * W stays below it)
constexpr uint32_t NAN_KEY = 0xFFFFFFFFu;        // order key of every NaN value: behind +inf, one key whatever the sign and payload

// float32.astype(int): truncation toward zero as an exact double; false for NaN and the infinities
AC_HD inline bool truncated(float v, double &out)
{
    if ((ac::f32_bits(v) & 0x7FFFFFFFu) >= 0x7F800000u) return false;
    out = trunc((double)v);
    return true;
}
// numpy's index rule: [-size, size), a negative index counted from the end
AC_HD inline bool wrapped(float v, int size, int &out)
{
    double t;
    if (!truncated(v, t) || !(t >= -(double)size && t < (double)size)) return false;
    out = (int)t + (t < 0.0 ? size : 0);
    return true;
}
// GDAL's row rule: [0, size)
AC_HD inline bool plain_row(float v, int size, int &out)
{
    double t;
    if (!truncated(v, t) || !(t >= 0.0 && t < (double)size)) return false;
    out = (int)t;
    return true;
}
// the pixel a key point lands on, NO_PIXEL when it is out of range
AC_HD inline uint32_t raster_pixel(float x0, float y0, int H, int W)
{
    int x, y;
    if (!wrapped(x0, W, x) || !plain_row(y0, H, y)) return NO_PIXEL;
    return (uint32_t)y * (uint32_t)W + (uint32_t)x;
}

// ---- box statistics
AC_HD inline uint32_t value_key(float v) { return v != v ? NAN_KEY : rp::order_key(v); }
AC_HD inline double key_as_double(uint32_t k)       // an order statistic: a zero is +0.0
{
    const float v = rp::key_value(k);
    return v == 0.0f ? 0.0 : (double)v;
}
enum { Q1 = 0, MED = 1, Q3 = 2, IQR = 3, CILO = 4, CIHI = 5, WHISLO = 6, WHISHI = 7, N_STATS = 8 };

// np.percentile(x, [25, 50, 75])[j] for n >= 1 sorted values without a NaN; `at(i)` gives the i-th as its order key
template <typename At> AC_HD inline double percentile(const At &at, int n, double q)
{
    const double vi = RP_DMUL((double)(n - 1), q);
    int lo, hi;
    double gamma;
    if (vi >= (double)(n - 1)) { lo = hi = n - 1; gamma = RP_DADD(vi, 1.0); }
    else { lo = (int)floor(vi); hi = lo + 1; gamma = RP_DSUB(vi, (double)lo); }
    const float a = rp::key_value(at(lo)), b = rp::key_value(at(hi));
    const float af = a == 0.0f ? 0.0f : a, bf = b == 0.0f ? 0.0f : b;
    const double diff = (double)RP_FSUB(bf, af);               // (numpy forms the neighbours' difference in float32)
    return gamma >= 0.5 ? RP_DSUB((double)bf, RP_DMUL(diff, RP_DSUB(1.0, gamma))) : RP_DADD((double)af, RP_DMUL(diff, gamma));
}
// the number of sorted values (order keys through `at`, no NaN) that are <= limit / < limit, compared as doubles; a NaN limit: 0
template <typename At> AC_HD inline int count_le(const At &at, int n, double limit)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)rp::key_value(at(mid)) <= limit) lo = mid + 1; else hi = mid;
    }
    return lo;
}
template <typename At> AC_HD inline int count_lt(const At &at, int n, double limit)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)rp::key_value(at(mid)) < limit) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// boxplot_stats(x, whis=1.5) but the mean, of the n >= 1 sorted order keys of one group (NaN keys last) -> out[N_STATS]
template <typename At> AC_HD inline void box_of_sorted(const At &at, int n, double *out)
{
    if (at(n - 1) == NAN_KEY) {
        const uint64_t nan_bits = 0x7FF8000000000000ull;
        double nan;
        __builtin_memcpy(&nan, &nan_bits, 8);
        for (int k = 0; k < N_STATS; k++) out[k] = nan;
        return;
    }
    const double q1 = percentile(at, n, 0.25), med = percentile(at, n, 0.5), q3 = percentile(at, n, 0.75);
    const double iqr = RP_DSUB(q3, q1);
    const double half = RP_DDIV(RP_DMUL(1.57, iqr), sqrt((double)n));
    const double spread = RP_DMUL(1.5, iqr);
    const double loval = RP_DSUB(q1, spread), hival = RP_DADD(q3, spread);
    const int below = count_le(at, n, hival);                  // x <= hival: the first `below` of the sorted values
    double whishi = q3;
    if (below > 0) { const double m = key_as_double(at(below - 1)); if (!(m < q3)) whishi = m; }
    const int under = count_lt(at, n, loval);                  // x >= loval: all but the first `under`
    double whislo = q1;
    if (loval == loval && under < n) { const double m = key_as_double(at(under)); if (!(m > q1)) whislo = m; }   // (a NaN fence: no x >= it)
    out[Q1] = q1; out[MED] = med; out[Q3] = q3; out[IQR] = iqr;
    out[CILO] = RP_DSUB(med, half); out[CIHI] = RP_DADD(med, half);
    out[WHISLO] = whislo; out[WHISHI] = whishi;
}
// the class of one value: 0 inside, 1 below the lower whisker, 2 above the upper one (a NaN on either side: 0)
AC_HD inline int8_t flier_class(float x, double whislo, double whishi)
{
    const double xd = (double)x;
    return xd > whishi ? 2 : xd < whislo ? 1 : 0;
}

}  // namespace pm
