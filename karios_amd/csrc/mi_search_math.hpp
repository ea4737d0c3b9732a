// The arithmetic of the mutual-information search around a key point (k_mi_search.hip, the host launcher of k_mi_search.hpp): the chip
// bounds rule of MutualInfoService._compute_mutual_info (mutual_info_service.py:99-130), the bins of
// np.histogram2d(chip_ref, chip_mon, bins=32) as integers (mi_math.hpp) or from numpy's float64 edges, and both scores from the counts
// through a table of c ln c as 64-bit integers (mi_clogc_q36.inc): a value is a function of the pixels alone, the same bits on every
// device and on the host, in whatever order the sums are taken.  Centres, skip rule, peak and parabola are zncc_math.hpp's, unchanged.
// tests/mi_search_restatement.py is the definition; compiled by hipcc for the device and by any C++ compiler for the host, always with
// -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mi_math.hpp"
#include "zncc_math.hpp"

namespace ms {

constexpr int CHIP = 57;
constexpr int MARGIN = 28;                // the chip's half, and the margin of the bounds rule
constexpr int NPX = CHIP * CHIP;          // 3249
constexpr int BINS = 32;
constexpr int CELLS = BINS * BINS;
constexpr int TABLE = NPX + 1;            // entries of mi_clogc_q36.inc

// the reference's bounds rule for a chip centred at column x, row y of a W x H raster
ZS_HD bool chip_inside(int x, int y, int W, int H) { return !(x - MARGIN < 0 || y - MARGIN < 0 || x >= W - MARGIN || y >= H - MARGIN); }

// Sx, Sy, Sxy: the sums of T over the row marginals, the column marginals and the cells; L = T[3249]
ZS_HD int64_t numerator(int64_t L, int64_t Sx, int64_t Sy) { return 2 * L - Sx - Sy; }
ZS_HD int64_t denominator(int64_t L, int64_t Sxy) { return L - Sxy; }
// (H(X) + H(Y)) / H(X,Y); NaN iff one cell is occupied
ZS_HD double studholme(int64_t num, int64_t den) { return den == 0 ? zs::quiet_nan() : (double)num / (double)den; }
// 2 (H(X) + H(Y) - H(X,Y)) / (H(X) + H(Y)); NaN iff one cell is occupied
ZS_HD double mi_score(int64_t num, int64_t den) { return num == 0 ? zs::quiet_nan() : (double)(2 * (num - den)) / (double)num; }

// ---- integer pixels: bin = min(floor(32 (v - lo) / R), 31), bin 16 for a constant chip (mi_math.hpp)
struct int_rule {
    unsigned lo, M;
    int R, sh;
};
ZS_HD int_rule int_bins(unsigned lo, unsigned hi)
{
    int_rule r;
    r.lo = lo; r.R = (int)(hi - lo);
    mi::magic(r.R, r.M, r.sh);
    return r;
}
ZS_HD int int_bin(unsigned v, const int_rule &r) { return mi::bin_of(mi::quotient(v - r.lo, r.M, r.sh), r.R); }

// ---- float32 pixels: numpy's edges on the float64 casts, i * step + lo with step = (hi - lo) / 32 and the last edge hi itself; a
// constant chip is widened by 0.5 on both sides
struct float_rule {
    double lo, hi, step;
};
ZS_HD float_rule float_bins(double lo, double hi)
{
    float_rule r;
    if (lo == hi) { lo = lo - 0.5; hi = hi + 0.5; }
    r.lo = lo; r.hi = hi; r.step = (hi - lo) / (double)BINS;
    return r;
}
ZS_HD double float_edge(int i, const float_rule &r) { return i == BINS ? r.hi : (double)i * r.step + r.lo; }
// searchsorted(edges, x, 'right') - 1 with the maximum folded into bin 31: a guess from one division, then the edges decide
ZS_HD int float_bin(double x, const float_rule &r, const double *edges)
{
    int b = (int)((x - r.lo) / r.step);
    b = b < 0 ? 0 : b > BINS - 1 ? BINS - 1 : b;
    while (b < BINS - 1 && x >= edges[b + 1]) b++;
    while (b > 0 && x < edges[b]) b--;
    return b;
}

// the outputs of one row from its two surfaces (Studholme: the peak is taken on it; the mi_score formula: monotone in it)
ZS_HD void finish(const double *z, const double *zmi, int R, int best, int X0, int Y0, int X1, int Y1, int32_t *offset, double *peak, double *peak_mi,
                  double *shift, uint8_t *status)
{
    zs::finish(z, R, best, X0, Y0, X1, Y1, offset, peak, shift, status);
    *peak_mi = best < 0 ? zs::quiet_nan() : zmi[best];
}

ZS_HD void skipped(int32_t *offset, double *peak, double *peak_mi, double *shift, uint8_t *status)
{
    zs::skipped(offset, peak, shift, status);
    *peak_mi = zs::quiet_nan();
}

}  // namespace ms
