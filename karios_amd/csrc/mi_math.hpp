// mi_math.hpp: the integer bin rule of the mutual-information kernel (k_mi.hip, integer pixel types) as plain C++, shared by the kernel and
// the CPU test (tests/test_score_host.py compiles tests/hoststub/mi_magic_main.cpp with g++ and walks every (R, d)).
// tests/score_restatement.py is the definition: bin = min(floor(32 d / R), 31) for 0 <= d <= R, bin 16 for a constant chip (R = 0).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MI_HD __host__ __device__
#else
#define MI_HD
#endif

namespace mi {

enum { BINS = 32, R_MAX = 65535 };

MI_HD inline int clz32(unsigned v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz((int)v);
#else
    return v ? __builtin_clz(v) : 32;
#endif
}

// floor(32 d / R) for 0 <= d <= R < 2^16 by ONE multiplication: with L = ceil(log2 R), s = 21 + L and M = ceil(2^s / R),
// M R = 2^s + e with 0 <= e < R <= 2^L, hence 32 d M / 2^s = 32 d / R + 32 d e / (R 2^s) and the excess is below
// 2^21 2^L / (R 2^s) = 1 / R: it cannot carry a quotient with fractional part <= (R - 1) / R over the next integer.  M <= 2^22, the
// product d M < 2^38: a 64-bit multiply-add and a 64-bit shift by s - 5.  (M from a float64 division: 2^s / R is an integer only
// for R a power of two, where the division is exact; otherwise it lies >= 1 / R from the integers, far beyond its 2^-31 error.)
MI_HD inline void magic(int R, unsigned &M, int &sh)
{
    const int L = R > 1 ? 32 - clz32((unsigned)(R - 1)) : 0;
    M = R ? (unsigned)ceil(ldexp(1.0, 21 + L) / (double)R) : 0u;
    sh = 21 + L - 5;
}

MI_HD inline int quotient(unsigned d, unsigned M, int sh) { return (int)(unsigned)(((unsigned long long)d * M) >> sh); }

// the maximum folds into the last bin (numpy's on_edge rule); a constant chip: numpy widens the range to [v - 0.5, v + 0.5], the samples sit
// in the middle bin 16
MI_HD inline int bin_of(int q, int R) { return R ? (q < BINS - 1 ? q : BINS - 1) : BINS / 2; }

}  // namespace mi
