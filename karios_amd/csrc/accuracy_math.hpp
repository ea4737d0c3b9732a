// accuracy_math.hpp: the float32 arithmetic of GeometricStat (karios/accuracy_analysis/accuracy_statistics.py:112-238) and the non-zero
// test of the valid-pixel count (karios/api/core.py:284-290) as plain C++, shared by the kernels (k_accuracy.hip), the host build of
// the launchers (k_accuracy.hpp) and the CPU test (tests/test_accuracy_host.py compiles this file with g++).
// tests/accuracy_restatement.py is the definition; every function here is held to it bit for bit, which needs -ffp-contract=off and
// correctly rounded float32 division / square root on every compiler that reads this text.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define AC_HD __host__ __device__
#else
#define AC_HD
#endif

namespace ac {

enum { BLOCK = 8192, LEAF = 128 };   // np.getbufsize() elements per call of the add loop; numpy's PW_BLOCKSIZE

AC_HD inline uint32_t f32_bits(float v) { uint32_t b; __builtin_memcpy(&b, &v, 4); return b; }
AC_HD inline float bits_f32(uint32_t b) { float v; __builtin_memcpy(&v, &b, 4); return v; }

// ---- numpy's pairwise sum inside one block of the reduction ---------------------------------------------------------------------------
// n <= LEAF: fewer than 8 left to right, else eight accumulators, their fixed combination, the remainder left to right
AC_HD inline float leaf_sum(const float *a, int n)
{
    if (n < 8) {
        float res = -0.0f;       // (numpy starts at -0 so that a sum of -0 stays -0; the reduction's own accumulator starts at +0)
        for (int i = 0; i < n; i++) res += a[i];
        return res;
    }
    float r[8];
    for (int j = 0; j < 8; j++) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++) r[j] += a[i + j];
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i];
    return res;
}
AC_HD inline int split(int n) { const int h = n / 2; return h - h % 8; }
// the tree over n <= BLOCK elements: above LEAF a node adds the sums of [0, split(n)) and [split(n), n).  Walked with a stack of its own
// (a full block is the perfect tree over 64 leaves, which the kernel takes by lanes instead)
AC_HD inline float block_sum(const float *a, int n)
{
    int off[24], len[24], stage[24];
    float left[24], ret = 0.0f;
    int sp = 0;
    off[0] = 0; len[0] = n; stage[0] = 0;
    while (sp >= 0) {
        if (len[sp] <= LEAF) { ret = leaf_sum(a + off[sp], len[sp]); sp--; continue; }
        const int n2 = split(len[sp]);
        if (stage[sp] == 0) {
            stage[sp] = 1;
            off[sp + 1] = off[sp]; len[sp + 1] = n2; stage[sp + 1] = 0; sp++;
        } else if (stage[sp] == 1) {
            left[sp] = ret; stage[sp] = 2;
            off[sp + 1] = off[sp] + n2; len[sp + 1] = len[sp] - n2; stage[sp + 1] = 0; sp++;
        } else {
            ret = left[sp] + ret; sp--;
        }
    }
    return ret;
}
// np.add.reduce over the block sums: left to right into an accumulator that starts at +0
AC_HD inline float fold_blocks(const float *bsum, int nblocks)
{
    float acc = 0.0f;
    for (int b = 0; b < nblocks; b++) acc += bsum[b];
    return acc;
}

// ---- element expressions ------------------------------------------------------------------------------------------------------------
AC_HD inline float dev_sq(float a, float mean) { const float d = a - mean; return d * d; }          // np.std: x = a - mean; x * x
AC_HD inline float radial(float dx, float dy, float factor)                                          // compute_percentile
{
    const float x = dx * factor, y = dy * factor;
    const float xx = x * x, yy = y * y;
    const float s = xx + yy;
    return sqrtf(s);
}
AC_HD inline float mean_of(float sum, int n) { return sum / (float)n; }
AC_HD inline float std_of(float sum_sq, int n) { return sqrtf(sum_sq / (float)n); }
AC_HD inline float median_even(float lo, float hi) { return (lo + hi) / 2.0f; }
AC_HD inline bool above(float score, double thr) { return (double)score > thr; }                     // Series.gt
AC_HD inline bool is_nan(float v) { return (f32_bits(v) & 0x7fffffffu) > 0x7f800000u; }

// np.count_nonzero's test, on the bits: NaN and denormals count, -0.0 does not; no float compare a flush mode could decide
AC_HD inline bool nonzero_f32_bits(uint32_t b) { return (b & 0x7fffffffu) != 0u; }

// ascending unsigned order == ascending float order (-0 below +0, NaNs at the two ends)
AC_HD inline uint32_t order_key(float v)
{
    const uint32_t b = f32_bits(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
AC_HD inline float order_value(uint32_t k) { return bits_f32((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ranks compute_percentile reads for `percent` of n > 0 values: p = percent * n (float64), k = int(p): r[k - 1] (index -1 = the largest)
// and r[k].  false: k is no index (the reference's IndexError)
AC_HD inline bool ce_ranks(double percent, int n, long long &lo, long long &hi)
{
    const double p = percent * (double)n;
    if (!(p > -1.0 && p < (double)n)) return false;
    const long long k = (long long)p;
    hi = k;
    lo = k - 1 < 0 ? (long long)n - 1 : k - 1;
    return true;
}

}  // namespace ac
