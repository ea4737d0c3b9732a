// clip_math.hpp: the tracker's iterative outlier clip (karios/matcher/klt.py:52-71) as plain C++ on top of accuracy_math.hpp, shared by the
// kernel (k_clip.hip), the host build of the launchers (k_clip.hpp) and the CPU test (tests/test_clip_host.py compiles this file with g++).
// tests/clip_restatement.py is the definition; every function here is held to it bit for bit (-ffp-contract=off, correctly rounded
// float32 division / square root).
//   round:  mu = mean(u), su = std(u) (numpy's float32 sums, accuracy_math.hpp), the same for v
//           keep = |u - mu| < 3 su  &  |v - mv| < 3 sv  &  |u - mu| < 20  &  |v - mv| < 20      (strict; NaN compares false)
//           every row kept, or none left: stop.  Else compact the survivors stably and go on with the compacted arrays.
#pragma once
#include "accuracy_math.hpp"

namespace cl {

enum {
    MAX_ROWS = 32768,        // rows of one clip (the working set of a unit: four columns of MAX_ROWS words)
    LEAVES_MAX = 128,        // room for the leaves of ac::block_sum's tree over n <= ac::BLOCK elements (the most is 65, at n = 8191: tests/test_clip_host.py walks every n)
    FULL_LEAVES = ac::BLOCK / ac::LEAF
};

struct result {              // km_clip_result of include/karios_hip.h
    int32_t count;           // survivors
    int32_t rounds;          // rounds computed (statistics taken): 0 for n = 0
};

// ---- the leaves of ac::block_sum's tree over n <= ac::BLOCK elements, left to right: leaf k covers [off[k], off[k] + len[k]).  Returns their
// number.  The same tree as ac::block_sum's, walked by a recursion that the compiler unrolls (DEPTH_MAX levels: a node of 8 q + r elements
// hands floor(q / 2) octets to the left and the rest to the right, so 8192 elements are seven levels deep at most): no stack, neither in
// memory nor in indexed registers - on the device one lane walks it every round
#define CL_INLINE AC_HD inline __attribute__((always_inline))
enum { DEPTH_MAX = 8 };
template <int D>
CL_INLINE void leaf_table_r(int o, int n, unsigned short *off, unsigned short *len, int &k)
{
    if (n <= ac::LEAF) { off[k] = (unsigned short)o; len[k] = (unsigned short)n; k++; return; }
    if constexpr (D > 0) {
        const int n2 = ac::split(n);
        leaf_table_r<D - 1>(o, n2, off, len, k);
        leaf_table_r<D - 1>(o + n2, n - n2, off, len, k);
    }
}
CL_INLINE int leaf_table(int n, unsigned short *off, unsigned short *len)
{
    int k = 0;
    leaf_table_r<DEPTH_MAX>(0, n, off, len, k);
    return k;
}
// ... and the tree's value from the sums of those leaves (leaf[k] in the table's order)
template <int D>
CL_INLINE float combine_r(const float *leaf, int n, int &k)
{
    if (n <= ac::LEAF) return leaf[k++];
    if constexpr (D > 0) {
        const int n2 = ac::split(n);
        const float left = combine_r<D - 1>(leaf, n2, k);
        const float right = combine_r<D - 1>(leaf, n - n2, k);
        return left + right;
    }
    return 0.0f;
}
CL_INLINE float combine(const float *leaf, int n)
{
    int k = 0;
    return combine_r<DEPTH_MAX>(leaf, n, k);
}

// ac::leaf_sum over the elements themselves (DEV false) or over their squared deviations from `mean` (np.std: x = a - mean; x * x)
template <bool DEV>
AC_HD inline float elem(float a, float mean) { return DEV ? ac::dev_sq(a, mean) : a; }
template <bool DEV>
AC_HD inline float leaf_sum(const float *a, int n, float mean)
{
    if (n < 8) {
        float res = -0.0f;
        for (int i = 0; i < n; i++) res += elem<DEV>(a[i], mean);
        return res;
    }
    float r[8];
    for (int j = 0; j < 8; j++) r[j] = elem<DEV>(a[j], mean);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++) r[j] += elem<DEV>(a[i + j], mean);
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += elem<DEV>(a[i], mean);
    return res;
}

// the leaves of an array of n elements: the FULL_LEAVES leaves of every full block, then the table of the last, shorter block
AC_HD inline int blocks_of(int n) { return (n + ac::BLOCK - 1) / ac::BLOCK; }
AC_HD inline int full_blocks_of(int n) { return n / ac::BLOCK; }

// np.add.reduce of a float32 column (or of its squared deviations), through the leaf table and the combine: what the kernel computes by lanes
template <bool DEV>
AC_HD inline float sum_f32(const float *a, int n, float mean)
{
    unsigned short off[LEAVES_MAX], len[LEAVES_MAX];
    float leaf[LEAVES_MAX], acc = 0.0f;
    for (int b = 0; b < n; b += ac::BLOCK) {
        const int m = n - b < ac::BLOCK ? n - b : ac::BLOCK;
        const int nl = leaf_table(m, off, len);
        for (int k = 0; k < nl; k++) leaf[k] = leaf_sum<DEV>(a + b + off[k], len[k], mean);
        acc += combine(leaf, m);
    }
    return acc;
}

// the rule of one round
AC_HD inline float limit_of(float std) { return 3.0f * std; }
AC_HD inline bool keeps(float u, float mu, float lu, float v, float mv, float lv)
{
    const float ou = fabsf(u - mu), ov = fabsf(v - mv);
    return ou < lu && ov < lv && ou < 20.0f && ov < 20.0f;
}
struct round_stats {
    float mu, lu, mv, lv;    // means and 3-sigma limits of the two columns
};
AC_HD inline round_stats stats_of(const float *u, const float *v, int n)
{
    round_stats s;
    s.mu = ac::mean_of(sum_f32<false>(u, n, 0.0f), n);
    s.mv = ac::mean_of(sum_f32<false>(v, n, 0.0f), n);
    s.lu = limit_of(ac::std_of(sum_f32<true>(u, n, s.mu), n));
    s.lv = limit_of(ac::std_of(sum_f32<true>(v, n, s.mv), n));
    return s;
}

// The whole clip on working columns u, v and idx (idx[i] = the row's name, carried along): compacts them in place, returns the result
AC_HD inline result clip_columns(float *u, float *v, int32_t *idx, int n)
{
    result r;
    r.rounds = 0;
    const int bound = n + 1;               // every round but the last drops a row
    for (int round = 0; round < bound && n > 0; round++) {
        const round_stats s = stats_of(u, v, n);
        r.rounds++;
        int m = 0;
        for (int i = 0; i < n; i++)
            if (keeps(u[i], s.mu, s.lu, v[i], s.mv, s.lv)) { u[m] = u[i]; v[m] = v[i]; idx[m] = idx[i]; m++; }
        if (m == n) break;
        n = m;
    }
    r.count = n;
    return r;
}

// ---- the clip of a frame block (km_frame_layout: header {rows, Ninit, flags, candidates}, six float32 columns of cap entries, column 5 = the
// row's position in the kept list).  u, v, idx, newlab: working columns of >= rows words each.
// scatter: kept-list position l of frame row j -> u[l] = dx[j], v[l] = dy[j], idx[l] = j
AC_HD inline int frame_rows(const int32_t *hdr, int cap) { const int r = hdr[0]; return r < 0 ? 0 : (r > cap ? cap : r); }
AC_HD inline result clip_frame_block(char *block, int cap, float *u, float *v, int32_t *idx, int32_t *newlab)
{
    int32_t *hdr = (int32_t *)block;
    float *col = (float *)(block + 16);
    const int rows = frame_rows(hdr, cap);
    for (int l = 0; l < rows; l++) { u[l] = 0.0f; v[l] = 0.0f; idx[l] = 0; newlab[l] = -1; }
    for (int j = 0; j < rows; j++) {
        const uint32_t l = ac::f32_bits(col[(size_t)5 * cap + j]);
        if (l < (uint32_t)rows) { u[l] = col[(size_t)2 * cap + j]; v[l] = col[(size_t)3 * cap + j]; idx[l] = j; }
    }
    const result r = clip_columns(u, v, idx, rows);
    if (r.count == rows) return r;         // nothing dropped: the block stands as it is
    for (int p = 0; p < r.count; p++)
        if ((uint32_t)idx[p] < (uint32_t)rows) newlab[idx[p]] = p;
    int m = 0;
    for (int j = 0; j < rows; j++) {
        if (newlab[j] < 0) continue;
        for (int c2 = 0; c2 < 5; c2++) col[(size_t)c2 * cap + m] = col[(size_t)c2 * cap + j];
        col[(size_t)5 * cap + m] = ac::bits_f32((uint32_t)newlab[j]);
        m++;
    }
    hdr[0] = m;
    return r;
}

}  // namespace cl
