// k_match.hip: brute-force L2 matching of SIFT descriptors (cv2.BFMatcher(NORM_L2).knnMatch, k <= 2) and the Lowe / mutual filter of
// the align step (karios/matcher/global_align.py:178-202), exact: tests/match_restatement.py is the definition (api_match.hip).
#pragma once
#include "common.hpp"

#define KMT_DIM 128          // descriptor length (SIFT)
#define KMT_QBLOCK 256       // query rows of one workgroup (4 waves x 64)
#define KMT_TILE 128         // train rows of one LDS tile
#define KMT_MAX_CHUNKS 1024  // pieces the train rows are split into at most (partial k-bests per (row, chunk))

// One packed descriptor set (a workspace slot): rows as int8 (x - 128), 128 bytes each, and the rows' sums of (x - 128)^2 behind them.
struct kmt_packed {
    const int8_t *rows;
    const int *norm;
    int n;
};
static inline size_t kmt_packed_bytes(int n) { return (size_t)n * KMT_DIM + (size_t)n * sizeof(int) + 256; }

// Device-side counters of one call (zeroed by kmt_state_reset): results of the filter, violations of the float32 pack.
struct kmt_state {
    unsigned long long first_bad[2];   // smallest row * 128 + column of an element that is no integer in 0 .. 255 (mon, ref); ~0: none
    unsigned n_bad[2];
    int counts[3];                     // raw, Lowe, mutual
    int pad;
};

int kmt_state_reset(km_ctx *c, kmt_state *st);
// dtype KM_U8 or KM_F32; `which` (0 / 1) selects the violation counters of st (st may be null for KM_U8).  d_dst: kmt_packed_bytes(n).
int kmt_pack(km_ctx *c, const void *d_src, int dtype, int n, ptrdiff_t stride, void *d_dst, kmt_state *st, int which, kmt_packed *out);
int kmt_chunks(const km_ctx *c, int n_q, int n_t);   // pieces of the train rows kmt_knn uses for this shape
// d_part: n_q * kmt_chunks * k keys of scratch.  d_idx / d_dist: [n_q, k]
int kmt_knn(km_ctx *c, const kmt_packed &q, const kmt_packed &t, int k, unsigned long long *d_part, int *d_idx, float *d_dist);
// d_flag: 2 * n_mon words of scratch (flags, then their exclusive scan); the outputs hold `cap` rows (rows beyond are counted, not written); st->counts is written
int kmt_filter(km_ctx *c, const int *d_fwd_idx, const float *d_fwd_dist, const int *d_bwd_idx, int n_mon, int n_ref, double ratio, unsigned *d_flag,
               int cap, int *d_qi, int *d_ti, float *d_dist, kmt_state *st);
