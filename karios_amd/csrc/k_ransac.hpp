// k_ransac.hip: the device half of cv2.findHomography(..., cv2.RANSAC, ...) (karios/matcher/global_align.py:223-230): the 4-point models
// of a batch of iterations, their inlier counts over all pairs, and the inlier mask of the winner.  The arithmetic is ransac_math.hpp's;
// tests/ransac_restatement.py is the definition (api_ransac.hip holds the sequential half).
#pragma once
#include "common.hpp"

#define KRS_HSTRIDE 12    // floats per iteration in the scoring table: 9 coefficients, padded to 48 bytes
#define KRS_PTS 4         // pairs a lane of the scoring kernel owns
#define KRS_BLOCK 256     // its workgroup: 4 waves, each with 64 * KRS_PTS pairs of its own
#define KRS_WAVE_PAIRS (64 * KRS_PTS)
#define KRS_TILE (KRS_BLOCK * KRS_PTS)
#define KRS_HC_SMALL 16   // iterations a wave walks when the launch would not fill the chip otherwise
#define KRS_HC 64         // ... at most (one count per lane)

// (x, y) of src and dst, strides in elements -> d_pairs[n] = (x, y, mx, my)
int krs_pack(km_ctx *c, const float *d_src, ptrdiff_t stride_src, const float *d_dst, ptrdiff_t stride_dst, int n, float *d_pairs);
// iterations [first, first + count): d_idx[4 it ..] -> d_H64[9 it ..], d_Hf[KRS_HSTRIDE it ..] (NaN when the solve gave no model),
// d_valid[it], d_count[it] = 0
int krs_solve(km_ctx *c, const float *d_pairs, int n, const int *d_idx, int first, int count, double *d_H64, float *d_Hf, int *d_valid, int *d_count);
// d_count[it] += pairs with err <= thr under d_Hf[it], it in [first, first + count)
int krs_score(km_ctx *c, const float *d_pairs, int n, const float *d_Hf, int first, int count, float thr, int *d_count);
// one model (host, 9 float32): d_mask[i] = err <= thr, *d_total = their number
int krs_mask(km_ctx *c, const float *d_pairs, int n, const float *Hf, float thr, uint8_t *d_mask, int *d_total);
