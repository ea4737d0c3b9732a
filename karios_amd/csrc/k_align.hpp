// k_align.hip: perspective warp, Sobel magnitude and the ECC kernels of the global align step (api_align.hip).
#pragma once
#include <algorithm>

#include "common.hpp"

#define KA_NSUM 66              // sums of one ECC iteration: N, S(mI), S(mI^2), S(mT), S(mT^2), S(mTI), 36 Hessian, 3 x 8 projections
#define KA_ECC_MAX_BLOCKS 2048  // workgroups of the iteration kernel (grid-stride beyond): its fp64 partials slab
#define KA_MASK 100             // ka_gauss5 source code: uint8 mask thresholded at > 0

struct ka_m9 { double m[9]; };
struct ka_h8 { float h[8]; };

int ka_warp_block_width(int dH, int dW);   // bw0 of WarpPerspectiveInvoker for a dH x dW destination
// warpPerspective with the INVERSE map (destination -> source), BORDER_CONSTANT
int ka_warp(km_ctx *c, const void *d_src, int dtype, int sH, int sW, ptrdiff_t ss, void *d_dst, int dH, int dW, ptrdiff_t ds, int linear,
            const double Minv[9], double border);
int ka_sobel_magnitude(km_ctx *c, const uint8_t *d_src, int H, int W, ptrdiff_t ss, float *d_out, unsigned *d_max);
int ka_gauss5(km_ctx *c, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, float *d_tmp, float *d_out);
int ka_ecc_plane(km_ctx *c, const float *d_blur, const float *d_pm_blur, int H, int W, float4 *d_plane);
int ka_ecc_blocks(int hs, int ws);
int ka_ecc_sums(km_ctx *c, const float *d_tmpl, int hs, int ws, const float4 *d_plane, int hd, int wd, const float map[9], double *d_partials,
                double *d_sums);
int ka_count_nonzero(km_ctx *c, const uint8_t *d_a, size_t n, unsigned long long *d_out);
