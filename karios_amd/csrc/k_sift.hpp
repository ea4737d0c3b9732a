// Kernels of SIFT detectAndCompute (k_sift.hip); api_sift.hip drives them octave by octave.  tests/sift_restatement.py is the
// definition, sift_math.hpp the per-candidate / per-key-point formulas both sides compile.
#pragma once
#include "common.hpp"
#include "sift_math.hpp"

// one side of a symmetric Gaussian kernel: k[0] the centre tap, k[j] the taps at distance j
struct ksf_taps {
    float k[sf::MAX_RADIUS + 1];
    int radius;
};
struct ksf_cand { int layer, r, c; };

int ksf_base(km_ctx *c, const uint8_t *d_img, int H, int W, ptrdiff_t stride, float *d_out);   // -> the doubled image, 2H x 2W, dense
// dst = blur(src); when dog != nullptr also dog = dst - src (the DoG level between the two).  tmp: the row pass, h x w floats
int ksf_blur(km_ctx *c, const float *src, int h, int w, const ksf_taps &taps, float *tmp, float *dst, float *dog);
int ksf_decimate(km_ctx *c, const float *src, int h, int w, float *dst);                       // dst: (h / 2) x (w / 2), every second sample
int ksf_scan(km_ctx *c, const float *dog, size_t plane, int h, int w, int n_layers, float threshold, ksf_cand *cand, unsigned cap, unsigned *counter);
int ksf_refine(km_ctx *c, const float *dog, size_t plane, int h, int w, int octv, const ksf_cand *cand, unsigned n_cand, int n_layers,
               double contrast_threshold, double edge_threshold, double sigma, sf::Refined *out, unsigned *counter);
int ksf_orient(km_ctx *c, const float *gauss, size_t plane, int h, int w, int octv, const sf::Refined *refined, unsigned n_refined, sf::Key *kp,
               unsigned cap, unsigned *counter);
int ksf_describe(km_ctx *c, const float *gauss, size_t plane, int h, int w, int octv, const sf::Key *kp, unsigned n, uint8_t *desc);
// the final order: entry i of the outputs is key point perm[i], halved back to the coordinates of the image that came in
int ksf_gather(km_ctx *c, const sf::Key *kp, const uint8_t *desc, const int *perm, int n, float *x, float *y, float *size, float *angle,
               float *response, int *octave, void *out_desc, int desc_dtype, ptrdiff_t desc_stride);
