// k_prep.hip: exact order statistics of a raster (radix select), the percentile stretch and CLAHE of the align step's _preprocess
// (api_prep.hip).
#pragma once
#include "common.hpp"

#define KP_MAX_Q 4                    // quantiles of one selection (api_prep.hip runs longer lists in groups of KP_MAX_Q)
#define KP_MAX_RANKS (2 * KP_MAX_Q)   // ranks tracked through the passes: floor(vi) and the one above it, per quantile
#define KP_BITS1 12                   // key bits a pass narrows: 12 + 10 + 10
#define KP_BITS23 10
#define KP_NB1 (1 << KP_BITS1)
#define KP_NB23 (1 << KP_BITS23)
#define KP_CLAHE_MAX_LUT_BYTES 65536  // all LUTs of a grid sit in the LDS of the apply kernel

// Device-side state of one selection (WS_PR_STATE); zeroed by kp_order_statistics before the first pass.
struct kp_state {
    unsigned long long hist1[KP_NB1];                     // pass 1: the top KP_BITS1 bits of every kept key
    unsigned long long hist2[KP_MAX_RANKS][KP_NB23];      // pass 2: the next KP_BITS23 bits of the keys under a tracked 12-bit prefix
    unsigned long long hist3[KP_MAX_RANKS][KP_NB23];      // pass 3: the last KP_BITS23 bits under a tracked 22-bit prefix
    unsigned long long rank_rem[KP_MAX_RANKS];            // rank of each wanted element inside its slot's keys
    unsigned prefix[KP_MAX_RANKS];                        // tracked prefixes, one per slot (distinct)
    int rank_slot[KP_MAX_RANKS];
    int n_slots, n_ranks;
    // results (one copy at the end)
    long long n;                                          // values kept
    double vi[KP_MAX_Q], v0[KP_MAX_Q], v1[KP_MAX_Q];
};

struct kp_q4 { double q[KP_MAX_Q]; };

// exclude 0: NaN left out; 1: every non-finite value left out.  n_q <= KP_MAX_Q.  `plain`: development A/B form of the LDS histogram
// (one atomic per pixel instead of one per run of equal bins)
int kp_order_statistics(km_ctx *c, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, int exclude, int n_q, const double *q, kp_state *st,
                        bool plain);
int kp_stretch(km_ctx *c, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, double lo, double hi, uint8_t *d_dst, ptrdiff_t ds);

struct kp_clahe_geom {
    int tiles_x, tiles_y, tile_w, tile_h;   // tile size of the (possibly extended) image
    int clip;                               // integer clip limit, 0 = no clipping
    float lut_scale;
};
// KM_E_ARG (error text set) for what the reflection cannot define; no launch
int kp_clahe_geometry(km_ctx *c, int H, int W, double clip_limit, int tiles_x, int tiles_y, kp_clahe_geom *g);
// d_hist: tiles * 256 unsigned counters, d_lut: tiles * 256 bytes
int kp_clahe(km_ctx *c, const uint8_t *d_src, int H, int W, ptrdiff_t ss, const kp_clahe_geom &g, unsigned *d_hist, uint8_t *d_lut, uint8_t *d_dst,
             ptrdiff_t ds);
