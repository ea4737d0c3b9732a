// k_prior.hip: what a geometric prior (prior_math.hpp) adds to the tile path - the corner mask under a prior (rule 4 of DESIGN.md
// section 21: a reference pixel may become a corner only where its guess meets a valid monitored pixel) and the seeded launch of the
// tracker's second form (k_lk2.hip).  tests/lk_prior_restatement.py is the definition.
// A compiler that is not hipcc (the host sanitizer build of the API files, the stand-alone program of tests/test_lk_prior_host.py) gets
// the mask launcher defined here as plain loops over the same header - device memory is host memory there, `c` is not touched - and
// the seeded tracker launch as the stand-in of the unseeded one (tests/hoststub: kernels are stand-ins there).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/karios_hip.h"
#include "prior_math.hpp"

struct kp_mask_args {
    const void *ref, *mon;             // H x W boxes of the two rasters, the same pixel type
    int dtype;                         // KM_U8 / KM_U16 / KM_I16 / KM_F32
    int H, W;
    ptrdiff_t sref, smon;              // row strides in pixels
    const uint8_t *base;               // nullptr (the reference's half of the automatic mask), or a user mask of H rows
    ptrdiff_t sbase;
    int has_nd_ref, has_nd_mon;
    double nd_ref, nd_mon;
    double P[9];
    double x_off, y_off;               // origin of the box in the coordinates the prior maps
    uint8_t *mask;                     // H x W, dense: 1 / 0
};

// every byte of the mask is written exactly once; KM_E_ARG: a pixel type the kernel does not read
int kp_prior_mask(km_ctx *c, const kp_mask_args &a);

// the masks of a batched submission's units (api_units.hip: km_klt_units_frame_prior_submit) in ONE launch: every unit its own boxes,
// base, prior, origin and output; one pixel type.  The table travels by value in the kernel arguments (16 entries: 3 KB of the 4)
#define KP_MASK_UNITS_MAX 16
struct kp_mask_units {
    int n;
    kp_mask_args a[KP_MASK_UNITS_MAX];
};
int kp_prior_mask_units(km_ctx *c, const kp_mask_units &A);

// the start positions of a seeded track: explicit guesses (n x 2 float32, device memory), or the prior evaluated per key point
struct kl_seed {
    const float *guess;                // nullptr: from P
    double P[9];
    double x_off, y_off;
};

#if !defined(__HIPCC__)
template <typename T>
inline void kp_prior_mask_host(const kp_mask_args &a)
{
    const T *ref = (const T *)a.ref, *mon = (const T *)a.mon;
    for (int y = 0; y < a.H; y++)
        for (int x = 0; x < a.W; x++) {
            bool ok = a.base ? a.base[(ptrdiff_t)y * a.sbase + x] != 0 : pm::valid<T>(ref[(ptrdiff_t)y * a.sref + x], a.has_nd_ref, a.nd_ref);
            int rx, ry;
            ok = ok && pm::target(a.P, a.x_off, a.y_off, x, y, a.W, a.H, rx, ry) && pm::valid<T>(mon[(ptrdiff_t)ry * a.smon + rx], a.has_nd_mon, a.nd_mon);
            a.mask[(size_t)y * a.W + x] = ok ? 1 : 0;
        }
}

inline int kp_prior_mask(km_ctx *, const kp_mask_args &a)
{
    switch (a.dtype) {
    case KM_U8: kp_prior_mask_host<uint8_t>(a); return KM_OK;
    case KM_U16: kp_prior_mask_host<uint16_t>(a); return KM_OK;
    case KM_I16: kp_prior_mask_host<int16_t>(a); return KM_OK;
    case KM_F32: kp_prior_mask_host<float>(a); return KM_OK;
    default: return KM_E_ARG;
    }
}

inline int kp_prior_mask_units(km_ctx *c, const kp_mask_units &A)
{
    for (int u = 0; u < A.n; u++)
        if (const int rc = kp_prior_mask(c, A.a[u])) return rc;
    return KM_OK;
}
#endif
