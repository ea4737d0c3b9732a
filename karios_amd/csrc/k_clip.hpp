// k_clip.hip: the tracker's iterative outlier clip (karios/matcher/klt.py:52-71) as a stage on a finished frame block, and on plain
// resident columns (km_sigma_clip_dev).  The arithmetic is clip_math.hpp's; tests/clip_restatement.py is the definition.
// A compiler that is not hipcc (the host sanitizer build of the API files, the stand-alone program of tests/test_clip_host.py) gets
// the launcher defined here, as plain loops over the same header: device memory is host memory there, `c` is not touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/karios_hip.h"
#include "clip_math.hpp"

#define KC_UNITS_MAX KM_UNITS_PER_SUBMISSION
#define KC_CHUNK 2048      // rows a 256-thread workgroup compacts between two barriers (eight per thread)

// What differs between the units of a clip launch (blockIdx.y = unit).  frame != nullptr: the block (`cap` rows per column) is clipped in
// place; else the columns dx, dy of n rows are clipped and the survivors' indices go to keep_index.  u, v, idx, lab: the unit's working
// columns, kc_ws_rows(rows) words each
struct kc_unit {
    char *frame;
    const float *dx, *dy;
    int32_t *keep_index;
    int n, cap;
    float *u, *v;
    int32_t *idx, *lab;
    km_clip_result *rec;                 // survivors and rounds (nullptr: not wanted)
};
struct kc_units {
    kc_unit u[KC_UNITS_MAX];
};
// words of one working column for `rows` rows: whole chunks, so that a thread's eight-row loads stay inside
AC_HD static inline size_t kc_ws_rows(int rows) { return ((size_t)(rows > 0 ? rows : 1) + KC_CHUNK - 1) / KC_CHUNK * KC_CHUNK; }
static_assert(sizeof(km_clip_result) == sizeof(cl::result), "km_clip_result");

#if defined(__HIPCC__)
// every unit of A (n_units <= KC_UNITS_MAX) in one launch on c->stream; no row count beyond cl::MAX_ROWS (the caller refuses those)
int kc_clip_units(km_ctx *c, const kc_units &A, int n_units);
#else
static inline int kc_clip_units(km_ctx *, const kc_units &A, int n_units)
{
    for (int k = 0; k < n_units; k++) {
        const kc_unit &U = A.u[k];
        cl::result r;
        if (U.frame) {
            r = cl::clip_frame_block(U.frame, U.cap, U.u, U.v, U.idx, U.lab);
        } else {
            for (int i = 0; i < U.n; i++) { U.u[i] = U.dx[i]; U.v[i] = U.dy[i]; U.idx[i] = i; }
            r = cl::clip_columns(U.u, U.v, U.idx, U.n);
            for (int i = 0; i < r.count; i++) U.keep_index[i] = U.idx[i];
        }
        if (U.rec) { U.rec->count = r.count; U.rec->rounds = r.rounds; }
    }
    return KM_OK;
}
#endif
