// Helpers shared by the entry-point translation units (api*.hip): the start of a call and its argument checks, the streams and events
// of a context, caller memory <-> device, the stages of a tile (api_tile.hip), the frame block - its ONE layout (km_frame_layout), its
// slots and its way out (api_frame.hip) - and the arena of the kernel-size search (api_auto.hip).
#pragma once
#include "common.hpp"
#include "k_prior.hpp"

#include <cstddef>
#include <cstring>

static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// stage timers are cleared per pipeline: the KLT entry points own [ST_MINMAX, ST_LK], ZNCC owns ST_ZNCC
enum { RESET_NONE = 0, RESET_KLT = 1, RESET_ZNCC = 2 };
int begin_call(km_ctx *c, int reset = RESET_NONE);   // start of every entry point: device, pending uploads, stale jobs, stage timers
int check_image(km_ctx *c, const void *p, int H, int W, ptrdiff_t stride, const char *what);
int check_params(km_ctx *c, const km_klt_params *p);
// ---- the argument checks the tile entry points share (api_tile.hip), in the order in which their errors win
int tile_call_begin(km_ctx *c, const char *who, const km_klt_params *prm, const void *ref, const void *mon, int H, int W, ptrdiff_t sref,
                    ptrdiff_t smon);                 // begin_call(RESET_KLT), the parameters, the two images
int check_dtype(km_ctx *c, const char *who, int dtype);
int check_frame_width(km_ctx *c, const char *who, const char *what, int W);   // the device-side frame ordering holds at most 65535 columns
int check_capacity(km_ctx *c, const km_klt_params *prm, int cap);
// a user mask as the kernels index it - dense rows: the mask itself, or the box of a larger resident mask packed into WS_MASK (1 B/px copy)
int dense_mask(km_ctx *c, const uint8_t *d_mask, ptrdiff_t smask, int H, int W, const uint8_t **dense);
// the arguments of the corner mask under a prior (k_prior.hpp) for one box: the tile call's, and every unit's of a batch under priors
static inline void fill_mask_args(kp_mask_args &a, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon,
                                  const uint8_t *d_base, ptrdiff_t sbase, const double *nodata_ref, const double *nodata_mon, const double *prior,
                                  double x_off, double y_off, uint8_t *d_mask)
{
    a.ref = d_ref; a.mon = d_mon; a.dtype = dtype; a.H = H; a.W = W; a.sref = sref; a.smon = smon; a.base = d_base; a.sbase = sbase;
    a.has_nd_ref = nodata_ref != nullptr; a.nd_ref = nodata_ref ? *nodata_ref : 0.0;
    a.has_nd_mon = nodata_mon != nullptr; a.nd_mon = nodata_mon ? *nodata_mon : 0.0;
    memcpy(a.P, prior, sizeof a.P);
    a.x_off = x_off; a.y_off = y_off; a.mask = d_mask;
}
static inline int corner_limit(const km_klt_params *prm, int cap) { return prm->max_corners > 0 && prm->max_corners < cap ? prm->max_corners : cap; }
// the corner part of a scalar block back to zero; the min / max and the valid-pixel count in front of it stay
static inline int clear_corner_scalars(km_ctx *c, km_scalars *sc)
{
    KM_HIP(c, hipMemsetAsync(&sc->max_eig_key, 0, sizeof(km_scalars) - offsetof(km_scalars, max_eig_key), c->stream));
    return KM_OK;
}
// the two-level pyramid of a unit: level 0 the Laplacian itself, level 1 in `l1`
static inline void pyr_two_level(km_pyr &P, const uint8_t *l0, const uint8_t *l1, int H, int W)
{
    P.img[0] = l0; P.H[0] = H; P.W[0] = W;
    P.img[1] = l1; P.H[1] = (H + 1) / 2; P.W[1] = (W + 1) / 2;
    P.levels = 1;
}
// c->stats from a km_scalars read-back: the maximum eigenvalue and the min / max always, of the rest what the caller's path owns
enum { KS_VALID = 1, KS_CANDIDATES = 2, KS_TIES = 4 };
static inline void stats_from_scalars(km_ctx *c, const km_scalars &h, int what)
{
    c->stats.max_eig = h.max_eig;
    c->stats.min_ref = h.mm[0]; c->stats.max_ref = h.mm[1]; c->stats.min_mon = h.mm[2]; c->stats.max_mon = h.mm[3];
    if (what & KS_VALID) c->stats.valid_pixels = (int64_t)h.valid;
    if (what & KS_CANDIDATES) c->stats.n_candidates = (int64_t)h.cut[3];
    if (what & KS_TIES) c->stats.tie_rows = (int32_t)h.tie_rows;
}

// ---- modes of one tile call.  The entry point creates it; it travels klt_tile_dev_impl -> klt_track_dev -> read_stats / fetch_tracks (api_tile.hip)
struct km_call_modes {
    bool spec_allowed = false;       // in: the entry point checks sc->flags with its result and repeats a flagged tile through the exact path
    bool mm_early_allowed = false;   // in: the entry point reads no min / max statistics back (km_klt_tile_frame_submit)
    bool spec_used = false;          // out: the call went through the speculative corner path
    unsigned spec_flags = 0;         // out: sc->flags of that run, once read back (read_stats)
    const kl_seed *seed = nullptr;   // in: the tracker starts every key point at its guess under this prior (km_klt_tile_frame_prior_dev)
};
// what every user of the synchronisation-free corner path (k_select2.hip) asks of the options and parameters; each adds what is its own
static inline bool spec_path_covers(const km_ctx *c, const km_klt_params *prm)
{
    return c->opt_speculative && c->fused_eig && prm->max_corners > 0 && prm->min_distance >= 1 && !c->opt_key_cap && !c->opt_stage_cap &&
           !c->opt_topk_factor && !c->opt_select_first;
}

// ---- api.hip: streams and events of a context
// The launchers enqueue on c->stream: inside this scope that is `s`; every way out, KM_HIP's included, restores the previous stream.
struct km_on_stream {
    km_ctx *c;
    hipStream_t prev;
    km_on_stream(km_ctx *ctx, hipStream_t s) : c(ctx), prev(ctx->stream) { c->stream = s; }
    ~km_on_stream() { c->stream = prev; }
    km_on_stream(const km_on_stream &) = delete;
};
int km_event(km_ctx *c, km_event_h *e);                   // creates *e (no timing) unless it exists
int km_stream(km_ctx *c, km_stream_h *s, int priority = 0);   // creates *s (non-blocking) unless it exists
int km_record(km_ctx *c, hipEvent_t ev, hipStream_t s);   // KM_OK or km_fail(...)
int km_wait(km_ctx *c, hipStream_t s, hipEvent_t ev);     // device-side wait of `s` for `ev`
int km_aux_stream(km_ctx *c);                             // the second stream with its fork / join events (created on first use)
int km_block_stream(km_ctx *c);                           // the block-copy stream (created on first use), behind c->stream's work so far

// results for the caller: DMA into the context's page-locked landing arena, then (KM_FLUSH) complete the stream and copy out
#define KM_D2H(c, dst, src, bytes)                                           \
    do {                                                                     \
        const int rq_ = km_d2h_queue((c), (dst), (src), (bytes));            \
        if (rq_) return rq_;                                                 \
    } while (0)
#define KM_FLUSH(c)                                                          \
    do {                                                                     \
        const int rq_ = km_d2h_flush(c);                                     \
        if (rq_) return rq_;                                                 \
    } while (0)


// ---- api.hip: caller memory <-> device (through the page-locked ring / landing arena, staging.hip)
int h2d_now(km_ctx *c, void *dst, const void *src, size_t bytes);
// caller columns -> one workspace slot: column i at *d + i * pitch, pitch = max(n, 1); a null column is skipped, n == 0 copies nothing
int upload_columns(km_ctx *c, int slot, const float *const *src, int k, int n, float **d);
int verify_upload(km_ctx *c, const char *when, int slot, const void *host, size_t elem, int H, int W, ptrdiff_t stride, const void *d);
int upload_image(km_ctx *c, int slot, const void *host, size_t elem, int H, int W, ptrdiff_t stride, void **dptr);
km_scalars *scalars(km_ctx *c);
// ---- api_tile.hip: the stages of a tile on dense device images
int build_pyramid_single(km_ctx *c, const uint8_t *d_img, int H, int W, int win, int max_level, uint8_t *store, km_pyr *P, size_t *used);
int build_pyramid_pair(km_ctx *c, const uint8_t *d_a, const uint8_t *d_b, int H, int W, int win, int max_level, km_pyr *A, km_pyr *B);
int gftt_dev(km_ctx *c, const uint8_t *d_img, const uint8_t *d_mask, int H, int W, int max_corners, double quality, double min_distance, int block,
             float *d_xy, int cap, km_scalars *sc);
int read_stats(km_ctx *c, km_scalars *sc, km_call_modes *m = nullptr);   // m: a call that may have taken the speculative corner path
int mark_lk_start(km_ctx *c);                        // records ev_lk_start on c->stream: the next unit's early min / max may start beside this LK launch

// ---- the frame block (the counterpart of karios_amd.frames.block_words / block_to_frame):
//   header (4 x int32: rows kept, corners, flags, candidates) | x0 | y0 | dx | dy | score | index bits (float32, cap each)
//   | zncc [| mutual_info_score | mi_score] (float64, cap each)
struct km_frame_layout {
    int cap = 0;
    size_t fb = 0;       // bytes up to the end of the float32 columns
    size_t ob = 0;       // bytes of a whole block
    size_t ob_al = 0;    // pitch of the blocks of a batch (256-byte aligned)
    km_frame_layout() = default;
    km_frame_layout(int cap_, bool with_zncc, bool with_mi)
        : cap(cap_), fb(16 + (size_t)cap_ * 6 * sizeof(float)),
          ob(fb + (with_zncc ? (size_t)cap_ * sizeof(double) : 0) + (with_mi ? (size_t)cap_ * 2 * sizeof(double) : 0)), ob_al(up256(ob)) {}
    enum { X0 = 0, Y0, DX, DY, SCORE, INDEX };                  // float32 columns
    enum { ZNCC = 0, MUTUAL_INFO, MI_SCORE };                   // float64 score columns
    const int *header(const char *block) const { return (const int *)block; }
    const float *col(const char *block, int i) const { return (const float *)(block + 16) + (size_t)i * cap; }
    double *score_col(char *block, int k) const { return (double *)(block + fb) + (size_t)k * cap; }
    // the rows a score kernel reads and the column it writes: ZNCC (out), or the two MI columns (out, out2)
    void score_unit(km_score_unit &s, char *block, bool mi) const
    {
        s.x0 = col(block, X0); s.y0 = col(block, Y0); s.dx = col(block, DX); s.dy = col(block, DY); s.score = col(block, SCORE);
        s.d_n = header(block);
        s.out = score_col(block, mi ? MUTUAL_INFO : ZNCC); s.out2 = mi ? score_col(block, MI_SCORE) : nullptr;
    }
};

// ---- api_frame.hip: the frame slots, the sink and a block's way out
int frame_block_free(km_ctx *c);                     // WS_FRAME may be rewritten once the previous submitted frame's block has left
int frame_sink_check(km_ctx *c, size_t pitch, int n, size_t ob);
// the next frame slot, free to be written (a block nobody waited for is waited for here), and c->ev_cur on its stage events.  who: the
// entry point that refuses a slot whose submission is still deferred (nullptr: none can be)
int frame_slot_claim(km_ctx *c, const char *who, int *k, km_frame_slot **slot);
int frame_slot_reserve(km_ctx *c, km_frame_slot *slot, size_t bytes);
int frame_blocks_out(km_ctx *c, km_frame_slot *slot, const char *d_out, const km_frame_layout &L, int n, void *sink, size_t sink_pitch, hipStream_t s);
void frame_slot_commit(km_ctx *c, int k, int *ticket);   // the claimed slot is pending: its ticket, and the ring moves on
// "frame_clip": the tracker's outlier clip (k_clip.hip) of n finished frame blocks of `cap` rows on c->stream, between the frame stage and the
// scores.  frame_clip_covers: what the stage takes - the entry points ask in front of their first launch
bool frame_clip_covers(int cap);
int frame_blocks_clip(km_ctx *c, char *const *d_blocks, int n, int cap);

// ---- api_auto.hip: the arena of the kernel-size search, offsets from a 256-byte aligned base
struct km_auto_arena {
    size_t na = 0, pts = 0, pyr_bytes = 0;          // pitches: a Laplacian, a point list, one image's pyramid levels
    size_t lap_ref = 0, lap_mon = 0;                // nk Laplacians each
    size_t pyr = 0;                                 // 2 nk pyramids: reference kernel k at 2k, its monitored twin at 2k + 1
    size_t p0 = 0;                                  // nk corner lists
    size_t trk = 0;                                 // nk * nk track pairs: p1 of a combination at 2 * combo, p0r at 2 * combo + 1
    size_t counts = 0, counts_bytes = 0;            // int32: [nk] corners per reference kernel, [nk * nk] kept tracks
    size_t total = 0;
};
static inline km_auto_arena km_auto_arena_of(int nk, int H, int W, size_t pyr_bytes, int cap)
{
    km_auto_arena a;
    const size_t k = (size_t)nk;
    a.na = up256((size_t)H * W); a.pts = up256((size_t)cap * 2 * sizeof(float)); a.pyr_bytes = pyr_bytes;
    a.lap_ref = 0; a.lap_mon = a.lap_ref + k * a.na; a.pyr = a.lap_mon + k * a.na;
    a.p0 = a.pyr + 2 * k * pyr_bytes; a.trk = a.p0 + k * a.pts;
    a.counts = a.trk + 2 * k * k * a.pts; a.counts_bytes = 4096;
    a.total = a.counts + a.counts_bytes;
    return a;
}
