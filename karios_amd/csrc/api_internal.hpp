// Helpers shared by the entry-point translation units (api*.hip).
#pragma once
#include "common.hpp"

// stage timers are cleared per pipeline: the KLT entry points own [ST_MINMAX, ST_LK], ZNCC owns ST_ZNCC
enum { RESET_NONE = 0, RESET_KLT = 1, RESET_ZNCC = 2 };
int begin_call(km_ctx *c, int reset = RESET_NONE);   // start of every entry point: device, pending uploads, stale jobs, stage timers
int check_image(km_ctx *c, const void *p, int H, int W, ptrdiff_t stride, const char *what);
int check_params(km_ctx *c, const km_klt_params *p);
int frame_block_free(km_ctx *c);                     // WS_FRAME may be rewritten once the previous submitted frame's block has left

// ---- modes of one tile call.  The entry point creates it; it travels klt_tile_dev_impl -> klt_track_dev -> read_stats / fetch_tracks (api_tile.hip)
struct km_call_modes {
    bool spec_allowed = false;       // in: the entry point checks sc->flags with its result and repeats a flagged tile through the exact path
    bool mm_early_allowed = false;   // in: the entry point reads no min / max statistics back (km_klt_tile_frame_submit)
    bool spec_used = false;          // out: the call went through the speculative corner path
    unsigned spec_flags = 0;         // out: sc->flags of that run, once read back (read_stats)
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
// ---- a frame block's way out (api_tile.hip): the slot's page-locked buffer and completion event; n blocks to the sink and to the slot
int frame_sink_check(km_ctx *c, size_t pitch, int n, size_t ob);
int frame_slot_reserve(km_ctx *c, km_frame_slot *slot, size_t bytes);
int frame_blocks_out(km_ctx *c, km_frame_slot *slot, const char *d_out, size_t ob, size_t ob_al, int n, void *sink, size_t sink_pitch, hipStream_t s);
