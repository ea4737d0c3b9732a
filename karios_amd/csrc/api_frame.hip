// The frame block's way out of the device, shared by the tile pipeline (api_tile.hip), the batched units (api_units.hip) and the
// kernel-size search (api_auto.hip): the frame slots (claim, reserve, commit), the frame sink, the copies of n blocks laid out by
// km_frame_layout (api_internal.hpp), and what the caller does with a ticket: km_frame_wait, km_stream_wait_frame, km_frame_stage_ms.
#include "api_internal.hpp"
#include "k_clip.hpp"
#include <time.h>
#include <sys/prctl.h>

// The previous submitted frame's block may still be on its way to the host (on the d2h stream): WS_FRAME may be rewritten once it
// has left - a device-side wait that never stalls in practice (the copy takes 13 us, the next frame is written ~1 ms later).
int frame_block_free(km_ctx *c)
{
    const int rc = c->frame_copy ? km_wait(c, c->stream, c->frame_copy) : KM_OK;
    if (rc == KM_OK) c->frame_copy = nullptr;
    return rc;
}

int frame_sink_check(km_ctx *c, size_t pitch, int n, size_t ob)
{
    if (!pitch) pitch = ob;
    if (!c->frame_sink || (pitch >= ob && c->frame_sink_cap >= pitch * (size_t)(n - 1) + ob)) return KM_OK;
    return km_fail(c, KM_E_ARG, "frame sink of %zu bytes (pitch %zu) is smaller than %d frame block(s) of %zu bytes", c->frame_sink_cap, pitch, n, ob);
}

// the slot of a submitted frame: `bytes` of page-locked memory (one eighth of head-room when it grows) and its completion event
int frame_slot_reserve(km_ctx *c, km_frame_slot *slot, size_t bytes)
{
    KM_HIP(c, slot->host.reserve(bytes, bytes / 8));
    return km_event(c, &slot->done);
}

// n frame blocks of ob bytes (device pitch ob_al) leave d_out on stream s: into the frame sink, if there is one (km_set_frame_sink: the
// device-side copy; km_stream_wait_frame lets a stream of the caller - the one an RCCL collective is issued on - wait for exactly this
// copy), and into the slot's page-locked buffer.  One block travels as a plain copy, several as one strided copy each way
int frame_blocks_out(km_ctx *c, km_frame_slot *slot, const char *d_out, const km_frame_layout &L, int n, void *sink, size_t sink_pitch, hipStream_t s)
{
    int rc;
    const size_t ob = L.ob, ob_al = L.ob_al;
    slot->sunk_valid = false;
    if (sink) {
        if (n == 1) KM_HIP(c, hipMemcpyAsync(sink, d_out, ob, hipMemcpyDeviceToDevice, s));
        else KM_HIP(c, hipMemcpy2DAsync(sink, sink_pitch ? sink_pitch : ob, d_out, ob_al, ob, (size_t)n, hipMemcpyDeviceToDevice, s));
        if ((rc = km_event(c, &slot->sunk)) || (rc = km_record(c, slot->sunk, s))) return rc;
        slot->sunk_valid = true;
    }
    if (n == 1) KM_HIP(c, hipMemcpyAsync(slot->host, d_out, ob, hipMemcpyDeviceToHost, s));
    else KM_HIP(c, hipMemcpy2DAsync(slot->host, ob, d_out, ob_al, ob, (size_t)n, hipMemcpyDeviceToHost, s));
    if ((rc = km_record(c, slot->done, s))) return rc;
    c->frame_copy = slot->done;
    slot->bytes = ob * n;
    return KM_OK;
}

bool frame_clip_covers(int cap) { return cap <= cl::MAX_ROWS; }

// unit k's working columns are slices of the lane's WS_CL_COLS; nobody reads the per-unit record here
int frame_blocks_clip(km_ctx *c, char *const *d_blocks, int n, int cap)
{
    if (n < 1 || n > KC_UNITS_MAX || !frame_clip_covers(cap)) return km_fail(c, KM_E_INTERNAL, "frame clip: %d blocks of %d rows", n, cap);
    const size_t rows = kc_ws_rows(cap);
    float *ws = (float *)km_ws(c, WS_CL_COLS, rows * 4 * sizeof(float) * (size_t)n);
    if (!ws) return KM_E_NOMEM;
    kc_units A;
    for (int k = 0; k < n; k++) {
        kc_unit &u = A.u[k];
        u = kc_unit();
        float *base = ws + rows * 4 * (size_t)k;
        u.frame = d_blocks[k]; u.cap = cap;
        u.u = base; u.v = base + rows; u.idx = (int32_t *)(base + 2 * rows); u.lab = (int32_t *)(base + 3 * rows);
    }
    return kc_clip_units(c, A, n);
}

int frame_slot_claim(km_ctx *c, const char *who, int *k_out, km_frame_slot **slot_out)
{
    const int k = c->fslot_next;
    km_frame_slot *slot = &c->fslot[k];
    if (slot->pending.load(std::memory_order_acquire)) {   // never waited for: its block is about to be overwritten
        if (who && slot->deferred.load(std::memory_order_acquire)) return km_fail(c, KM_E_ARG, "%s: frame slot %d still holds a deferred submission", who, k);
        KM_HIP(c, hipEventSynchronize(slot->done));
        slot->pending.store(0, std::memory_order_release);
    }
    c->ev_cur = 1 + k;
    *k_out = k; *slot_out = slot;
    return KM_OK;
}

void frame_slot_commit(km_ctx *c, int k, int *ticket)
{
    c->fslot[k].pending.store(1, std::memory_order_release);
    c->fslot_next = (k + 1) % KM_FRAME_SLOTS;
    *ticket = k;
}

extern "C" {

// Touches only the slot (no context state, no error string): safe from another thread while the context is submitting.
int km_frame_wait(km_ctx *c, int ticket, const void **block, size_t *bytes)
{
    if (!c || ticket < 0 || ticket >= KM_FRAME_SLOTS || !block) return KM_E_ARG;
    km_frame_slot *slot = &c->fslot[ticket];
    if (!slot->done || !slot->pending.load(std::memory_order_acquire)) return KM_E_ARG;
    // The waiting thread has nothing else to do: poll and SLEEP (hipEventSynchronize spins - also on an event created with
    // hipEventBlockingSync - and kept one CPU per rank at 100 %: 0.72 of every 0.91-ms step; eight ranks want those CPUs for RCCL's proxies)
    // (the kernel rounds a sleep up by the thread's timer slack, 50 us by default: 1 us for the threads that wait here)
    // (the slack is this thread's for the duration of the wait only: the caller may be an application thread - ADVICE r5)
    const int slack_before = prctl(PR_GET_TIMERSLACK, 0UL, 0UL, 0UL, 0UL);
    (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL);
    struct slack_restore { int v; ~slack_restore() { if (v > 0) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)v, 0UL, 0UL, 0UL); } } slack_guard{slack_before};
    // a pipelined batched submission enqueues its tail (LK .. copy-out) with the NEXT submission or km_frame_flush: wait for that first.
    // Nobody doing either for 100 ms is a caller that forgot to flush - the tail is then enqueued from here (under the context's
    // enqueue lock; every other entry point of the submitting thread flushes before it touches the context)
    for (int spins = 0; slot->deferred.load(std::memory_order_acquire); spins++) {
        if (spins >= 5000) { const int rf = km_units_flush(c, false); if (rf) return rf; break; }
        struct timespec ts = {0, 20000};
        nanosleep(&ts, nullptr);
    }
    for (;;) {
        const hipError_t e = hipEventQuery(slot->done);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) return KM_E_HIP;
        struct timespec ts = {0, 20000};                  // 20 us: a hundredth of a batched submission
        nanosleep(&ts, nullptr);
    }
    slot->pending.store(0, std::memory_order_release);
    *block = slot->host;
    if (bytes) *bytes = slot->bytes;
    return KM_OK;
}

// Device-side hand-over of a submitted frame's block to a stream of the CALLER: `hip_stream` (a hipStream_t, e.g. the stream an RCCL
// all-gather of the frame sink is issued on) waits - on the device, the host does not block - until the block of frame `ticket` has
// been written to the frame sink that was set when the frame was submitted.
int km_stream_wait_frame(km_ctx *c, int ticket, void *hip_stream)
{
    if (!c || ticket < 0 || ticket >= KM_FRAME_SLOTS) return km_fail(c, KM_E_ARG, "km_stream_wait_frame: bad ticket %d", ticket);
    km_frame_slot *slot = &c->fslot[ticket];
    if (!slot->sunk || !slot->sunk_valid) return km_fail(c, KM_E_ARG, "km_stream_wait_frame: frame %d was submitted without a frame sink", ticket);
    KM_HIP(c, hipStreamWaitEvent((hipStream_t)hip_stream, slot->sunk, 0));
    return KM_OK;
}

// Stage spans of frame `ticket` (after km_frame_wait; profiling enabled), same order as km_get_stage_ms.
int km_frame_stage_ms(km_ctx *c, int ticket, float *out, int cap, int *n)
{
    if (!c || ticket < 0 || ticket >= KM_FRAME_SLOTS || !out) return KM_E_ARG;
    const int m = cap < ST_COUNT ? cap : ST_COUNT;
    for (int i = 0; i < m; i++) {
        out[i] = 0.f;
        float ms = 0.f;
        if (c->ev_ready && c->evs_used[1 + ticket][i] &&
            hipEventElapsedTime(&ms, c->evs[1 + ticket][i][0], c->evs[1 + ticket][i][1]) == hipSuccess)
            out[i] = ms;
    }
    if (n) *n = m;
    return KM_OK;
}

}  // extern "C"
