// km_klt_units_frame_submit: U independent work units - the tiles of `KLT.match` (reference karios/matcher/klt.py:220-253: no halo, per-tile
// uint8 stretch, per-tile quality threshold and maxCorners), of one pair or of several bands - through ONE device pipeline.
//
// Why.  Submitted one by one, every 30-Mpx unit pays the fixed costs of 20 000 corners serially: a corner-selection chain of nine
// latency-bound launches (0.12 ms at 4 % VALU occupancy), an LK launch with its fill + drain, three small frame launches, and dense
// kernels whose items are too short to amortise their halo (a 5490^2 unit fills two thirds of ONE round of resident waves).  Here
//   * min / max, stretch + Laplacians + mask, the fused eigenvalue pass and the pyramids take the unit as part of their linear item
//     space: one launch each, items as tall as a single 10980^2 tile's;
//   * the selection chain runs its U latency chains side by side (unit = blockIdx.z): nine launches for all units;
//   * ONE LK launch tracks every unit's corners, one frame / ZNCC / MI launch each scores them;
//   * the U frame blocks leave in one copy (host slot) / one strided copy (frame sink: the send buffer of the all-gather).
// Results are the unit-by-unit results bit for bit (tests/test_gpu_units.py): every kernel runs exactly the single-unit item code on
// the unit's own rasters, scalar block, key buffer and grid.  A unit the fixed capacities of the synchronisation-free corner path do
// not fit is flagged in its block's header (word 2) and repeated exactly by the caller, as for km_klt_tile_frame_submit.
#include "api_internal.hpp"
#include "k_prior.hpp"

#include <cmath>
#include <cstring>

// ---- software pipeline over consecutive submissions ("units_pipeline" 1; karios_amd.stream.FrameStream switches it on)
// A submission is three instruction-bound dense stages - L (stretch + Laplacians + mask), E (fused eigenvalue pass), K (LK) - and two
// latency-bound chains - C (corner selection: nine launches, between E and K) and F (FB test / frame order / ZNCC / MI, behind K).  In
// stream order the chains leave the GPU idle: 0.57 ms of a 3.5-ms submission of four 10980^2 pairs (profiles/timeline_r06_a.txt).  With
// the pipeline on, two LANES (workspace sets) alternate and the dense stages of consecutive submissions interleave on the main stream,
//     ... o.E | n.L | o.K | n.E | n'.L | n.K | n'.E ...            (o = previous submission, n = this one, n' = the next)
// while the chains run on a second stream beside the other lane's dense kernels: o.C beside n.L, o.F beside n.E.  The tail of a
// submission (K, F, copy-out) is therefore enqueued by the NEXT submission - or by km_frame_flush / any other entry point / km_ctx_sync.
// The chains' workgroups are 256 threads (k_select2.hip KF_T): they take the slots single retiring dense workgroups leave.
// Same kernels on the same data in the same per-submission order: frames are bit-identical to the unpipelined form.
enum { EV_MM = 0, EV_FORK, EV_JOIN, EV_E_DONE, EV_C_DONE, EV_K_DONE, EV_F_DONE, EV_SETUP };
static_assert(EV_SETUP < KM_LANE_EVENTS, "lane events");

struct km_units_tail {
    bool armed = false;
    int lane = 0, slot = 0;
    km_units U;
    km_klt_params prm;
    int n = 0, n_max = 0, cap = 0, dtype = 0;
    bool with_zncc = false, with_mi = false, with_clip = false, piped = false, profile_skip = false;
    bool seeded = false;                  // its LK is the seeded family's, on the seeds beside its own lane's table (km_klt_units_frame_prior_submit)
    double zncc_threshold = 0.0;
    km_frame_layout L;
    char *d_out = nullptr;
    void *sink = nullptr;                 // the frame sink as it was set at submission time
    size_t sink_pitch = 0;
};

// Lane, stage-event set and (tail: profile sampling) of one submission or of its tail; every way out restores what it found
struct units_scope {
    km_ctx *c;
    const int lane, ev;
    const bool skip, in_submit, tail;
    units_scope(km_ctx *ctx, bool is_tail) : c(ctx), lane(ctx->lane), ev(ctx->ev_cur), skip(ctx->profile_skip), in_submit(ctx->in_units_submit), tail(is_tail) {}
    ~units_scope() { c->lane = lane; c->ev_cur = ev; c->in_units_submit = in_submit; if (tail) c->profile_skip = skip; }
};

// K, F and the copy-out of a submission.  piped: K on the main stream behind the lane's chain, F on the chain stream behind K.
static int units_tail(km_ctx *c, km_units_tail &T)
{
    int rc;
    km_units &U = T.U;
    const int n = T.n;
    km_frame_slot *slot = &c->fslot[T.slot];
    hipStream_t const main_stream = c->stream;
    units_scope scope(c, true);
    c->lane = T.lane;
    c->ev_cur = 1 + T.slot;
    c->profile_skip = T.profile_skip;             // (the stage events of THIS submission: sampled with its own tick)
    km_event_h *ev = c->ev_lane[T.lane];
    if ((rc = km_wait(c, main_stream, ev[EV_JOIN])) || (T.piped && (rc = km_wait(c, main_stream, ev[EV_C_DONE])))) return rc;
    // ---- K7: LK forward + backward of every unit's corners in one launch
    {
        km_stage_timer t(c, ST_LK);
        if (!T.piped && (rc = mark_lk_start(c))) return rc;          // (unpipelined: the next submission's early min / max starts here)
        if ((rc = T.seeded ? kl_units_launch_seeded(c, n, T.n_max, T.prm.win_size) : kl_units_launch(c, n, T.n_max, T.prm.win_size))) return rc;
    }
    if (T.piped && ((rc = km_record(c, ev[EV_K_DONE], main_stream)) || (rc = km_wait(c, c->chain_stream, ev[EV_K_DONE])))) return rc;
    km_on_stream on(c, T.piped ? c->chain_stream : main_stream);
    // ---- K8: FB test, score, (x0, y0) order; K9 / K12: scores of the confident rows
    if ((rc = frame_block_free(c))) return rc;
    {
        km_stage_timer t(c, ST_FRAME);
        if ((rc = kf_frame_units(c, U, T.n_max, T.cap, 0.1f))) return rc;
        if (T.with_clip && (rc = frame_blocks_clip(c, U.frame, n, T.cap))) return rc;     // ("frame_clip" as it was when THIS submission was made)
    }
    if (T.with_zncc) {
        km_score_units S;
        for (int u = 0; u < n; u++) {
            km_score_unit &s = S.u[u];
            s.ref = U.ref_full[u]; s.mon = U.mon_full[u]; s.Href = s.Hmon = U.Hf[u]; s.Wref = s.Wmon = U.Wf[u]; s.sref = U.sref_f[u]; s.smon = U.smon_f[u];
            T.L.score_unit(s, U.frame[u], false);
            s.win = U.win[u];
        }
        {
            km_stage_timer t(c, ST_ZNCC);
            if ((rc = kz_zncc_units(c, S, n, T.dtype, T.n_max, (float)T.zncc_threshold))) return rc;
        }
        if (T.with_mi) {
            for (int u = 0; u < n; u++) T.L.score_unit(S.u[u], U.frame[u], true);
            km_stage_timer t(c, ST_MI);
            if ((rc = kmi_units(c, S, n, T.dtype, T.n_max, (float)T.zncc_threshold))) return rc;
        }
    }
    // ---- the blocks leave: one strided device copy into the frame sink, one copy into the slot's page-locked buffer.  Unpipelined: on the
    // block-copy stream (the next submission's dense kernels queue behind this tail on the main stream).  Pipelined: in the chain stream's
    // own order - one stream fewer: the runtime maps streams onto FOUR hardware queues, and whenever the copy stream shared one with the
    // main stream its device-side wait for this chain held the next eigenvalue pass up (1 ms per 16-unit step, profiles/timeline_r06_c4.txt)
    if (!T.piped && (rc = km_block_stream(c))) return rc;
    if ((rc = frame_blocks_out(c, slot, T.d_out, T.L, n, T.sink, T.sink_pitch, T.piped ? c->chain_stream : c->d2h_stream))) return rc;
    if (T.piped) {      // the lane's next submission may rewrite its scalars / points / frame buffers once this chain (copies included) is through
        if ((rc = km_record(c, ev[EV_F_DONE], c->chain_stream))) return rc;
        c->lane_f_recorded[T.lane] = true;
        c->frame_copy = nullptr;                        // (every lane owns its frame buffer and waits for EV_F_DONE)
    }
    slot->deferred.store(0, std::memory_order_release);
    return KM_OK;
}

// whatever follows on `s` may reuse a lane's workspace: behind the lane's frame stage and copies
static int wait_lane_done(km_ctx *c, int l, hipStream_t s) { return s && c->lane_f_recorded[l] ? km_wait(c, s, c->ev_lane[l][EV_F_DONE]) : KM_OK; }
// ... the main and the second stream behind both lanes
static int join_lanes(km_ctx *c)
{
    for (int l = 0; l < 2; l++) {
        int rc;
        if ((rc = wait_lane_done(c, l, c->stream)) || (rc = wait_lane_done(c, l, c->aux_stream))) return rc;
        c->lane_f_recorded[l] = false;
    }
    return KM_OK;
}

// the deferred tail, if any (submitting thread, or the fallback of km_frame_wait: under c->enqueue_mu)
static int units_flush_locked(km_ctx *c)
{
    if (!c->utail || !c->utail->armed) return KM_OK;
    c->utail->armed = false;
    const int rc = units_tail(c, *c->utail);
    if (rc) c->fslot[c->utail->slot].deferred.store(0, std::memory_order_release);   // (a waiter must not spin for ever: its wait fails on the event)
    return rc;
}

// (here, not in the header: the context owns its deferred tail, and km_units_tail is complete in this file only)
km_ctx::km_ctx() = default;
km_ctx::~km_ctx() = default;

// join = true (any entry point other than the next batched submission, km_ctx_sync, the option going off): the library's streams also
// wait for both lanes' chains - whatever follows on them may reuse lane 0's workspace in plain stream order
extern "C++" int km_units_flush(km_ctx *c, bool join)
{
    if (!c || !c->utail) return KM_OK;
    std::lock_guard<std::mutex> lk(c->enqueue_mu);
    if (c->utail->armed) KM_HIP(c, hipSetDevice(c->device));      // (the fallback of km_frame_wait runs on a thread of the caller's)
    const int rc = units_flush_locked(c);
    return rc || !join ? rc : join_lanes(c);
}

// the argument checks of a batched submission, and what the batch form does not cover (KM_E_UNSUPPORTED, no message: unit by unit then)
static int units_check_args(km_ctx *c, const km_unit *units, int n, int dtype, const km_klt_params *prm, int cap, const int *ticket)
{
    int rc;
    if (!c) return km_fail(nullptr, KM_E_ARG, "null context");
    if (!ticket || !units) return km_fail(c, KM_E_ARG, "klt_units_frame_submit: null argument");
    if (n < 1 || n > KM_UNITS_MAX) return km_fail(c, KM_E_ARG, "klt_units_frame_submit: %d units (1 .. %d per submission)", n, KM_UNITS_MAX);
    if ((rc = check_params(c, prm))) return rc;
    if (!km_dtype_size(dtype)) return km_fail(c, KM_E_ARG, "klt_units_frame_submit: bad dtype %d", dtype);
    if (cap <= 0 || prm->max_corners <= 0 || cap < prm->max_corners) return km_fail(c, KM_E_ARG, "klt_units_frame_submit: capacity %d / maxCorners %d", cap, prm->max_corners);
    // the batch form IS the synchronisation-free corner path: whatever that path does not cover goes unit by unit (no message).  Every
    // coverage check sits HERE, in front of the first launch: a refused batch has queued nothing
    if (!spec_path_covers(c, prm) || prm->max_level != 1 || cap > 32768) return KM_E_UNSUPPORTED;
    if (prm->block_size < 1 || prm->block_size > 15 || (prm->block_size & 1) == 0 || !c->opt_eig3 || !c->opt_lk2 || prm->win_size <= 2 || prm->win_size > 40)
        return KM_E_UNSUPPORTED;
    if (!km_lap_ksize_ok(prm->ksize_ref) || !km_lap_ksize_ok(prm->ksize_mon)) return KM_E_UNSUPPORTED;
    const bool with_zncc = units[0].d_ref_full != nullptr;
    const bool user_mask = units[0].d_mask != nullptr;
    if (with_zncc && dtype == KM_F32) return KM_E_UNSUPPORTED;
    for (int u = 0; u < n; u++) {
        const km_unit &q = units[u];
        if ((rc = check_image(c, q.d_ref, q.H, q.W, q.sref, "klt_units_frame_submit")) || (rc = check_image(c, q.d_mon, q.H, q.W, q.smon, "klt_units_frame_submit")))
            return rc;
        if ((q.d_ref_full != nullptr) != with_zncc) return km_fail(c, KM_E_ARG, "klt_units_frame_submit: either every unit carries full rasters or none");
        if ((q.d_mask != nullptr) != user_mask) return km_fail(c, KM_E_ARG, "klt_units_frame_submit: either every unit carries a user mask or none");
        if (user_mask && q.smask < q.W) return km_fail(c, KM_E_ARG, "klt_units_frame_submit: mask stride %td < width %d", q.smask, q.W);
        if (with_zncc && ((rc = check_image(c, q.d_ref_full, q.Hf, q.Wf, q.sref_f, "klt_units_frame_submit")) ||
                          (rc = check_image(c, q.d_mon_full, q.Hf, q.Wf, q.smon_f, "klt_units_frame_submit"))))
            return rc;
        if ((rc = check_frame_width(c, "klt_units_frame_submit", "unit", q.W))) return rc;
        if (q.W < 512 || q.H < 2 * prm->block_size + 8 || (q.W + 1) / 2 <= prm->win_size || (q.H + 1) / 2 <= prm->win_size) return KM_E_UNSUPPORTED;
        if ((prm->ksize_ref == 11 || prm->ksize_mon == 11) && q.H < 16) return KM_E_UNSUPPORTED;      // (the marching kernel's radius-5 form: kd_stretch_laplacian_units)
    }
    return KM_OK;
}

// ... and of a submission under priors (km_klt_units_frame_prior_submit), in the same position: a refused call has queued nothing
static int units_check_priors(km_ctx *c, const km_unit *units, int n, const double *priors)
{
    if (!priors) return km_fail(c, KM_E_ARG, "klt_units_frame_prior_submit: null priors");
    for (int u = 0; u < n; u++)
        for (int i = 0; i < 9; i++)
            if (!std::isfinite(priors[9 * u + i])) return km_fail(c, KM_E_ARG, "klt_units_frame_prior_submit: unit %d: prior[%d] is not finite", u, i);
    if (c->opt_frame_clip)
        return km_fail(c, KM_E_UNSUPPORTED, "klt_units_frame_prior_submit: \"frame_clip\" is on (the clip under a prior runs on the residuals, behind the frame)");
    for (int u = 0; u < n; u++)
        if (units[u].win_H != 0) return km_fail(c, KM_E_UNSUPPORTED, "klt_units_frame_prior_submit: unit %d carries an image window", u);
    return KM_OK;
}

static int units_submit(km_ctx *c, const km_unit *units, int n, int dtype, const double *nodata_ref, const double *nodata_mon, const km_klt_params *prm,
                        double zncc_threshold, int cap, const double *priors, int *ticket);

extern "C" {

// Enqueue whatever a pipelined batched submission deferred (include/karios_hip.h).  The submitting thread calls it when no further
// submission follows (FrameStream.drain, PendingBatch.wait on the submitting thread); every other entry point and km_ctx_sync do it
// themselves.
int km_frame_flush(km_ctx *c, int ticket)
{
    if (!c) return km_fail(nullptr, KM_E_ARG, "null context");
    if (ticket >= 0 && (ticket >= KM_FRAME_SLOTS || !c->fslot[ticket].deferred.load(std::memory_order_acquire))) return KM_OK;   // not the deferred one
    return km_units_flush(c, false);
}

int km_klt_units_frame_submit(km_ctx *c, const km_unit *units, int n, int dtype, const double *nodata_ref, const double *nodata_mon,
                              const km_klt_params *prm, double zncc_threshold, int cap, int *ticket)
{
    return units_submit(c, units, n, dtype, nodata_ref, nodata_mon, prm, zncc_threshold, cap, nullptr, ticket);
}

// The batched submission under a geometric prior per unit: block u is the block km_klt_tile_frame_prior_dev writes for
// unit u alone under priors + 9 u.  Two things differ from the unseeded submission: the corner mask of every unit is the prior's (one
// launch in front of the Laplacian pass, which takes it as the unit's user mask), and LK is the seeded family on the seeds that travel
// with the lane's table.
int km_klt_units_frame_prior_submit(km_ctx *c, const km_unit *units, int n, int dtype, const double *nodata_ref, const double *nodata_mon,
                                    const km_klt_params *prm, double zncc_threshold, int cap, const double *priors, int *ticket)
{
    int rc;
    if ((rc = units_check_args(c, units, n, dtype, prm, cap, ticket)) || (rc = units_check_priors(c, units, n, priors))) return rc;
    return units_submit(c, units, n, dtype, nodata_ref, nodata_mon, prm, zncc_threshold, cap, priors, ticket);
}

}  // extern "C"

// priors == nullptr: km_klt_units_frame_submit
static int units_submit(km_ctx *c, const km_unit *units, int n, int dtype, const double *nodata_ref, const double *nodata_mon, const km_klt_params *prm,
                        double zncc_threshold, int cap, const double *priors, int *ticket)
{
    int rc;
    if (!priors && (rc = units_check_args(c, units, n, dtype, prm, cap, ticket))) return rc;
    const bool with_zncc = units[0].d_ref_full != nullptr;
    const bool user_mask = units[0].d_mask != nullptr;
    const bool with_mi = with_zncc && c->opt_frame_mi;
    const bool with_clip = c->opt_frame_clip;      // (units_check_args refused cap > 32768, which is also what the clip takes)
    if (!c->utail) c->utail.reset(new km_units_tail);
    std::lock_guard<std::mutex> enqueue_lock(c->enqueue_mu);
    km_units_tail &old_tail = *c->utail;
    const bool piped = c->opt_units_pipeline && dtype != KM_U8;
    // (a pipelined submission was the previous one: its tail first, and this one behind both lanes' chains)
    if (!piped && ((rc = units_flush_locked(c)) || (rc = join_lanes(c)))) return rc;
    const int lane = piped ? (old_tail.armed ? 1 - old_tail.lane : 0) : 0;
    const bool pipe_start = piped && !old_tail.armed;      // (no pipelined submission directly in front of this one)
    hipStream_t const main_stream = c->stream;
    units_scope scope(c, false);
    int k;
    km_frame_slot *slot;
    if ((rc = frame_slot_claim(c, "klt_units_frame_submit", &k, &slot))) return rc;
    c->in_units_submit = true;
    if ((rc = begin_call(c, RESET_KLT))) return rc;
    memset(&c->stats, 0, sizeof c->stats);
    c->evs_used[c->ev_cur][ST_ZNCC] = false; c->evs_used[c->ev_cur][ST_MI] = false;
    c->lane = lane;
    if ((rc = km_aux_stream(c))) return rc;
    for (int i = 0; i < KM_LANE_EVENTS; i++)
        if ((rc = km_event(c, &c->ev_lane[lane][i]))) return rc;
    if (piped && (rc = km_stream(c, &c->chain_stream))) return rc;
    // Pipeline start: the second stream goes behind whatever the main stream holds at this point.  A pipelined submission runs its min / max
    // and its setup there AT ONCE, and takes lane 0 - the workspace of every other entry point: a tile still in flight on the main stream
    // (km_klt_tile_frame_submit) owns lane 0's scalar block, LK table and partials, the call in front may have written the rasters on the
    // main stream (km_shift_image_dev), and a second stream created a few lines up has seen none of the uploads the main stream was made to
    // wait for (join_uploads, km_upload_join).  One device-side wait per pipeline start; behind another pipelined submission the lanes' own
    // events order everything and nothing is added.
    if (pipe_start && ((rc = km_event(c, &c->ev_units_start)) || (rc = km_record(c, c->ev_units_start, c->stream)) || (rc = km_wait(c, c->aux_stream, c->ev_units_start))))
        return rc;
    km_event_h *ev = c->ev_lane[lane];

    // ---- layout: unit u's slices of the lane's workspace slots
    km_units U;
    U.n = n; U.dtype = dtype; U.has_user_mask = user_mask;
    size_t px_total = 0, pyr_total = 0, max_px = 0;
    size_t px_off[KM_UNITS_MAX], pyr_off[KM_UNITS_MAX];
    for (int u = 0; u < n; u++) {
        const km_unit &q = units[u];
        U.H[u] = q.H; U.W[u] = q.W; U.ref[u] = q.d_ref; U.mon[u] = q.d_mon; U.sref[u] = q.sref; U.smon[u] = q.smon; U.x_off[u] = q.x_off; U.y_off[u] = q.y_off;
        U.ref_full[u] = q.d_ref_full; U.mon_full[u] = q.d_mon_full; U.Hf[u] = q.Hf; U.Wf[u] = q.Wf; U.sref_f[u] = q.sref_f; U.smon_f[u] = q.smon_f;
        U.win[u].ox = q.win_ox; U.win[u].oy = q.win_oy; U.win[u].H = q.win_H; U.win[u].W = q.win_W;
        U.user_mask[u] = q.d_mask; U.user_smask[u] = q.smask;
        const size_t px = (size_t)q.H * q.W;
        px_off[u] = px_total; px_total += up256(px);
        max_px = px > max_px ? px : max_px;
        pyr_off[u] = pyr_total; pyr_total += up256((size_t)((q.H + 1) / 2) * ((q.W + 1) / 2));
    }
    c->units_sc_n = n;
    U.capk = max_px / 8 + 4096 * KM_NSHARD;
    const size_t sc_stride = up256(sizeof(km_scalars)), pb = up256((size_t)cap * 2 * sizeof(float));
    const km_frame_layout L(cap, with_zncc, with_mi);
    const size_t ob = L.ob, ob_al = L.ob_al;
    uint8_t *lap_ref = (uint8_t *)km_ws(c, WS_U8_A, px_total), *lap_mon = (uint8_t *)km_ws(c, WS_U8_B, px_total), *mask = (uint8_t *)km_ws(c, WS_MASK, px_total);
    unsigned long long *keys = (unsigned long long *)km_ws(c, WS_KEYS0, U.capk * sizeof(unsigned long long) * n);
    char *sc = (char *)km_ws(c, WS_SCALARS, sc_stride * n);
    char *p0 = (char *)km_ws(c, WS_PTS0, pb * n), *p1 = (char *)km_ws(c, WS_PTS1, pb * n), *p0r = (char *)km_ws(c, WS_PTS2, pb * n);
    uint8_t *pyr_a = (uint8_t *)km_ws(c, WS_PYR_A, pyr_total), *pyr_b = (uint8_t *)km_ws(c, WS_PYR_B, pyr_total);
    char *d_out = (char *)km_ws(c, WS_FRAME, ob_al * n);
    if (!lap_ref || !lap_mon || !mask || !keys || !sc || !p0 || !p1 || !p0r || !pyr_a || !pyr_b || !d_out) return KM_E_NOMEM;
    for (int u = 0; u < n; u++) {
        U.lap_ref[u] = lap_ref + px_off[u]; U.lap_mon[u] = lap_mon + px_off[u]; U.mask[u] = mask + px_off[u];
        U.keys[u] = keys + U.capk * u;
        U.sc[u] = (km_scalars *)(sc + sc_stride * u);
        U.mm[u] = U.sc[u]->mm;
        U.p0[u] = (float *)(p0 + pb * u); U.p1[u] = (float *)(p1 + pb * u); U.p0r[u] = (float *)(p0r + pb * u);
        U.frame[u] = d_out + ob_al * u;
        U.eig_partial[u] = nullptr; U.eig_npartial[u] = 0;
        c->units_sc[u] = U.sc[u];
        pyr_two_level(U.A[u], U.lap_ref[u], pyr_a + pyr_off[u], U.H[u], U.W[u]);
        pyr_two_level(U.B[u], U.lap_mon[u], pyr_b + pyr_off[u], U.H[u], U.W[u]);
    }
    if ((rc = frame_sink_check(c, c->frame_sink_pitch, n, ob)) || (rc = frame_slot_reserve(c, slot, ob * n))) return rc;
    // The lane's previous submission must have left its frame stage before its scalars, points and frame buffers are reset - the scalar
    // blocks' reset and the LK table's small copy ("setup").  Unpipelined: here, on the main stream.  Pipelined: on the second stream
    // BEHIND the min / max (below): the min / max touches none of those buffers, and with the wait in front of it the Laplacians of this
    // submission - which need the min / max only - stood behind the other lane's frame stage, which runs beside the previous
    // eigenvalue pass and outlasts it (16 units of 5490^2: 0.8 ms of an idle main stream per step, tools/investigations/stage_order.py).  The main
    // stream waits for the setup in front of the eigenvalue pass, the first kernel of this submission that touches the scalars.
    const int n_max = corner_limit(prm, cap);
    const bool setup_on_aux = piped && dtype != KM_U8;
    auto setup = [&]() -> int {
        KM_HIP(c, hipMemsetAsync(sc, 0, sc_stride * n, c->stream));
        return priors ? kl_units_prepare_seeded(c, U, priors, n_max, prm->win_size, prm->max_count, prm->epsilon)
                      : kl_units_prepare(c, U, n_max, prm->win_size, prm->max_count, prm->epsilon);
    };
    if (!setup_on_aux) {
        if ((rc = wait_lane_done(c, lane, c->stream)) || (rc = wait_lane_done(c, lane, c->aux_stream))) return rc;
        c->lane_f_recorded[lane] = false;
        if ((rc = setup())) return rc;
    }

    // ---- K1: min / max of every raster, on the second stream.  Pipelined: at once - beside whatever dense kernel the older submissions
    // are in (HBM-bound work under instruction-bound kernels).  Unpipelined, directly behind another submission: beside its LK.
    if (dtype != KM_U8) {
        double *out[KM_UNITS_MAX];
        const bool early = piped || (c->opt_mm_early && c->lk_start_prev);
        if (early) {
            double *slot_mm = (double *)km_ws(c, WS_UNITS_MM, (size_t)4 * KM_UNITS_MAX * sizeof(double));
            if (!slot_mm) return KM_E_NOMEM;
            for (int u = 0; u < n; u++) { out[u] = slot_mm + 4 * u; U.mm[u] = out[u]; }
            if (!piped && (rc = km_wait(c, c->aux_stream, c->ev_lk_start))) return rc;
            {
                km_on_stream on(c, c->aux_stream);
                {
                    km_stage_timer t(c, ST_MINMAX);
                    if ((rc = kd_minmax_units(c, U, out, WS_MM_PARTIAL))) return rc;
                }
                if ((rc = km_record(c, ev[EV_MM], c->aux_stream))) return rc;
                if (setup_on_aux) {      // the setup, behind the min / max and behind the lane's previous frame stage
                    rc = wait_lane_done(c, lane, c->aux_stream);
                    c->lane_f_recorded[lane] = false;
                    if (rc || (rc = setup()) || (rc = km_record(c, ev[EV_SETUP], c->aux_stream))) return rc;
                }
            }
            if ((rc = km_wait(c, c->stream, ev[EV_MM]))) return rc;
            c->stats.path_flags |= KM_PATH_MM_EARLY;
        } else {
            for (int u = 0; u < n; u++) out[u] = U.sc[u]->mm;
            km_stage_timer t(c, ST_MINMAX);
            if ((rc = kd_minmax_units(c, U, out, WS_PARTIAL))) return rc;
        }
    }
    // ---- under priors: every unit's corner mask (k_prior.hip), on the main stream directly in front of the pass that takes it.  It is
    // written into the unit's slice of the lane's WS_MASK and handed on as the unit's user mask IN PLACE (stride W), as the tile call does:
    // the pack kernel of the Laplacian pass reads and writes a byte in the same thread (k_lap.hip mask_pack_units_kernel), so source ==
    // destination is a copy onto itself.  (That kernel declares both pointers __restrict__, which source == destination does not honour
    // to the letter: what keeps it sound is that no thread reads a byte another thread - or an earlier iteration of its own - wrote, so
    // no reordering the qualifier permits can change a value; the qualifiers stay, for the kernel's code is the parent's.)  Stream order: whatever ordered that pass's writes of the lane's mask orders these.
    if (priors) {
        kp_mask_units M;
        M.n = n;
        for (int u = 0; u < n; u++)
            fill_mask_args(M.a[u], U.ref[u], U.mon[u], dtype, U.H[u], U.W[u], U.sref[u], U.smon[u], U.user_mask[u], U.user_smask[u], nodata_ref, nodata_mon,
                           priors + 9 * u, (double)U.x_off[u], (double)U.y_off[u], U.mask[u]);
        if ((rc = kp_prior_mask_units(c, M))) return rc;
        for (int u = 0; u < n; u++) { U.user_mask[u] = U.mask[u]; U.user_smask[u] = U.W[u]; }
        U.has_user_mask = true;
    }
    // ---- K2: stretch + Laplacians + automatic mask
    km_valid_units vjob;
    {
        km_stage_timer t(c, ST_LAPLACIAN);
        if ((rc = kd_stretch_laplacian_units(c, U, prm->ksize_ref, prm->ksize_mon, prm->invert_mon, nodata_ref, nodata_mon, &vjob))) return rc;
    }
    // The eigenvalue pass of THIS submission reads the Laplacian pass's per-item counts (k_eig3.hip: item classes).  Stream order: E of
    // submission n is enqueued on the main stream behind n.L, which wrote them, and the table lies in this lane's WS_LAP_VALID - the
    // next submission's Laplacian pass, which may run before n.E, writes the OTHER lane's; the lane's own next one (n + 2) follows n.E on
    // the main stream.  The sums on the second stream only read it.
    if (c->opt_eig3_valid_items) {
        for (int u = 0; u < n; u++) { U.lap_counts[u] = vjob.item_counts[u]; U.lap_nstrips[u] = vjob.item_nstrips[u]; }
        U.lap_rows = vjob.item_rows; U.lap_strip_w = vjob.item_strip_w;
    }
    // ---- the valid-pixel sums and the pyramids (they depend on the Laplacians only) on the second stream
    {
        if ((rc = km_record(c, ev[EV_FORK], c->stream)) || (rc = km_wait(c, c->aux_stream, ev[EV_FORK]))) return rc;
        km_on_stream on(c, c->aux_stream);
        if ((rc = kd_valid_sum_units(c, vjob))) return rc;
        {
            km_stage_timer tp(c, ST_PYRAMID);
            if ((rc = kd_pyrdown_units(c, U, 1))) return rc;
        }
        if ((rc = km_record(c, ev[EV_JOIN], c->aux_stream))) return rc;
    }
    // ---- pipelined: the PREVIOUS submission's LK goes here, between this one's Laplacians and its eigenvalue pass (its frame stage and
    // scores follow on the chain stream, beside this submission's eigenvalue pass)
    if (piped && (rc = units_flush_locked(c))) { (void)hipStreamWaitEvent(c->stream, ev[EV_JOIN], 0); return rc; }
    if (setup_on_aux && (rc = km_wait(c, c->stream, ev[EV_SETUP]))) return rc;      // (scalars reset, the lane's previous frame stage through)
    // ---- K3 + K4 fused
    {
        km_stage_timer t(c, ST_EIGEN);
        rc = k3_eig_candidates_units(c, U, prm->block_size, prm->quality_level);
    }
    if (rc) { (void)hipStreamWaitEvent(c->stream, ev[EV_JOIN], 0); return rc; }
    // ---- K5: ranking + greedy selection, every unit's chain side by side (pipelined: on the chain stream, beside the next submission's Laplacians)
    if (piped && ((rc = km_record(c, ev[EV_E_DONE], main_stream)) || (rc = km_wait(c, c->chain_stream, ev[EV_E_DONE])))) return rc;
    {
        km_on_stream on(c, piped ? c->chain_stream : main_stream);
        {
            km_stage_timer t(c, ST_SELECT);
            rc = kf_rank_select_units(c, U, prm->max_corners, prm->quality_level, prm->min_distance, cap);
        }
        if (piped && rc == KM_OK) rc = km_record(c, ev[EV_C_DONE], c->chain_stream);
    }
    if (rc) { (void)hipStreamWaitEvent(c->stream, ev[EV_JOIN], 0); return rc; }
    // ---- the tail: LK, frame stage, scores, copy-out - now, or with the next submission
    km_units_tail &T = *c->utail;
    T.lane = lane; T.slot = k; T.U = U; T.prm = *prm; T.n = n; T.n_max = n_max; T.cap = cap; T.dtype = dtype;
    T.with_zncc = with_zncc; T.with_mi = with_mi; T.with_clip = with_clip; T.piped = piped; T.zncc_threshold = zncc_threshold; T.profile_skip = c->profile_skip;
    T.L = L; T.d_out = d_out; T.seeded = priors != nullptr;
    T.sink = c->frame_sink; T.sink_pitch = c->frame_sink_pitch;
    slot->sunk_valid = false;
    if (piped) {
        T.armed = true;
        slot->deferred.store(1, std::memory_order_release);
    } else if ((rc = units_tail(c, T)))
        return rc;
    frame_slot_commit(c, k, ticket);
    return KM_OK;
}
