// Tile entry points of libkarios_hip.so: the device-resident KLT tile pipeline (KLT._match_tile, klt.py:236-349: stretch -> Laplacians -> mask
// -> goodFeaturesToTrack -> LK forward / backward), the frame forms (FB test, score, (x0, y0) order and the score columns in the same
// device call) and the asynchronous submission.  Batched units: api_units.hip; the kernel-size search: api_auto.hip; the frame block's
// slots and its way out: api_frame.hip.
#include "api_internal.hpp"
#include "k_prior.hpp"

#include <cmath>
#include <cstring>

// pyramid of one image into caller-provided storage (levels >= 1 packed from `store`); returns the bytes used
int build_pyramid_single(km_ctx *c, const uint8_t *d_img, int H, int W, int win, int max_level, uint8_t *store, km_pyr *P, size_t *used)
{
    P->img[0] = d_img; P->H[0] = H; P->W[0] = W; P->levels = 0;
    if (max_level > 4) max_level = 4;
    size_t off = 0;
    int w = W, h = H;
    for (int l = 1; l <= max_level; l++) {
        const int nw = (w + 1) / 2, nh = (h + 1) / 2;
        if (nw <= win || nh <= win) break;
        if (store) {
            int rc = kd_pyrdown_u8(c, P->img[l - 1], h, w, store + off);
            if (rc) return rc;
            P->img[l] = store + off;
        }
        P->H[l] = nh; P->W[l] = nw; P->levels = l;
        off += ((size_t)nw * nh + 255) & ~(size_t)255;
        w = nw; h = nh;
    }
    if (used) *used = off;
    return KM_OK;
}

// both pyramids of a pair, one launch per level
int build_pyramid_pair(km_ctx *c, const uint8_t *d_a, const uint8_t *d_b, int H, int W, int win, int max_level, km_pyr *A, km_pyr *B)
{
    A->img[0] = d_a; B->img[0] = d_b;
    A->H[0] = B->H[0] = H; A->W[0] = B->W[0] = W; A->levels = B->levels = 0;
    if (max_level > 4) max_level = 4;
    size_t total = 0;
    int w = W, h = H, nl = 0;
    int hs[5], wsz[5];
    for (int l = 0; l < max_level; l++) {
        const int nw = (w + 1) / 2, nh = (h + 1) / 2;
        if (nw <= win || nh <= win) break;
        nl = l + 1; hs[nl] = nh; wsz[nl] = nw;
        total += ((size_t)nw * nh + 255) & ~(size_t)255;
        w = nw; h = nh;
    }
    if (nl == 0) return KM_OK;
    uint8_t *ba = (uint8_t *)km_ws(c, WS_PYR_A, total), *bb = (uint8_t *)km_ws(c, WS_PYR_B, total);
    if (!ba || !bb) return KM_E_NOMEM;
    size_t off = 0;
    for (int l = 1; l <= nl; l++) {
        int rc = kd_pyrdown_u8_pair(c, A->img[l - 1], B->img[l - 1], A->H[l - 1], A->W[l - 1], ba + off, bb + off);
        if (rc) return rc;
        A->img[l] = ba + off; B->img[l] = bb + off;
        A->H[l] = B->H[l] = hs[l]; A->W[l] = B->W[l] = wsz[l];
        off += ((size_t)wsz[l] * hs[l] + 255) & ~(size_t)255;
    }
    A->levels = B->levels = nl;
    return KM_OK;
}

// goodFeaturesToTrack on a dense device u8 image.  Leaves the corner count in scalars->n_corners
// (device) and the corner list in d_xy.  One host sync (candidate count).
int gftt_dev(km_ctx *c, const uint8_t *d_img, const uint8_t *d_mask, int H, int W, int max_corners, double quality,
                    double min_distance, int block, float *d_xy, int cap, km_scalars *sc)
{
    int rc;
    // Strongest-first shortcut: rank and select on the top slice only (a rank prefix, so a sufficient slice gives the
    // exact result); fall back to the complete list when that slice cannot supply maxCorners corners.
    size_t k_target = (max_corners > 0 && min_distance >= 1) ? (size_t)max_corners * (c->opt_topk_factor > 0 ? c->opt_topk_factor : 8) : 0;
    size_t capk = (size_t)H * W / 8 + 4096 * KM_NSHARD;
    if (c->opt_key_cap > 0) capk = (size_t)c->opt_key_cap * KM_NSHARD;   // test knob: tiny shards, so that the regrow path runs
    unsigned long long *kept = nullptr;
    size_t nkept = 0, ntotal = 0;
    km_scalars hs;
    bool fused_overflow = false;   // a row group overflowed the fused kernel's candidate stage (plateau image): use the two-kernel path
    for (int attempt = 0; attempt < 4; attempt++) {
        unsigned long long *keys = (unsigned long long *)km_ws(c, WS_KEYS0, capk * sizeof(unsigned long long));
        if (!keys) return KM_E_NOMEM;
        // K3 + K4 fused (2 pixels per lane, no eig map: k_eig2.hip) when it covers the case, else eig map + candidate kernel.
        // km_set_option("fused_eig", 0) selects the two-kernel path.
        bool fused = false;
        if (c->fused_eig && !fused_overflow) {
            km_stage_timer t(c, ST_EIGEN);
            rc = k2_eig_candidates(c, d_img, d_mask, H, W, block, quality, sc, keys, capk, attempt > 0);
            if (rc == KM_OK) fused = true;
            else if (rc != KM_E_UNSUPPORTED) return rc;
        }
        if (!fused) {
            float *eig = (float *)km_ws(c, WS_EIG, (size_t)H * W * sizeof(float));
            if (!eig) return KM_E_NOMEM;
            {
                km_stage_timer t(c, ST_EIGEN);
                if ((rc = kd_min_eigen(c, d_img, d_mask, H, W, block, eig, &sc->max_eig_key))) return rc;
            }
            {
                km_stage_timer t(c, ST_CANDIDATES);
                if ((rc = kd_candidates(c, eig, d_mask, H, W, quality, sc, keys, capk, attempt > 0))) return rc;
            }
        }
        {
            km_stage_timer t(c, ST_SORT);
            if ((rc = ks_topk_prefilter(c, keys, capk, k_target, sc, quality, &kept, &nkept, &ntotal, &hs, attempt > 0))) return rc;
        }
        stats_from_scalars(c, hs, KS_VALID);
        if (fused && hs.pad0 != 0u) {   // candidates were dropped: repeat with the eig-map + candidate kernels
            fused_overflow = true;
            c->stats.path_flags |= KM_PATH_STAGE_FALLBACK;
            KM_HIP(c, hipMemsetAsync(&sc->run_max_key, 0, (2 + KM_NSHARD) * sizeof(unsigned), c->stream));
            continue;
        }
        if ((size_t)hs.n_cand <= capk) break;
        capk = (size_t)hs.n_cand + hs.n_cand / 4 + 4096 * KM_NSHARD;   // a shard overflowed: grow the key buffer and redo
        c->stats.path_flags |= KM_PATH_KEY_REGROW;
        if (attempt == 3) return km_fail(c, KM_E_INTERNAL, "candidate buffer kept overflowing");
    }
    c->stats.n_candidates = (int64_t)ntotal;
    c->stats.emitted_ratio = ntotal ? (float)((double)hs.n_cand / (double)ntotal) : 0.f;
    unsigned long long *keys = (unsigned long long *)c->ws[WS_KEYS0].p;
    for (int pass = 0; pass < 2; pass++) {
        unsigned long long *sorted = kept;
        if (nkept > 0) {
            km_stage_timer t(c, ST_SORT);
            if ((rc = ks_sort_keys_desc(c, kept, nkept, &sorted))) return rc;
        }
        int found = -1;
        {
            km_stage_timer t(c, ST_SELECT);
            if ((rc = ks_select(c, sorted, nkept, H, W, max_corners, min_distance, d_xy, cap, sc, nkept < ntotal ? &found : nullptr, pass == 0))) return rc;
        }
        if (nkept >= ntotal || found >= max_corners) break;
        // the top slice did not contain maxCorners mutually distant corners: repeat on every candidate
        k_target = 0;
        c->stats.path_flags |= KM_PATH_SECOND_PASS;
        km_scalars hs2;
        if ((rc = ks_topk_prefilter(c, keys, capk, 0, sc, quality, &kept, &nkept, &ntotal, &hs2, true))) return rc;
    }
    return KM_OK;
}

int read_stats(km_ctx *c, km_scalars *sc, km_call_modes *m)
{
    km_scalars h;
    KM_D2H(c, &h, sc, sizeof h);
    KM_FLUSH(c);
    c->stats.n_init = h.n_corners;
    c->stats.n_select_batches = h.n_batches;
    const bool spec = m && m->spec_used;   // the speculative corner path read nothing back on the way: its diagnostics arrive here
    stats_from_scalars(c, h, KS_TIES | (spec ? KS_VALID | KS_CANDIDATES : 0));
    if (spec) m->spec_flags = h.flags;
    if (h.n_cand == 0xffffffffu) return km_fail(c, KM_E_INTERNAL, "corner grid cell overflow");
    return KM_OK;
}

int mark_lk_start(km_ctx *c)
{
    int rc;
    if ((rc = km_event(c, &c->ev_lk_start)) || (rc = km_record(c, c->ev_lk_start, c->stream))) return rc;
    c->lk_start_valid = true;
    return KM_OK;
}

// klt_tracker numeric core on dense device u8 images (klt.py:103-142).  vjob: the valid-pixel sum the Laplacian pass left to this call (empty: none)
static int klt_track_dev(km_ctx *c, km_call_modes &m, km_valid_job vjob, const uint8_t *d_ref_lap, const uint8_t *d_mon_lap, const uint8_t *d_mask, int H,
                         int W, const km_klt_params *prm, const float *d_p0_in, int n_p0, float *d_p0, float *d_p1, float *d_p0r, int cap, km_scalars *sc)
{
    int rc;
    if (d_p0_in) {
        if (n_p0 > cap) return km_fail(c, KM_E_ARG, "p0 count %d exceeds capacity %d", n_p0, cap);
        if (n_p0 > 0 && d_p0_in != d_p0)
            KM_HIP(c, hipMemcpyAsync(d_p0, d_p0_in, (size_t)n_p0 * 2 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        { const int rch = h2d_now(c, &sc->n_corners, &n_p0, sizeof(int)); if (rch) return rch; }   // (n_p0 is a stack variable: staged)
    }
    km_pyr A, B;
    // Speculative corner path (k_select2.hip): no host synchronisation, fixed capacities, flags instead of retries.  The
    // caller reads sc->flags with the tile's result and repeats a flagged tile with spec_allowed = false.
    bool spec = !d_p0_in && m.spec_allowed && spec_path_covers(c, prm);
    if (!spec && (rc = kd_run_valid_sum(c, &vjob))) return rc;  // (... and the valid-pixel sum)
    if (spec) {
        const size_t capk = (size_t)H * W / 8 + 4096 * KM_NSHARD;
        unsigned long long *keys = (unsigned long long *)km_ws(c, WS_KEYS0, capk * sizeof(unsigned long long));
        if (!keys) return KM_E_NOMEM;
        // The pyramids depend on the Laplacians only: they run on a second stream, joined before LK.  Forked BEFORE the fused
        // eigenvalue pass ("aux_early", default): that kernel is bound by instruction issue at 3 waves per SIMD and leaves the
        // memory system idle, and the ranking / selection chain behind it (small latency-bound kernels) then has the GPU to itself;
        // forked behind it (round 2) the pyramids stretched the chain's one-workgroup kernels from 8 to 36 us.
        bool forked = false;
        auto fork_pyramids = [&]() -> int {
            int r;
            if ((r = km_aux_stream(c)) || (r = km_record(c, c->ev_fork, c->stream)) || (r = km_wait(c, c->aux_stream, c->ev_fork))) return r;
            km_on_stream on(c, c->aux_stream);
            if ((r = kd_run_valid_sum(c, &vjob))) return r;   // (the Laplacian pass's deferred valid-pixel sum: off the main stream)
            {
                km_stage_timer t(c, ST_PYRAMID);
                if ((r = build_pyramid_pair(c, d_ref_lap, d_mon_lap, H, W, prm->win_size, prm->max_level, &A, &B))) return r;
            }
            if ((r = km_record(c, c->ev_join, c->aux_stream))) return r;
            forked = true;
            return KM_OK;
        };
        km_eig_partials partials;   // per-wave maxima of the fused pass: the ranking's first launch reduces them itself
        {
            // (the stage's start event sits in front of the fork: recorded between the fork and the kernel it would let the pyramid
            // kernels take the compute units first, and the bracketed kernel would measure 0.48 instead of 0.33 ms)
            km_stage_timer t(c, ST_EIGEN);
            if (c->opt_aux_pyramid && c->opt_aux_early && (rc = fork_pyramids())) return rc;
            rc = k2_eig_candidates(c, d_ref_lap, d_mask, H, W, prm->block_size, prm->quality_level, sc, keys, capk, false, &partials);
        }
        if (rc == KM_E_UNSUPPORTED) {
            spec = false;
            if (forked) { KM_HIP(c, hipStreamWaitEvent(c->stream, c->ev_join, 0)); forked = false; }   // (the general path builds its own pyramids in the same buffers)
        } else if (rc) return rc;
        else {
            if (c->opt_aux_pyramid && !forked && (rc = fork_pyramids())) return rc;
            {
                km_stage_timer t(c, ST_SORT);
                rc = kf_rank(c, keys, capk, H, W, prm->max_corners, prm->quality_level, prm->min_distance, sc, partials);
            }
            if (rc == KM_OK) {
                km_stage_timer t(c, ST_SELECT);
                rc = kf_select(c, H, W, prm->max_corners, prm->min_distance, d_p0, cap, sc);
            }
            if (forked) KM_HIP(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));   // (whatever happens next reuses the pyramid buffers)
            if (rc == KM_E_UNSUPPORTED) {   // (grid too large for the fixed-slot cells: nothing irreversible was enqueued)
                spec = false;
                if ((rc = clear_corner_scalars(c, sc))) return rc;
            } else if (rc) return rc;
        }
        if (spec) {
            m.spec_used = true;
            if (!forked) {
                km_stage_timer t(c, ST_PYRAMID);
                if ((rc = build_pyramid_pair(c, d_ref_lap, d_mon_lap, H, W, prm->win_size, prm->max_level, &A, &B))) return rc;
            }
        }
    }
    if ((rc = kd_run_valid_sum(c, &vjob))) return rc;    // (a path that never forked the second stream)
    if (spec) {
        // corners, their count and the pyramids are enqueued
    } else if (d_p0_in) {
        km_stage_timer t(c, ST_PYRAMID);
        if ((rc = build_pyramid_pair(c, d_ref_lap, d_mon_lap, H, W, prm->win_size, prm->max_level, &A, &B))) return rc;
    } else {
        // the pyramids do not depend on the corners: they are queued as deferred jobs and fill the GPU during the two
        // host read-backs of the corner selection (km_wait_readback); whatever is left runs right after it
        c->deferred.clear();
        size_t pyr_bytes = 0;
        build_pyramid_single(c, d_ref_lap, H, W, prm->win_size, prm->max_level, nullptr, &A, &pyr_bytes);   // sizes only
        uint8_t *store_a = pyr_bytes ? (uint8_t *)km_ws(c, WS_PYR_A, pyr_bytes) : nullptr, *store_b = pyr_bytes ? (uint8_t *)km_ws(c, WS_PYR_B, pyr_bytes) : nullptr;
        if (pyr_bytes && (!store_a || !store_b)) return KM_E_NOMEM;
        B = A; B.img[0] = d_mon_lap;
        if (pyr_bytes) {                       // one job per image: one for each of the two read-backs
            c->deferred.push_back([=, &A]() -> int {
                km_stage_timer t(c, ST_PYRAMID);
                return build_pyramid_single(c, d_ref_lap, H, W, prm->win_size, prm->max_level, store_a, &A, nullptr);
            });
            c->deferred.push_back([=, &B]() -> int { return build_pyramid_single(c, d_mon_lap, H, W, prm->win_size, prm->max_level, store_b, &B, nullptr); });
        }
        rc = gftt_dev(c, d_ref_lap, d_mask, H, W, prm->max_corners, prm->quality_level, prm->min_distance, prm->block_size, d_p0, cap, sc);
        const int rc2 = rc ? (c->deferred.clear(), rc) : km_run_deferred(c);
        if (rc2) return rc2;
    }
    const int n_max = d_p0_in ? n_p0 : corner_limit(prm, cap);
    {
        km_stage_timer t(c, ST_LK);
        if (spec && !c->lk_start_valid) {
            // (the next unit's early min / max starts here: beside LK - in front of the selection sweeps, the ranking or behind LK it
            // measured slower, CHANGELOG.md round 4)
            if ((rc = mark_lk_start(c))) return rc;
        }
        if (m.seed) rc = kl_track_seeded(c, A, B, d_p0, &sc->n_corners, n_max, prm->win_size, prm->max_count, prm->epsilon, true, d_p1, d_p0r, *m.seed);
        else rc = kl_track(c, A, B, d_p0, &sc->n_corners, n_max, prm->win_size, prm->max_count, prm->epsilon, true, d_p1, d_p0r);
        if (rc) return rc;
    }
    return KM_OK;
}

int check_params(km_ctx *c, const km_klt_params *p)
{
    if (!p) return km_fail(c, KM_E_ARG, "null params");
    if (p->block_size < 1) return km_fail(c, KM_E_ARG, "blockSize %d < 1", p->block_size);
    if (p->win_size <= 2) return km_fail(c, KM_E_ARG, "winSize %d must be > 2", p->win_size);
    if (p->max_level < 0) return km_fail(c, KM_E_ARG, "maxLevel %d < 0", p->max_level);
    if (!(p->quality_level > 0)) return km_fail(c, KM_E_ARG, "qualityLevel must be > 0");
    if (p->min_distance < 0) return km_fail(c, KM_E_ARG, "minDistance must be >= 0");
    return KM_OK;
}

int tile_call_begin(km_ctx *c, const char *who, const km_klt_params *prm, const void *ref, const void *mon, int H, int W, ptrdiff_t sref, ptrdiff_t smon)
{
    int rc;
    if ((rc = begin_call(c, RESET_KLT)) || (rc = check_params(c, prm)) || (rc = check_image(c, ref, H, W, sref, who)) || (rc = check_image(c, mon, H, W, smon, who)))
        return rc;
    return KM_OK;
}

int check_dtype(km_ctx *c, const char *who, int dtype) { return km_dtype_size(dtype) ? KM_OK : km_fail(c, KM_E_ARG, "%s: bad dtype %d", who, dtype); }

// the frame's (x0, y0) ordering buckets the rows by tile column (k_frame.hip: x0 - x_off < 65536); wider tiles are refused, not mis-ordered
int check_frame_width(km_ctx *c, const char *who, const char *what, int W)
{
    return W <= 65535 ? KM_OK : km_fail(c, KM_E_ARG, "%s: %s of %d columns (the device-side frame ordering holds at most 65535)", who, what, W);
}

int check_capacity(km_ctx *c, const km_klt_params *prm, int cap)
{
    return prm->max_corners > 0 && cap < prm->max_corners ? km_fail(c, KM_E_ARG, "capacity %d < maxCorners %d", cap, prm->max_corners) : KM_OK;
}

int dense_mask(km_ctx *c, const uint8_t *d_mask, ptrdiff_t smask, int H, int W, const uint8_t **dense)
{
    *dense = d_mask;
    if (smask == W) return KM_OK;
    // box of a larger resident mask: the kernels index masks densely, so pack the box first (1 B/px copy)
    if (smask < W) return km_fail(c, KM_E_ARG, "mask stride %td < width %d", smask, W);
    uint8_t *packed = (uint8_t *)km_ws(c, WS_MASK, (size_t)H * W);
    if (!packed) return KM_E_NOMEM;
    KM_HIP(c, hipMemcpy2DAsync(packed, (size_t)W, d_mask, (size_t)smask, (size_t)W, (size_t)H, hipMemcpyDeviceToDevice, c->stream));
    *dense = packed;
    return KM_OK;
}

static int klt_tile_dev_impl(km_ctx *c, km_call_modes &m, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon,
                             const uint8_t *d_mask, ptrdiff_t smask, const double *nodata_ref, const double *nodata_mon, const km_klt_params *prm,
                             float *d_p0, float *d_p1, float *d_p0r, int cap, km_scalars *sc)
{
    int rc;
    const size_t n = (size_t)H * W;
    uint8_t *lap_ref = (uint8_t *)km_ws(c, WS_U8_A, n), *lap_mon = (uint8_t *)km_ws(c, WS_U8_B, n);
    if (!lap_ref || !lap_mon) return KM_E_NOMEM;
    uint8_t *mask_auto = nullptr;
    if (!d_mask) { mask_auto = (uint8_t *)km_ws(c, WS_MASK, n); if (!mask_auto) return KM_E_NOMEM; }
    else if ((rc = dense_mask(c, d_mask, smask, H, W, &d_mask))) return rc;
    const double *mm = sc->mm;
    km_valid_job vjob;
    if (dtype != KM_U8 && m.mm_early_allowed && c->opt_mm_early && c->lk_start_prev && c->aux_stream) {
        // Early min / max: K1 of THIS unit does not queue behind the tail of the previous one (LK, FB test, ZNCC - instruction-bound
        // kernels of short-lived waves that leave HBM idle) but starts on the second stream the moment the previous unit's LK launch
        // starts, and streams the two rasters beside it.  The previous tile call of this context recorded ev_lk_start; if the GPU is
        // already past it, the kernel simply runs at once.  Result and partials live in slots of their own (the scalar block is
        // zeroed on the main stream at the start of every call, WS_PARTIAL belongs to the kernels of the unit still running).
        double *mm_early = (double *)km_ws(c, WS_MM_EARLY, 4 * sizeof(double));
        if (!mm_early) return KM_E_NOMEM;
        if ((rc = km_event(c, &c->ev_mm)) || (rc = km_wait(c, c->aux_stream, c->ev_lk_start))) return rc;
        {
            km_on_stream on(c, c->aux_stream);
            {
                km_stage_timer t(c, ST_MINMAX);
                if ((rc = kd_minmax(c, d_ref, dtype, H, W, sref, mm_early, d_mon, smon, WS_MM_PARTIAL))) return rc;
            }
            if ((rc = km_record(c, c->ev_mm, c->aux_stream))) return rc;
        }
        if ((rc = km_wait(c, c->stream, c->ev_mm))) return rc;
        mm = mm_early;
        c->stats.path_flags |= KM_PATH_MM_EARLY;
    } else if (dtype != KM_U8) {
        km_stage_timer t(c, ST_MINMAX);
        if ((rc = kd_minmax(c, d_ref, dtype, H, W, sref, &sc->mm[0], d_mon, smon))) return rc;
    }   // (u8 input: mm stays 0 from the scalar block the entry point zeroed)
    {
        km_stage_timer t(c, ST_LAPLACIAN);
        if (d_mask) { if ((rc = kd_count_nonzero(c, d_mask, n, &sc->valid))) return rc; }
        // on the sync-free path with the pyramids on a second stream the valid-pixel sum goes there too (klt_track_dev launches it)
        const bool defer = c->opt_defer_valid && c->opt_aux_pyramid && m.spec_allowed && spec_path_covers(c, prm);
        if ((rc = kd_stretch_laplacian_pair(c, d_ref, d_mon, dtype, H, W, sref, smon, mm, prm->ksize_ref, prm->ksize_mon, prm->invert_mon, nodata_ref,
                                            nodata_mon, lap_ref, lap_mon, mask_auto, &sc->valid, defer ? &vjob : nullptr)))
            return rc;
    }
    // "No valid pixels" (klt.py:276-279) needs no early exit: an all-zero mask gives max-eig 0, no candidate, no corner.
    // The count itself reaches the host with the candidate count (gftt_dev), i.e. without an extra synchronisation.
    return klt_track_dev(c, m, vjob, lap_ref, lap_mon, d_mask ? d_mask : mask_auto, H, W, prm, nullptr, 0, d_p0, d_p1, d_p0r, cap, sc);
}

static int fetch_tracks(km_ctx *c, km_call_modes &m, km_scalars *sc, const float *d_p0, const float *d_p1, const float *d_p0r, float *p0, float *p1,
                        float *p0r, int cap, int *out_n)
{
    int rc;
    if ((rc = read_stats(c, sc, &m))) return rc;
    int n = c->stats.n_init;
    if (n > cap) return km_fail(c, KM_E_ARG, "%d corners exceed capacity %d", n, cap);
    if (n > 0) {
        const size_t b = (size_t)n * 2 * sizeof(float);
        KM_D2H(c, p0, d_p0, b);
        KM_D2H(c, p1, d_p1, b);
        KM_D2H(c, p0r, d_p0r, b);
        KM_FLUSH(c);
    }
    *out_n = n;
    return KM_OK;
}

extern "C" {

int km_klt_track(km_ctx *c, const uint8_t *ref_lap, const uint8_t *mon_lap, const uint8_t *mask, int H, int W, const km_klt_params *prm,
                 const float *p0_in, int n_p0, float *p0, float *p1, float *p0r, int cap, int *out_n)
{
    int rc;
    if ((rc = tile_call_begin(c, "klt_track", prm, ref_lap, mon_lap, H, W, W, W))) return rc;
    if (!p0 || !p1 || !p0r || !out_n || cap <= 0) return km_fail(c, KM_E_ARG, "klt_track: null output");
    if (!p0_in && (rc = check_capacity(c, prm, cap))) return rc;
    memset(&c->stats, 0, sizeof c->stats);
    void *d_ref, *d_mon, *d_mask = nullptr;
    if ((rc = upload_image(c, WS_U8_A, ref_lap, 1, H, W, W, &d_ref)) || (rc = upload_image(c, WS_U8_B, mon_lap, 1, H, W, W, &d_mon))) return rc;
    if (mask && (rc = upload_image(c, WS_MASK_IN, mask, 1, H, W, W, &d_mask))) return rc;
    km_scalars *sc = scalars(c);
    const size_t pb = (size_t)cap * 2 * sizeof(float);
    float *d_p0 = (float *)km_ws(c, WS_PTS0, pb), *d_p1 = (float *)km_ws(c, WS_PTS1, pb), *d_p0r = (float *)km_ws(c, WS_PTS2, pb);
    if (!sc || !d_p0 || !d_p1 || !d_p0r) return KM_E_NOMEM;
    KM_HIP(c, hipMemsetAsync(sc, 0, sizeof *sc, c->stream));
    const float *d_p0_in = nullptr;
    if (p0_in) {
        if (n_p0 < 0 || n_p0 > cap) return km_fail(c, KM_E_ARG, "klt_track: p0 count %d (capacity %d)", n_p0, cap);
        if (n_p0 > 0) { const int rch = h2d_now(c, d_p0, p0_in, (size_t)n_p0 * 2 * sizeof(float)); if (rch) return rch; }
        d_p0_in = d_p0;
    }
    km_call_modes m;
    if ((rc = klt_track_dev(c, m, km_valid_job(), (const uint8_t *)d_ref, (const uint8_t *)d_mon, (const uint8_t *)d_mask, H, W, prm, d_p0_in, n_p0, d_p0,
                            d_p1, d_p0r, cap, sc)))
        return rc;
    return fetch_tracks(c, m, sc, d_p0, d_p1, d_p0r, p0, p1, p0r, cap, out_n);
}

int km_klt_tile(km_ctx *c, const void *ref, const void *mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon, const uint8_t *mask,
                const double *nodata_ref, const double *nodata_mon, const km_klt_params *prm, float *p0, float *p1, float *p0r, int cap,
                int *out_n)
{
    int rc;
    if ((rc = tile_call_begin(c, "klt_tile", prm, ref, mon, H, W, sref, smon)) || (rc = check_dtype(c, "klt_tile", dtype))) return rc;
    const size_t es = km_dtype_size(dtype);
    if (!p0 || !p1 || !p0r || !out_n || cap <= 0) return km_fail(c, KM_E_ARG, "klt_tile: null output");
    if ((rc = check_capacity(c, prm, cap))) return rc;
    memset(&c->stats, 0, sizeof c->stats);
    void *d_ref, *d_mon, *d_mask = nullptr;
    if ((rc = upload_image(c, WS_RAW_A, ref, es, H, W, sref, &d_ref)) || (rc = upload_image(c, WS_RAW_B, mon, es, H, W, smon, &d_mon))) return rc;
    if (mask && (rc = upload_image(c, WS_MASK_IN, mask, 1, H, W, W, &d_mask))) return rc;
    km_scalars *sc = scalars(c);
    const size_t pb = (size_t)cap * 2 * sizeof(float);
    float *d_p0 = (float *)km_ws(c, WS_PTS0, pb), *d_p1 = (float *)km_ws(c, WS_PTS1, pb), *d_p0r = (float *)km_ws(c, WS_PTS2, pb);
    if (!sc || !d_p0 || !d_p1 || !d_p0r) return KM_E_NOMEM;
    for (int attempt = 0; attempt < 2; attempt++) {
        KM_HIP(c, hipMemsetAsync(sc, 0, sizeof *sc, c->stream));
        km_call_modes m;
        m.spec_allowed = attempt == 0;
        if ((rc = klt_tile_dev_impl(c, m, d_ref, d_mon, dtype, H, W, W, W, (const uint8_t *)d_mask, W, nodata_ref, nodata_mon, prm, d_p0, d_p1, d_p0r, cap, sc)))
            return rc;
        if ((rc = fetch_tracks(c, m, sc, d_p0, d_p1, d_p0r, p0, p1, p0r, cap, out_n))) return rc;
        (void)verify_upload(c, "end of km_klt_tile (ref)", WS_RAW_A, ref, es, H, W, sref, d_ref);
        (void)verify_upload(c, "end of km_klt_tile (mon)", WS_RAW_B, mon, es, H, W, smon, d_mon);
        if (!(m.spec_used && m.spec_flags)) break;         // flagged speculative run: once more through the exact path
        memset(&c->stats, 0, sizeof c->stats);
        c->stats.path_flags |= KM_PATH_SPEC_RETRY;
    }
    return KM_OK;
}

// KLT._match_tile pre-filter on host buffers: uint8 stretch + Laplacian of both images and the automatic mask in the
// fused kernel the tile path uses (klt.py:268-273, 407-436).  out_mask may be null (then no mask is derived).
int km_tile_prefilter(km_ctx *c, const void *ref, const void *mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon,
                      const double *nodata_ref, const double *nodata_mon, int ksize_ref, int ksize_mon, int invert_mon, uint8_t *out_lap_ref,
                      uint8_t *out_lap_mon, uint8_t *out_mask, int64_t *out_valid)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, ref, H, W, sref, "tile_prefilter")) || (rc = check_image(c, mon, H, W, smon, "tile_prefilter")))
        return rc;
    const size_t es = km_dtype_size(dtype);
    if (!es) return km_fail(c, KM_E_ARG, "tile_prefilter: bad dtype %d", dtype);
    if (!out_lap_ref || !out_lap_mon) return km_fail(c, KM_E_ARG, "tile_prefilter: null output");
    void *d_ref, *d_mon;
    if ((rc = upload_image(c, WS_RAW_A, ref, es, H, W, sref, &d_ref)) || (rc = upload_image(c, WS_RAW_B, mon, es, H, W, smon, &d_mon))) return rc;
    const size_t n = (size_t)H * W;
    km_scalars *sc = scalars(c);
    uint8_t *lap_ref = (uint8_t *)km_ws(c, WS_U8_A, n), *lap_mon = (uint8_t *)km_ws(c, WS_U8_B, n);
    uint8_t *d_mask = out_mask ? (uint8_t *)km_ws(c, WS_MASK, n) : nullptr;
    if (!sc || !lap_ref || !lap_mon || (out_mask && !d_mask)) return KM_E_NOMEM;
    KM_HIP(c, hipMemsetAsync(sc, 0, sizeof *sc, c->stream));
    if (dtype != KM_U8) {
        if ((rc = kd_minmax(c, d_ref, dtype, H, W, W, &sc->mm[0])) || (rc = kd_minmax(c, d_mon, dtype, H, W, W, &sc->mm[2]))) return rc;
    }
    if ((rc = kd_stretch_laplacian_pair(c, d_ref, d_mon, dtype, H, W, W, W, sc->mm, ksize_ref, ksize_mon, invert_mon, nodata_ref, nodata_mon,
                                        lap_ref, lap_mon, d_mask, &sc->valid)))
        return rc;
    unsigned long long valid = 0;
    KM_D2H(c, out_lap_ref, lap_ref, n);
    KM_D2H(c, out_lap_mon, lap_mon, n);
    if (out_mask) {
        KM_D2H(c, out_mask, d_mask, n);
        KM_D2H(c, &valid, &sc->valid, sizeof valid);
    }
    KM_FLUSH(c);
    if (out_valid) *out_valid = out_mask ? (int64_t)valid : -1;
    return KM_OK;
}

int km_klt_tile_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon,
                    const uint8_t *d_mask, ptrdiff_t smask, const double *nodata_ref, const double *nodata_mon, const km_klt_params *prm, float *d_p0,
                    float *d_p1, float *d_p0r, int cap, int *d_n)
{
    int rc;
    if ((rc = tile_call_begin(c, "klt_tile_dev", prm, d_ref, d_mon, H, W, sref, smon)) || (rc = check_dtype(c, "klt_tile_dev", dtype))) return rc;
    if (!d_p0 || !d_p1 || !d_p0r || !d_n || cap <= 0) return km_fail(c, KM_E_ARG, "klt_tile_dev: null output");
    if ((rc = check_capacity(c, prm, cap))) return rc;
    memset(&c->stats, 0, sizeof c->stats);
    km_scalars *sc = scalars(c);
    if (!sc) return KM_E_NOMEM;
    KM_HIP(c, hipMemsetAsync(sc, 0, sizeof *sc, c->stream));
    km_call_modes m;           // (nobody reads this call's flags: the exact corner path)
    if ((rc = klt_tile_dev_impl(c, m, d_ref, d_mon, dtype, H, W, sref, smon, d_mask, smask, nodata_ref, nodata_mon, prm, d_p0, d_p1, d_p0r, cap, sc))) return rc;
    KM_HIP(c, hipMemcpyAsync(d_n, &sc->n_corners, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    return KM_OK;
}

// the score columns of a tile's frame block: ZNCC of the confident rows [and the two MI scores]
static int tile_frame_scores(km_ctx *c, const km_frame_layout &L, char *d_out, const void *d_ref_full, const void *d_mon_full, int dtype, int Hf, int Wf,
                             ptrdiff_t sref_f, ptrdiff_t smon_f, int n_max, double zncc_threshold, bool with_mi)
{
    int rc;
    km_score_unit s;
    {
        km_stage_timer t(c, ST_ZNCC);
        L.score_unit(s, d_out, false);
        if ((rc = kz_zncc_filtered(c, d_ref_full, d_mon_full, dtype, Hf, Wf, Hf, Wf, sref_f, smon_f, s.x0, s.y0, s.dx, s.dy, n_max, s.d_n, s.score,
                                   (float)zncc_threshold, s.out)))
            return rc;
    }
    if (with_mi) {
        // the other two scores of _handle_klt_results (core.py:894-907) for the same rows, behind ZNCC in the same call: the chips of
        // a key point (57 x 57, around the 43 x 43 ZNCC window) are still in the XCD's L2
        km_stage_timer t(c, ST_MI);
        L.score_unit(s, d_out, true);
        if ((rc = kmi_batch(c, d_ref_full, d_mon_full, dtype, Hf, Wf, Hf, Wf, sref_f, smon_f, s.x0, s.y0, s.dx, s.dy, n_max, s.d_n, s.score,
                            (float)zncc_threshold, s.out, s.out2)))
            return rc;
    }
    return KM_OK;
}

// a prior's 9 values: finite, or KM_E_ARG
static int check_prior(km_ctx *c, const char *who, const double *prior)
{
    if (!prior) return km_fail(c, KM_E_ARG, "%s: null prior", who);
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(prior[i])) return km_fail(c, KM_E_ARG, "%s: prior[%d] is not finite", who, i);
    return KM_OK;
}

// the two-level tracker serves an H x W box: its pyramid has a level 1 (build_pyramid_pair's rule) and the window fits the second form
static bool prior_tracker_covers(const km_ctx *c, int H, int W, int win, int max_level)
{
    return c->opt_lk2 && max_level == 1 && win > 2 && win <= 40 && (W + 1) / 2 > win && (H + 1) / 2 > win;
}

// prior != nullptr (km_klt_tile_frame_prior_dev): the corner mask is the prior's (k_prior.hip, taken by the
// pre-filter as a user mask) and the tracker starts every key point at its guess; everything else is the unseeded call's
static int tile_frame_impl(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon,
                           const uint8_t *d_mask, ptrdiff_t smask, const double *nodata_ref, const double *nodata_mon, const km_klt_params *prm, float x_off,
                           float y_off, const void *d_ref_full, const void *d_mon_full, int Hf, int Wf, ptrdiff_t sref_f, ptrdiff_t smon_f,
                           bool with_zncc, double zncc_threshold, void *host_out, int cap, km_frame_slot *slot = nullptr, const double *prior = nullptr)
{
    // slot != nullptr: km_klt_tile_frame_submit - the block goes to the slot's pinned buffer and the call returns without
    // waiting for the tail of the pipeline (LK, FB test, ZNCC, copy), which then overlaps the caller's next submission
    int rc;
    if ((rc = tile_call_begin(c, "klt_tile_frame_dev", prm, d_ref, d_mon, H, W, sref, smon))) return rc;
    if (with_zncc && ((rc = check_image(c, d_ref_full, Hf, Wf, sref_f, "klt_tile_frame_zncc_dev")) ||
                      (rc = check_image(c, d_mon_full, Hf, Wf, smon_f, "klt_tile_frame_zncc_dev"))))
        return rc;
    if ((rc = check_dtype(c, "klt_tile_frame_dev", dtype)) || (rc = check_frame_width(c, "klt_tile_frame_dev", "tile", W))) return rc;
    if ((!host_out && !slot) || cap <= 0) return km_fail(c, KM_E_ARG, "klt_tile_frame_dev: null output");
    if ((rc = check_capacity(c, prm, cap))) return rc;
    kl_seed seed;
    if (prior) {
        // what a prior does not serve is refused here, in front of the first launch
        if ((rc = check_prior(c, "klt_tile_frame_prior_dev", prior))) return rc;
        if (d_mask && smask < W) return km_fail(c, KM_E_ARG, "mask stride %td < width %d", smask, W);
        if (c->window.H) return km_fail(c, KM_E_UNSUPPORTED, "klt_tile_frame_prior_dev: an image window is set (km_set_image_window)");
        if (c->opt_frame_clip) return km_fail(c, KM_E_UNSUPPORTED, "klt_tile_frame_prior_dev: \"frame_clip\" is on (the clip under a prior runs on the residuals, behind the frame)");
        if (!prior_tracker_covers(c, H, W, prm->win_size, prm->max_level))
            return km_fail(c, KM_E_UNSUPPORTED, "klt_tile_frame_prior_dev: a prior needs the two-level tracker (box %d x %d, winSize %d, maxLevel %d)", W, H,
                           prm->win_size, prm->max_level);
        seed.guess = nullptr; memcpy(seed.P, prior, sizeof seed.P); seed.x_off = (double)x_off; seed.y_off = (double)y_off;
    }
    const bool with_clip = c->opt_frame_clip;
    if (with_clip && !frame_clip_covers(cap)) return km_fail(c, KM_E_UNSUPPORTED, "klt_tile_frame_dev: the outlier clip holds at most 32768 rows (capacity %d)", cap);
    memset(&c->stats, 0, sizeof c->stats);
    c->evs_used[c->ev_cur][ST_ZNCC] = false; c->evs_used[c->ev_cur][ST_MI] = false;
    km_scalars *sc = scalars(c);
    const size_t pb = (size_t)cap * 2 * sizeof(float);
    const bool with_mi = with_zncc && c->opt_frame_mi;
    const km_frame_layout L(cap, with_zncc, with_mi);
    const size_t ob = L.ob;
    float *d_p0 = (float *)km_ws(c, WS_PTS0, pb), *d_p1 = (float *)km_ws(c, WS_PTS1, pb), *d_p0r = (float *)km_ws(c, WS_PTS2, pb);
    char *d_out = (char *)km_ws(c, WS_FRAME, ob);
    if (!sc || !d_p0 || !d_p1 || !d_p0r || !d_out) return KM_E_NOMEM;
    if (prior) {
        uint8_t *pmask = (uint8_t *)km_ws(c, WS_MASK, (size_t)H * W);
        if (!pmask) return KM_E_NOMEM;
        kp_mask_args a;
        fill_mask_args(a, d_ref, d_mon, dtype, H, W, sref, smon, d_mask, smask, nodata_ref, nodata_mon, prior, (double)x_off, (double)y_off, pmask);
        if ((rc = kp_prior_mask(c, a))) return rc;
        d_mask = pmask; smask = W;
    }
    for (int attempt = 0;; attempt++) {
        KM_HIP(c, hipMemsetAsync(sc, 0, sizeof *sc, c->stream));
        // corners without a host synchronisation where the case allows it; header word 2 of the frame block carries the flags of
        // that speculative path: the synchronous variants repeat a flagged tile right here, a submitted one is repeated by the
        // caller that waits for it (karios_amd.resident)
        km_call_modes m;
        m.spec_allowed = attempt == 0;
        m.mm_early_allowed = slot != nullptr;     // (the synchronous forms report min / max in their statistics: scalar block)
        m.seed = prior ? &seed : nullptr;
        if ((rc = klt_tile_dev_impl(c, m, d_ref, d_mon, dtype, H, W, sref, smon, d_mask, smask, nodata_ref, nodata_mon, prm, d_p0, d_p1, d_p0r, cap, sc))) return rc;
        const int n_max = corner_limit(prm, cap);
        if ((rc = frame_block_free(c))) return rc;
        {
            km_stage_timer t(c, ST_FRAME);
            if ((rc = kf_frame(c, d_p0, d_p1, d_p0r, &sc->n_corners, n_max, cap, 0.1f, x_off, y_off, d_out, m.spec_used ? sc : nullptr, W))) return rc;
            if (with_clip && (rc = frame_blocks_clip(c, &d_out, 1, cap))) return rc;      // ("frame_clip": the scores are the survivors')
        }
        if (with_zncc && (rc = tile_frame_scores(c, L, d_out, d_ref_full, d_mon_full, dtype, Hf, Wf, sref_f, smon_f, n_max, zncc_threshold, with_mi))) return rc;
        if ((rc = frame_sink_check(c, 0, 1, ob))) return rc;      // (a single block ignores the sink's pitch)
        if (slot) {
            // the block leaves on a stream of its own: 13 us of DMA that the next submission's first kernels need not wait for
            // (the next frame is written into WS_FRAME ~1 ms later, behind a wait for this copy: see frame_block_free); the
            // device-side copy into the frame sink leaves there too: on the compute stream it cost the next unit 11 us
            if ((rc = frame_slot_reserve(c, slot, ob)) || (rc = km_block_stream(c))) return rc;
            return frame_blocks_out(c, slot, d_out, L, 1, c->frame_sink, 0, c->d2h_stream);
        }
        if (c->frame_sink) KM_HIP(c, hipMemcpyAsync(c->frame_sink, d_out, ob, hipMemcpyDeviceToDevice, c->stream));
        km_scalars *land = m.spec_used ? (km_scalars *)km_pinned_rb(c, sizeof(km_scalars)) : nullptr;
        if (land) KM_HIP(c, hipMemcpyAsync(land, sc, sizeof *land, hipMemcpyDeviceToHost, c->stream));   // diagnostics of the sync-free corner path
        KM_D2H(c, host_out, d_out, ob);
        KM_FLUSH(c);
        c->stats.n_init = L.header((const char *)host_out)[1];
        if (land) {
            stats_from_scalars(c, *land, KS_VALID | KS_CANDIDATES | KS_TIES);
            if (land->flags) {                                   // did not fit the fixed capacities: the exact path decides
                memset(&c->stats, 0, sizeof c->stats);
                c->stats.path_flags |= KM_PATH_SPEC_RETRY;
                continue;
            }
        }
        return KM_OK;
    }
}

int km_klt_tile_frame_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon,
                          const uint8_t *d_mask, ptrdiff_t smask, const double *nodata_ref, const double *nodata_mon, const km_klt_params *prm,
                          float x_off, float y_off, void *host_out, int cap)
{
    return tile_frame_impl(c, d_ref, d_mon, dtype, H, W, sref, smon, d_mask, smask, nodata_ref, nodata_mon, prm, x_off, y_off, nullptr, nullptr, 0, 0,
                           0, 0, false, 0.0, host_out, cap);
}

int km_klt_tile_frame_zncc_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon,
                               const uint8_t *d_mask, ptrdiff_t smask, const double *nodata_ref, const double *nodata_mon,
                               const km_klt_params *prm, float x_off, float y_off, const void *d_ref_full, const void *d_mon_full, int Hf,
                               int Wf, ptrdiff_t sref_f, ptrdiff_t smon_f, double zncc_threshold, void *host_out, int cap)
{
    return tile_frame_impl(c, d_ref, d_mon, dtype, H, W, sref, smon, d_mask, smask, nodata_ref, nodata_mon, prm, x_off, y_off, d_ref_full, d_mon_full,
                           Hf, Wf, sref_f, smon_f, true, zncc_threshold, host_out, cap);
}

int km_klt_tile_frame_prior_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon,
                                const uint8_t *d_mask, ptrdiff_t smask, const double *nodata_ref, const double *nodata_mon,
                                const km_klt_params *prm, float x_off, float y_off, const void *d_ref_full, const void *d_mon_full, int Hf,
                                int Wf, ptrdiff_t sref_f, ptrdiff_t smon_f, double zncc_threshold, const double prior[9], void *host_out, int cap)
{
    if (!c) return km_fail(nullptr, KM_E_ARG, "null context");
    if (!prior) return km_fail(c, KM_E_ARG, "klt_tile_frame_prior_dev: null prior");
    return tile_frame_impl(c, d_ref, d_mon, dtype, H, W, sref, smon, d_mask, smask, nodata_ref, nodata_mon, prm, x_off, y_off, d_ref_full, d_mon_full,
                           Hf, Wf, sref_f, smon_f, true, zncc_threshold, host_out, cap, nullptr, prior);
}

// rule 4 of DESIGN.md section 21 on device rasters; the mask stays on the device (dense rows), the work queued on the context stream
int km_prior_mask_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon, const uint8_t *d_base,
                      ptrdiff_t sbase, const double *nodata_ref, const double *nodata_mon, const double prior[9], double x_off, double y_off, uint8_t *d_mask)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, d_ref, H, W, sref, "prior_mask")) || (rc = check_image(c, d_mon, H, W, smon, "prior_mask")) ||
        (rc = check_dtype(c, "prior_mask", dtype)) || (rc = check_prior(c, "prior_mask", prior)))
        return rc;
    if (!d_mask) return km_fail(c, KM_E_ARG, "prior_mask: null output");
    if (d_base && sbase < W) return km_fail(c, KM_E_ARG, "prior_mask: mask stride %td < width %d", sbase, W);
    if (!std::isfinite(x_off) || !std::isfinite(y_off)) return km_fail(c, KM_E_ARG, "prior_mask: the origin is not finite");
    kp_mask_args a;
    fill_mask_args(a, d_ref, d_mon, dtype, H, W, sref, smon, d_base, sbase, nodata_ref, nodata_mon, prior, x_off, y_off, d_mask);
    return kp_prior_mask(c, a);
}

int km_prior_mask(km_ctx *c, const void *ref, const void *mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon, const uint8_t *base,
                  ptrdiff_t sbase, const double *nodata_ref, const double *nodata_mon, const double prior[9], double x_off, double y_off, uint8_t *mask)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, ref, H, W, sref, "prior_mask")) || (rc = check_image(c, mon, H, W, smon, "prior_mask")) ||
        (rc = check_dtype(c, "prior_mask", dtype)) || (rc = check_prior(c, "prior_mask", prior)))
        return rc;
    if (!mask) return km_fail(c, KM_E_ARG, "prior_mask: null output");
    if (base && sbase < W) return km_fail(c, KM_E_ARG, "prior_mask: mask stride %td < width %d", sbase, W);
    if (!std::isfinite(x_off) || !std::isfinite(y_off)) return km_fail(c, KM_E_ARG, "prior_mask: the origin is not finite");
    const size_t es = km_dtype_size(dtype), n = (size_t)H * W;
    void *d_ref, *d_mon, *d_base = nullptr;
    if ((rc = upload_image(c, WS_RAW_A, ref, es, H, W, sref, &d_ref)) || (rc = upload_image(c, WS_RAW_B, mon, es, H, W, smon, &d_mon))) return rc;
    if (base && (rc = upload_image(c, WS_MASK_IN, base, 1, H, W, sbase, &d_base))) return rc;
    uint8_t *d_mask = (uint8_t *)km_ws(c, WS_MASK, n);
    if (!d_mask) return KM_E_NOMEM;
    kp_mask_args a;
    fill_mask_args(a, d_ref, d_mon, dtype, H, W, W, W, (const uint8_t *)d_base, W, nodata_ref, nodata_mon, prior, x_off, y_off, d_mask);
    if ((rc = kp_prior_mask(c, a))) return rc;
    KM_D2H(c, mask, d_mask, n);
    KM_FLUSH(c);
    return KM_OK;
}

// cv2.calcOpticalFlowPyrLK with OPTFLOW_USE_INITIAL_FLOW: one direction, every point from its own guess
int km_pyrlk_initial(km_ctx *c, const uint8_t *prev, const uint8_t *next, int H, int W, const float *pts, const float *guess, int n, int win,
                     int max_level, int max_count, double epsilon, float *out_pts)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = check_image(c, prev, H, W, W, "pyrlk_initial")) || (rc = check_image(c, next, H, W, W, "pyrlk_initial"))) return rc;
    if (n < 0 || (n > 0 && (!pts || !guess || !out_pts))) return km_fail(c, KM_E_ARG, "pyrlk_initial: bad points");
    if (win <= 2 || max_level < 0) return km_fail(c, KM_E_ARG, "pyrlk_initial: winSize %d / maxLevel %d", win, max_level);
    for (int i = 0; i < 2 * n; i++)
        if (!std::isfinite(pts[i]) || !std::isfinite(guess[i])) return km_fail(c, KM_E_ARG, "pyrlk_initial: point %d is not finite", i / 2);
    if (max_level != 1 || win > 40) return km_fail(c, KM_E_UNSUPPORTED, "pyrlk_initial: winSize %d / maxLevel %d (the seeded tracker: maxLevel 1, winSize <= 40)", win, max_level);
    if (!prior_tracker_covers(c, H, W, win, max_level))
        return km_fail(c, KM_E_UNSUPPORTED, "pyrlk_initial: a %d x %d image has no pyramid level 1 at winSize %d (or \"lk2\" is off)", W, H, win);
    if (n == 0) return KM_OK;
    void *d_prev, *d_next;
    if ((rc = upload_image(c, WS_U8_A, prev, 1, H, W, W, &d_prev)) || (rc = upload_image(c, WS_U8_B, next, 1, H, W, W, &d_next))) return rc;
    float *d_in = (float *)km_ws(c, WS_PTS0, (size_t)n * 2 * sizeof(float));
    float *d_out = (float *)km_ws(c, WS_PTS1, (size_t)n * 2 * sizeof(float));
    float *d_guess = (float *)km_ws(c, WS_PTS2, (size_t)n * 2 * sizeof(float));
    if (!d_in || !d_out || !d_guess) return KM_E_NOMEM;
    { const int rch = h2d_now(c, d_in, pts, (size_t)n * 2 * sizeof(float)); if (rch) return rch; }
    { const int rch = h2d_now(c, d_guess, guess, (size_t)n * 2 * sizeof(float)); if (rch) return rch; }
    km_pyr A, B;
    if ((rc = build_pyramid_pair(c, (const uint8_t *)d_prev, (const uint8_t *)d_next, H, W, win, max_level, &A, &B))) return rc;
    kl_seed seed;
    memset(&seed, 0, sizeof seed);
    seed.guess = d_guess;
    if ((rc = kl_track_seeded(c, A, B, d_in, nullptr, n, win, max_count, epsilon, false, d_out, nullptr, seed))) return rc;
    KM_D2H(c, out_pts, d_out, (size_t)n * 2 * sizeof(float));
    KM_FLUSH(c);
    return KM_OK;
}

// Asynchronous form of km_klt_tile_frame[_zncc]_dev for a stream of tiles / band pairs: returns as soon as the last
// kernel and the copy of the frame block are ENQUEUED (the corner selection still synchronises inside), so the caller's
// next submission queues its dense stages right behind this frame's tail and the GPU never idles between frames.
// km_frame_wait (any thread) blocks until frame `ticket` is complete and hands out its block in pinned host memory, valid
// until KM_FRAME_SLOTS further submissions.  d_ref_full == NULL: no ZNCC column.
int km_klt_tile_frame_submit(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon,
                             const uint8_t *d_mask, ptrdiff_t smask, const double *nodata_ref, const double *nodata_mon,
                             const km_klt_params *prm, float x_off, float y_off, const void *d_ref_full, const void *d_mon_full, int Hf,
                             int Wf, ptrdiff_t sref_f, ptrdiff_t smon_f, double zncc_threshold, int cap, int *ticket)
{
    if (!c) return km_fail(nullptr, KM_E_ARG, "null context");
    if (!ticket) return km_fail(c, KM_E_ARG, "klt_tile_frame_submit: null ticket");
    int k;
    km_frame_slot *slot;
    int rc = frame_slot_claim(c, nullptr, &k, &slot);
    if (rc) return rc;
    rc = tile_frame_impl(c, d_ref, d_mon, dtype, H, W, sref, smon, d_mask, smask, nodata_ref, nodata_mon, prm, x_off, y_off, d_ref_full,
                                   d_mon_full, Hf, Wf, sref_f, smon_f, d_ref_full != nullptr, zncc_threshold, nullptr, cap, slot);
    c->ev_cur = 0;
    if (rc) return rc;
    frame_slot_commit(c, k, ticket);
    return KM_OK;
}
}  // extern "C"
