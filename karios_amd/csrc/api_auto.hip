// The kernel-size search of libkarios_hip.so, km_klt_auto_ksize_frame_dev, as a sequence of stages over one table (auto_search).
// KLT._match_tile_auto_ksize (klt.py:465-545) on resident data: every Laplacian, pyramid and corner list is built ONCE
// and stays on the device; the nk*nk tracker runs reuse them.  Best pair = highest inlier ratio, first wins ties, in
// itertools.product order (mon outer, ref inner).
#include "api_internal.hpp"

#include <cstring>

// the search's tables: what the stages hand to each other
struct auto_search {
    int nk = 0, H = 0, W = 0, cap = 0, n_lim = 0;
    const int *ksizes = nullptr;
    const km_klt_params *prm = nullptr;
    // scalar blocks: [0] the call's own (min / max, valid pixels, the exact corner path), [1 + k] the corner detection of reference kernel k
    char *sc_base = nullptr;
    size_t sc_stride = 0;
    km_scalars *sc = nullptr;
    const uint8_t *mask = nullptr;
    uint8_t *mask_auto = nullptr;      // the automatic mask: the FIRST Laplacian pass derives it from the raw rasters
    km_auto_arena a;
    uint8_t *arena = nullptr;
    int pyr_levels = 0;                // of the box at the call's window and maxLevel
    km_pyr PR[8], PM[8];
    int n_p0[8];                       // corners of reference kernel k, on the host ...
    const int *d_np0[8];               // ... and the device word holding them
    int *d_counts = nullptr;           // [nk] corners per ref kernel, [nk*nk] kept tracks

    km_scalars *unit_sc(int k) const { return (km_scalars *)(sc_base + sc_stride * (size_t)(k + 1)); }
    uint8_t *lap_ref(int k) const { return arena + a.lap_ref + (size_t)k * a.na; }
    uint8_t *lap_mon(int k) const { return arena + a.lap_mon + (size_t)k * a.na; }
    uint8_t *pyr_ref(int k) const { return arena + a.pyr + (size_t)(2 * k) * a.pyr_bytes; }
    uint8_t *pyr_mon(int k) const { return arena + a.pyr + (size_t)(2 * k + 1) * a.pyr_bytes; }
    float *p0(int k) const { return (float *)(arena + a.p0 + (size_t)k * a.pts); }
    float *p1(int combo) const { return (float *)(arena + a.trk + (size_t)(2 * combo) * a.pts); }
    float *p0r(int combo) const { return (float *)(arena + a.trk + (size_t)(2 * combo + 1) * a.pts); }
};

// ---- mask: the user's (packed to the box) - or the automatic one, which the FIRST Laplacian pass below derives from the raw rasters;
// min / max of both rasters
static int auto_mask_minmax(km_ctx *c, auto_search &S, const void *d_ref, const void *d_mon, int dtype, ptrdiff_t sref, ptrdiff_t smon, const uint8_t *d_mask,
                            ptrdiff_t smask)
{
    int rc;
    const size_t n = (size_t)S.H * S.W;
    if (!d_mask) {
        S.mask_auto = (uint8_t *)km_ws(c, WS_MASK, n);
        if (!S.mask_auto) return KM_E_NOMEM;
        S.mask = S.mask_auto;
    } else {
        if ((rc = dense_mask(c, d_mask, smask, S.H, S.W, &S.mask)) || (rc = kd_count_nonzero(c, S.mask, n, &S.sc->valid))) return rc;
    }
    if (dtype != KM_U8) {
        km_stage_timer t(c, ST_MINMAX);
        if ((rc = kd_minmax(c, d_ref, dtype, S.H, S.W, sref, &S.sc->mm[0], d_mon, smon))) return rc;
    }
    return KM_OK;
}

// ---- arena: 2*nk Laplacians, 2*nk pyramids, nk corner lists, nk*nk track pairs, counters
static int auto_arena(km_ctx *c, auto_search &S)
{
    km_pyr probe;
    size_t pyr_bytes = 0;
    build_pyramid_single(c, nullptr, S.H, S.W, S.prm->win_size, S.prm->max_level, nullptr, &probe, &pyr_bytes);
    S.pyr_levels = probe.levels;
    S.a = km_auto_arena_of(S.nk, S.H, S.W, pyr_bytes, S.cap);
    S.arena = (uint8_t *)km_ws(c, WS_AUTO, S.a.total);
    if (!S.arena) return KM_E_NOMEM;
    S.d_counts = (int *)(S.arena + S.a.counts);
    KM_HIP(c, hipMemsetAsync(S.d_counts, 0, (size_t)(S.nk + S.nk * S.nk) * sizeof(int), c->stream));
    return KM_OK;
}

static int auto_laplacians(km_ctx *c, auto_search &S, const void *d_ref, const void *d_mon, int dtype, ptrdiff_t sref, ptrdiff_t smon, const double *nodata_ref,
                           const double *nodata_mon)
{
    // the uint8 stretch (klt.py:42-49; [+ 255 - x, klt.py:419]) rides in every Laplacian pass, as in the tile pipeline: both images
    // of a kernel size in ONE launch from the raw rasters - the marching kernel for k <= 7; no uint8 copies of the rasters exist
    km_stage_timer t(c, ST_LAPLACIAN);
    for (int k = 0; k < S.nk; k++) {
        const bool first = k == 0 && S.mask_auto != nullptr;
        const int rc = kd_stretch_laplacian_pair(c, d_ref, d_mon, dtype, S.H, S.W, sref, smon, S.sc->mm, S.ksizes[k], S.ksizes[k], S.prm->invert_mon, nodata_ref,
                                                 nodata_mon, S.lap_ref(k), S.lap_mon(k), first ? S.mask_auto : nullptr, first ? &S.sc->valid : nullptr);
        if (rc) return rc;
    }
    return KM_OK;
}

// the corners of reference kernel k through the exact path, into the call's own scalar block: gftt_dev starts from a clean one; the
// min / max and the valid-pixel count gathered above stay
static int auto_corners_exact(km_ctx *c, auto_search &S, int k)
{
    const km_klt_params *prm = S.prm;
    int rc;
    if ((rc = clear_corner_scalars(c, S.sc))) return rc;
    return gftt_dev(c, S.lap_ref(k), S.mask, S.H, S.W, prm->max_corners, prm->quality_level, prm->min_distance, prm->block_size, S.p0(k), S.cap, S.sc);
}

// ---- ONE pipeline for the whole search where the batched forms cover the case (round 6; two-level pyramids, maxCorners > 0, the
// synchronisation-free corner path): the 2 nk pyramids in one launch, the nk corner detections as one batch of units (fused
// eigenvalue pass + selection chains side by side, nothing read back in between), the nk^2 tracker runs as ONE LK launch and one
// count launch.  Two host synchronisations per search (corner counts + flags; inlier counts) instead of nk + 2, 4 + 2 nk launches of
// dense kernels instead of 7 nk + 2 nk^2.  Anything the batched forms refuse goes through the loops below, run by run.
static bool auto_batchable(const km_ctx *c, const auto_search &S)
{
    const km_klt_params *prm = S.prm;
    return prm->max_level == 1 && S.pyr_levels == 1 && S.nk <= KM_UNITS_MAX && S.nk * S.nk <= KM_LK_JOBS_MAX && spec_path_covers(c, prm) && c->opt_eig3 &&
           c->opt_lk2 && S.W >= 512 && S.H >= 2 * prm->block_size + 8;
}

// pyramids and corners of every reference kernel as one batch of units.  KM_E_UNSUPPORTED: the batched kernels refused, nothing of the
// corner tables is valid (the pyramids are rebuilt one by one)
static int auto_corners_batched(km_ctx *c, auto_search &S)
{
    int rc;
    const int nk = S.nk;
    const km_klt_params *prm = S.prm;
    km_units U;
    U.n = nk; U.dtype = KM_U8; U.capk = (size_t)S.H * S.W / 8 + 4096 * KM_NSHARD;
    unsigned long long *keys = (unsigned long long *)km_ws(c, WS_KEYS0, U.capk * sizeof(unsigned long long) * (size_t)nk);
    if (!keys) return KM_E_NOMEM;
    for (int k = 0; k < nk; k++) {
        U.H[k] = S.H; U.W[k] = S.W; U.x_off[k] = 0.f; U.y_off[k] = 0.f;
        U.lap_ref[k] = S.lap_ref(k); U.lap_mon[k] = S.lap_mon(k); U.mask[k] = const_cast<uint8_t *>(S.mask);
        U.sc[k] = S.unit_sc(k);
        U.keys[k] = keys + U.capk * (size_t)k;
        U.p0[k] = S.p0(k);
        U.eig_partial[k] = nullptr; U.eig_npartial[k] = 0;
        pyr_two_level(U.A[k], U.lap_ref[k], S.pyr_ref(k), S.H, S.W);
        pyr_two_level(U.B[k], U.lap_mon[k], S.pyr_mon(k), S.H, S.W);
        S.d_np0[k] = &U.sc[k]->n_corners;
    }
    {
        km_stage_timer t(c, ST_PYRAMID);
        if ((rc = kd_pyrdown_units(c, U, 1))) return rc;
    }
    for (int k = 0; k < nk; k++) { S.PR[k] = U.A[k]; S.PM[k] = U.B[k]; }
    {
        km_stage_timer t(c, ST_EIGEN);
        rc = k3_eig_candidates_units(c, U, prm->block_size, prm->quality_level);
    }
    if (rc == KM_OK) {
        km_stage_timer t(c, ST_SELECT);
        rc = kf_rank_select_units(c, U, prm->max_corners, prm->quality_level, prm->min_distance, S.cap);
    }
    if (rc) return rc;
    unsigned flags[8];
    for (int k = 0; k < nk; k++) { KM_D2H(c, &S.n_p0[k], &U.sc[k]->n_corners, sizeof(int)); KM_D2H(c, &flags[k], &U.sc[k]->flags, sizeof(unsigned)); }
    KM_FLUSH(c);
    for (int k = 0; k < nk; k++) {
        if (!flags[k]) continue;
        // the unit did not fit the fixed capacities of the synchronisation-free corner path: its corners through the exact one
        c->stats.path_flags |= KM_PATH_SPEC_RETRY;
        if ((rc = auto_corners_exact(c, S, k))) return rc;
        KM_HIP(c, hipMemcpyAsync(&U.sc[k]->n_corners, &S.sc->n_corners, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
        KM_D2H(c, &S.n_p0[k], &S.sc->n_corners, sizeof(int));
        KM_FLUSH(c);
    }
    return KM_OK;
}

static int auto_corners_each(km_ctx *c, auto_search &S)
{
    int rc;
    const km_klt_params *prm = S.prm;
    {
        km_stage_timer t(c, ST_PYRAMID);
        for (int k = 0; k < S.nk; k++)
            if ((rc = build_pyramid_single(c, S.lap_ref(k), S.H, S.W, prm->win_size, prm->max_level, S.pyr_ref(k), &S.PR[k], nullptr)) ||
                (rc = build_pyramid_single(c, S.lap_mon(k), S.H, S.W, prm->win_size, prm->max_level, S.pyr_mon(k), &S.PM[k], nullptr)))
                return rc;
    }
    // ---- corners of every reference Laplacian (klt.py:494), one after the other
    for (int k = 0; k < S.nk; k++) {
        if ((rc = auto_corners_exact(c, S, k))) return rc;
        KM_HIP(c, hipMemcpyAsync(&S.d_counts[k], &S.sc->n_corners, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
        KM_D2H(c, &S.n_p0[k], &S.sc->n_corners, sizeof(int));
        S.d_np0[k] = &S.d_counts[k];
    }
    KM_FLUSH(c);
    return KM_OK;
}

// ---- nk*nk tracker runs (mon kernel outer, ref kernel inner): one LK launch and one count launch.  KM_E_UNSUPPORTED: run by run
static int auto_tracks_batched(km_ctx *c, auto_search &S)
{
    const int nk = S.nk;
    km_lk_job jobs[KM_LK_JOBS_MAX];
    km_count_jobs CJ;
    for (int im = 0; im < nk; im++)
        for (int ir = 0; ir < nk; ir++) {
            const int combo = im * nk + ir;
            km_lk_job &j = jobs[combo];
            j.A = S.PR[ir]; j.B = S.PM[im]; j.pts_in = S.p0(ir); j.d_n = S.d_np0[ir];
            j.p1 = S.p1(combo); j.p0r = S.p0r(combo);
            CJ.p0[combo] = j.pts_in; CJ.p0r[combo] = j.p0r; CJ.d_n[combo] = j.d_n;      // (a reference kernel without corners: 0 points, count 0)
        }
    km_stage_timer t(c, ST_LK);
    const int rc = kl_jobs_launch(c, jobs, nk * nk, S.n_lim, S.prm->win_size, S.prm->max_count, S.prm->epsilon);
    return rc ? rc : kf_count_kept_jobs(c, CJ, nk * nk, S.n_lim, 0.1f, &S.d_counts[nk]);
}

static int auto_tracks_each(km_ctx *c, auto_search &S)
{
    const int nk = S.nk;
    const km_klt_params *prm = S.prm;
    km_stage_timer t(c, ST_LK);
    for (int im = 0; im < nk; im++)
        for (int ir = 0; ir < nk; ir++) {
            if (S.n_p0[ir] <= 0) continue;
            const int combo = im * nk + ir;
            int rc;
            if ((rc = kl_track(c, S.PR[ir], S.PM[im], S.p0(ir), S.d_np0[ir], S.n_lim, prm->win_size, prm->max_count, prm->epsilon, true, S.p1(combo), S.p0r(combo))) ||
                (rc = kf_count_kept(c, S.p0(ir), S.p0r(combo), S.d_np0[ir], S.n_lim, 0.1f, &S.d_counts[nk + combo])))
                return rc;
        }
    return KM_OK;
}

// the inlier ratio of every combination; the best one (-1: no reference kernel found a corner)
static int auto_ratios(km_ctx *c, auto_search &S, double *out_ratios, int *out_best)
{
    const int nk = S.nk;
    int kept[64];
    KM_D2H(c, kept, S.d_counts + nk, (size_t)nk * nk * sizeof(int));
    unsigned long long valid = 0;
    KM_D2H(c, &valid, &S.sc->valid, sizeof valid);
    KM_FLUSH(c);
    c->stats.valid_pixels = (int64_t)valid;
    double best_ratio = -1.0;
    int best = -1;
    for (int im = 0; im < nk; im++)
        for (int ir = 0; ir < nk; ir++) {
            const int combo = im * nk + ir;
            if (S.n_p0[ir] <= 0) { out_ratios[combo] = 0.0; continue; }          // klt_tracker returned None: score 0, never the best
            const double ratio = (double)kept[combo] / (double)S.n_p0[ir];
            out_ratios[combo] = ratio;
            if (ratio > best_ratio) { best_ratio = ratio; best = combo; }
        }
    *out_best = best;
    return KM_OK;
}

// the frame of the winning combination (no score columns), read back into host_out
static int auto_winner_frame(km_ctx *c, auto_search &S, int best, float x_off, float y_off, void *host_out, int *out_best)
{
    int rc;
    const km_frame_layout L(S.cap, false, false);
    char *d_out = (char *)km_ws(c, WS_FRAME, L.ob);
    if (!d_out) return KM_E_NOMEM;
    if ((rc = frame_block_free(c))) return rc;
    out_best[0] = out_best[1] = -1;
    if (best < 0) {
        memset(host_out, 0, 16);
        return KM_OK;
    }
    const int bm = best / S.nk, br = best % S.nk;
    out_best[0] = S.ksizes[bm]; out_best[1] = S.ksizes[br];
    {
        km_stage_timer t(c, ST_FRAME);
        if ((rc = kf_frame(c, S.p0(br), S.p1(best), S.p0r(best), S.d_np0[br], S.n_lim, S.cap, 0.1f, x_off, y_off, d_out, nullptr, S.W))) return rc;
    }
    KM_D2H(c, host_out, d_out, L.ob);
    KM_FLUSH(c);
    c->stats.n_init = L.header((const char *)host_out)[1];
    return KM_OK;
}

extern "C" int km_klt_auto_ksize_frame_dev(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon,
                                           const uint8_t *d_mask, ptrdiff_t smask, const double *nodata_ref, const double *nodata_mon,
                                           const km_klt_params *prm, const int *ksizes, int nk, float x_off, float y_off, void *host_out, int cap,
                                           double *out_ratios, int *out_best)
{
    int rc;
    if ((rc = tile_call_begin(c, "klt_auto_ksize", prm, d_ref, d_mon, H, W, sref, smon)) || (rc = check_dtype(c, "klt_auto_ksize", dtype)) ||
        (rc = check_frame_width(c, "klt_auto_ksize", "tile", W)))
        return rc;
    if (!ksizes || nk < 1 || nk > 8 || !host_out || !out_ratios || !out_best || cap <= 0) return km_fail(c, KM_E_ARG, "klt_auto_ksize: bad arguments");
    if ((rc = check_capacity(c, prm, cap))) return rc;
    memset(&c->stats, 0, sizeof c->stats);
    auto_search S;
    S.nk = nk; S.H = H; S.W = W; S.cap = cap; S.n_lim = corner_limit(prm, cap); S.ksizes = ksizes; S.prm = prm;
    S.sc_stride = up256(sizeof(km_scalars));
    S.sc_base = (char *)km_ws(c, WS_SCALARS, S.sc_stride * (size_t)(nk + 1));
    S.sc = (km_scalars *)S.sc_base;
    if (!S.sc) return KM_E_NOMEM;
    KM_HIP(c, hipMemsetAsync(S.sc_base, 0, S.sc_stride * (size_t)(nk + 1), c->stream));
    if ((rc = auto_mask_minmax(c, S, d_ref, d_mon, dtype, sref, smon, d_mask, smask)) || (rc = auto_arena(c, S)) ||
        (rc = auto_laplacians(c, S, d_ref, d_mon, dtype, sref, smon, nodata_ref, nodata_mon)))
        return rc;
    // corners, then trackers: batched where the batched forms cover the case, else - or where they refuse - one by one
    rc = auto_batchable(c, S) ? auto_corners_batched(c, S) : KM_E_UNSUPPORTED;
    const bool corners_batched = rc == KM_OK;
    if (rc == KM_E_UNSUPPORTED) rc = auto_corners_each(c, S);
    if (rc) return rc;
    rc = corners_batched ? auto_tracks_batched(c, S) : KM_E_UNSUPPORTED;
    if (rc == KM_E_UNSUPPORTED) rc = auto_tracks_each(c, S);
    if (rc) return rc;
    int best = -1;
    if ((rc = auto_ratios(c, S, out_ratios, &best))) return rc;
    return auto_winner_frame(c, S, best, x_off, y_off, host_out, out_best);
}
