/*
 * karios_hip.h -- C ABI of libkarios_hip.so, the MI355X (gfx950) implementation of
 * the KARIOS image-matching hot path.
 *
 * The reference (telespazio-tim/karios) has no FFI of its own: the seam is the
 * Python module surface of `karios.matcher`.  Each entry
 * point below replaces the third-party C++ the reference reaches through cv2 /
 * skimage / numpy at the cited call site (paths relative to the reference root).
 * INTEGRATION.md shows the ctypes stub a KARIOS maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types.
 *   - every function returns an int status: 0 = OK, <0 = error (KM_E_*);
 *     km_last_error(ctx) gives the message.  Nothing throws across the boundary.
 *   - "host" entry points take caller-owned host buffers (numpy) and do the
 *     H2D/D2H copies themselves; "_dev" entry points take device pointers
 *     (hipMalloc'ed or a torch CUDA tensor's data_ptr) and run entirely on the
 *     context's stream.  No pointer is retained after return.
 *   - images are row-major, `stride` is in ELEMENTS between rows.
 *   - a context owns one HIP stream plus a grow-only device workspace; it is not
 *     thread-safe: use one context per calling thread (the reference calls
 *     klt_tracker from a ThreadPoolExecutor, klt.py:526-527).
 */
#ifndef KARIOS_HIP_H
#define KARIOS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct km_ctx km_ctx;

/* pixel types accepted for raw images (KM_F64 / KM_I32 / KM_U32: km_zncc_windows only) */
enum { KM_U8 = 0, KM_U16 = 1, KM_I16 = 2, KM_F32 = 3, KM_F64 = 4, KM_I32 = 5, KM_U32 = 6 };

/* status codes */
enum {
    KM_OK = 0,
    KM_E_ARG = -1,      /* malformed argument (cv2.error equivalent) */
    KM_E_HIP = -2,      /* HIP runtime failure */
    KM_E_NOMEM = -3,
    KM_E_UNSUPPORTED = -4,
    KM_E_NO_DEVICE = -5,
    KM_E_INTERNAL = -6,
    KM_E_NO_CONVERGENCE = -7,  /* km_find_transform_ecc*: NaN correlation or lambda_d <= 0 (cv2.error StsNoConv) */
    KM_E_CAPACITY = -8         /* km_sift_detect_and_compute*: more key points than the outputs have room for (the first `cap` are written) */
};

/* KLTConfiguration fields (core/configuration.py:36-50) + the fixed LK criteria of
 * klt.py:128-132 (maxLevel 1, COUNT|EPS 30 / 0.03) + back_threshold klt.py:143. */
typedef struct km_klt_params {
    int32_t max_corners;      /* maxCorners */
    int32_t block_size;       /* blocksize */
    int32_t win_size;         /* matching_winsize */
    int32_t max_level;        /* 1 */
    int32_t max_count;        /* 30 */
    int32_t ksize_mon;        /* laplacian_kernel_size (mon) */
    int32_t ksize_ref;        /* laplacian_kernel_size (ref) */
    int32_t invert_mon;       /* laplacian_invert_polarity */
    double quality_level;     /* qualityLevel */
    double min_distance;      /* minDistance */
    double epsilon;           /* 0.03 */
} km_klt_params;

/* diagnostics of the last km_klt_* / km_good_features call on a context */
typedef struct km_klt_stats {
    int64_t valid_pixels;     /* mask > 0 count (klt.py:276) */
    int64_t n_candidates;     /* local maxima above threshold */
    int32_t n_init;           /* corners selected (Ninit, klt.py:150) */
    int32_t n_select_batches; /* greedy-selection batches executed */
    double min_ref, max_ref, min_mon, max_mon; /* _to_uint8 stretch bounds */
    float max_eig;            /* maxVal of minMaxLoc */
    float emitted_ratio;      /* candidate keys emitted by the fused eig kernel / exact candidate count */
    int32_t path_flags;       /* KM_PATH_* bits: which retry paths of the corner detector the call went through */
    int32_t tie_rows;         /* (wavefront, row) steps of the fused 8-px eigenvalue pass in which a lane held more than two candidates
                                 of its 8 pixels (ties / plateaus): the per-pixel emission path; diagnostics of the blocking tile entry points */
} km_klt_stats;
#define KM_PATH_KEY_REGROW 1      /* a key-buffer shard overflowed: buffer regrown, detection repeated */
#define KM_PATH_STAGE_FALLBACK 2  /* the fused kernel's key stage overflowed: eig map + candidate kernel instead */
#define KM_PATH_SECOND_PASS 4     /* the top-K slice held too few mutually distant corners: selection on all candidates */
#define KM_PATH_PREFIX_GROWN 8    /* the selection's first ranked prefix was enlarged */
#define KM_PATH_SPEC_RETRY 16     /* the speculative (no host synchronisation) corner path flagged the tile: repeated exactly */
#define KM_PATH_MM_EARLY 32      /* a submitted unit's min / max ran on the second stream beside the previous unit's LK ("mm_early") */

/* ---- context ------------------------------------------------------------ */
int km_version(void);
int km_ctx_create(int device, km_ctx **out);
int km_ctx_destroy(km_ctx *ctx);
const char *km_last_error(km_ctx *ctx);   /* ctx may be NULL: last global error */
int km_ctx_sync(km_ctx *ctx);
/* enable (1) / disable (0) hipEvent stage timing; read back after a call */
int km_set_profiling(km_ctx *ctx, int enable);
/* Options (no counterpart in the reference).  Results NEVER depend on them: every option selects between forms the parity suite
 * holds bit-identical, or shrinks a capacity so that a retry path runs (tests/test_gpu_forced_paths.py, tests/test_gpu_parity.py).
 * The RELEASE library accepts exactly the names below and returns KM_E_ARG for anything else (tests/test_host_logic.py checks that
 * the development names are rejected); the development build (make DEV=1, km_is_dev_build) adds A/B switches of settled choices.
 *  forms
 *   "fused_eig"    1 (default): GFTT's minimum-eigenvalue + candidate detection fused in one pass (no eig map); 0: eig map + candidate
 *                  scan.  Initial value from the environment variable KARIOS_HIP_FUSED_EIG
 *   "eig3"         1 (default): the fused pass runs 8 pixels per lane (k_eig3.hip) on images >= 512 columns wide; 0: always the
 *                  2-pixels-per-lane kernel (k_eig2.hip).  Initial value from KARIOS_HIP_EIG3
 *   "eig3_valid_items" 1 (default): in a batched submission (km_klt_units_frame_submit) with the automatic mask, a strip item of the
 *                  8-pixel fused pass first reads the valid-pixel counts the Laplacian pass of the same submission left for the
 *                  Laplacian items that overlap the item's mask rectangle: no valid pixel - the item returns at once; all valid -
 *                  its interior rows run without the mask; otherwise, with a user mask, and with 0: every item reads the mask
 *                  row by row.  km_eig3_item_classes counts the items of each class
 *   "lk2"          1 (default): LK on four resident patches per key point (two-level pyramids); 0: the first form (one patch per
 *                  direction and level), which also serves deeper pyramids and row bands
 *   "lk_reuse"     1 (default): an LK iteration of the "lk2" form reads the search patch (LDS) and cuts its byte pairs again only when
 *                  the window's integer position moved since the previous iteration; 0: every iteration does (same integers either way)
 *   "speculative"  1 (default): the tile entry points detect corners without a host synchronisation and without sorts (fixed
 *                  capacities, k_select2.hip); a tile that does not fit is flagged (frame header word 2) and repeated through the exact
 *                  path - inside the call for the blocking entry points, by the caller of km_frame_wait for submitted frames
 *                  (PendingFrame.result()).  0: always the exact path (two scalar read-backs per tile, k_select.hip + k_sort.hip).
 *                  Initial value from KARIOS_HIP_SPECULATIVE
 *   "aux_pyramid"  1 (default): on the synchronisation-free path the two pyramids are built on a second stream beside the fused
 *                  eigenvalue pass and joined before LK; 0: on the library's stream.  Initial value from KARIOS_HIP_AUX_PYRAMID
 *   "mm_early"     1 (default): a unit submitted (km_klt_tile_frame_submit / km_klt_units_frame_submit) directly behind another one
 *                  starts its min / max on the second stream as soon as the previous unit's LK launch starts (KM_PATH_MM_EARLY);
 *                  0: on the library's stream, behind the previous unit's tail
 *   "units_pipeline" 1: consecutive km_klt_units_frame_submit calls on this context form a SOFTWARE PIPELINE (csrc/api_units.hip): two
 *                  workspace sets alternate, the dense stages of neighbouring submissions interleave on the library's stream and the
 *                  latency-bound chains of one (corner selection; frame stage + scores) run on a second stream beside the dense kernels
 *                  of the other.  The tail of a submission (LK, frame stage, scores, copy-out) is then enqueued by the NEXT submission,
 *                  by km_frame_flush, by any other entry point or by km_ctx_sync; km_frame_wait on such a frame waits for one of them
 *                  (and enqueues the tail itself after 100 ms).  Frames are bit-identical.  0 (default): every submission is complete
 *                  in stream order when the call returns.  karios_amd.stream.FrameStream switches it on for the contexts it drives
 *   "frame_mi"     1: frame blocks that carry the ZNCC column also carry `mutual_info_score` (MutualInfoService,
 *                  mutual_info_service.py:73-130) and `mi_score` (ZNCCService.compute_mi, zncc_service.py:240-287) of the same rows -
 *                  the whole scoring of KariosAPI._handle_klt_results (api/core.py:894-907) in the tile call: two more float64 columns
 *                  of `cap` entries behind the zncc column (NaN where score < threshold or the chip leaves the image); 0 (default)
 *   "frame_clip"   1: every entry point that produces a frame block (km_klt_tile_frame_dev, km_klt_tile_frame_zncc_dev,
 *                  km_klt_tile_frame_submit, km_klt_units_frame_submit) applies the tracker's iterative 3-sigma / 20-px outlier clip
 *                  (klt.py:52-71, `outliers_filtering`; km_sigma_clip_dev) to the block between the frame stage and the scores: header
 *                  word 0 becomes the number of survivors, the rows stay in (x0, y0) order, the index column becomes the row's position
 *                  among the survivors, the score columns are those of the survivors.  A block of more than 32768 rows is refused
 *                  (KM_E_UNSUPPORTED, nothing queued).  The value is read when the call is made: a pipelined submission keeps the
 *                  value of its own call.  0 (default)
 *   "phase_fp64"   1: km_phase_shift* always evaluates in double precision (k_fft64.hip), the reference's precision; 0 (default):
 *                  hand-written float32 FFT where the image sides factor into {2,3,5,7,61}, double precision only when the
 *                  float32 correlation peak is not at least 1 % above every other sample
 *   "fft61"        1 (default): rows of length 61 M of the float32 transform through the wave-local form; 0: the generic row kernel
 *   "fft_herm"     1 (default): the inverse float32 transform works on the Hermitian half of the cross-power spectrum; 0: full plane
 *   "f64_pair"     1 (default): the inverse along the rows of the double-precision transform packs two image rows into one complex
 *                  transform (the correlation surface of two real images is real); 0: one row per transform
 *   "f64_half"     1 (default): ... and its inverse column levels only run the columns kx <= W / 2; 0: all columns
 *   "f64_plain"    1: the double-precision transform packs the images in a pass of its own and finds the arg-max in two passes behind
 *                  the last level - the form that serves sides with a Bluestein dimension - on every shape (default 0: both ends ride in
 *                  the level kernels where the shape allows)
 *   "ransac_first_batch" iterations of the first batch of km_find_homography_ransac* (batches end at B0, 2 B0, 4 B0, ... iterations);
 *                  0 (default): chosen from the number of pairs and the chip (csrc/api_ransac.hip).  Only the number of iterations
 *                  evaluated beyond the sequential loop's end depends on it
 *  test knobs that shrink internal capacities so that the corner detector's retry paths run on every call (0 = default)
 *   "key_cap"      candidate keys per shard of the first attempt          -> key-buffer overflow + regrow
 *   "stage_cap"    usable slots of the fused kernel's per-wave key stage  -> stage overflow + two-kernel repeat
 *   "topk_factor"  top-K pre-filter keeps factor * maxCorners keys (8)    -> second selection pass on all candidates
 *   "select_first" first ranked prefix of the selection sweeps (3 * maxCorners) -> prefix growth
 *   "stash_cap"    kept keys a workgroup of the scatter launch stashes in LDS -> its second read of the keys
 *   "spec_flag"    KM_FLAG bits the synchronisation-free path raises artificially -> the flag-and-repeat logic
 *   "defer"        0: pyramid jobs of the exact path run after the selection's read-back waits instead of under them
 *   "mask_edge_chunk" edges of a feature the polygon fill (km_rasterize_polygons*) stages in LDS at a time (0 = default 896; 1 .. 896)
 *                  -> many chunks per feature
 *  profiling
 *   "profile_stage" with km_set_profiling(1): time only stage i of km_stage_name (every timed span records two events on the
 *                  library stream and the kernels either side no longer overlap: ~6 us per span); -1 (default): every stage
 *   "profile_every" N: only every N-th tile call records its stage events
 *   "roctx"        1: every stage's host-side enqueue span becomes a roctx range (rocprofv3 --marker-trace; resolved at run time)
 * Environment variables read by the release library: KARIOS_HIP_FUSED_EIG, KARIOS_HIP_EIG3, KARIOS_HIP_AUX_PYRAMID,
 * KARIOS_HIP_SPECULATIVE (initial option values, above) and KARIOS_HIP_UPLOAD_CHECKSUM (km_upload_check_stats). */
int km_set_option(km_ctx *ctx, const char *name, int value);
/* 1: development build (make -C karios_amd/csrc DEV=1): km_set_option additionally accepts A/B switches of settled choices and the
 * library reads KARIOS_HIP_* tuning variables; 0: release build (the default; what __graft_entry__.build() produces) */
int km_is_dev_build(void);
/* development build only (KM_E_UNSUPPORTED otherwise): counters of the "eig3_count" option after a blocking tile call */
int km_dev_counters(km_ctx *ctx, unsigned long long out[2]);
/* out = {strip items without a valid pixel, all valid, general; tie rows (km_klt_stats.tie_rows)} of the 8-pixel fused eigenvalue pass
 * for unit `unit` of the context's last km_klt_units_frame_submit.  Synchronises the context (km_ctx_sync) before it reads. */
int km_eig3_item_classes(km_ctx *ctx, int unit, uint32_t out[4]);
/* stage times (ms) of the last pipeline call; names via km_stage_name(i) */
int km_get_stage_ms(km_ctx *ctx, float *out, int cap, int *n);
const char *km_stage_name(int i);
int km_get_klt_stats(km_ctx *ctx, km_klt_stats *out);

/* ---- device memory helpers (bench / multi-GPU plumbing) ----------------- */
int km_dev_alloc(km_ctx *ctx, size_t bytes, void **dptr);
int km_dev_free(km_ctx *ctx, void *dptr);
int km_h2d(km_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int km_d2h(km_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* Page-locked host memory for image buffers that GDAL (or numpy) fills and the GPU fetches: an upload from such a buffer
 * runs at full PCIe rate and asynchronously (a pageable source is staged chunk by chunk and blocks the caller). */
int km_host_alloc(km_ctx *ctx, size_t bytes, void **hptr);
int km_host_free(km_ctx *ctx /* may be NULL: the block outlived its context */, void *hptr);
/* Asynchronous strided upload on the context's COPY stream: `rows` rows of `width_bytes` bytes, pitches in bytes.  Returns
 * at once when `src_host` is page-locked; a pageable source is packed into the context's page-locked ring chunk by chunk
 * (csrc/staging.hip) and has been read completely when the call returns - no runtime copy ever touches pageable memory; every later call on
 * the context that launches kernels waits (on the device, not
 * on the host) for the uploads queued so far, so pair / tile i+1 can travel while pair / tile i computes.  The caller keeps
 * `src_host` alive and unmodified, and `dst_dev` unused by earlier work, until km_upload_wait or that later call returns. */
int km_upload_async(km_ctx *ctx, void *dst_dev, size_t dst_pitch, const void *src_host, size_t src_pitch,
                    size_t width_bytes, size_t rows);
int km_upload_wait(km_ctx *ctx);   /* host-side wait for the uploads queued so far */
/* Diagnosis of klt.py:252-253 ("a tile is matched as read"): with KARIOS_HIP_UPLOAD_CHECKSUM=1 in the environment a row-checksum
 * kernel runs on the library stream right behind every host-buffer upload of the blocking entry points and is compared with the
 * host's checksum of the source rows when the call completes (mismatches are reported on stderr, see csrc/staging.hip).
 * *armed = uploads checked so far on this context, *missed = uploads whose first consumer saw rows that differ from the source. */
int km_upload_check_stats(km_ctx *ctx, int64_t *armed, int64_t *missed);
/* Finer ordering for pipelines: km_upload_mark returns a ticket for "the uploads queued so far" and takes them out of the
 * automatic wait above; km_upload_join makes the compute stream wait (on the device) for that ticket only.  Upload pair i+1,
 * mark, launch the kernels of pair i, join, launch the kernels of pair i+1: the copy hides under pair i's compute. */
int km_upload_mark(km_ctx *ctx, int *ticket);
int km_upload_join(km_ctx *ctx, int ticket);
/* The buffers passed as full images to the ZNCC / MI entry points (km_klt_tile_frame_zncc_dev, km_klt_tile_frame_submit,
 * km_zncc_batch[_dev], km_mi_batch[_dev]) hold only a WINDOW of the H_image x W_image image, starting at image pixel (ox, oy) -
 * a multi-GPU rank keeps just its tile plus a margin resident.  Key-point coordinates stay image coordinates (the float32
 * sum x0 + dx that the reference rounds, zncc_service.py:195-196, depends on their magnitude), the reference's bounds rule
 * is applied with the image size, pixels are fetched relative to (ox, oy).  A chip inside the image but outside the window
 * scores the NaN with bit pattern KM_NAN_OUTSIDE_WINDOW (the caller's margin was too small).  H_image = W_image = 0: off. */
#define KM_NAN_OUTSIDE_WINDOW 0x7ff80000dead0000ull
int km_set_image_window(km_ctx *ctx, int ox, int oy, int H_image, int W_image);
/* Which evaluation the last km_phase_shift* call used: *path = 1 float32 hand-written FFT (k_fft.hip), 2 double precision
 * (hand-written too, k_fft64.hip); *margin = (largest - second largest) / largest sample of |cross-correlation| seen by the
 * float32 path. */
int km_phase_info(km_ctx *ctx, int *path, double *margin);
/* Test hook, host only (no device, no context): how the double-precision transform behind km_phase_shift* (large_offset.py:39)
 * decomposes a side of n pixels - levels[2 i] = length of level i, levels[2 i + 1] = 0 (radices 2/3/5/7 in LDS) or 1 (one prime,
 * 11 .. 127); *bluestein = length of the chirp-z convolution when n has a larger prime factor (then no levels), else 0;
 * negpos[pos] (n ints, may be NULL) = position at which the forward levels leave the negated frequency of position pos. */
int km_phase_plan(int n, int along_columns, int *levels, int cap_levels, int *n_levels, int *bluestein, int *negpos);
/* Optional device-side copy of every frame block the km_klt_tile_frame_* entry points produce (same layout), e.g. a slice of
 * the send buffer of an RCCL all-gather: the block then never bounces through host memory.  NULL switches it off. */
int km_set_frame_sink(km_ctx *ctx, void *d_dst, size_t capacity_bytes);
/* ... for batched submissions (km_klt_units_frame_submit): unit k's block goes to d_dst + k * pitch_bytes (pitch 0: the block size),
 * e.g. the rows of an all-gather's send buffer that carry a unit id in front of every block */
int km_set_frame_sink_pitch(km_ctx *ctx, void *d_dst, size_t capacity_bytes, size_t pitch_bytes);
/* Hand-over of a SUBMITTED frame (km_klt_tile_frame_submit with a frame sink set) to a stream of the caller without the host:
 * `hip_stream` (a hipStream_t - e.g. the stream the RCCL all-gather of the per-tile blocks, klt.py:220-253 / SURVEY 8e, is issued
 * on) waits on the device until the block of frame `ticket` has reached the sink. */
int km_stream_wait_frame(km_ctx *ctx, int ticket, void *hip_stream);

/* ---- batched units ------------------------------------------------------- */
/* One work unit of a batched submission: a tile of `KLT.match` (klt.py:220-253) - a box of a resident pair - with the rasters its
 * ZNCC / MI chips are cut from (the whole pair, or the window of it a rank holds: win_* as km_set_image_window, win_H = 0: none). */
typedef struct km_unit {
    const void *d_ref, *d_mon;              /* first pixel of the box in the reference / monitored raster (device) */
    ptrdiff_t sref, smon;                   /* row strides in elements */
    const void *d_ref_full, *d_mon_full;    /* rasters of the score columns (NULL: bare frames; all units alike) */
    ptrdiff_t sref_f, smon_f;
    int32_t H, W;                           /* box size */
    int32_t Hf, Wf;                         /* size of the full rasters */
    float x_off, y_off;                     /* origin added to the key points (klt.py:341-342) */
    int32_t win_ox, win_oy, win_H, win_W;
    const uint8_t *d_mask;                  /* user mask of the box (klt.py:258-266; != 0: valid), NULL: the automatic mask (klt.py:268-273); all units alike */
    ptrdiff_t smask;                        /* its row stride in bytes */
} km_unit;
#define KM_UNITS_PER_SUBMISSION 16
/* km_klt_tile_frame_submit for n <= KM_UNITS_PER_SUBMISSION independent units of one pixel type and one parameter set in ONE device
 * pipeline (csrc/api_units.hip): every dense kernel, the corner-selection chain, LK, the frame stage and the scores are launched once
 * for all units.  The frame blocks (layout of km_klt_tile_frame_zncc_dev, unit order) are bit-identical to the unit-by-unit calls';
 * km_frame_wait(ticket) hands out n consecutive blocks, a frame sink receives them at its pitch.  Header word 2 of a block != 0: that
 * unit did not fit the fixed capacities of the synchronisation-free corner path - repeat it alone through km_klt_tile_frame_zncc_dev
 * with "speculative" 0.  Returns KM_E_UNSUPPORTED (no error text) when the batch form does not cover the case (maxCorners 0,
 * minDistance < 1, a unit narrower than 512 columns or without a level-1 pyramid, float32 score columns,
 * a shrunken test capacity): submit the units one by one then.  Either every unit carries a user mask (km_unit.d_mask) or none. */
int km_klt_units_frame_submit(km_ctx *ctx, const km_unit *units, int n_units, int dtype, const double *nodata_ref, const double *nodata_mon,
                              const km_klt_params *prm, double zncc_threshold, int cap, int *ticket);
/* km_klt_units_frame_submit under a geometric prior per unit (`priors`: n_units x 9 float64 in unit order, each as the `prior` of
 * km_klt_tile_frame_prior_dev): every key point of unit u starts at its guess under priors + 9 u on the rasters as they are, and only
 * pixels whose guess meets a valid monitored pixel of the unit's box may become corners.  Block u is bit for bit the block
 * km_klt_tile_frame_prior_dev writes for unit u alone (same x_off, y_off, the unit's user mask as base, the same score columns; bare
 * frames without full rasters); a block whose header word 2 != 0 is repeated alone through that call.  Tickets, km_frame_wait, the frame
 * sink, km_frame_flush and "units_pipeline" behave as for km_klt_units_frame_submit, and the two kinds of submission may alternate.
 * KM_E_ARG: null or non-finite priors (the text names unit and index).  KM_E_UNSUPPORTED: whatever km_klt_units_frame_submit does not
 * cover, "frame_clip" 1 (under a prior the clip runs on the residuals, behind the frame) or a unit with a window (win_H != 0).  A refused
 * call has queued nothing. */
int km_klt_units_frame_prior_submit(km_ctx *ctx, const km_unit *units, int n_units, int dtype, const double *nodata_ref, const double *nodata_mon,
                                    const km_klt_params *prm, double zncc_threshold, int cap, const double *priors, int *ticket);
/* "units_pipeline": enqueue what the last km_klt_units_frame_submit deferred (its LK, frame stage, scores and copy-out) - if that
 * submission is frame `ticket` (ticket < 0: whichever it is).  Call it on the submitting thread when no further submission follows
 * before the frame is waited for; a no-op otherwise. */
int km_frame_flush(km_ctx *ctx, int ticket);

/* ---- fine-grained mirrors (host buffers) -------------------------------- */
/* _to_uint8 (matcher/klt.py:42-49) [+ 255-x, klt.py:419]; out_minmax[2] nullable */
int km_to_uint8(km_ctx *ctx, const void *img, int dtype, int H, int W, ptrdiff_t stride,
                int invert, uint8_t *out, double *out_minmax);
/* automatic validity mask (klt.py:268-273); nodata pointers nullable */
int km_auto_mask(km_ctx *ctx, const void *mon, const void *ref, int dtype, int H, int W,
                 ptrdiff_t stride_mon, ptrdiff_t stride_ref, const double *nodata_mon,
                 const double *nodata_ref, uint8_t *mask, int64_t *valid);
/* Test hook: the oscillation stop of the LK kernels' iteration (cv2.calcOpticalFlowPyrLK, klt.py:134-140; OpenCV compares the
 * float32 |delta + prevDelta| with the DOUBLE literal 0.01) evaluated on the device for n host quadruples (ddx, pdx, ddy, pdy). */
int km_lk_oscillation_probe(km_ctx *ctx, const float *quads, int n, uint8_t *out);
/* Test hook: the frame stage alone (klt.py:142-168, 341-348: forward-backward distance, the cut d < 0.1f, score, tile origin, dx / dy,
 * stable compaction, (x0, y0) row order with pandas' labels) on host point lists of n_units (1 .. 16) units.  p0 / p1 / p0r: n_units x
 * n_max x 2 floats; n[k]: the unit's count word (rows behind it are not read; larger than n_max: clamped), negative = the unit has no
 * count word; width[k]: columns of the unit (corner columns < width), 0 = unknown; out: n_units blocks of 4 int32 {rows, Ninit, 0, 0} +
 * 6 * cap float32 (x0 | y0 | dx | dy | score | index bits).  One unit runs as a tile's frame does, several as a batched submission's
 * (at most 32768 rows each; there every unit has a count word: a negative n[k] becomes n_max, an unknown width the widest map).  The first n[k] corners of a unit must be integer-valued and non-negative: the caller checks. */
int km_frame_from_tracks(km_ctx *ctx, int n_units, const float *p0, const float *p1, const float *p0r, const int *n, const float *x_off,
                         const float *y_off, const int *width, int n_max, int cap, void *out);
/* cv2.Laplacian(u8, CV_8U, ksize) (klt.py:359-360, 427-434, 480-483) */
int km_laplacian_u8(km_ctx *ctx, const uint8_t *src, int H, int W, int ksize, uint8_t *dst);
/* cornerMinEigenVal inside cv2.goodFeaturesToTrack (klt.py:120) */
int km_min_eigen(km_ctx *ctx, const uint8_t *src, int H, int W, int block_size, float *eig);
/* cv2.goodFeaturesToTrack(img, mask=, maxCorners, qualityLevel, minDistance, blockSize)
 * (klt.py:120, 494).  out_xy: 2*cap floats (x,y interleaved); *out_n = 0 <=> None */
int km_good_features(km_ctx *ctx, const uint8_t *img, const uint8_t *mask, int H, int W,
                     int max_corners, double quality_level, double min_distance,
                     int block_size, float *out_xy, int cap, int *out_n);
/* cv::pyrDown u8 (pyramid level of calcOpticalFlowPyrLK) */
int km_pyrdown_u8(km_ctx *ctx, const uint8_t *src, int H, int W, uint8_t *dst);
/* cv2.calcOpticalFlowPyrLK(prev, next, pts, None, winSize=(w,w), maxLevel, criteria)
 * (klt.py:134-140); status/err are not produced (discarded at klt.py:142-153) */
int km_pyrlk(km_ctx *ctx, const uint8_t *prev, const uint8_t *next, int H, int W,
             const float *pts, int n, int win_size, int max_level, int max_count,
             double epsilon, float *out_pts);
/* ---- a geometric prior (no counterpart in the reference's call graph: it resamples the monitored raster instead;
 * tests/lk_prior_restatement.py is the definition).  A prior is 9 float64 values P, row-major, that map
 * reference pixel coordinates to monitored pixel coordinates: w = (P[6] x + P[7] y) + P[8], qx = ((P[0] x + P[1] y) + P[2]) / w,
 * qy likewise, every float64 operation rounded on its own; the guess of a key point is ((float)qx, (float)qy); a position with w not
 * finite or <= 0 has no guess.  For a box at (x_off, y_off) the map is applied to (x + x_off, y + y_off) and the offsets are
 * subtracted from q.  A shift (sx, sy) is {1,0,sx, 0,1,sy, 0,0,1}.
 *
 * km_pyrlk_initial: cv2.calcOpticalFlowPyrLK(prev, next, pts, guess, ..., flags=OPTFLOW_USE_INITIAL_FLOW): km_pyrlk, but the search
 * of point k starts at guess[k] (at guess[k] * 2^-maxLevel on the top level) where km_pyrlk starts it at pts[k]; out_pts are positions
 * in `next`.  KM_E_ARG as km_pyrlk, and for a point or guess that is not finite; KM_E_UNSUPPORTED, nothing queued: max_level != 1,
 * win_size > 40, an image without a pyramid level 1 ((W + 1) / 2 <= win_size or (H + 1) / 2 <= win_size), "lk2" 0 - the seeded tracker
 * is the second LK form. */
int km_pyrlk_initial(km_ctx *ctx, const uint8_t *prev, const uint8_t *next, int H, int W, const float *pts, const float *guess, int n,
                     int win_size, int max_level, int max_count, double epsilon, float *out_pts);
/* The corner mask under a prior: mask[y][x] = base[y][x] && has_guess && 0 <= rx < W && 0 <= ry < H && valid_mon(mon[ry][rx]), with
 * (rx, ry) = (qx, qy) rounded half to even.  base: a user mask (!= 0: valid; stride in bytes) or, NULL, the reference's half of the
 * automatic mask (klt.py:268-273): ref != 0, finite, != *nodata_ref; valid_mon is the monitored half.  Without this rule a guess
 * outside the monitored box stays where it is in both directions and scores a perfect track.  Strides in pixels; mask: H x W bytes,
 * 1 / 0, dense.  The device form leaves its work queued on the context stream. */
int km_prior_mask(km_ctx *ctx, const void *ref, const void *mon, int dtype, int H, int W, ptrdiff_t stride_ref, ptrdiff_t stride_mon,
                  const uint8_t *base, ptrdiff_t stride_base, const double *nodata_ref, const double *nodata_mon, const double prior[9],
                  double x_off, double y_off, uint8_t *mask);
int km_prior_mask_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t stride_ref,
                      ptrdiff_t stride_mon, const uint8_t *d_base, ptrdiff_t stride_base, const double *nodata_ref,
                      const double *nodata_mon, const double prior[9], double x_off, double y_off, uint8_t *d_mask);
/* klt_tracker body up to the forward-backward distance (klt.py:103-142):
 * GFTT on ref (unless p0 given) + LK ref->mon + LK mon->ref.
 * Outputs, each 2*cap floats: p0, p1, p0r; *out_n = Ninit (0 <=> "No features"). */
int km_klt_track(km_ctx *ctx, const uint8_t *ref_lap, const uint8_t *mon_lap,
                 const uint8_t *mask, int H, int W, const km_klt_params *prm,
                 const float *p0_in, int n_p0, float *p0, float *p1, float *p0r, int cap,
                 int *out_n);
/* KLT._match_tile numeric core for one box (klt.py:252-301, 407-436): raw images ->
 * uint8 stretch -> Laplacians -> auto mask (if mask NULL) -> klt_track.
 * *out_n = 0 with stats.valid_pixels == 0 <=> "No valid pixels" (klt.py:276-279). */
int km_klt_tile(km_ctx *ctx, const void *ref, const void *mon, int dtype, int H, int W,
                ptrdiff_t stride_ref, ptrdiff_t stride_mon, const uint8_t *mask,
                const double *nodata_ref, const double *nodata_mon,
                const km_klt_params *prm, float *p0, float *p1, float *p0r, int cap,
                int *out_n);
/* Pre-filter of KLT._match_tile on one tile (klt.py:268-273 automatic mask, :407-436 `_to_uint8` + inversion +
 * cv2.Laplacian of both images) exactly as the tile entry points run it: ONE fused kernel for both images.
 * out_mask may be NULL (no mask derived, *out_valid = -1), else *out_valid = count of valid pixels. */
int km_tile_prefilter(km_ctx *ctx, const void *ref, const void *mon, int dtype, int H, int W,
                      ptrdiff_t stride_ref, ptrdiff_t stride_mon, const double *nodata_ref,
                      const double *nodata_mon, int ksize_ref, int ksize_mon, int invert_mon,
                      uint8_t *out_lap_ref, uint8_t *out_lap_mon, uint8_t *out_mask,
                      int64_t *out_valid);
/* ZNCCService.compute_zncc per keypoint (matcher/zncc_service.py:186-238, _zncc2 :45-126):
 * out[k] = NaN where the reference returns NaN */
int km_zncc_batch(km_ctx *ctx, const void *ref, const void *mon, int dtype, int Href,
                  int Wref, int Hmon, int Wmon, ptrdiff_t stride_ref, ptrdiff_t stride_mon,
                  const float *x0, const float *y0, const float *dx, const float *dy, int n,
                  double *out);
/* _zncc2(img1, img2, u1, v1, u2, v2, n) for `count` window pairs of any half-size n >= 0 (matcher/zncc_service.py:45-126;
 * the reference's known-answer tests use 3x3 and 5x5 windows, tests/test_zncc_service.py:107-125) and any two pixel types:
 * uv = u1[count] | v1[count] | u2[count] | v2[count] (rows, columns of the window centres).  out[k] = NaN for a window
 * without variance; out_outside[k] = 1 (and NaN) where a window leaves its image - the reference raises IndexError there. */
int km_zncc_windows(km_ctx *ctx, const void *img1, const void *img2, int dtype1, int dtype2, int H1, int W1, int H2,
                    int W2, ptrdiff_t stride1, ptrdiff_t stride2, const int32_t *uv, int half_size, int count,
                    double *out, uint8_t *out_outside);
/* ---- the ZNCC search around each key point (no counterpart in the reference's call graph; tests/zncc_search_restatement.py is the
 * definition).  Centres and skip rule are km_zncc_batch's: X0 = int(x0), X1 = round(x0 + dx) on the float32 sum.  For oy, ox in
 * -radius .. radius (S = 2 radius + 1, 1 <= radius <= 8), surface[oy][ox] = _zncc2(ref, mon, Y0, X0, Y1 + oy, X1 + ox, 21): NaN where
 * the 43 x 43 window leaves `mon` or a window has no variance; the value at (0, 0) is km_zncc_batch's.  Integer pixel types take the
 * value from exact integer moments (a function of the pixels alone, the same bits on the host and the device); float32 from two-pass
 * float64 sums.  The peak is the largest value, the first in raster order among equals; per axis the vertex of the parabola through
 * the peak and its two neighbours refines it (float64, (zl - 2 zc) + zr in the denominator, |step| <= 0.5).
 *   out_offset[k] = (bx, by); out_peak[k]; out_shift[k] = (X1 + bx - X0 + sx, Y1 + by - Y0 + sy)
 *   out_status[k] bits: 1 row skipped (outputs NaN, offset 0); 2 no offset has a value (the same); 4 the peak lies on the rim of the
 *   square or a neighbour has no value, in x (then sx = 0); 8 the same in y
 *   out_surface: NULL, or n x S x S
 * Strides in pixels; 0 <= n <= 2^20 (n == 0: KM_OK, nothing launched).  KM_E_ARG: a bad dtype, radius, n, or a null array with n > 0.
 * With an image window set (km_set_image_window) both forms return KM_E_UNSUPPORTED and queue nothing.  The device form leaves its
 * work queued on the context stream. */
int km_zncc_search(km_ctx *ctx, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon,
                   ptrdiff_t stride_ref, ptrdiff_t stride_mon, const float *x0, const float *y0, const float *dx, const float *dy,
                   int n, int radius, int32_t *out_offset, double *out_peak, double *out_shift, uint8_t *out_status, double *out_surface);
int km_zncc_search_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int Href, int Wref, int Hmon, int Wmon,
                       ptrdiff_t stride_ref, ptrdiff_t stride_mon, const float *d_x0, const float *d_y0, const float *d_dx,
                       const float *d_dy, int n, int radius, int32_t *d_offset, double *d_peak, double *d_shift, uint8_t *d_status,
                       double *d_surface);
/* Mutual-information scores per keypoint on the 57x57 chips (next to ZNCC in _handle_klt_results, api/core.py:894-907):
 * out_studholme[k] = MutualInfoService._mutual_info  (matcher/mutual_info_service.py:32-63, column mutual_info_score)
 * out_nmi[k]       = ZNCCService._mutual_information (matcher/zncc_service.py:129-151,      column mi_score)
 * either output may be NULL; NaN where the reference returns NaN */
int km_mi_batch(km_ctx *ctx, const void *ref, const void *mon, int dtype, int Href, int Wref,
                int Hmon, int Wmon, ptrdiff_t stride_ref, ptrdiff_t stride_mon, const float *x0,
                const float *y0, const float *dx, const float *dy, int n, double *out_studholme,
                double *out_nmi);
/* ---- the mutual-information search around each key point (no counterpart in the reference's call graph; tests/mi_search_restatement.py
 * is the definition): km_zncc_search's counterpart for pairs whose contrast is non-linear or inverted.  Centres and skip rule are
 * km_mi_batch's (and km_zncc_search's): X0 = int(x0), X1 = round(x0 + dx) on the float32 sum, the 57 x 57 bounds rule with margin 28 on
 * both rasters.  For oy, ox in -radius .. radius (S = 2 radius + 1, 1 <= radius <= 8), surface[oy][ox] = MutualInfoService._mutual_info of
 * the chip of `ref` at (X0, Y0) and the chip of `mon` at (X1 + ox, Y1 + oy): NaN where that centre fails the bounds rule on `mon`
 * (X - 28 < 0 or X >= Wmon - 28, likewise in y), where one cell of the histogram is occupied, and, for float32, where the monitored chip
 * holds a non-finite sample (a non-finite sample in the reference chip: the whole row).  The 32 x 32 table of counts is that of
 * np.histogram2d(chip_ref, chip_mon, bins=32): the reference chip's bins are fixed per row, the monitored chip's range and bins are taken
 * anew at every offset (integer types: bin = min(floor(32 (v - lo) / (hi - lo)), 31), a constant chip in bin 16; float32: numpy's edges
 * i * step + lo on the float64 casts, the maximum folded into bin 31).
 * From counts to value, exactly: T[c] = round_half_even(c ln c 2^36) for c = 0 .. 3249 as 64-bit integers (T[0] = T[1] = 0,
 * csrc/mi_clogc_q36.inc), L = T[3249]; Sx, Sy, Sxy = the sums of T over the row marginals, the column marginals and the cells;
 * num = 2 L - Sx - Sy, den = L - Sxy (all below 2^53).  surface = (double)num / (double)den, NaN iff den == 0; the mi_score formula
 * (ZNCCService._mutual_information) is (double)(2 (num - den)) / (double)num, NaN iff num == 0.  A value is a function of the pixels
 * alone: the same bits on the host and the device, for all four pixel types; within 1e-9 of km_mi_batch at offset (0, 0).
 * The peak is the largest value of the surface, the first in raster order among equals; the sub-pixel step and the status bits are
 * km_zncc_search's (bits 1, 2, 4, 8).
 *   out_offset[k] = (bx, by); out_peak[k] = the surface at the peak; out_peak_mi[k] = the mi_score formula at the same offset;
 *   out_shift[k] = (X1 + bx - X0 + sx, Y1 + by - Y0 + sy); out_status[k]; out_surface: NULL, or n x S x S
 * Strides in pixels; 0 <= n <= 2^20 (n == 0: KM_OK, nothing launched).  KM_E_ARG: a bad dtype (the 32-bit integer and float64 types
 * included), radius, n, or a null array with n > 0.  With an image window set (km_set_image_window) both forms return
 * KM_E_UNSUPPORTED and queue nothing.  The device form leaves its work queued on the context stream. */
int km_mi_search(km_ctx *ctx, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon,
                 ptrdiff_t stride_ref, ptrdiff_t stride_mon, const float *x0, const float *y0, const float *dx, const float *dy,
                 int n, int radius, int32_t *out_offset, double *out_peak, double *out_peak_mi, double *out_shift, uint8_t *out_status,
                 double *out_surface);
int km_mi_search_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int Href, int Wref, int Hmon, int Wmon,
                     ptrdiff_t stride_ref, ptrdiff_t stride_mon, const float *d_x0, const float *d_y0, const float *d_dx,
                     const float *d_dy, int n, int radius, int32_t *d_offset, double *d_peak, double *d_peak_mi, double *d_shift,
                     uint8_t *d_status, double *d_surface);
/* skimage.registration.phase_cross_correlation(reference_image, moving_image)[0]
 * (matcher/large_offset.py:39): out_rc = [row, col] */
int km_phase_shift(km_ctx *ctx, const void *reference_image, const void *moving_image,
                   int dtype, int H, int W, ptrdiff_t stride_a, ptrdiff_t stride_b,
                   double out_rc[2]);
/* shift_image (core/image.py:70-101); elem_size in bytes (1, 2, 4 or 8) */
int km_shift_image(km_ctx *ctx, const void *img, int elem_size, int H, int W,
                   ptrdiff_t stride, int y_off, int x_off, void *out);

/* ---- device-resident pipeline (inputs already in HBM) -------------------- */
/* same as km_klt_tile with d_ref/d_mon/d_mask device pointers (the mask, if any, has its own row stride:
 * a box of a full-resolution resident mask); outputs are device
 * pointers too (each 2*cap floats) plus a device int for the count.  Asynchronous on
 * the context stream; call km_ctx_sync before reading results. */
int km_klt_tile_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int H,
                    int W, ptrdiff_t stride_ref, ptrdiff_t stride_mon,
                    const uint8_t *d_mask, ptrdiff_t stride_mask, const double *nodata_ref,
                    const double *nodata_mon, const km_klt_params *prm, float *d_p0,
                    float *d_p1, float *d_p0r, int cap, int *d_n);
/* KLT._match_tile end to end on resident data (klt.py:236-349): km_klt_tile_dev, then the forward-backward
 * test / score of klt_tracker (klt.py:142-155) and the (x0, y0) ordering (klt.py:341-348) on the device.
 * host_out receives, in ONE device-to-host copy, 4 int32 {n_rows, n_init, 0, 0} followed by 6*cap float32:
 * x0 | y0 | dx | dy | score | index (int32 bit pattern: the row's label after pandas' in-place sort).
 * The optional 3-sigma outlier filter (klt.py:161-163) is applied with km_set_option "frame_clip" 1 (cap <= 32768), not otherwise. */
int km_klt_tile_frame_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int H, int W,
                          ptrdiff_t stride_ref, ptrdiff_t stride_mon, const uint8_t *d_mask,
                          ptrdiff_t stride_mask, const double *nodata_ref, const double *nodata_mon,
                          const km_klt_params *prm, float x_off, float y_off, void *host_out, int cap);
/* Same, plus the ZNCC column of _handle_klt_results (core.py:876-893) for the rows with score >= zncc_threshold,
 * computed on the FULL-resolution resident images (key points carry full-image coordinates through x_off / y_off).
 * host_out: the layout above followed by cap float64 (NaN where not scored). */
int km_klt_tile_frame_zncc_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int H, int W,
                               ptrdiff_t stride_ref, ptrdiff_t stride_mon, const uint8_t *d_mask,
                               ptrdiff_t stride_mask, const double *nodata_ref, const double *nodata_mon,
                               const km_klt_params *prm, float x_off, float y_off, const void *d_ref_full, const void *d_mon_full,
                               int H_full, int W_full, ptrdiff_t stride_ref_full, ptrdiff_t stride_mon_full,
                               double zncc_threshold, void *host_out, int cap);
/* km_klt_tile_frame_zncc_dev under a prior (above): corners are selected under km_prior_mask's mask (base = d_mask, or the reference's
 * half of the automatic mask), the forward pass of a key point p0 starts at its guess g, the backward pass at p1 - (g - p0) (float32,
 * in that order; it never reads p0), the rasters are neither shifted nor resampled.  dx, dy are total displacements, the block layout
 * is the same and the ZNCC column is scored at round(x0 + dx) on the full rasters.  The identity prior gives the unseeded call's bits.
 * KM_E_UNSUPPORTED, nothing queued: an image window is set (km_set_image_window), "frame_clip" is 1 (under a prior the clip belongs on
 * the residuals dx - (gx - x0): karios_amd applies it behind the frame), the box has no pyramid level 1 at this winSize, maxLevel != 1,
 * winSize > 40 or "lk2" 0.  KM_E_ARG: a prior value that is not finite. */
int km_klt_tile_frame_prior_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int H, int W,
                                ptrdiff_t stride_ref, ptrdiff_t stride_mon, const uint8_t *d_mask,
                                ptrdiff_t stride_mask, const double *nodata_ref, const double *nodata_mon,
                                const km_klt_params *prm, float x_off, float y_off, const void *d_ref_full, const void *d_mon_full,
                                int H_full, int W_full, ptrdiff_t stride_ref_full, ptrdiff_t stride_mon_full,
                                double zncc_threshold, const double prior[9], void *host_out, int cap);
/* Stream-of-tiles form of the two calls above (a KLT.match loop over tiles, klt.py:220-234, or the per-band loop of
 * KariosAPI, core.py:845-871): km_klt_tile_frame_submit returns once the last kernel and the copy of the frame block
 * are ENQUEUED; the next submission then queues its dense stages right behind this frame's tail.  d_ref_full == NULL:
 * no ZNCC column.  km_frame_wait blocks until frame `ticket` is complete and returns its block (layout above) in pinned
 * host memory owned by the context, valid until KM_FRAME_SLOTS (3) further submissions; it touches nothing but that
 * frame's slot, so another thread may call it while this context is already submitting the next frame.
 * km_frame_stage_ms: the frame's stage spans (km_set_profiling), order of km_stage_name. */
int km_klt_tile_frame_submit(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int H, int W,
                             ptrdiff_t stride_ref, ptrdiff_t stride_mon, const uint8_t *d_mask,
                             ptrdiff_t stride_mask, const double *nodata_ref, const double *nodata_mon,
                             const km_klt_params *prm, float x_off, float y_off, const void *d_ref_full,
                             const void *d_mon_full, int H_full, int W_full, ptrdiff_t stride_ref_full,
                             ptrdiff_t stride_mon_full, double zncc_threshold, int cap, int *ticket);
int km_frame_wait(km_ctx *ctx, int ticket, const void **block, size_t *bytes);
int km_frame_stage_ms(km_ctx *ctx, int ticket, float *out, int cap, int *n);
int km_zncc_batch_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype,
                      int Href, int Wref, int Hmon, int Wmon, ptrdiff_t stride_ref,
                      ptrdiff_t stride_mon, const float *d_x0, const float *d_y0,
                      const float *d_dx, const float *d_dy, int n, double *d_out);
int km_mi_batch_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int Href, int Wref,
                    int Hmon, int Wmon, ptrdiff_t stride_ref, ptrdiff_t stride_mon, const float *d_x0,
                    const float *d_y0, const float *d_dx, const float *d_dy, int n, double *d_out_studholme,
                    double *d_out_nmi);
/* KLT._match_tile_auto_ksize (klt.py:465-545) on resident data: the nk Laplacians of each image, their
 * pyramids and the nk corner lists (goodFeaturesToTrack of every reference Laplacian) are built once and stay on the
 * device; the nk*nk tracker runs (mon kernel outer, ref kernel inner = itertools.product order) reuse them.
 * out_ratios[im*nk + ir] = inlier ratio len(points)/Ninit of (ksizes[im], ksizes[ir]) (0 where the reference's
 * klt_tracker returns None); the best pair is the first maximum; out_best = {mon_ksize, ref_ksize} or {-1,-1}.
 * host_out: frame block of the best pair (layout of km_klt_tile_frame_dev).  prm->ksize_* are ignored, prm->invert_mon
 * applies (255 - uint8(mon) before the Laplacians, klt.py:419); outlier filtering is not part of this entry point ("frame_clip" is
 * ignored here: the inlier ratios would need a clip per combination). */
int km_klt_auto_ksize_frame_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int H,
                                int W, ptrdiff_t stride_ref, ptrdiff_t stride_mon,
                                const uint8_t *d_mask, ptrdiff_t stride_mask,
                                const double *nodata_ref, const double *nodata_mon,
                                const km_klt_params *prm, const int *ksizes, int nk, float x_off,
                                float y_off, void *host_out, int cap, double *out_ratios,
                                int *out_best);
/* KariosAPI._filter_by_dn_values (api/core.py:650-737) on resident images: key point i (x = int(x0[i]), y = int(y0[i]))
 * is dropped (keep[i] = 0) when the reference OR the monitored pixel equals one of `no_values`, or when a pixel equals
 * its own image's no-data value (nodata_* nullable).  x0 / y0 / no_values / keep are host arrays; a key point outside
 * the image is an error. */
int km_dn_keep_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int H, int W,
                   ptrdiff_t stride_ref, ptrdiff_t stride_mon, const float *x0, const float *y0,
                   int n, const double *no_values, int n_no, const double *nodata_ref,
                   const double *nodata_mon, uint8_t *keep);
int km_phase_shift_dev(km_ctx *ctx, const void *d_reference_image,
                       const void *d_moving_image, int dtype, int H, int W,
                       ptrdiff_t stride_a, ptrdiff_t stride_b, double out_rc[2]);
int km_shift_image_dev(km_ctx *ctx, const void *d_img, int elem_size, int H, int W,
                       ptrdiff_t stride, int y_off, int x_off, void *d_out);

/* ---- ONE tile matched exactly by several GPUs (row bands) ---------------------------------------------
 * The reference's default is a single tile (tile_size 20000 > 10980): one global min / max for the uint8 stretch, one global
 * maximum eigenvalue, ONE ranked greedy selection and one maxCorners cut (klt.py:42-49, 120).  A rank holds the rows of its band
 * plus a halo; karios_amd.parallel.match_tile_banded runs these steps and exchanges, between them, min / max and the maximum
 * eigenvalue key (all-reduce), the ranks' strongest candidate keys (all-gather) and finally the tracks.  Row origins must be
 * even (pyramid alignment). */
int km_minmax_dev(km_ctx *ctx, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, double out_minmax[2]);
/* stretch with the GIVEN minmax = {min_ref, max_ref, min_mon, max_mon}, Laplacians, automatic (or user) mask cleared outside the
 * band's own rows [own_y0, own_y1); *valid_owned = valid pixels in those rows */
int km_band_prefilter_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t stride_ref,
                          ptrdiff_t stride_mon, const double minmax[4], const double *nodata_ref, const double *nodata_mon,
                          int ksize_ref, int ksize_mon, int invert_mon, int own_y0, int own_y1, const uint8_t *d_user_mask,
                          uint8_t *d_lap_ref, uint8_t *d_lap_mon, uint8_t *d_mask, int64_t *valid_owned);
/* cornerMinEigenVal + candidate detection of the band; *local_max_key = ordered key of its maximum over the mask (0: none) */
int km_band_eigen_dev(km_ctx *ctx, const uint8_t *d_lap_ref, const uint8_t *d_mask, int H, int W, int block_size, double quality_level,
                      unsigned *local_max_key);
/* the band's candidate keys (value bits << 32 | raster index IN THE BAND IMAGE) above quality_level * global maximum: all of
 * them (k_target = 0) or the strongest value bins holding at least k_target */
int km_band_keys_dev(km_ctx *ctx, const uint8_t *d_mask, int H, int W, double quality_level, unsigned global_max_key, size_t k_target,
                     unsigned long long *out_keys, size_t cap, size_t *n_out, size_t *n_total);
/* goodFeaturesToTrack steps 6-8 (rank, greedy minDistance selection, maxCorners) on candidate keys of an H x W image, any order */
int km_select_keys(km_ctx *ctx, const unsigned long long *keys, size_t n, int H, int W, int max_corners, double min_distance,
                   float *out_xy, int cap, int *out_n);
/* The ordering primitives behind the exact paths (k_sort.hip: rank of every candidate in cv::goodFeaturesToTrack's order, row order
 * of frames beyond 32 768 rows), on host buffers.  km_sort_pairs_u64: stable sort of n 64-bit keys in place, ascending or
 * descending; vals (NULL or n 32-bit words) travel with their keys.  km_exclusive_scan_u32: out[i] = sum of in[j], j < i;
 * count_ones != 0: sum of (in[j] == 1) instead. */
int km_sort_pairs_u64(km_ctx *ctx, unsigned long long *keys, unsigned *vals, size_t n, int descending);
int km_exclusive_scan_u32(km_ctx *ctx, const unsigned *in, unsigned *out, size_t n, int count_ones);
/* LK forward + backward of n points in IMAGE coordinates; rows [oy, oy + H) of the H_image-row Laplacian pair are resident.
 * *left_band = 1: a window needed rows outside the band (halo too small for this displacement) */
int km_band_track_dev(km_ctx *ctx, const uint8_t *d_lap_ref, const uint8_t *d_lap_mon, int H, int W, int oy, int H_image,
                      const km_klt_params *prm, const float *p0, int n, float *p1, float *p0r, int *left_band);

/* ---- Global align step (karios/matcher/global_align.py; api_align.hip, k_align.hip) ---------------------------------------------
 * The arithmetic is OpenCV 4.8's, restated in tests/align_restatement.py (the definition the kernels are tested against).
 *
 * cv2.warpPerspective(src, M, (dW, dH), flags, BORDER_CONSTANT, border_value) of a single-channel KM_U8 / KM_F32 image:
 * interpolation 0 = INTER_NEAREST, 1 = INTER_LINEAR; inverse != 0: M maps destination -> source (WARP_INVERSE_MAP), else M is
 * inverted first (3 x 3 closed form in fp64).  Positions are quantised to 1/32 px as OpenCV does.  The host form writes a
 * contiguous dH x dW destination. */
int km_warp_perspective(km_ctx *ctx, const void *src, int dtype, int sH, int sW, ptrdiff_t src_stride, void *dst, int dH, int dW,
                        int interpolation, int inverse, double border_value, const double M[9]);
int km_warp_perspective_dev(km_ctx *ctx, const void *d_src, int dtype, int sH, int sW, ptrdiff_t src_stride, void *d_dst, int dH,
                            int dW, ptrdiff_t dst_stride, int interpolation, int inverse, double border_value, const double M[9]);
/* _sobel_magnitude: 3 x 3 Sobel of a uint8 image (REFLECT_101), magnitude, divided by its maximum (unchanged when that is 0);
 * out: contiguous H x W float32 */
int km_sobel_magnitude(km_ctx *ctx, const uint8_t *img, int H, int W, ptrdiff_t stride, float *out);
int km_sobel_magnitude_dev(km_ctx *ctx, const uint8_t *d_img, int H, int W, ptrdiff_t stride, float *d_out);
/* cv2.findTransformECC(template, input, map, MOTION_HOMOGRAPHY, (COUNT | EPS, max_iter, eps), mask, gauss_filt_size): template
 * hs x ws and input hd x wd (KM_U8 or KM_F32, same type), mask: NULL or hd x wd uint8 (> 0 = valid).  map: float32 3 x 3, in and
 * out (host memory in both forms).  gauss_filt_size 5 only (KM_E_UNSUPPORTED otherwise).  *cc = the last correlation
 * coefficient, *iterations = iterations run.  KM_E_NO_CONVERGENCE where OpenCV raises StsNoConv. */
int km_find_transform_ecc(km_ctx *ctx, const void *template_image, const void *input_image, int dtype, int hs, int ws,
                          ptrdiff_t template_stride, int hd, int wd, ptrdiff_t input_stride, const uint8_t *mask, ptrdiff_t mask_stride,
                          float map[9], int max_iter, double eps, int gauss_filt_size, double *cc, int *iterations);
int km_find_transform_ecc_dev(km_ctx *ctx, const void *d_template_image, const void *d_input_image, int dtype, int hs, int ws,
                              ptrdiff_t template_stride, int hd, int wd, ptrdiff_t input_stride, const uint8_t *d_mask,
                              ptrdiff_t mask_stride, float map[9], int max_iter, double eps, int gauss_filt_size, double *cc,
                              int *iterations);
/* For tests: the intermediates of km_find_transform_ecc at one map (host pointers only).  Runs the same set-up on the same image
 * arguments, then the kernels of one iteration at map (float32 3 x 3, read only), and copies out: t_blur = the blurred template,
 * hs x ws float32; plane = hd x wd x 4 float32 {blurred input, gx * pre-mask, gy * pre-mask, pre-mask}; sums = the 66 fp64 sums the
 * iteration's host algebra works on: N, S(mI), S(mI^2), S(mT), S(mT^2), S(mTI), the 36 Hessian terms (upper triangle, row by
 * row), S(J_k I), S(J_k m), S(J_k m T), k = 0 .. 7.  Bitwise identical from call to call. */
int km_ecc_stages(km_ctx *ctx, const void *template_image, const void *input_image, int dtype, int hs, int ws,
                  ptrdiff_t template_stride, int hd, int wd, ptrdiff_t input_stride, const uint8_t *mask, ptrdiff_t mask_stride,
                  const float map[9], float *t_blur, float *plane, double *sums);
/* _refine_with_ecc for n initial 3 x 3 fp64 matrices (mon -> ref) on uint8 mon (hm x wm) / ref (hr x wr): mon pre-warped onto ref's
 * canvas with (float)init, candidates with fewer than 1000 non-zero pixels skipped, ECC on the Sobel magnitudes (the template's
 * computed once) from the identity with mask = pre-warped mon > 0.  Per candidate (host arrays): final = residual @ init (fp64,
 * 9 values), the float32 residual (9), cc, iterations, valid pixels and status (KM_ECC_*).  The call itself returns KM_OK when
 * a candidate only failed to converge. */
#define KM_ECC_CONVERGED 0
#define KM_ECC_SKIPPED 1         /* fewer than 1000 valid pixels after the pre-warp: no ECC launch */
#define KM_ECC_NO_CONVERGENCE 2  /* findTransformECC would raise: the reference returns (None, nan) */
int km_refine_ecc_candidates(km_ctx *ctx, const uint8_t *mon, int hm, int wm, ptrdiff_t mon_stride, const uint8_t *ref, int hr, int wr,
                             ptrdiff_t ref_stride, int n, const double *inits, int max_iter, double eps, double *final_out,
                             float *residual_out, double *cc_out, int *iterations_out, int64_t *valid_out, int *status_out);
int km_refine_ecc_candidates_dev(km_ctx *ctx, const uint8_t *d_mon, int hm, int wm, ptrdiff_t mon_stride, const uint8_t *d_ref, int hr,
                                 int wr, ptrdiff_t ref_stride, int n, const double *inits, int max_iter, double eps, double *final_out,
                                 float *residual_out, double *cc_out, int *iterations_out, int64_t *valid_out, int *status_out);

/* ---- Preprocessing of the global align step and the quality check's percentiles (api_prep.hip, k_prep.hip) -------------------------
 * _to_uint8 / _preprocess of karios/matcher/global_align.py:87-108 and the np.nanpercentile calls of karios/api/core.py:491-506.
 * The arithmetic is restated in tests/prep_restatement.py (the definition the kernels are tested against, bit for bit).
 *
 * Exact order statistics of an H x W raster (KM_U8, KM_U16, KM_I16 or KM_F32; anything else KM_E_ARG).  Every pixel is taken as a
 * float32 (exact for the integer types).  exclude 0: NaN is left out (np.nanpercentile); 1: every non-finite value is left out
 * (_to_uint8).  *n = number of values kept.  For each of the n_q quantiles q[j] in [0, 1], with vi = (double)(n - 1) * q[j] (the
 * virtual index of numpy's 'linear' method): v0[j] = the value of rank floor(vi) among the kept values in ascending order,
 * v1[j] = the value of rank min(floor(vi) + 1, n - 1), vi_out[j] = vi.  The values are exact (a radix select on an
 * order-preserving key of the float32 bit pattern, three passes over the raster, integer counters: bitwise repeatable); -0.0 sorts
 * below +0.0.  n = 0 is not an error: *n = 0 and v0 / v1 / vi_out are left alone.  The interpolation between v0 and v1 is the
 * caller's (numpy does it in the source dtype: karios_amd/ops/prep.py).  q, n, v0, v1, vi_out: host memory in both forms. */
int km_order_statistics(km_ctx *ctx, const void *img, int dtype, int H, int W, ptrdiff_t stride, int exclude, int n_q, const double *q,
                        int64_t *n, double *v0, double *v1, double *vi_out);
int km_order_statistics_dev(km_ctx *ctx, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, int exclude, int n_q,
                            const double *q, int64_t *n, double *v0, double *v1, double *vi_out);
/* The stretch of _to_uint8 between two percentiles lo < hi, in float64 with every operation rounded on its own (what numpy >= 2
 * evaluates: the percentiles are float64 scalars): v = (double)(float)pixel, t = ((v - lo) / (hi - lo)) * 255.0, clipped to
 * [0, 255] and truncated toward zero.  NaN -> 0 (project choice: the C cast is undefined, x86 numpy gives 0), +inf -> 255,
 * -inf -> 0.  Not (hi > lo): all zeros.  Same four dtypes.  The host form writes a contiguous H x W uint8 image. */
int km_stretch_percentile_u8(km_ctx *ctx, const void *img, int dtype, int H, int W, ptrdiff_t stride, double lo, double hi,
                             uint8_t *out);
int km_stretch_percentile_u8_dev(km_ctx *ctx, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, double lo, double hi,
                                 uint8_t *d_out, ptrdiff_t out_stride);
/* cv2.createCLAHE(clip_limit, (tiles_x, tiles_y)).apply(img) of a uint8 image, OpenCV 4.8's CLAHE_Impl::apply restated:
 *   - W % tiles_x == 0 and H % tiles_y == 0: the tiles divide the image.  Otherwise the image is extended on the right by
 *     tiles_x - W % tiles_x and at the bottom by tiles_y - H % tiles_y with BORDER_REFLECT_101 (a dimension that IS divisible is then
 *     extended by a whole tiles_x / tiles_y); tile size = extended size / grid;
 *   - clip = max((int)(clip_limit * tile_area / 256), 1) (double arithmetic) when clip_limit > 0, else no clipping;
 *     lut_scale = 255.0f / tile_area (float32);
 *   - per tile: 256-bin histogram; bins above clip are cut to it, the excess summed; excess / 256 goes to every bin, the residual
 *     one each to bins 0, step, 2 step, ... (step = max(256 / residual, 1)); LUT[i] = saturate_cast<uchar>(cumsum_i * lut_scale)
 *     (int -> float32, one float32 multiply, round half to even);
 *   - over the original H x W: txf = x * (1.0f / tile_w) - 0.5f, tx1 = floor(txf), tx2 = tx1 + 1, xa = txf - tx1, xa1 = 1.0f - xa,
 *     tx1 = max(tx1, 0), tx2 = min(tx2, tiles_x - 1), the same in y;
 *     res = (L[ty1][tx1][v] * xa1 + L[ty1][tx2][v] * xa) * ya1 + (L[ty2][tx1][v] * xa1 + L[ty2][tx2][v] * xa) * ya, every operation a
 *     float32 rounding of its own in this order (no fused multiply-add), rounded half to even and saturated.
 * KM_E_ARG for what the reflection cannot define: an extension larger than size - 1 in a dimension, a grid with more than 64 KB
 * of LUTs (tiles_x * tiles_y > 256), fewer than one pixel per tile.  The host form writes a contiguous H x W image; in-place
 * (d_out == d_img) is not supported. */
int km_clahe(km_ctx *ctx, const uint8_t *img, int H, int W, ptrdiff_t stride, double clip_limit, int tiles_x, int tiles_y, uint8_t *out);
int km_clahe_dev(km_ctx *ctx, const uint8_t *d_img, int H, int W, ptrdiff_t stride, double clip_limit, int tiles_x, int tiles_y,
                 uint8_t *d_out, ptrdiff_t out_stride);

/* ---- Descriptor matching of the global align step (api_match.hip, k_match.hip) --------------------------------------------------------
 * The arithmetic is restated in tests/match_restatement.py (the definition the kernels are tested against, bit for bit).
 * Descriptors are rows of `dim` = 128 integers 0 .. 255 (what OpenCV's SIFT stores); anything else than 128 is KM_E_UNSUPPORTED.
 * The squared distance d2 of two rows is an exact integer (int8 MFMA contraction), the distance the float32 nearest to sqrt(d2).
 *
 * cv2.BFMatcher(NORM_L2).knnMatch(query, train, k) of karios/matcher/global_align.py:178-179, 193 for k = 1 or 2 (anything else
 * KM_E_ARG): the train rows of every query row ranked ascending by (float32 distance, train index) - among equal float32 distances
 * the lower index comes first, even where its d2 is the larger one.  idx: int32 [n_q, k], dist: float32 [n_q, k]; columns beyond
 * n_t hold -1 / +inf.  Strides in elements.  n_q == 0: nothing to do.  n_t == 0: status 0, nothing is launched; the host form fills
 * -1 / +inf, the device form leaves its outputs alone. */
int km_knn_match_u8(km_ctx *ctx, const uint8_t *query, int n_q, ptrdiff_t stride_q, const uint8_t *train, int n_t, ptrdiff_t stride_t,
                    int dim, int k, int *idx, float *dist);
int km_knn_match_u8_dev(km_ctx *ctx, const uint8_t *d_query, int n_q, ptrdiff_t stride_q, const uint8_t *d_train, int n_t,
                        ptrdiff_t stride_t, int dim, int k, int *d_idx, float *d_dist);
/* karios/matcher/global_align.py:178-202 in one call: the two nearest ref rows of every mon row, Lowe's test
 * (double)dist1 < ratio * (double)dist2 (one float64 product; false without a second neighbour), the nearest mon row of every ref
 * row, and the mutual check.  Rows that pass, in ascending mon index: query_idx (mon row), train_idx (ref row), distance; room for
 * `cap` rows each (n_mon always suffices).  counts[3] = {raw = n_mon, rows passing Lowe, mutual rows}, host memory in both forms.
 * dtype KM_U8, or KM_F32 with every element an integer 0 .. 255 as cv2 hands descriptors out: any other value (NaN and infinities
 * included) is KM_E_ARG, the message naming the first such (row, column) - nothing is rounded.  More mutual rows than cap: KM_E_ARG
 * after counts was written.  n_mon == 0 or n_ref == 0: status 0, no matches, nothing launched.  No host synchronisation between the
 * stages; the device form's only copy is the counters. */
int km_match_lowe_mutual(km_ctx *ctx, const void *mon, int n_mon, ptrdiff_t stride_mon, const void *ref, int n_ref, ptrdiff_t stride_ref,
                         int dtype, int dim, double ratio, int cap, int *query_idx, int *train_idx, float *distance, int *counts);
int km_match_lowe_mutual_dev(km_ctx *ctx, const void *d_mon, int n_mon, ptrdiff_t stride_mon, const void *d_ref, int n_ref,
                             ptrdiff_t stride_ref, int dtype, int dim, double ratio, int cap, int *d_query_idx, int *d_train_idx,
                             float *d_distance, int *counts);

/* ---- RANSAC homography of the global align step (api_ransac.hip, k_ransac.hip, ransac_math.hpp) ----------------------------------------
 * cv2.findHomography(src_pts, dst_pts, cv2.RANSAC, threshold, maxIters=max_iters, confidence=confidence) of
 * karios/matcher/global_align.py:223-230, as OpenCV 4.8 defines it: restated in tests/ransac_restatement.py (the definition the
 * library is held to, bit for bit; parity with cv2 itself is unpinned).  src / dst: n points (x, y) as float32 with a row stride in
 * elements (>= 2).  H: 9 float64 (row-major 3 x 3), mask: n bytes (1 = inlier), *found: 1 when a model was found.  Not found is no
 * error: status 0, *found = 0, H and mask zero.  n == 4: the direct solve with a mask of ones; n > 4: the RANSAC loop (random stream
 * RNG(-1), 4-point models, inliers err <= (float)(threshold^2); threshold <= 0 means 3), then the solve on all inliers and at most
 * 10 Levenberg-Marquardt iterations, both sequential float64 on the host.  The models and inlier counts of a batch of iterations
 * are evaluated on the device at once and the loop's bookkeeping replayed over them in iteration order: the outcome is the
 * sequential loop's (see csrc/api_ransac.hip for the batch schedule and the option "ransac_first_batch").
 * KM_E_ARG: n < 4, confidence outside (0, 1), max_iters above 2^24, a coordinate that is NaN or infinite (the message names the
 * first).  stats (8 words, may be NULL): [0] iterations the sequential loop ran, [1] iterations evaluated, [2] index of the winning
 * iteration (-1: none), [3] its inlier count, [4] Levenberg-Marquardt iterations, [5] size of the first batch, [6] batches, [7] 0.
 * iter_counts / iter_valid (each max(max_iters, 1) ints, may be NULL; for tests): inlier count and "the 4-point solve gave a
 * model" flag of every evaluated iteration.  Host form: everything in host memory.  Device form: src, dst and mask on the device;
 * H, found, stats and iter_* on the host; the pairs travel back once (16 bytes each) for the sequential parts. */
int km_find_homography_ransac(km_ctx *ctx, const float *src, ptrdiff_t stride_src, const float *dst, ptrdiff_t stride_dst, int n,
                              double threshold, int max_iters, double confidence, double H[9], uint8_t *mask, int *found, int64_t *stats,
                              int *iter_counts, int *iter_valid);
int km_find_homography_ransac_dev(km_ctx *ctx, const float *d_src, ptrdiff_t stride_src, const float *d_dst, ptrdiff_t stride_dst, int n,
                                  double threshold, int max_iters, double confidence, double H[9], uint8_t *d_mask, int *found,
                                  int64_t *stats, int *iter_counts, int *iter_valid);

/* ---- SIFT of the global align step (api_sift.hip, k_sift.hip, sift_math.hpp) -----------------------------------------------------------
 * cv2.SIFT_create(nfeatures=0, nOctaveLayers=n_octave_layers, contrastThreshold=, edgeThreshold=, sigma=).detectAndCompute(img, None)
 * of karios/matcher/global_align.py:48-50, 160-166, as OpenCV 4.8 defines it with the float pyramid: restated in
 * tests/sift_restatement.py (the definition the library is held to, bit for bit; parity with cv2 itself is unpinned).  img: H x W
 * uint8 with a row stride in elements, at most 32767 a side.  nfeatures: 0 only (KM_E_UNSUPPORTED otherwise); n_octave_layers 1 .. 8;
 * a sigma whose widest Gaussian kernel exceeds 65 taps is KM_E_UNSUPPORTED.
 * Outputs, each with room for `cap` key points: x, y, size, angle, response (float32) and octave (int32, cv2's packed field) as a
 * struct of arrays, descriptors as [cap, 128] rows of desc_dtype (KM_U8 or KM_F32, the same integers 0 .. 255) with a row stride in
 * elements (>= 128; the host form takes dense rows only).  *count is the true number of key points, always.  More key points than
 * cap: the first cap entries of the final order are written and the call returns KM_E_CAPACITY - call again with cap >= *count.
 * The order is cv2's: x, y ascending, size descending, angle ascending, response and octave descending; duplicates in (x, y, size,
 * angle) are dropped.
 * stats (160 words, may be NULL): [0] octaves, [1] key points before and [2] after the duplicates went, [3] peak workspace bytes of
 * the call, then per octave o: [4 + 3 o] extrema candidates, [5 + 3 o] candidates that passed the refinement, [6 + 3 o] key points
 * (one per orientation peak).  Times in microseconds: [52] the base image, [53] the final order on the host, [54] the gather,
 * [55] the whole call (host clock), and per octave o device time of [56 + 5 o] blur + DoG + decimation, [57 + 5 o] extrema scan,
 * [58 + 5 o] refinement, [59 + 5 o] orientations, [60 + 5 o] descriptors; [136] / [137] how often the candidate /
 * key-point list of an octave was too small and its stage ran again with room.  Host form: everything in host memory.  Device form: img and the outputs on the device; count and
 * stats on the host; the call returns with the outputs complete.  The key-point records travel to the host once (24 bytes each)
 * for the final order. */
int km_sift_detect_and_compute(km_ctx *ctx, const uint8_t *img, int H, int W, ptrdiff_t stride, int nfeatures, int n_octave_layers,
                               double contrast_threshold, double edge_threshold, double sigma, int cap, float *x, float *y, float *size,
                               float *angle, float *response, int *octave, void *desc, int desc_dtype, ptrdiff_t desc_stride, int *count,
                               int64_t *stats);
int km_sift_detect_and_compute_dev(km_ctx *ctx, const uint8_t *d_img, int H, int W, ptrdiff_t stride, int nfeatures, int n_octave_layers,
                                   double contrast_threshold, double edge_threshold, double sigma, int cap, float *d_x, float *d_y,
                                   float *d_size, float *d_angle, float *d_response, int *d_octave, void *d_desc, int desc_dtype,
                                   ptrdiff_t desc_stride, int *count, int64_t *stats);

/* ---- KariosAPI.analyze_accuracy on resident data (api_accuracy.hip, k_accuracy.hip, accuracy_math.hpp) -----------------------------------
 * The arithmetic is restated in tests/accuracy_restatement.py (the definition the library is held to, bit for bit).
 *
 * np.count_nonzero of the monitored raster with the pixels under mask == 0 set to 0 (karios/api/core.py:284-290): an H x W raster
 * (KM_U8, KM_U16, KM_I16 or KM_F32; anything else KM_E_ARG) with a row stride in elements, mask NULL or H x W uint8 with a row
 * stride in bytes.  A pixel counts when it is non-zero - float32 by its bits: NaN and denormals count, -0.0 does not - and its
 * mask byte, if any, is non-zero.  *count is host memory in both forms.  The count is a sum of integers: the same whatever the
 * order.  The device form's only synchronisation is the copy of the 8-byte result. */
int km_count_valid_pixels(km_ctx *ctx, const void *img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *mask, ptrdiff_t mask_stride,
                          int64_t *count);
int km_count_valid_pixels_dev(km_ctx *ctx, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *d_mask,
                              ptrdiff_t mask_stride, int64_t *count);
/* GeometricStat of karios/accuracy_analysis/accuracy_statistics.py: apply_confidence (:82-110), compute_stats (:112-156) and the
 * sorted radial errors compute_percentile (:224-238) reads, for float32 columns dx, dy, score of n rows (n <= 2^24).
 * The sample is the rows with (double)score > thr in row order; carto != 0 negates dy first (:73-74).  stats: for x, y and the
 * score in turn {min, max, median, mean, std} as numpy 2 computes them in float32 (the sum in blocks of 8192 elements, numpy's
 * pairwise tree inside a block; mean = sum / (float)n; std from the float32 squares of the float32 deviations).  order: for
 * percent k the elements [k' - 1] and [k'] of the ascending radial errors sqrt(x x + y y), x = dx (float)factor, y = dy (float)factor,
 * every operation a float32 rounding of its own; p = percents[k] * sample in float64, k' = (int)p, index -1 is the largest element;
 * NaN where k' is no index (sample == 0, percent >= 1).  The interpolation between the two stays with the caller.  With
 * n_nan != 0 (a NaN in dx or dy of the sample) minimum, maximum and median are not numpy's: take them from numpy.  sample == 0
 * leaves stats NaN.  n_percent <= KM_ACC_MAX_PERCENTS.  `out` is host memory in both forms; the device form reads dx, dy and score
 * from the device and copies nothing else than `out`. */
#define KM_ACC_MAX_PERCENTS 8
typedef struct km_accuracy_result {
    int64_t sample;                            /* rows above the threshold */
    int64_t n_nan;                             /* ... of which dx or dy is NaN */
    float stats[15];                           /* {min, max, median, mean, std} of x, of y, of the score */
    float pad;
    float order[2 * KM_ACC_MAX_PERCENTS];      /* r[k' - 1], r[k'] per percent */
} km_accuracy_result;
int km_accuracy_stats(km_ctx *ctx, const float *dx, const float *dy, const float *score, int n, double thr, int carto, double factor,
                      int n_percent, const double *percents, km_accuracy_result *out);
int km_accuracy_stats_dev(km_ctx *ctx, const float *d_dx, const float *d_dy, const float *d_score, int n, double thr, int carto, double factor,
                          int n_percent, const double *percents, km_accuracy_result *out);

/* The tracker's iterative outlier clip (karios/matcher/klt.py:52-71) on resident float32 displacement columns, for n_units <=
 * KM_UNITS_PER_SUBMISSION independent units in ONE launch.  Unit k: d_dx[k], d_dy[k] of n[k] <= 32768 rows (KM_E_UNSUPPORTED beyond).
 * Repeat: mu = mean, s = std of each column as numpy 2 computes them in float32 (km_accuracy_stats); keep the rows with
 * |dx - mu_x| < 3 s_x, |dy - mu_y| < 3 s_y, |dx - mu_x| < 20 and |dy - mu_y| < 20 (float32, strict; NaN compares false); stop when
 * a round keeps every row or none is left, else go on with the compacted columns.  d_keep_index[k] (n[k] int32, device) receives the
 * survivors' row indices in ascending order, d_result[k] (device) their number and the rounds computed.  The pointer tables and n
 * are host arrays.  Asynchronous on the context stream; call km_ctx_sync (or copy with km_d2h) before reading results. */
typedef struct km_clip_result {
    int32_t count;                             /* survivors */
    int32_t rounds;                            /* rounds whose statistics were computed (0 for an empty unit) */
} km_clip_result;
int km_sigma_clip_dev(km_ctx *ctx, const float *const *d_dx, const float *const *d_dy, const int *n, int n_units, int32_t *const *d_keep_index,
                      km_clip_result *d_result);

/* ---- ChipService.generate_chips (karios/report/chip_service.py) on resident data ------------------------------------------------
 * The arithmetic is restated in tests/chips_restatement.py (the definition the library is held to, bit for bit).
 *
 * CenterAndQuarterCellPointSelector.select_points (:46-306) for the float32 columns x0, y0, score of n rows (n <= 2^24, finite
 * coordinates) on a width x height image under a grid of grid_rows x grid_cols cells (1 .. KM_CHIP_MAX_GRID each).  Rows pass with
 * (double)score >= thr, where thr is `threshold` itself (threshold_f64 != 0: an np.float64 threshold compares in float64) or
 * (double)(float)threshold (a Python float compares in float32).  cell = clip(floor(x0 / (float)(width / cols))) ...; per cell,
 * in cell order: the row nearest to the cell's centre, then for each quarter 0 .. 3 the row (the centre row apart) whose distance
 * is nearest to the quarter's median distance; ties go to the larger score, then to the first row.  Every float32 operation is a
 * rounding of its own.  out_index receives at most KM_CHIP_PICKS * grid_rows * grid_cols row indices in the reference's output
 * order (empty cells and quarters left out), *out_count their number.  Both forms write *out_count to host memory; the device form
 * reads the columns from the device and writes out_index there. */
#define KM_CHIP_SIZE 57
#define KM_CHIP_MAX_GRID 16
#define KM_CHIP_PICKS 5
int km_chip_select(km_ctx *ctx, const float *x0, const float *y0, const float *score, int n, int width, int height, double threshold,
                   int threshold_f64, int grid_rows, int grid_cols, int32_t *out_index, int32_t *out_count);
int km_chip_select_dev(km_ctx *ctx, const float *d_x0, const float *d_y0, const float *d_score, int n, int width, int height, double threshold,
                       int threshold_f64, int grid_rows, int grid_cols, int32_t *d_out_index, int32_t *out_count);
/* _to_chips_gdal_dataset (:544-648) for n rows (0 .. 2^20) of float32 columns x0, y0, dx, dy on two rasters of one pixel type (KM_U8,
 * KM_U16, KM_I16, KM_F32), each at least 57 x 57 with its own shape and row stride in elements.  Window centres: ref (int)x0,
 * (int)y0; mon round(x0 + dx), round(y0 + dy) - the float64 sum, half to even.  ok[i] is 0 when either 57 x 57 window leaves its
 * raster, or a centre is not finite or beyond 2^30 (reported as 0).  Per row i, at [i][57][57]: the raw chips in the rasters' type,
 * their uint8 stretch by the chip's own minimum and maximum (_to_uint8: NaN ignored for the range and mapped to 0, a flat or
 * all-NaN chip gives zeros) and, for ksize != 0 (1, 3, 5, 7, 9 or 11; ref_lap / mon_lap may be NULL for 0), cv2.Laplacian(u8,
 * CV_8U, ksize) with the border reflected at the chip's own edge.  windows[i] = {X0, Y0, X1, Y1}.  A row with ok == 0 has zeros in
 * every image.  The host form takes and fills host memory; the device form device memory, asynchronously on the context stream. */
typedef struct km_chip_outputs {
    void *ref_raw, *mon_raw;                   /* n x 57 x 57 of the rasters' type */
    uint8_t *ref_u8, *mon_u8;                  /* n x 57 x 57 */
    uint8_t *ref_lap, *mon_lap;                /* n x 57 x 57, NULL with ksize 0 */
    uint8_t *ok;                               /* n */
    int32_t *windows;                          /* n x 4 */
} km_chip_outputs;
int km_chips(km_ctx *ctx, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref, ptrdiff_t smon,
             const float *x0, const float *y0, const float *dx, const float *dy, int n, int ksize_ref, int ksize_mon, const km_chip_outputs *out);
int km_chips_dev(km_ctx *ctx, const void *d_ref, const void *d_mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref,
                 ptrdiff_t smon, const float *d_x0, const float *d_y0, const float *d_dx, const float *d_dy, int n, int ksize_ref, int ksize_mon,
                 const km_chip_outputs *d_out);

/* ---- the report's numbers on resident data (karios/report/overview_plot.py:134-194, karios/report/commons.py:49-71);
 * tests/report_restatement.py is the definition.
 *
 * Display range of one raster (KM_U8, KM_U16, KM_I16, KM_F32; H x W, row stride in elements).  A pixel is INVALID when its byte of
 * the optional uint8 mask (own row stride, NULL: no mask) is 0, when it equals one of the n_no_values (0 .. KM_DISPLAY_MAX_NO_VALUES)
 * DN values, or when it equals *nodata (NULL: none).  Comparisons are by value, (double)pixel == v: a value the pixel type cannot
 * hold and a NaN match nothing, 0 matches -0.0.  A pixel is VALID when it is finite, not zero and not invalid.  Results, in host
 * memory in both forms: out->n_valid; out->n_invalid (counted whatever the pixel's value); out->raster_min / raster_max, the
 * minimum and maximum of every pixel that is not NaN (a zero as +0.0; NaN when there is none); and per quantile q[j] in [0, 1]
 * of the valid pixels v0 / v1 / vi with the meaning km_order_statistics gives them (untouched when n_valid is 0, which is no error);
 * for a KM_F32 raster vi = float32(n_valid - 1) * float32(q[j]), the float32 product np.percentile forms for a float32 array.
 * Exact (a radix select under the predicate, integer counters): two calls give the same bits.  Every argument error is KM_E_ARG
 * before anything is launched.  The device form reads device memory and completes the context stream before it returns. */
#define KM_DISPLAY_MAX_NO_VALUES 16
typedef struct km_display_range_result {
    int64_t n_valid, n_invalid;
    double raster_min, raster_max;
} km_display_range_result;
int km_display_range(km_ctx *ctx, const void *img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *mask, ptrdiff_t mask_stride,
                     const double *nodata, const double *no_values, int n_no_values, int n_q, const double *q, km_display_range_result *out,
                     double *v0, double *v1, double *vi);
int km_display_range_dev(km_ctx *ctx, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *d_mask, ptrdiff_t mask_stride,
                         const double *nodata, const double *no_values, int n_no_values, int n_q, const double *q, km_display_range_result *out,
                         double *v0, double *v1, double *vi);
/* mean_profile (commons.py:49-71) of n_prof (1 .. KM_PROFILE_MAX) profiles over the same n rows (0 .. 2^20): per profile float32
 * columns `values` and `positions` and a bin size (1 .. 2^24).  Rows are grouped by np.floor_divide(positions, float32(bin_size))
 * (numpy's divmod rule; a NaN key - NaN or infinite position - drops the row; -0.0 and 0.0 are one group), the groups ascending.
 * Per group g, into outputs of capacity n: key[g]; position[g] = int32(float32(float32(key * bin) + float32(bin / 2))); count[g] =
 * the rows whose value is not NaN; mean[g] = pandas' Kahan sum in float32 over those rows in row order / float32(count), NaN for
 * count 0; std[g] = float32(sqrt(M2 / (count - 1))) of pandas' Welford recurrence in float64, NaN for count < 2.  n_groups[p] and
 * n_out_of_range[p] (groups whose float32 position int32 cannot hold; their position[g] is 0) are host memory in both forms; the
 * columns and outputs are host memory in the host form, device memory in the device form, which completes the context stream. */
#define KM_PROFILE_MAX 8
typedef struct km_profile {
    const float *values, *positions;           /* n each */
    float *key;                                /* outputs, n each */
    int32_t *position, *count;
    float *mean, *std;
    int32_t bin_size;
} km_profile;
int km_mean_profiles(km_ctx *ctx, int n, int n_prof, const km_profile *prof, int32_t *n_groups, int32_t *n_out_of_range);
int km_mean_profiles_dev(km_ctx *ctx, int n, int n_prof, const km_profile *d_prof, int32_t *n_groups, int32_t *n_out_of_range);

/* ---- the report's products and the altitude figure's numbers on resident data (karios/report/product_generator.py:138-218,
 * karios/api/core.py:1049-1053, karios/report/shift_by_alt_plot.py:127-171); tests/products_restatement.py is the definition.
 * In all three the host form reads and writes host memory, the device form device memory; the counts (n_out_of_range, n_groups) are
 * host memory in both, and the device form completes the context stream before it returns.  Every argument error is KM_E_ARG before
 * anything is launched.
 *
 * Point rasters of n (0 .. 2^20) key points on an H x W grid (fewer than 2^32 - 1 pixels): `mask` (NULL: none; row stride in bytes)
 * becomes 0 with 1 at every key point, `delta` (NULL: none; band b, row y at delta + b * band_stride + y * row_stride, strides in
 * floats) becomes two bands of NaN (bits 0x7FC00000) with dx / dy, copied by bits, at the key points.  Nothing outside the H x W
 * windows is written.  The pixel of a row is (int)y0, (int)x0 - float32 truncated toward zero; a column in [-W, W), a negative one
 * counted from the right edge as numpy's assignment into a row buffer does; a row in [0, H).  Several rows on one pixel: the last in
 * input order.  A row with a NaN or infinite coordinate or outside those ranges stores nothing and is counted in *n_out_of_range
 * (the reference raises IndexError there; the matcher produces no such row).  dx / dy are read only when there is a delta raster. */
int km_point_rasters(km_ctx *ctx, int n, const float *x0, const float *y0, const float *dx, const float *dy, int H, int W, uint8_t *mask,
                     ptrdiff_t mask_stride, float *delta, ptrdiff_t band_stride, ptrdiff_t row_stride, int32_t *n_out_of_range);
int km_point_rasters_dev(km_ctx *ctx, int n, const float *d_x0, const float *d_y0, const float *d_dx, const float *d_dy, int H, int W,
                         uint8_t *d_mask, ptrdiff_t mask_stride, float *d_delta, ptrdiff_t band_stride, ptrdiff_t row_stride,
                         int32_t *n_out_of_range);
/* out[i] = raster[(int)y0[i], (int)x0[i]] of a KM_U8 / KM_U16 / KM_I16 / KM_F32 raster (H x W, row stride in elements), in the
 * raster's type, for n (0 .. 2^20) rows: numpy's fancy indexing - both indices truncated toward zero, [-size, size), a negative one
 * counted from the end.  A row outside that, or with a NaN or infinite coordinate, reads as 0 and is counted in *n_out_of_range. */
int km_sample_points(km_ctx *ctx, const void *raster, int dtype, int H, int W, ptrdiff_t stride, int n, const float *x0, const float *y0,
                     void *out, int32_t *n_out_of_range);
int km_sample_points_dev(km_ctx *ctx, const void *d_raster, int dtype, int H, int W, ptrdiff_t stride, int n, const float *d_x0,
                         const float *d_y0, void *d_out, int32_t *n_out_of_range);
/* matplotlib.cbook.boxplot_stats(x, whis=1.5) of every group of n (0 .. 2^20) rows, grouped as km_mean_profiles groups them
 * (np.floor_divide(positions, float32(bin_size)), bin_size 1 .. 2^24, a NaN key drops the row, the groups ascending); x = the group's
 * values in row order, NaN values included.  Per group g, into outputs of capacity n: key[g]; count[g] = len(x); mean[g] =
 * np.mean(x) (numpy's pairwise float32 sum over blocks of 8192 / float32(count)); and KM_BOX_STATS float64 columns of n each in
 * `stats`, column k at stats + k * n, in the order q1, med, q3 (np.percentile(x, [25, 50, 75]): float64 interpolation between float32
 * order statistics whose difference is formed in float32), iqr = q3 - q1, cilo / cihi = med -/+ 1.57 * iqr / sqrt(count), whislo,
 * whishi (the smallest x >= q1 - 1.5 iqr / the largest x <= q3 + 1.5 iqr, compared in float64; q1 / q3 when there is none or it lies
 * inside the box).  Order statistics and whisker ends that are zero are +0.0.  A group holding a NaN value has NaN statistics.
 * cls[i] per ROW: 0 inside the whiskers, 1 below whislo, 2 above whishi (matplotlib's fliers are the 1s in row order, then the 2s), -1
 * for a dropped row.  *n_groups: the number of groups. */
#define KM_BOX_STATS 8
int km_box_stats(km_ctx *ctx, int n, const float *values, const float *positions, int bin_size, float *key, int32_t *count, float *mean,
                 double *stats, int8_t *cls, int32_t *n_groups);
int km_box_stats_dev(km_ctx *ctx, int n, const float *d_values, const float *d_positions, int bin_size, float *d_key, int32_t *d_count,
                     float *d_mean, double *d_stats, int8_t *d_cls, int32_t *n_groups);

/* ---- vector masks on the device (karios/core/image.py:104-191 rasterize_vector_mask, karios/api/core.py:538-620 _load_mask);
 * tests/rasterize_restatement.py is the definition: GDAL's polygon burn with BURN=1 and ALL_TOUCHED=TRUE, restated from knowledge of
 * GDAL 3.x (the scan-line fill at pixel centres, OR the all-touched line pass over every ring); parity with GDAL itself is unpinned.
 *
 * n_features features; feature f owns the next feature_rings[f] rings, ring r the next ring_sizes[r] vertices of `xy` (x, y pairs of
 * float64 in pixel / line space; n_rings rings and n_vertices vertices in all, at most 2^20 vertices).  Every ring is closed (last
 * vertex == first) and has at least 2 vertices; every coordinate is finite with |v| <= 2^30; H x W has fewer than 2^32 - 1 pixels:
 * anything else is KM_E_ARG before a launch.  All three tables are HOST memory in both forms.  `out` (host memory; device memory for
 * _dev; row stride in bytes) becomes 1 where a feature burns and 0 elsewhere: every byte of the H x W window is written exactly once
 * by the fill, nothing outside it.  A walk of the line pass that exceeds 4 (H + W) + 64 steps is KM_E_INTERNAL (none is known).
 * The device form completes the context stream before it returns. */
int km_rasterize_polygons(km_ctx *ctx, const double *xy, int n_vertices, const int32_t *ring_sizes, int n_rings, const int32_t *feature_rings,
                          int n_features, int H, int W, uint8_t *out, ptrdiff_t out_stride);
int km_rasterize_polygons_dev(km_ctx *ctx, const double *xy, int n_vertices, const int32_t *ring_sizes, int n_rings, const int32_t *feature_rings,
                              int n_features, int H, int W, uint8_t *d_out, ptrdiff_t out_stride);
/* kernel time of the two passes of the last km_rasterize_polygons* call, which ran under km_set_profiling(1) (KM_E_ARG otherwise): the
 * fill and the line pass, in milliseconds, between events on the library's stream (tools/ubench/mask_rasterize.py) */
int km_mask_pass_ms(km_ctx *ctx, float *fill_ms, float *lines_ms);
/* out = (a > 0) & (b > 0) as uint8 0 / 1 of two H x W uint8 masks (row strides in bytes), and from the same pass counts[3] = pixels
 * with a > 0, with b > 0, with both (the three numbers _load_mask logs).  counts is host memory in both forms. */
int km_mask_and(km_ctx *ctx, const uint8_t *a, ptrdiff_t a_stride, const uint8_t *b, ptrdiff_t b_stride, int H, int W, uint8_t *out,
                ptrdiff_t out_stride, int64_t *counts);
int km_mask_and_dev(km_ctx *ctx, const uint8_t *d_a, ptrdiff_t a_stride, const uint8_t *d_b, ptrdiff_t b_stride, int H, int W, uint8_t *d_out,
                    ptrdiff_t out_stride, int64_t *counts);

/* ---- the numbers of the circular-error figure on resident data (karios/report/circular_error_plot.py:181-228, 254-303, 359-368);
 * tests/ce_figure_restatement.py is the definition.  numpy builds the bin edges and scipy fits the spline, both on the host and from
 * a handful of numbers, so one figure is THREE calls with the same columns, in this order; the context keeps the sample between them.
 *
 * KM_CE_SAMPLE  the sample of km_accuracy_stats (rows with (double)score > thr in row order, dy negated with carto != 0; n <= 2^24),
 *               scaled: x = dx (float)res, y = +-dy (float)res, radial error sqrt(x x + y y), each operation one float32 rounding.
 *               *block: the sample's size, its rows with a NaN in dx or dy (the caller then takes numpy: nothing below is defined),
 *               minimum and maximum of dx, +-dy, x, y, and np.mean / np.std of x and of y in float32 as km_accuracy_stats forms them.
 *               An empty sample leaves the extremes undefined.
 * KM_CE_COUNTS  np.histogram of x on edges_x (bins_x + 1 float32 edges, numpy's linspace over the range; bins_x <= KM_CE_MAX_BINS;
 *               0 skips the axis) -> hist_x[bins_x], the same for y, and np.histogram2d(x, y, bins=10) on edges_grid (11 edges of x,
 *               then 11 of y) -> counts_grid[100], row-major with x first.  Edges and counts are host memory in both forms.
 * KM_CE_CURVES  z = the bicubic spline (tx, ty: 14 knots each, coef: 100 coefficients, as scipy's RectBivariateSpline on the 10 bin
 *               centres gives them) at every point inside box = {cx[0], cx[9], cy[0], cy[9]} (float32 comparisons), evaluated as
 *               FITPACK's bispeu does in float64 and rounded to float32; NaN outside.  scatter_x / _y / _z: the sample in the stable
 *               ascending order of z, NaN last; radial: the radial errors ascending (capacity n each: host memory in the host form,
 *               device memory in the device form).  *tail: the elements [k - 1], [k] of `radial` for 0.9 and for 0.95 as
 *               km_accuracy_stats picks them, and the number of NaN in z.
 * block and tail are host memory in both forms.  The device form reads the columns from the device and copies nothing else to the
 * host than the block, the counts and the tail; it completes the context stream before it returns. */
#define KM_CE_SAMPLE 0
#define KM_CE_COUNTS 1
#define KM_CE_CURVES 2
#define KM_CE_MAX_BINS 65536
typedef struct km_ce_block {
    int32_t sample, n_nan;
    float ext[8];                              /* min, max of dx; of +-dy; of x; of y */
    float mu_x, sigma_x, mu_y, sigma_y;
    float pad[2];
} km_ce_block;
typedef struct km_ce_tail {
    float order[4];                            /* r[k - 1], r[k] for 0.9, then for 0.95 */
    int32_t n_outside;                         /* points outside the grid of centres: NaN in z */
    int32_t pad[3];
} km_ce_tail;
typedef struct km_ce_job {
    int32_t stage, n, carto, pad;
    const float *dx, *dy, *score;              /* every stage: the same columns */
    double thr, res;
    km_ce_block *block;                        /* KM_CE_SAMPLE */
    const float *edges_x, *edges_y, *edges_grid;   /* KM_CE_COUNTS */
    int32_t bins_x, bins_y;
    uint32_t *hist_x, *hist_y, *counts_grid;
    const double *tx, *ty, *coef;              /* KM_CE_CURVES */
    const float *box;
    float *scatter_x, *scatter_y, *scatter_z, *radial;
    km_ce_tail *tail;
} km_ce_job;
int km_ce_figure(km_ctx *ctx, const km_ce_job *job);
int km_ce_figure_dev(km_ctx *ctx, const km_ce_job *job);

#ifdef __cplusplus
}
#endif
#endif /* KARIOS_HIP_H */
