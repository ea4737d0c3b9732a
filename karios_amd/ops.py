"""numpy-facing wrappers over the C ABI, one per third-party call on the KARIOS hot path.

Names and argument meaning follow the calls the reference makes (cv2.Laplacian,
cv2.goodFeaturesToTrack, cv2.calcOpticalFlowPyrLK, skimage phase_cross_correlation,
karios.core.image.shift_image); file:line citations are relative to the reference tree.
All compute happens in libkarios_hip.so on the GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Context, KariosHipError, KltParams, as_image, default_context, dtype_code, ptr, row_stride


def _ctx(ctx):
    return ctx if ctx is not None else default_context()


def to_uint8(arr, invert: bool = False, ctx: Context | None = None, return_minmax: bool = False):
    """_to_uint8 (matcher/klt.py:42-49) [+ `255 - x`, klt.py:419]."""
    c = _ctx(ctx)
    a = as_image(arr)
    out = np.empty(a.shape, np.uint8)
    mm = (C.c_double * 2)()
    c.check(c.lib.km_to_uint8(c.handle, ptr(a), dtype_code(a), a.shape[0], a.shape[1], row_stride(a),
                              int(bool(invert)), ptr(out), mm), "km_to_uint8")
    return (out, (mm[0], mm[1])) if return_minmax else out


def auto_mask(mon, ref, nodata_mon=None, nodata_ref=None, ctx: Context | None = None):
    """Automatic validity mask (klt.py:268-273) -> (uint8 mask, valid pixel count)."""
    c = _ctx(ctx)
    m, r = as_image(mon), as_image(ref)
    if m.shape != r.shape or m.dtype != r.dtype:
        raise KariosHipError("auto_mask: mon/ref shape or dtype mismatch")
    mask = np.empty(m.shape, np.uint8)
    valid = C.c_int64()
    nm = C.byref(C.c_double(float(nodata_mon))) if nodata_mon is not None else None
    nr = C.byref(C.c_double(float(nodata_ref))) if nodata_ref is not None else None
    c.check(c.lib.km_auto_mask(c.handle, ptr(m), ptr(r), dtype_code(m), m.shape[0], m.shape[1], row_stride(m),
                               row_stride(r), nm, nr, ptr(mask), C.byref(valid)), "km_auto_mask")
    return mask, int(valid.value)


def laplacian_u8(img, ksize: int, ctx: Context | None = None):
    """cv2.Laplacian(img, cv2.CV_8U, ksize=ksize) (klt.py:433-434)."""
    c = _ctx(ctx)
    a = np.ascontiguousarray(img, np.uint8)
    if a.ndim != 2:
        raise KariosHipError("laplacian_u8: expected a 2-D uint8 image")
    out = np.empty_like(a)
    c.check(c.lib.km_laplacian_u8(c.handle, ptr(a), a.shape[0], a.shape[1], int(ksize), ptr(out)), "km_laplacian_u8")
    return out


def min_eigen(img, block_size: int, ctx: Context | None = None):
    """cornerMinEigenVal map used inside goodFeaturesToTrack."""
    c = _ctx(ctx)
    a = np.ascontiguousarray(img, np.uint8)
    out = np.empty(a.shape, np.float32)
    c.check(c.lib.km_min_eigen(c.handle, ptr(a), a.shape[0], a.shape[1], int(block_size), ptr(out)), "km_min_eigen")
    return out


def good_features_to_track(image, maxCorners, qualityLevel, minDistance, mask=None, blockSize=3,
                           ctx: Context | None = None):
    """cv2.goodFeaturesToTrack(image, mask=, maxCorners, qualityLevel, minDistance, blockSize)
    (klt.py:120, 494) -> (N,1,2) float32, or None when no corner is found."""
    c = _ctx(ctx)
    a = np.ascontiguousarray(image, np.uint8)
    if a.ndim != 2:
        raise KariosHipError("goodFeaturesToTrack: expected a 2-D uint8 image")
    m = None
    if mask is not None:
        m = np.ascontiguousarray(mask, np.uint8)
        if m.shape != a.shape:
            raise KariosHipError("goodFeaturesToTrack: mask shape mismatch")
    cap = int(maxCorners) if maxCorners > 0 else max(1, (a.shape[0] * a.shape[1]) // 4)
    out = np.empty((cap, 2), np.float32)
    n = C.c_int()
    c.check(c.lib.km_good_features(c.handle, ptr(a), ptr(m), a.shape[0], a.shape[1], int(maxCorners),
                                   float(qualityLevel), float(minDistance), int(blockSize), ptr(out), cap, C.byref(n)),
            "km_good_features")
    if n.value == 0:
        return None
    return out[:n.value].reshape(-1, 1, 2).copy()


def pyr_down(img, ctx: Context | None = None):
    c = _ctx(ctx)
    a = np.ascontiguousarray(img, np.uint8)
    out = np.empty(((a.shape[0] + 1) // 2, (a.shape[1] + 1) // 2), np.uint8)
    c.check(c.lib.km_pyrdown_u8(c.handle, ptr(a), a.shape[0], a.shape[1], ptr(out)), "km_pyrdown_u8")
    return out


def calc_optical_flow_pyr_lk(prev_img, next_img, prev_pts, winSize=(25, 25), maxLevel=1, maxCount=30, epsilon=0.03,
                             ctx: Context | None = None):
    """cv2.calcOpticalFlowPyrLK(prev, next, pts, None, winSize=, maxLevel=, criteria=(EPS|COUNT, maxCount, epsilon))
    (klt.py:128-140) -> next points (N,1,2) float32.  status / err are not produced: KARIOS overwrites
    status and never uses err (klt.py:142-153)."""
    c = _ctx(ctx)
    a = np.ascontiguousarray(prev_img, np.uint8)
    b = np.ascontiguousarray(next_img, np.uint8)
    if a.shape != b.shape or a.ndim != 2:
        raise KariosHipError("calcOpticalFlowPyrLK: image shape mismatch")
    if winSize[0] != winSize[1]:
        raise KariosHipError("calcOpticalFlowPyrLK: only square windows (KARIOS uses (w, w))")
    p = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
    out = np.empty_like(p)
    c.check(c.lib.km_pyrlk(c.handle, ptr(a), ptr(b), a.shape[0], a.shape[1], ptr(p), p.shape[0], int(winSize[0]),
                           int(maxLevel), int(maxCount), float(epsilon), ptr(out)), "km_pyrlk")
    return out.reshape(-1, 1, 2)


def lk_oscillation_probe(quads, ctx: Context | None = None):
    """Test hook: the LK kernels' oscillation stop (OpenCV: float32 |delta + prevDelta| against the double literal 0.01,
    klt.py:134-140) evaluated on the device for (n, 4) float32 rows (ddx, pdx, ddy, pdy) -> bool array."""
    c = _ctx(ctx)
    q = np.ascontiguousarray(quads, np.float32).reshape(-1, 4)
    out = np.zeros(q.shape[0], np.uint8)
    c.check(c.lib.km_lk_oscillation_probe(c.handle, ptr(q), q.shape[0], ptr(out)), "km_lk_oscillation_probe")
    return out.astype(bool)


def frame_from_tracks(units, n_max: int, cap: int, ctx: Context | None = None, raw: bool = False):
    """Test hook: the frame stage of the device pipelines alone (klt.py:142-168, 341-348) on host point lists.

    `units`: 1 to 16 mappings with `p0`, `p1`, `p0r` (`n_max` points each), `n` (the count word the kernels read; negative: the
    unit has none), `x_off`, `y_off` (tile origin) and `width` (columns of the unit, 0: unknown).  One unit runs as a tile's frame
    does, several as one batched submission's (there a unit
    without a count word gets `n_max` as its count).  -> list of DataFrame / None (`frames.block_to_frame`); `raw`: the blocks instead.
    The ordering key of the device code assumes integer-valued, non-negative corners and origins: anything else among the rows
    in front of `n` is refused here."""
    from . import frames
    c = _ctx(ctx)
    units = list(units)
    n_max, cap, k = int(n_max), int(cap), len(units)
    if not 1 <= k <= _lib.UNITS_PER_SUBMISSION or n_max <= 0 or cap <= 0:
        raise KariosHipError(f"frame_from_tracks: {k} units of {n_max} points, capacity {cap}")
    lists = np.empty((3, k, n_max, 2), np.float32)
    counts, widths = np.empty(k, np.int32), np.empty(k, np.int32)
    origins = np.empty((2, k), np.float32)
    for j, u in enumerate(units):
        for i, name in enumerate(("p0", "p1", "p0r")):
            a = np.asarray(u[name], np.float32).reshape(-1, 2)
            if a.shape[0] != n_max:
                raise KariosHipError(f"frame_from_tracks: unit {j}: {name} holds {a.shape[0]} points, not {n_max}")
            lists[i, j] = a
        counts[j], widths[j] = int(u["n"]), int(u.get("width", 0))
        origins[0, j], origins[1, j] = u.get("x_off", 0), u.get("y_off", 0)
        live = lists[0, j, :n_max if counts[j] < 0 else min(int(counts[j]), n_max)]
        if not (np.isfinite(live).all() and (live >= 0).all() and (live == np.floor(live)).all() and (live <= 2.0 ** 24).all()):
            raise KariosHipError(f"frame_from_tracks: unit {j}: corners must be non-negative integers up to 2^24")
        if not (np.isfinite(origins[:, j]).all() and (origins[:, j] == np.floor(origins[:, j])).all()):
            raise KariosHipError(f"frame_from_tracks: unit {j}: the tile origin must be integer-valued")
    words = frames.block_words(cap)
    out = np.empty((k, words), np.float32)
    x_off, y_off = np.ascontiguousarray(origins[0]), np.ascontiguousarray(origins[1])
    c.check(c.lib.km_frame_from_tracks(c.handle, k, ptr(lists[0]), ptr(lists[1]), ptr(lists[2]), ptr(counts), ptr(x_off), ptr(y_off),
                                       ptr(widths), n_max, cap, ptr(out)), "km_frame_from_tracks")
    return list(out) if raw else [frames.block_to_frame(b, cap) for b in out]


def make_params(conf, mon_ksize=1, ref_ksize=1, invert_mon=False) -> KltParams:
    """KLTConfiguration duck type (core/configuration.py:36-50) -> km_klt_params with the fixed
    LK criteria of klt.py:128-132."""
    p = KltParams()
    p.max_corners = int(conf.maxCorners)
    p.block_size = int(conf.blocksize)
    p.win_size = int(conf.matching_winsize)
    p.max_level = 1
    p.max_count = 30
    p.ksize_mon = int(mon_ksize)
    p.ksize_ref = int(ref_ksize)
    p.invert_mon = int(bool(invert_mon))
    p.quality_level = float(conf.qualityLevel)
    p.min_distance = float(conf.minDistance)
    p.epsilon = 0.03
    return p


def _track_outputs(cap):
    return (np.empty((cap, 2), np.float32), np.empty((cap, 2), np.float32), np.empty((cap, 2), np.float32))


def klt_track(ref_lap, mon_lap, mask, conf, p0=None, ctx: Context | None = None):
    """GFTT on ref (unless p0) + LK ref->mon + LK mon->ref (klt.py:103-140).
    -> (p0, p1, p0r) each (N,1,2) float32, or None when no feature was extracted."""
    c = _ctx(ctx)
    a = np.ascontiguousarray(ref_lap, np.uint8)
    b = np.ascontiguousarray(mon_lap, np.uint8)
    if a.shape != b.shape or a.ndim != 2:
        raise KariosHipError("klt_track: image shape mismatch")
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    prm = make_params(conf)
    p0_in, n_p0 = None, 0
    if p0 is not None:
        p0_in = np.ascontiguousarray(p0, np.float32).reshape(-1, 2)
        n_p0 = p0_in.shape[0]
        cap = max(n_p0, 1)
    else:
        cap = prm.max_corners if prm.max_corners > 0 else max(1, a.size // 4)
    o0, o1, o2 = _track_outputs(cap)
    n = C.c_int()
    c.check(c.lib.km_klt_track(c.handle, ptr(a), ptr(b), ptr(m), a.shape[0], a.shape[1], C.byref(prm), ptr(p0_in), n_p0,
                               ptr(o0), ptr(o1), ptr(o2), cap, C.byref(n)), "km_klt_track")
    if n.value == 0:
        return None
    k = n.value
    return o0[:k].reshape(-1, 1, 2), o1[:k].reshape(-1, 1, 2), o2[:k].reshape(-1, 1, 2)


def klt_tile(ref_box, mon_box, conf, mask_box=None, nodata_ref=None, nodata_mon=None, mon_ksize=1, ref_ksize=1,
             invert_mon=False, ctx: Context | None = None):
    """Numeric core of KLT._match_tile for one box (klt.py:252-301, 407-436), fused on the GPU:
    uint8 stretch -> Laplacians -> (auto) mask -> GFTT -> LK fwd/bwd.
    -> ("ok", (p0, p1, p0r)) | ("no_valid_pixels", None) | ("no_features", None)."""
    c = _ctx(ctx)
    r, m = as_image(ref_box), as_image(mon_box)
    if r.shape != m.shape or r.dtype != m.dtype:
        raise KariosHipError("klt_tile: ref/mon shape or dtype mismatch")
    mk = None
    if mask_box is not None:
        mk = np.ascontiguousarray(mask_box, np.uint8)
        if mk.shape != r.shape:
            raise KariosHipError("klt_tile: mask shape mismatch")
    prm = make_params(conf, mon_ksize, ref_ksize, invert_mon)
    cap = prm.max_corners if prm.max_corners > 0 else max(1, r.size // 4)
    o0, o1, o2 = _track_outputs(cap)
    n = C.c_int()
    nr = C.byref(C.c_double(float(nodata_ref))) if nodata_ref is not None else None
    nm = C.byref(C.c_double(float(nodata_mon))) if nodata_mon is not None else None
    c.check(c.lib.km_klt_tile(c.handle, ptr(r), ptr(m), dtype_code(r), r.shape[0], r.shape[1], row_stride(r), row_stride(m),
                              ptr(mk), nr, nm, C.byref(prm), ptr(o0), ptr(o1), ptr(o2), cap, C.byref(n)), "km_klt_tile")
    if n.value == 0:
        return ("no_valid_pixels" if c.stats().valid_pixels == 0 else "no_features"), None
    k = n.value
    return "ok", (o0[:k].reshape(-1, 1, 2), o1[:k].reshape(-1, 1, 2), o2[:k].reshape(-1, 1, 2))


def tile_prefilter(ref_box, mon_box, nodata_ref=None, nodata_mon=None, ref_ksize=1, mon_ksize=1, invert_mon=False,
                   with_mask=True, ctx: Context | None = None):
    """Pre-filter of KLT._match_tile (klt.py:268-273, 407-436) in the fused kernel of the tile path:
    -> (laplacian(uint8(ref)), laplacian(uint8(mon) or its inverse), auto mask | None, valid pixel count | None)."""
    c = _ctx(ctx)
    r, m = as_image(ref_box), as_image(mon_box)
    if r.shape != m.shape or r.dtype != m.dtype:
        raise KariosHipError("tile_prefilter: ref/mon shape or dtype mismatch")
    lr, lm = np.empty(r.shape, np.uint8), np.empty(r.shape, np.uint8)
    mk = np.empty(r.shape, np.uint8) if with_mask else None
    nv = C.c_int64()
    nr = C.byref(C.c_double(float(nodata_ref))) if nodata_ref is not None else None
    nm = C.byref(C.c_double(float(nodata_mon))) if nodata_mon is not None else None
    c.check(c.lib.km_tile_prefilter(c.handle, ptr(r), ptr(m), dtype_code(r), r.shape[0], r.shape[1], row_stride(r), row_stride(m),
                                    nr, nm, int(ref_ksize), int(mon_ksize), int(bool(invert_mon)), ptr(lr), ptr(lm), ptr(mk),
                                    C.byref(nv)), "km_tile_prefilter")
    return lr, lm, mk, (int(nv.value) if with_mask else None)


def zncc_batch(ref, mon, x0, y0, dx, dy, ctx: Context | None = None):
    """ZNCCService._compute_zncc for every keypoint (zncc_service.py:186-238) -> float64[n]."""
    c = _ctx(ctx)
    r, m = as_image(ref), as_image(mon)
    if r.dtype != m.dtype:
        raise KariosHipError("zncc_batch: dtype mismatch")
    x0, y0, dx, dy = (np.ascontiguousarray(v, np.float32) for v in (x0, y0, dx, dy))
    n = len(x0)
    out = np.empty(n, np.float64)
    if n == 0:
        return out
    c.check(c.lib.km_zncc_batch(c.handle, ptr(r), ptr(m), dtype_code(r), r.shape[0], r.shape[1], m.shape[0], m.shape[1],
                                row_stride(r), row_stride(m), ptr(x0), ptr(y0), ptr(dx), ptr(dy), n, ptr(out)),
            "km_zncc_batch")
    return out


def zncc_windows(img1, img2, u1, v1, u2, v2, half_size: int, ctx: Context | None = None):
    """`_zncc2(img1, img2, u1, v1, u2, v2, n)` (zncc_service.py:45-126) for arrays of window centres (rows u, columns v),
    any half-size n >= 0 and any two numeric pixel types (other types are read as float64).
    -> (float64 values, bool mask of the windows that leave their image: the reference raises IndexError for those)."""
    c = _ctx(ctx)
    a, b = np.asarray(img1), np.asarray(img2)
    if a.dtype not in _lib._DTYPES and a.dtype not in _lib._ANY_DTYPES:
        a = a.astype(np.float64)
    if b.dtype not in _lib._DTYPES and b.dtype not in _lib._ANY_DTYPES:
        b = b.astype(np.float64)
    a, b = as_image(a), as_image(b)
    uv = np.ascontiguousarray(np.stack([np.asarray(v).ravel() for v in (u1, v1, u2, v2)]), np.int32)
    count = uv.shape[1]
    out, outside = np.empty(count, np.float64), np.zeros(count, np.uint8)
    if count:
        c.check(c.lib.km_zncc_windows(c.handle, ptr(a), ptr(b), _lib.any_dtype_code(a), _lib.any_dtype_code(b), a.shape[0], a.shape[1],
                                      b.shape[0], b.shape[1], row_stride(a), row_stride(b), ptr(uv), int(half_size), count, ptr(out),
                                      ptr(outside)), "km_zncc_windows")
    return out, outside.astype(bool)


def mi_batch(ref, mon, x0, y0, dx, dy, ctx: Context | None = None):
    """Per-keypoint mutual-information scores on the 57x57 chips -> (studholme, nmi) float64 arrays:
    `MutualInfoService._compute_mutual_info` (mutual_info_service.py:99-130, (H(X)+H(Y))/H(X,Y) in [1,2]) and
    `ZNCCService._compute_mi` (zncc_service.py:260-287, 2*MI/(H(X)+H(Y)) in [0,1])."""
    c = _ctx(ctx)
    r, m = as_image(ref), as_image(mon)
    if r.dtype != m.dtype:
        raise KariosHipError("mi_batch: dtype mismatch")
    x0, y0, dx, dy = (np.ascontiguousarray(v, np.float32) for v in (x0, y0, dx, dy))
    n = len(x0)
    a, b = np.empty(n, np.float64), np.empty(n, np.float64)
    if n == 0:
        return a, b
    c.check(c.lib.km_mi_batch(c.handle, ptr(r), ptr(m), dtype_code(r), r.shape[0], r.shape[1], m.shape[0], m.shape[1],
                              row_stride(r), row_stride(m), ptr(x0), ptr(y0), ptr(dx), ptr(dy), n, ptr(a), ptr(b)), "km_mi_batch")
    return a, b


def phase_cross_correlation(reference_image, moving_image, ctx: Context | None = None):
    """skimage.registration.phase_cross_correlation(reference_image, moving_image)[0] with the 0.24
    defaults (large_offset.py:39) -> array([row, col]) float64 holding integers."""
    c = _ctx(ctx)
    a, b = as_image(reference_image), as_image(moving_image)
    if a.shape != b.shape or a.dtype != b.dtype:
        raise KariosHipError("phase_cross_correlation: images must have the same shape and dtype")
    out = (C.c_double * 2)()
    c.check(c.lib.km_phase_shift(c.handle, ptr(a), ptr(b), dtype_code(a), a.shape[0], a.shape[1], row_stride(a), row_stride(b),
                                 out), "km_phase_shift")
    return np.array([out[0], out[1]], np.float64)


def shift_image(img, y_off=0, x_off=0, ctx: Context | None = None):
    """shift_image (core/image.py:70-101): integer shift, zero fill, dtype/shape preserved."""
    c = _ctx(ctx)
    a = np.asarray(img)
    if a.ndim != 2 or a.itemsize not in (1, 2, 4, 8):
        raise KariosHipError("shift_image: expected a 2-D array of 1/2/4/8-byte elements")
    a = as_image(a)
    y_off, x_off = int(round(y_off)), int(round(x_off))
    out = np.empty(a.shape, a.dtype)
    c.check(c.lib.km_shift_image(c.handle, ptr(a), a.itemsize, a.shape[0], a.shape[1], row_stride(a), y_off, x_off, ptr(out)),
            "km_shift_image")
    return out


__all__ = ["Context", "KariosHipError", "to_uint8", "auto_mask", "laplacian_u8", "min_eigen", "good_features_to_track",
           "pyr_down", "calc_optical_flow_pyr_lk", "klt_track", "klt_tile", "zncc_batch", "zncc_windows", "mi_batch", "phase_cross_correlation",
           "shift_image", "make_params", "_lib"]


# ---- global align step (karios/matcher/global_align.py; csrc/api_align.hip) ------------------------------------------------
INTER_NEAREST, INTER_LINEAR, WARP_INVERSE_MAP = 0, 1, 16
TERM_CRITERIA_COUNT, TERM_CRITERIA_EPS = 1, 2


def warp_perspective(src, M, dsize, flags=INTER_LINEAR, border_value=0.0, ctx: Context | None = None):
    """cv2.warpPerspective(src, M, dsize=(width, height), flags, BORDER_CONSTANT, borderValue) of a uint8 / float32 image
    (global_align.py:328, 423, 469, 490).  flags: INTER_LINEAR or INTER_NEAREST, | WARP_INVERSE_MAP."""
    c = _ctx(ctx)
    a = as_image(src)
    if a.dtype not in (np.uint8, np.float32):
        raise KariosHipError(f"warp_perspective: dtype {a.dtype} (uint8 and float32 only)")
    interp = int(flags) & 15
    if interp not in (INTER_NEAREST, INTER_LINEAR):
        raise KariosHipError(f"warp_perspective: interpolation {interp} (INTER_NEAREST / INTER_LINEAR only)")
    m = np.ascontiguousarray(np.asarray(M).reshape(3, 3), np.float64)   # Mat::convertTo(CV_64F), exact from float32
    W, H = int(dsize[0]), int(dsize[1])
    out = np.empty((H, W), a.dtype)
    c.check(c.lib.km_warp_perspective(c.handle, ptr(a), dtype_code(a), a.shape[0], a.shape[1], row_stride(a), ptr(out), H, W, interp,
                                      int(bool(int(flags) & WARP_INVERSE_MAP)), float(border_value),
                                      m.ctypes.data_as(C.POINTER(C.c_double))), "km_warp_perspective")
    return out


def sobel_magnitude(img, ctx: Context | None = None):
    """_sobel_magnitude (global_align.py:295-306): Sobel gradient magnitude of a uint8 image over its maximum, float32."""
    c = _ctx(ctx)
    a = as_image(img)
    if a.dtype != np.uint8:
        raise KariosHipError("sobel_magnitude: expected a uint8 image")
    out = np.empty(a.shape, np.float32)
    c.check(c.lib.km_sobel_magnitude(c.handle, ptr(a), a.shape[0], a.shape[1], row_stride(a), ptr(out)), "km_sobel_magnitude")
    return out


def _criteria(criteria):
    ctype, max_count, eps = criteria
    return (int(max_count) if int(ctype) & TERM_CRITERIA_COUNT else 200), (float(eps) if int(ctype) & TERM_CRITERIA_EPS else -1.0)


def find_transform_ecc(template, image, warp, criteria, input_mask=None, gauss_filt_size=5, ctx: Context | None = None,
                       return_iterations: bool = False):
    """cv2.findTransformECC(template, image, warp, MOTION_HOMOGRAPHY, criteria, inputMask, gaussFiltSize) -> (cc, warp float32).
    Raises KariosHipError with code E_NO_CONVERGENCE where OpenCV raises StsNoConv."""
    c = _ctx(ctx)
    images, mp = _ecc_images(template, image, warp, input_mask, "find_transform_ecc")
    n_it, eps = _criteria(criteria)
    cc, it = C.c_double(), C.c_int()
    c.check(c.lib.km_find_transform_ecc(c.handle, *images, ptr(mp), n_it, eps, int(gauss_filt_size), C.byref(cc), C.byref(it)),
            "km_find_transform_ecc")
    return (cc.value, mp, it.value) if return_iterations else (cc.value, mp)


def _ecc_images(template, image, warp, input_mask, who):
    """-> (the image arguments km_find_transform_ecc and km_ecc_stages share, the float32 map)"""
    t, a = as_image(template), as_image(image)
    if t.dtype != a.dtype or t.dtype not in (np.uint8, np.float32):
        raise KariosHipError(f"{who}: both images uint8 or both float32")
    mp = np.array(np.asarray(warp).reshape(3, 3), np.float32)
    m = None
    if input_mask is not None:
        m = as_image(np.asarray(input_mask).astype(np.uint8, copy=False))
        if m.shape != a.shape:
            raise KariosHipError(f"{who}: mask shape differs from the input's")
    # (ndarray.ctypes.data_as keeps its array alive: the pointers outlive this function's locals)
    return (ptr(t), ptr(a), dtype_code(t), t.shape[0], t.shape[1], row_stride(t), a.shape[0], a.shape[1], row_stride(a),
            ptr(m), row_stride(m) if m is not None else 0), mp


def ecc_stages(template, image, warp, input_mask=None, ctx: Context | None = None):
    """For tests: the intermediates of find_transform_ecc at the map `warp` -> (t_blur float32 [hs, ws], plane float32 [hd, wd, 4] =
    {blurred input, gx * pre-mask, gy * pre-mask, pre-mask}, sums float64 [66], the sums one iteration's host algebra works on)."""
    c = _ctx(ctx)
    images, mp = _ecc_images(template, image, warp, input_mask, "ecc_stages")
    hs, ws, hd, wd = images[3], images[4], images[6], images[7]
    t_blur, plane, sums = np.empty((hs, ws), np.float32), np.empty((hd, wd, 4), np.float32), np.empty(66, np.float64)
    c.check(c.lib.km_ecc_stages(c.handle, *images, ptr(mp), ptr(t_blur), ptr(plane), sums.ctypes.data_as(C.POINTER(C.c_double))),
            "km_ecc_stages")
    return t_blur, plane, sums


def refine_ecc_candidates(mon_u8, ref_u8, inits, max_iters=200, eps=1e-6, ctx: Context | None = None):
    """_refine_with_ecc (global_align.py:309-359) for several initial matrices at once -> list of
    (final fp64 3 x 3 or None, cc or nan, iterations, valid pixels, status, float32 residual or None); status _lib.ECC_*."""
    c = _ctx(ctx)
    mon, ref = as_image(mon_u8), as_image(ref_u8)
    if mon.dtype != np.uint8 or ref.dtype != np.uint8:
        raise KariosHipError("refine_ecc_candidates: uint8 images expected")
    n = len(inits)
    ini = np.ascontiguousarray(np.array([np.asarray(m, np.float64).reshape(3, 3) for m in inits]).reshape(n, 9))
    fin = np.empty((n, 9)); res = np.empty((n, 9), np.float32); cc = np.empty(n)
    it = np.empty(n, np.int32); valid = np.empty(n, np.int64); st = np.empty(n, np.int32)
    c.check(c.lib.km_refine_ecc_candidates(c.handle, ptr(mon), mon.shape[0], mon.shape[1], row_stride(mon), ptr(ref), ref.shape[0],
                                           ref.shape[1], row_stride(ref), n, ptr(ini), int(max_iters), float(eps), ptr(fin), ptr(res),
                                           ptr(cc), ptr(it), ptr(valid), ptr(st)), "km_refine_ecc_candidates")
    out = []
    for k in range(n):
        ok = st[k] == _lib.ECC_CONVERGED
        out.append((fin[k].reshape(3, 3) if ok else None, float(cc[k]), int(it[k]), int(valid[k]), int(st[k]),
                    res[k].reshape(3, 3) if ok else None))
    return out


# ---- preprocessing of the align step and the quality check's percentiles (csrc/api_prep.hip) ---------------------------------------
PREP_DTYPES = (np.dtype("uint8"), np.dtype("uint16"), np.dtype("int16"), np.dtype("float32"))
EXCLUDE_NAN, EXCLUDE_NONFINITE = 0, 1


def _stats_call(c, fn, what, image_args, exclude, q):
    qq = np.ascontiguousarray(np.atleast_1d(np.asarray(q, np.float64)))
    if qq.ndim != 1:
        raise KariosHipError(f"{what}: q must be a scalar or a 1-D sequence")
    n = C.c_int64()
    v0, v1, vi = np.full(qq.size, np.nan), np.full(qq.size, np.nan), np.full(qq.size, np.nan)
    pd = C.POINTER(C.c_double)
    c.check(fn(c.handle, *image_args, int(exclude), qq.size, qq.ctypes.data_as(pd), C.byref(n), v0.ctypes.data_as(pd), v1.ctypes.data_as(pd),
               vi.ctypes.data_as(pd)), what)
    return int(n.value), v0, v1, vi


def order_statistics(arr, q, exclude: int = EXCLUDE_NAN, ctx: Context | None = None):
    """Exact order statistics of a uint8 / uint16 / int16 / float32 raster for the quantiles q in [0, 1] -> (n, v0, v1, vi):
    n values kept (exclude EXCLUDE_NAN: all but NaN; EXCLUDE_NONFINITE: the finite ones); with vi = (n - 1) * q, v0 = the value of
    rank floor(vi) and v1 the value of rank min(floor(vi) + 1, n - 1), float64.  n = 0 leaves v0 / v1 / vi NaN."""
    c = _ctx(ctx)
    a = as_image(arr)
    return _stats_call(c, c.lib.km_order_statistics, "km_order_statistics",
                       (ptr(a), dtype_code(a), a.shape[0], a.shape[1], row_stride(a)), exclude, q)


def lerp_linear(v0, v1, vi, n, dtype):
    """The interpolation of numpy's 'linear' quantile between its two neighbours (numpy 2.x _get_indexes / _get_gamma / _lerp), on
    arrays of dtype `dtype` as numpy has them: `b - a` is a float32 subtraction for float32 and wraps for int16.  -> float64."""
    dtype = np.dtype(dtype)
    a = np.atleast_1d(np.asarray(v0)).astype(dtype)       # exact: the values came out of a raster of this dtype
    b = np.atleast_1d(np.asarray(v1)).astype(dtype)
    vi = np.atleast_1d(np.asarray(vi, np.float64))
    prev = np.floor(vi)
    prev[vi >= n - 1] = -1                                # numpy indexes the last element as -1 there, and takes gamma from that index
    gamma = vi - prev.astype(np.intp)
    diff = np.subtract(b, a)
    out = np.asanyarray(np.add(a, diff * gamma))
    np.subtract(b, diff * (1 - gamma), out=out, where=gamma >= 0.5, casting="unsafe", dtype=type(out.dtype))
    return out


def _percentile(arr, q, exclude, nan_poisons, ctx):
    a = as_image(arr)
    qq = np.true_divide(np.asarray(q, np.float64), 100)
    if np.any(qq < 0) or np.any(qq > 1) or np.any(np.isnan(qq)):
        raise ValueError("Percentiles must be in the range [0, 100]")
    n, v0, v1, vi = order_statistics(a, qq.reshape(-1), exclude, ctx)
    if n == 0 or (nan_poisons and n < a.size):
        res = np.full(qq.size, np.nan)
    else:
        res = lerp_linear(v0, v1, vi, n, a.dtype)
    return res[0] if qq.ndim == 0 else res


def nanpercentile(arr, q, ctx: Context | None = None):
    """np.nanpercentile(arr, q) of a 2-D uint8 / uint16 / int16 / float32 raster (method 'linear', q taken as float64), float64;
    NaN when nothing but NaN is there."""
    return _percentile(arr, q, EXCLUDE_NAN, False, ctx)


def percentile(arr, q, ctx: Context | None = None):
    """np.percentile(arr, q) of a 2-D uint8 / uint16 / int16 / float32 raster (method 'linear', q taken as float64), float64; NaN
    when the raster holds a NaN, as numpy gives."""
    return _percentile(arr, q, EXCLUDE_NAN, True, ctx)


def stretch_percentile_u8(arr, lo, hi, ctx: Context | None = None):
    """clip(((a - lo) / (hi - lo)) * 255, 0, 255).astype(uint8) in float64 (global_align.py:97-101); zeros unless hi > lo."""
    c = _ctx(ctx)
    a = as_image(arr)
    out = np.empty(a.shape, np.uint8)
    c.check(c.lib.km_stretch_percentile_u8(c.handle, ptr(a), dtype_code(a), a.shape[0], a.shape[1], row_stride(a), float(lo), float(hi),
                                           ptr(out)), "km_stretch_percentile_u8")
    return out


def _as_prep_raster(arr):
    """Dtypes outside the four go through astype(float32) on the host first, as the reference's _to_uint8 does for every input."""
    a = np.asarray(arr)
    if a.ndim != 2:
        raise KariosHipError(f"expected a 2-D image, got shape {a.shape}")
    return np.ascontiguousarray(a if a.dtype in PREP_DTYPES else a.astype(np.float32))


def _preprocess_resident(arr, q, clahe_args, ctx):
    """_to_uint8 [+ CLAHE] with one upload: order statistics, stretch and CLAHE through the _dev entry points on pooled device
    buffers, the host synchronisation of the interpolation in between."""
    c = _ctx(ctx)
    a = _as_prep_raster(arr)
    H, W = a.shape
    code = dtype_code(a)
    qq = np.asarray(q, np.float64).reshape(-1) / 100
    held = []

    def alloc(nbytes):
        p, cap = c.dev_alloc(nbytes)
        held.append((p, cap))
        return C.c_void_p(p)

    try:
        if a.dtype == np.uint8:
            d_u8 = alloc(a.nbytes)                          # _to_uint8: uint8 passes through untouched
            c.check(c.lib.km_h2d(c.handle, d_u8, ptr(a), a.nbytes), "km_h2d")
        else:
            d_raw, d_u8 = alloc(a.nbytes), alloc(H * W)
            c.check(c.lib.km_h2d(c.handle, d_raw, ptr(a), a.nbytes), "km_h2d")
            n, v0, v1, vi = _stats_call(c, c.lib.km_order_statistics_dev, "km_order_statistics_dev", (d_raw, code, H, W, W),
                                        EXCLUDE_NONFINITE, qq)
            if n == 0:
                lo = hi = float("nan")                      # nothing finite: zeros
            else:
                lo, hi = lerp_linear(v0, v1, vi, n, np.float32)   # the reference ranks arr.astype(float32): float32 arithmetic
            c.check(c.lib.km_stretch_percentile_u8_dev(c.handle, d_raw, code, H, W, W, float(lo), float(hi), d_u8, W),
                    "km_stretch_percentile_u8_dev")
        d_res = d_u8
        if clahe_args is not None:
            clip_limit, (tiles_x, tiles_y) = clahe_args
            d_res = alloc(H * W)
            c.check(c.lib.km_clahe_dev(c.handle, d_u8, H, W, W, float(clip_limit), int(tiles_x), int(tiles_y), d_res, W), "km_clahe_dev")
        out = np.empty((H, W), np.uint8)
        c.check(c.lib.km_d2h(c.handle, ptr(out), d_res, out.nbytes), "km_d2h")
        return out
    finally:
        for p, cap in held:
            c.dev_release(p, cap)


def to_uint8_percentile(arr, q=(2.0, 98.0), ctx: Context | None = None):
    """_to_uint8 (global_align.py:87-101): stretch between the q-th percentiles of the finite values; uint8 input passes through
    untouched, nothing finite gives zeros."""
    a = np.asarray(arr)
    if a.dtype == np.uint8:
        return a
    return _preprocess_resident(a, q, None, ctx)


def clahe(img, clip_limit: float = 2.0, tile_grid=(8, 8), ctx: Context | None = None):
    """cv2.createCLAHE(clipLimit=clip_limit, tileGridSize=tile_grid).apply(img) of a uint8 image (global_align.py:106-107);
    tile_grid = (tiles along x, tiles along y)."""
    c = _ctx(ctx)
    a = as_image(img)
    if a.dtype != np.uint8:
        raise KariosHipError("clahe: expected a uint8 image")
    out = np.empty(a.shape, np.uint8)
    c.check(c.lib.km_clahe(c.handle, ptr(a), a.shape[0], a.shape[1], row_stride(a), float(clip_limit), int(tile_grid[0]), int(tile_grid[1]),
                           ptr(out)), "km_clahe")
    return out


def preprocess(arr, q=(2.0, 98.0), clip_limit: float = 2.0, tile_grid=(8, 8), ctx: Context | None = None):
    """_preprocess (global_align.py:104-108): _to_uint8, then CLAHE; the raster is uploaded once and stays on the device in between."""
    return _preprocess_resident(arr, q, (clip_limit, tile_grid), ctx)


# ---- descriptor matching of the align step (csrc/api_match.hip) -------------------------------------------------------------------
DESCRIPTOR_DIM = 128


def _as_descriptors(arr, what):
    """uint8 or float32 [n, 128] with contiguous rows, as sift.detectAndCompute returns them; ValueError for anything else."""
    a = np.asarray(arr)
    if a.ndim != 2 or a.shape[1] != DESCRIPTOR_DIM:
        raise ValueError(f"{what}: expected descriptors of shape [n, {DESCRIPTOR_DIM}], got {a.shape}")
    if a.dtype != np.uint8 and a.dtype != np.float32:
        raise ValueError(f"{what}: expected uint8 or float32 descriptors, got {a.dtype}")
    if a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or (a.shape[0] > 1 and a.strides[0] < DESCRIPTOR_DIM * a.itemsize):
        raise ValueError(f"{what}: rows must be contiguous")
    return a


def _u8_descriptors(a, what):
    """float32 descriptors as uint8; ValueError (naming the element) when one is not an integer in 0 .. 255."""
    if a.dtype == np.uint8:
        return a
    with np.errstate(invalid="ignore"):
        bad = ~((a >= 0) & (a <= 255) & (a == np.trunc(a)))
    if bad.any():
        r, col = np.argwhere(bad)[0]
        raise ValueError(f"{what}: element (row {r}, column {col}) = {a[r, col]!r} is not an integer in 0 .. 255")
    return a.astype(np.uint8)


def knn_match(query, train, k: int = 2, ctx: Context | None = None):
    """cv2.BFMatcher(NORM_L2).knnMatch(query, train, k) (global_align.py:178-179, 193) for k = 1 or 2 -> (idx int32 [n, k],
    dist float32 [n, k]): the train rows ranked by (float32 distance, train index); columns beyond len(train) hold -1 / +inf."""
    q, t = _as_descriptors(query, "knn_match query"), _as_descriptors(train, "knn_match train")
    if k not in (1, 2):
        raise ValueError(f"knn_match: k = {k} (1 or 2)")
    q, t = _u8_descriptors(q, "knn_match query"), _u8_descriptors(t, "knn_match train")
    idx = np.full((q.shape[0], k), -1, np.int32)
    dist = np.full((q.shape[0], k), np.inf, np.float32)
    if q.shape[0] and t.shape[0]:
        c = _ctx(ctx)
        c.check(c.lib.km_knn_match_u8(c.handle, ptr(q), q.shape[0], row_stride(q), ptr(t), t.shape[0], row_stride(t), DESCRIPTOR_DIM, int(k),
                                      ptr(idx), ptr(dist)), "km_knn_match_u8")
    return idx, dist


def match_lowe_mutual(desc_mon, desc_ref, ratio: float = 0.75, ctx: Context | None = None):
    """knnMatch(mon, ref, 2), Lowe's ratio test, knnMatch(ref, mon, 1) and the mutual check (global_align.py:178-202) in one call
    -> (query_idx int32, train_idx int32, distance float32, (raw, lowe, mutual)): the mutual rows in ascending mon index.  float32
    descriptors must hold integers 0 .. 255 (KariosHipError with code E_ARG otherwise)."""
    m, r = _as_descriptors(desc_mon, "match_lowe_mutual mon"), _as_descriptors(desc_ref, "match_lowe_mutual ref")
    if m.dtype != r.dtype:
        raise ValueError(f"match_lowe_mutual: descriptor dtypes differ ({m.dtype}, {r.dtype})")
    n = m.shape[0]
    qi, ti, dist = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
    counts = (C.c_int * 3)(n, 0, 0)
    if n and r.shape[0]:
        c = _ctx(ctx)
        c.check(c.lib.km_match_lowe_mutual(c.handle, ptr(m), n, row_stride(m), ptr(r), r.shape[0], row_stride(r), dtype_code(m), DESCRIPTOR_DIM,
                                           float(ratio), n, ptr(qi), ptr(ti), ptr(dist), counts), "km_match_lowe_mutual")
    k = counts[2]
    return qi[:k], ti[:k], dist[:k], (counts[0], counts[1], counts[2])


# ---- RANSAC homography of the align step (csrc/api_ransac.hip) --------------------------------------------------------------------
RANSAC_STATS = ("ran", "evaluated", "best_iter", "best_count", "lm_iters", "first_batch", "batches")


def _as_points(arr, what):
    """float32 [n, 2] whose rows hold x, y next to each other (a row stride is fine); cv2's [n, 1, 2] is accepted."""
    a = np.asarray(arr)
    if a.ndim == 3 and a.shape[1] == 1:
        a = a[:, 0, :]
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{what}: expected points of shape [n, 2], got {a.shape}")
    if a.dtype != np.float32:
        a = a.astype(np.float32)
    if a.strides[1] != 4 or a.strides[0] % 4 or (a.shape[0] > 1 and a.strides[0] < 8):
        a = np.ascontiguousarray(a)
    return a


def find_homography(src_pts, dst_pts, ransac_reproj_threshold: float = 3.0, max_iters: int = 10000, confidence: float = 0.999,
                    ctx: Context | None = None, return_stats: bool = False, return_iterations: bool = False):
    """cv2.findHomography(src_pts, dst_pts, cv2.RANSAC, ransac_reproj_threshold, maxIters=max_iters, confidence=confidence)
    (global_align.py:223-230) -> (matrix float64 [3, 3] or None, mask uint8 [n, 1]), cv2's return shape.  Points: float32 [n, 2]
    numpy arrays, or torch tensors on the context's device (the device form; the mask still comes back as a numpy array).
    return_stats adds a dict of RANSAC_STATS; return_iterations adds (inlier counts, valid flags) of every evaluated iteration."""
    c = _ctx(ctx)
    on_device = hasattr(src_pts, "data_ptr")
    if on_device:
        import torch
        s, d = src_pts, dst_pts
        if s.dtype != torch.float32 or d.dtype != torch.float32 or s.dim() != 2 or d.dim() != 2 or s.shape[1] != 2 or d.shape[1] != 2:
            raise ValueError("find_homography: device points must be float32 tensors of shape [n, 2]")
        if s.stride(1) != 1 or d.stride(1) != 1:
            raise ValueError("find_homography: x and y of a device point must be adjacent")
        n, ss, sd = s.shape[0], (s.stride(0) if s.shape[0] > 1 else 2), (d.stride(0) if d.shape[0] > 1 else 2)
        d_mask = torch.zeros(max(n, 1), dtype=torch.uint8, device=s.device)
        args = (C.c_void_p(s.data_ptr()), ss, C.c_void_p(d.data_ptr()), sd)
        mask_arg, fn, what = C.c_void_p(d_mask.data_ptr()), c.lib.km_find_homography_ransac_dev, "km_find_homography_ransac_dev"
        torch.cuda.synchronize(s.device)
    else:
        s, d = _as_points(src_pts, "find_homography src_pts"), _as_points(dst_pts, "find_homography dst_pts")
        n, ss, sd = s.shape[0], (s.strides[0] // 4 if s.shape[0] > 1 else 2), (d.strides[0] // 4 if d.shape[0] > 1 else 2)
        args = (ptr(s), ss, ptr(d), sd)
        mask = np.zeros((n, 1), np.uint8)
        mask_arg, fn, what = ptr(mask), c.lib.km_find_homography_ransac, "km_find_homography_ransac"
    if d.shape[0] != n:
        raise ValueError(f"find_homography: {n} source points, {d.shape[0]} destination points")
    H = np.zeros(9, np.float64)
    found = C.c_int(0)
    stats = (C.c_int64 * 8)()
    room = max(int(max_iters), 1)
    it_counts = np.zeros(room if return_iterations else 0, np.int32)
    it_valid = np.zeros(room if return_iterations else 0, np.int32)
    c.check(fn(c.handle, *args, n, float(ransac_reproj_threshold), int(max_iters), float(confidence), H.ctypes.data_as(C.POINTER(C.c_double)),
               mask_arg, C.byref(found), stats, ptr(it_counts) if return_iterations else None, ptr(it_valid) if return_iterations else None), what)
    if on_device:
        mask = d_mask[:n].cpu().numpy().reshape(n, 1)
    out = (H.reshape(3, 3) if found.value else None, mask)
    if return_stats:
        out += (dict(zip(RANSAC_STATS, (int(v) for v in stats))),)
    if return_iterations:
        k = int(stats[1])
        out += ((it_counts[:k], it_valid[:k]),)
    return out


# ---- SIFT of the align step (csrc/api_sift.hip) -------------------------------------------------------------------------------------
SIFT_KEYPOINT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32),
                                ("response", np.float32), ("octave", np.int32)])
SIFT_FIELDS = SIFT_KEYPOINT_DTYPE.names


def _sift_stats(stats):
    n = int(stats[0])
    per = [int(v) for v in stats[4:4 + 3 * n]]
    return {"octaves": n, "before_dedup": int(stats[1]), "after_dedup": int(stats[2]), "workspace_bytes": int(stats[3]),
            "candidates": per[0::3], "refined": per[1::3], "keypoints": per[2::3]}


SIFT_STAGES = ("blur_dog", "scan", "refine", "orient", "describe")


def _sift_times(stats):
    """Microseconds: device time per stage and octave (between stream events), host time of the final order and of the call."""
    n = int(stats[0])
    out = {"base": int(stats[52]), "sort_host": int(stats[53]), "gather": int(stats[54]), "call_host": int(stats[55])}
    for k, name in enumerate(SIFT_STAGES):
        out[name] = [int(stats[56 + 5 * o + k]) for o in range(n)]
    return out

def sift_capacity_estimate(H, W):
    """Room the first call gives the outputs: one key point per 16 pixels (textures measure one per 30 to 40) and a little."""
    return H * W // 16 + 256


def sift_detect_and_compute(image, *, contrast_threshold: float = 0.02, edge_threshold: float = 10, n_octave_layers: int = 3,
                            sigma: float = 1.6, descriptor_dtype=np.float32, return_stats: bool = False, capacity: int | None = None,
                            ctx: Context | None = None):
    """cv2.SIFT_create(nfeatures=0, nOctaveLayers=, contrastThreshold=, edgeThreshold=, sigma=).detectAndCompute(image, None)
    (global_align.py:48-50, 160-166) -> (key points, descriptors [n, 128] of descriptor_dtype: uint8 or float32, the same integers).
    A uint8 numpy image (rows contiguous, a row stride is fine) gives a structured array of SIFT_KEYPOINT_DTYPE and a numpy array;
    a uint8 torch tensor on the context's device gives a dict of device tensors keyed by SIFT_FIELDS and a device tensor - nothing
    but the count and the records of the final order travel to the host.  The outputs are sized by an estimate (`capacity`
    overrides it: the result is then the first `capacity` key points of the final order, and only the stats' count tells that
    there are more); when there are more key points than the estimate the call is repeated once with room for all of them.
    return_stats adds a dict: octaves, candidates / refined / keypoints per octave, before_dedup, after_dedup, workspace_bytes, count, times_us (microseconds per stage), regrows (candidate list, key-point list), calls."""
    ddt = np.dtype(descriptor_dtype)
    if ddt != np.uint8 and ddt != np.float32:
        raise ValueError(f"sift_detect_and_compute: descriptor_dtype {ddt} (uint8 or float32)")
    on_device = hasattr(image, "data_ptr")
    if on_device:
        import torch
        if image.dtype != torch.uint8 or image.dim() != 2 or (image.shape[1] > 1 and image.stride(1) != 1):
            raise ValueError("sift_detect_and_compute: expected a 2-D uint8 tensor with contiguous rows")
        H, W = int(image.shape[0]), int(image.shape[1])
        stride = int(image.stride(0)) if H > 1 else W
        img_arg = C.c_void_p(image.data_ptr())
        what = "km_sift_detect_and_compute_dev"
    else:
        a = np.asarray(image)
        if a.dtype != np.uint8:
            raise ValueError(f"sift_detect_and_compute: expected a uint8 image, got {a.dtype}")
        a = as_image(a)
        H, W = a.shape
        stride = row_stride(a)
        img_arg = ptr(a)
        what = "km_sift_detect_and_compute"
    if H < 1 or W < 1:
        raise ValueError(f"sift_detect_and_compute: empty image {H} x {W}")
    c = _ctx(ctx)                                                  # after the argument checks: they need no device
    fn = getattr(c.lib, what)
    if on_device:
        torch.cuda.synchronize(image.device)
    cap = int(capacity) if capacity is not None else sift_capacity_estimate(H, W)
    count = C.c_int(0)
    stats = (C.c_int64 * 160)()
    code = _lib._DTYPES[ddt]
    for attempt in range(2):
        if on_device:
            fields = torch.empty((6, max(cap, 1)), dtype=torch.float32, device=image.device)
            desc = torch.empty((max(cap, 1), DESCRIPTOR_DIM), dtype=torch.uint8 if ddt == np.uint8 else torch.float32, device=image.device)
            fp = [C.c_void_p(fields[k].data_ptr()) for k in range(6)]
            dp = C.c_void_p(desc.data_ptr())
        else:
            fields = np.empty((6, max(cap, 1)), np.float32)
            desc = np.empty((max(cap, 1), DESCRIPTOR_DIM), ddt)
            fp = [ptr(fields[k]) for k in range(6)]
            dp = ptr(desc)
        rc = fn(c.handle, img_arg, H, W, stride, 0, int(n_octave_layers), float(contrast_threshold), float(edge_threshold), float(sigma),
                cap, *fp, dp, code, DESCRIPTOR_DIM, C.byref(count), stats)
        if rc == _lib.E_CAPACITY and attempt == 0 and capacity is None:
            cap = count.value
            continue
        if rc != _lib.E_CAPACITY:
            c.check(rc, what)
        break
    n = min(count.value, cap)
    if on_device:
        kp = {name: fields[k, :n] for k, name in enumerate(SIFT_FIELDS[:5])}
        kp["octave"] = fields[5, :n].view(torch.int32)
        out = (kp, desc[:n])
    else:
        kp = np.empty(n, SIFT_KEYPOINT_DTYPE)
        for k, name in enumerate(SIFT_FIELDS[:5]):
            kp[name] = fields[k, :n]
        kp["octave"] = fields[5, :n].view(np.int32)
        out = (kp, desc[:n])
    if return_stats:
        st = _sift_stats(stats)
        st["count"] = count.value
        st["times_us"] = _sift_times(stats)
        st["regrows"] = (int(stats[136]), int(stats[137]))
        st["calls"] = attempt + 1
        out += (st,)
    return out


# ---- KariosAPI.analyze_accuracy (csrc/api_accuracy.hip, k_accuracy.hip) ------------------------------------------------------------
ACCURACY_STAT_NAMES = tuple(f"{k}_{col}" for col in "xyc" for k in ("min", "max", "median", "mean", "std"))
ACCURACY_MAX_ROWS = 1 << 24          # beyond it float32(n) is not n: numpy on the host


def _on_device(a):
    return hasattr(a, "data_ptr")


def _torch_np_dtype(t):
    return np.dtype(str(t.dtype).replace("torch.", ""))


def _raster_arg(a, what, dtype=None):
    """A 2-D raster with contiguous rows, numpy array or device tensor -> (on device, pointer argument, numpy dtype, H, W, row
    stride, device or None).  `dtype` names the pixel type of a tensor that only stores its bit pattern."""
    if not _on_device(a):
        a = as_image(a)
        return False, ptr(a), a.dtype, a.shape[0], a.shape[1], row_stride(a), None
    if a.dim() != 2 or (a.shape[1] > 1 and a.stride(1) != 1):
        raise ValueError(f"{what}: expected a 2-D tensor with contiguous rows")
    dt = _torch_np_dtype(a)
    if dtype is not None:
        if np.dtype(dtype).itemsize != dt.itemsize:
            raise ValueError(f"{what}: pixel type {np.dtype(dtype)} in {dt} storage")
        dt = np.dtype(dtype)
    H, W = int(a.shape[0]), int(a.shape[1])
    return True, C.c_void_p(a.data_ptr()), dt, H, W, (int(a.stride(0)) if H > 1 else W), a.device


def _mask_arg(mask, dev, H, W, what):
    """The optional uint8 mask of an H x W raster, living where the raster lives -> (pointer argument or None, row stride)."""
    if mask is None:
        return None, 0
    if dev:
        import torch
        if not _on_device(mask) or mask.dtype != torch.uint8 or tuple(mask.shape) != (H, W) or (W > 1 and mask.stride(1) != 1):
            raise ValueError(f"{what}: the mask must be a uint8 tensor of the raster's shape with contiguous rows")
        return C.c_void_p(mask.data_ptr()), (int(mask.stride(0)) if H > 1 else W)
    m = np.asarray(mask)
    if m.shape != (H, W):
        raise ValueError(f"{what}: mask shape differs from the raster's")
    m = as_image(m if m.dtype == np.uint8 else (m != 0).astype(np.uint8))
    return ptr(m), row_stride(m)


def _empty(shape, np_dtype, device):
    """An uninitialised tensor on `device`, or a numpy array when `device` is None."""
    if device is None:
        return np.empty(shape, np_dtype)
    import torch
    return torch.empty(shape, dtype=getattr(torch, np.dtype(np_dtype).name), device=device)


def count_valid_pixels(arr, mask=None, ctx: Context | None = None) -> int:
    """np.count_nonzero of `arr` with the pixels under mask == 0 set to 0 (core.py:284-290): a 2-D uint8 / uint16 / int16 /
    float32 raster and an optional uint8 mask of its shape, both numpy arrays or both torch tensors on the context's device (rows
    contiguous, a row stride is fine).  float32 counts by its bits: NaN and denormals are non-zero, -0.0 is zero."""
    dev, img_arg, dt, H, W, stride, device = _raster_arg(arr, "count_valid_pixels")
    mask_arg, mstride = _mask_arg(mask, dev, H, W, "count_valid_pixels")
    what = "km_count_valid_pixels_dev" if dev else "km_count_valid_pixels"
    if dt not in PREP_DTYPES:
        raise KariosHipError(f"count_valid_pixels: unsupported pixel type {dt} (uint8, uint16, int16, float32)")
    if H < 1 or W < 1:
        return 0
    c = _ctx(ctx)
    if dev:
        import torch
        torch.cuda.synchronize(device)
    n = C.c_int64()
    c.check(getattr(c.lib, what)(c.handle, img_arg, _lib._DTYPES[dt], H, W, stride, mask_arg, mstride, C.byref(n)), what)
    return int(n.value)


class AccuracyStatistics:
    """Result of `accuracy_statistics`: `sample` rows above the threshold, `n_nan` of them with a NaN in dx or dy, `stats` a dict of
    np.float32 by ACCURACY_STAT_NAMES (None for an empty sample), `ce` one np.float32 per percent (None where the reference's
    index expression raises IndexError), `path` "device" or "host"."""

    def __init__(self, sample, n_nan, stats, ce, path):
        self.sample, self.n_nan, self.stats, self.ce, self.path = sample, n_nan, stats, ce, path


def _ce_ranks(percent, n):
    """compute_percentile's indices (accuracy_statistics.py:231-236) -> (k - 1, k, p - k) or None where it raises IndexError."""
    if n == 0:
        return None
    p = float(percent) * n
    k = int(p)
    return (k - 1, k, p - k) if 0 <= k < n else None


def _accuracy_host(dx, dy, score, confidence, carto, factor, percents):
    """The reference's own numpy expressions (accuracy_statistics.py:82-238) on host arrays of any dtype."""
    dx, dy, score = np.asarray(dx), np.asarray(dy), np.asarray(score)
    keep = score > confidence
    x, y, c = dx[keep], (-dy if carto else dy)[keep], score[keep]
    n = int(x.size)
    n_nan = int(np.count_nonzero(np.isnan(x) | np.isnan(y)))
    stats = None
    if n:
        with np.errstate(invalid="ignore"):
            vals = [f(v) for v in (x, y, c) for f in (np.min, np.max, np.median, np.mean, np.std)]
        stats = dict(zip(ACCURACY_STAT_NAMES, vals))
    ce = []
    if percents:
        xs, ys = x * factor, y * factor
        v_s = np.sort(np.sqrt(xs * xs + ys * ys))
        for percent in percents:
            r = _ce_ranks(percent, n)
            ce.append(None if r is None else v_s[r[0]] + (v_s[r[1]] - v_s[r[0]]) * r[2])
    return AccuracyStatistics(n, n_nan, stats, tuple(ce), "host")


def accuracy_statistics(dx, dy, score, confidence, carto: bool = False, factor=1.0, percents=(0.9, 0.95), ctx: Context | None = None):
    """GeometricStat's numbers (accuracy_statistics.py:82-238) for the columns dx, dy, score of a frame -> AccuracyStatistics: the
    sample `score > confidence` (a Python float compares in float32 like `Series.gt`, an np.float64 in float64), dy negated with
    `carto`, minimum / maximum / median / mean / standard deviation of x, y and the score as numpy computes them in float32, and
    compute_percentile(percent, factor) for every percent.  float32 numpy arrays, or float32 torch tensors on the context's
    device: the sample, the sums and the order statistics are computed on the GPU and 96 bytes come back.  numpy on the host takes
    the call where the GPU form is not defined: columns that are not float32, more than 2^24 rows, an np.float64 `factor` (numpy
    then computes the radial errors in float64) and - after the device call reported it - a NaN in dx or dy of the sample."""
    percents = tuple(float(p) for p in percents)
    dev = _on_device(dx)
    if dev != _on_device(dy) or dev != _on_device(score):
        raise ValueError("accuracy_statistics: dx, dy and score must all be numpy arrays or all be device tensors")

    def to_host(a):
        return a.detach().cpu().numpy() if dev else np.asarray(a)

    cols = (dx, dy, score)
    if dev:
        import torch
        f32_cols = all(a.dtype == torch.float32 and a.dim() == 1 and a.is_contiguous() for a in cols)
        n = int(dx.shape[0])
    else:
        cols = tuple(np.asarray(a) for a in cols)
        f32_cols = all(a.dtype == np.float32 and a.ndim == 1 for a in cols)
        n = int(cols[0].shape[0]) if cols[0].ndim else 0
    if any(int(a.shape[0]) != n for a in cols if len(a.shape)):
        raise ValueError("accuracy_statistics: dx, dy and score differ in length")
    if len(percents) > _lib.ACC_MAX_PERCENTS or any(not p >= 0 for p in percents):
        raise ValueError(f"accuracy_statistics: at most {_lib.ACC_MAX_PERCENTS} percents, none negative")
    if not f32_cols or n > ACCURACY_MAX_ROWS or isinstance(factor, np.float64) or not isinstance(confidence, (float, int, np.floating, np.integer)):
        return _accuracy_host(*(to_host(a) for a in cols), confidence, carto, factor, percents)
    thr = float(confidence) if isinstance(confidence, np.float64) else float(np.float32(confidence))
    c = _ctx(ctx)
    if dev:
        torch.cuda.synchronize(dx.device)
    else:
        cols = tuple(np.ascontiguousarray(a) for a in cols)
    what = "km_accuracy_stats_dev" if dev else "km_accuracy_stats"
    res = _lib.AccuracyResult()
    q = (C.c_double * max(len(percents), 1))(*percents)
    c.check(getattr(c.lib, what)(c.handle, *_col_args(dev, cols, n), n, thr, int(bool(carto)), float(np.float32(factor)), len(percents), q, C.byref(res)), what)
    if res.n_nan:
        return _accuracy_host(*(to_host(a) for a in cols), confidence, carto, factor, percents)
    sample = int(res.sample)
    stats = dict(zip(ACCURACY_STAT_NAMES, np.array(res.stats, np.float32))) if sample else None
    order = np.array(res.order, np.float32)
    ce = []
    for k, percent in enumerate(percents):
        r = _ce_ranks(percent, sample)
        # the interpolation of accuracy_statistics.py:237 on the two float32 order statistics (the fraction is a Python float)
        ce.append(None if r is None else order[2 * k] + (order[2 * k + 1] - order[2 * k]) * r[2])
    return AccuracyStatistics(sample, 0, stats, tuple(ce), "device")


# ---- ChipService.generate_chips (csrc/api_chips.hip km_chip_select / km_chips, k_chips.hip) ----------------------------------------
CHIP_SIZE = _lib.CHIP_SIZE
CHIP_KSIZES = (1, 3, 5, 7, 9, 11)


def _f32_columns(cols, what, names):
    """The columns of one call, all numpy or all device tensors -> (on device, columns as the library reads them, rows)."""
    dev = _on_device(cols[0])
    if any(_on_device(a) != dev for a in cols):
        raise ValueError(f"{what}: {names} must all be numpy arrays or all be device tensors")
    if dev:
        import torch
        if any(a.dtype != torch.float32 or a.dim() != 1 or not a.is_contiguous() for a in cols):
            raise ValueError(f"{what}: {names} must be contiguous 1-D float32 tensors")
    else:
        cols = tuple(np.asarray(a) for a in cols)
        if any(a.dtype != np.float32 or a.ndim != 1 for a in cols):
            raise ValueError(f"{what}: {names} must be 1-D float32 arrays")
        cols = tuple(np.ascontiguousarray(a) for a in cols)
    n = int(cols[0].shape[0])
    if any(int(a.shape[0]) != n for a in cols):
        raise ValueError(f"{what}: {names} differ in length")
    return dev, cols, n


def _col_args(dev, cols, n):
    if not n:
        return [None] * len(cols)
    return [C.c_void_p(a.data_ptr()) for a in cols] if dev else [ptr(a) for a in cols]


def select_chip_points(x0, y0, score, width, height, threshold, grid=(5, 5), ctx: Context | None = None):
    """CenterAndQuarterCellPointSelector.select_points (report/chip_service.py:46-306) on the rows with score >= threshold, for
    float32 columns: the row indices (int32) in the reference's output order - per cell of the `grid` (rows, cols) over a
    width x height image the row nearest to the centre, then one row per quarter.  A Python-float threshold compares in float32
    like the reference's frame does, an np.float64 in float64.  numpy columns give a numpy array, device tensors a device tensor."""
    dev, cols, n = _f32_columns((x0, y0, score), "select_chip_points", "x0, y0 and score")
    rows, ncols = (int(v) for v in grid)
    if not (1 <= rows <= _lib.CHIP_MAX_GRID and 1 <= ncols <= _lib.CHIP_MAX_GRID):
        raise ValueError(f"select_chip_points: grid {grid} (1 .. {_lib.CHIP_MAX_GRID} cells per axis)")
    if n > _lib.CHIP_SELECT_MAX_ROWS:
        raise ValueError(f"select_chip_points: {n} rows (at most 2^24)")
    c = _ctx(ctx)
    cap = rows * ncols * _lib.CHIP_PICKS
    count = C.c_int32()
    tail = (n, int(width), int(height), float(threshold), int(isinstance(threshold, np.float64)), rows, ncols)
    if dev:
        import torch
        torch.cuda.synchronize(cols[0].device)
    out = _empty(cap, np.int32, cols[0].device if dev else None)
    what = "km_chip_select_dev" if dev else "km_chip_select"
    c.check(getattr(c.lib, what)(c.handle, *_col_args(dev, cols, n), *tail, *_col_args(dev, (out,), cap), C.byref(count)), what)
    return out[:count.value]


class ChipImages:
    """Result of `extract_chips` for n rows: `ok` (n, bool), `windows` (n, 4: X0, Y0 of ref and X1, Y1 of mon, the chip centres),
    `ref_raw` / `mon_raw` (n, 57, 57 in the rasters' type), `ref_u8` / `mon_u8`, `ref_lap` / `mon_lap` (uint8; None without a
    kernel size).  Rows that are not ok are zero in every image."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def chip_ksize(k):
    """Kernel size argument of the library: None -> 0 (no Laplacian), else one of CHIP_KSIZES."""
    if k is None:
        return 0
    if int(k) != k or int(k) not in CHIP_KSIZES:
        raise ValueError(f"Laplacian kernel size {k} (one of {CHIP_KSIZES} or None)")
    return int(k)


def extract_chips(ref, mon, x0, y0, dx, dy, ksize_ref=None, ksize_mon=None, ctx: Context | None = None) -> ChipImages:
    """The chips of `_to_chips_gdal_dataset` (report/chip_service.py:544-648) for the rows x0, y0, dx, dy (float32): the 57 x 57
    windows of `ref` around (int(x0), int(y0)) and of `mon` around (round(x0 + dx), round(y0 + dy)), their uint8 stretch by each
    chip's own minimum and maximum and, with a kernel size, cv2.Laplacian(u8, CV_8U, ksize) of each chip.  Rasters: 2-D uint8 /
    uint16 / int16 / float32 of one type, each at least 57 x 57 (windows of wider buffers are fine); numpy in gives numpy out,
    device tensors in give device tensors out."""
    kr, km = chip_ksize(ksize_ref), chip_ksize(ksize_mon)
    dev, cols, n = _f32_columns((x0, y0, dx, dy), "extract_chips", "x0, y0, dx and dy")
    if dev != _on_device(ref) or dev != _on_device(mon):
        raise ValueError("extract_chips: rasters and columns must all be numpy arrays or all be device tensors")
    if n > _lib.CHIP_MAX_ROWS:
        raise ValueError(f"extract_chips: {n} rows (at most 2^20)")
    if dev and any(a.dim() != 2 or (a.shape[1] > 1 and a.stride(1) != 1) for a in (ref, mon)):
        raise ValueError("extract_chips: expected 2-D tensors with contiguous rows")
    _, ref_arg, dt, Hr, Wr, sref, device = _raster_arg(ref, "extract_chips")
    _, mon_arg, dt_m, Hm, Wm, smon, _ = _raster_arg(mon, "extract_chips")
    if dt != dt_m or dt not in PREP_DTYPES:
        raise KariosHipError(f"extract_chips: rasters of {dt} and {dt_m} (one of uint8, uint16, int16, float32 for both)")
    if min(Hr, Wr, Hm, Wm) < CHIP_SIZE:
        raise ValueError(f"extract_chips: rasters of {(Hr, Wr)} and {(Hm, Wm)} (at least {CHIP_SIZE} x {CHIP_SIZE})")
    shape = (n, CHIP_SIZE, CHIP_SIZE)
    res = ChipImages(ok=_empty((n,), np.uint8, device), windows=_empty((n, 4), np.int32, device), ref_raw=_empty(shape, dt, device),
                     mon_raw=_empty(shape, dt, device), ref_u8=_empty(shape, np.uint8, device), mon_u8=_empty(shape, np.uint8, device),
                     ref_lap=_empty(shape, np.uint8, device) if kr else None, mon_lap=_empty(shape, np.uint8, device) if km else None)
    if n:
        c = _ctx(ctx)
        if dev:
            import torch
            torch.cuda.synchronize(device)
        out = _lib.ChipOutputs(*((a.data_ptr() if dev else a.ctypes.data) if a is not None else None
                                 for a in (res.ref_raw, res.mon_raw, res.ref_u8, res.mon_u8, res.ref_lap, res.mon_lap, res.ok, res.windows)))
        what = "km_chips_dev" if dev else "km_chips"
        c.check(getattr(c.lib, what)(c.handle, ref_arg, mon_arg, _lib._DTYPES[dt], Hr, Wr, Hm, Wm, sref, smon, *_col_args(dev, cols, n), n, kr, km, C.byref(out)),
                what)
        if dev:
            c.sync()
    res.ok = res.ok != 0
    return res


# ---- the tracker's outlier clip (csrc/api_accuracy.hip km_sigma_clip_dev, k_clip.hip) -----------------------------------------------
CLIP_MAX_ROWS = _lib.CLIP_MAX_ROWS


def _sigma_clip_host(dx, dy):
    """`frames.sigma_clip` with the number of rounds: numpy's own expressions on host arrays of any dtype and length."""
    dx, dy = np.asarray(dx), np.asarray(dy)
    alive, rounds = np.arange(len(dx)), 0
    with np.errstate(all="ignore"):
        while len(alive):
            u, v = dx[alive], dy[alive]
            off_u, off_v = np.abs(u - u.mean()), np.abs(v - v.mean())
            ok = (off_u < 3.0 * u.std()) & (off_v < 3.0 * v.std()) & (off_u < 20.0) & (off_v < 20.0)
            rounds += 1
            if ok.all():
                break
            alive = alive[ok]
    return alive, rounds


def sigma_clip_batch(units, ctx: Context | None = None):
    """The reference's iterative 3-sigma / 20-px outlier clip (klt.py:52-71, `frames.sigma_clip`) for up to 16 independent
    (dx, dy) column pairs in ONE device launch -> [(indices of the survivors in row order, rounds computed), ...].  Every pair is two
    float32 numpy arrays (indices come back as an int64 array) or two contiguous float32 torch tensors on the context's device (an
    int64 tensor on that device).  The means and standard deviations are numpy's float32 ones bit for bit, so the indices are
    `frames.sigma_clip`'s.  numpy on the host takes a numpy pair the device form does not hold: another dtype, more than 32768 rows."""
    units = [(dx, dy) for dx, dy in units]
    if not 1 <= len(units) <= _lib.UNITS_PER_SUBMISSION:
        raise ValueError(f"sigma_clip_batch: 1 .. {_lib.UNITS_PER_SUBMISSION} column pairs per call")
    dev = _on_device(units[0][0])
    if any(_on_device(a) != dev for pair in units for a in pair):
        raise ValueError("sigma_clip_batch: all columns must be numpy arrays or all be device tensors")
    k = len(units)
    tab = lambda: (C.c_void_p * k)()
    t_dx, t_dy, t_keep, ns = tab(), tab(), tab(), (C.c_int * k)()
    res = np.zeros((k, 2), np.int32)
    if dev:
        import torch
        for dx, dy in units:
            if any(a.dtype != torch.float32 or a.dim() != 1 or not a.is_contiguous() for a in (dx, dy)) or dx.shape != dy.shape:
                raise ValueError("sigma_clip_batch: expected two contiguous 1-D float32 tensors of equal length")
            if dx.shape[0] > CLIP_MAX_ROWS:
                raise KariosHipError(f"sigma_clip_batch: {dx.shape[0]} rows (the device form holds {CLIP_MAX_ROWS})")
        device = units[0][0].device
        keeps = [torch.empty(max(int(dx.shape[0]), 1), dtype=torch.int32, device=device) for dx, _ in units]
        d_res = torch.zeros((k, 2), dtype=torch.int32, device=device)
        for i, (dx, dy) in enumerate(units):
            ns[i] = int(dx.shape[0])
            t_dx[i], t_dy[i], t_keep[i] = dx.data_ptr(), dy.data_ptr(), keeps[i].data_ptr()
        c = _ctx(ctx)
        torch.cuda.synchronize(device)                       # the library runs on its own stream
        c.check(c.lib.km_sigma_clip_dev(c.handle, t_dx, t_dy, ns, k, t_keep, C.c_void_p(d_res.data_ptr())), "km_sigma_clip_dev")
        c.sync()
        res = d_res.cpu().numpy()
        return [(keeps[i][:int(res[i, 0])].to(torch.int64), int(res[i, 1])) for i in range(k)]
    cols = [(np.asarray(dx), np.asarray(dy)) for dx, dy in units]
    for dx, dy in cols:
        if dx.ndim != 1 or dx.shape != dy.shape:
            raise ValueError("sigma_clip_batch: expected two 1-D arrays of equal length")
    on_host = [dx.dtype != np.float32 or dy.dtype != np.float32 or len(dx) > CLIP_MAX_ROWS for dx, dy in cols]
    if all(on_host):
        return [_sigma_clip_host(dx, dy) for dx, dy in cols]
    if any(on_host):
        out = iter(sigma_clip_batch([p for p, h in zip(cols, on_host) if not h], ctx))
        return [_sigma_clip_host(*p) if h else next(out) for p, h in zip(cols, on_host)]
    c = _ctx(ctx)
    up = lambda n: (max(n, 1) * 4 + 255) & ~255
    total = sum(3 * up(len(dx)) for dx, _ in cols) + 256
    base, cap = c.dev_alloc(total)
    try:
        at = base
        keep_at = []
        for i, (dx, dy) in enumerate(cols):
            n = len(dx)
            ns[i] = n
            for tbl, a in ((t_dx, dx), (t_dy, dy)):
                tbl[i] = at
                if n:
                    a = np.ascontiguousarray(a)
                    c.check(c.lib.km_h2d(c.handle, C.c_void_p(at), ptr(a), n * 4), "km_h2d")
                at += up(n)
            t_keep[i] = at
            keep_at.append(at)
            at += up(n)
        c.check(c.lib.km_sigma_clip_dev(c.handle, t_dx, t_dy, ns, k, t_keep, C.c_void_p(at)), "km_sigma_clip_dev")
        c.check(c.lib.km_d2h(c.handle, ptr(res), C.c_void_p(at), res.nbytes), "km_d2h")
        out = []
        for i in range(k):
            keep = np.empty(int(res[i, 0]), np.int32)
            if keep.size:
                c.check(c.lib.km_d2h(c.handle, ptr(keep), C.c_void_p(keep_at[i]), keep.nbytes), "km_d2h")
            out.append((keep.astype(np.int64), int(res[i, 1])))
        return out
    finally:
        c.dev_release(base, cap)


def sigma_clip(dx, dy, ctx: Context | None = None, return_rounds: bool = False):
    """`frames.sigma_clip(dx, dy)` on the device: the indices of the displacements that survive the reference's outlier loop
    (klt.py:52-71).  numpy in / numpy out, or device tensors in / a device tensor out; `return_rounds`: (indices, rounds)."""
    keep, rounds = sigma_clip_batch([(dx, dy)], ctx)[0]
    return (keep, rounds) if return_rounds else keep


# ---- the report's numbers (csrc/api_prep.hip km_display_range, csrc/api_report.hip km_mean_profiles, k_report.hip) ------------------
DISPLAY_MAX_NO_VALUES = _lib.DISPLAY_MAX_NO_VALUES
PROFILE_MAX, PROFILE_MAX_ROWS, PROFILE_MAX_BIN = _lib.PROFILE_MAX, _lib.PROFILE_MAX_ROWS, _lib.PROFILE_MAX_BIN


class DisplayRange:
    """Result of `display_range`: `values` one per percent (`v_min` the first, `v_max` the last) with the value and type
    np.percentile returns - or, when no pixel is valid, np.nanmin / np.nanmax of the raster; `n_valid`, `n_invalid`; `raster_min` /
    `raster_max` in the raster's type (a zero as +0.0, NaN for a raster of nothing but NaN)."""

    def __init__(self, values, n_valid, n_invalid, raster_min, raster_max):
        self.values, self.n_valid, self.n_invalid, self.raster_min, self.raster_max = values, n_valid, n_invalid, raster_min, raster_max
        self.v_min, self.v_max = (values[0], values[-1]) if len(values) else (None, None)


def _lerp_as_numpy(v0, v1, vi, n, dtype):
    """np.percentile's interpolation between its two neighbours -> one scalar per quantile, as numpy returns them: float64 through
    `lerp_linear` for the integer types; for float32 every step in float32, the virtual index included."""
    if np.dtype(dtype) != np.float32:
        return list(lerp_linear(v0, v1, vi, n, dtype))
    f32 = np.float32
    out = []
    with np.errstate(all="ignore"):
        for a, b, v in zip(np.asarray(v0, np.float64).astype(f32), np.asarray(v1, np.float64).astype(f32), np.asarray(vi, np.float64).astype(f32)):
            prev = f32(-1) if v >= n - 1 else np.floor(v)
            gamma = f32(v - prev)
            diff = f32(b - a)
            out.append(f32(b - f32(diff * f32(f32(1) - gamma))) if gamma >= 0.5 else f32(a + f32(diff * gamma)))
    return out


def _display_range_lists(no_values, percents):
    values = [] if no_values is None else [float(v) for v in no_values]
    if len(values) > DISPLAY_MAX_NO_VALUES:
        raise ValueError(f"display_range: {len(values)} DN values (at most {DISPLAY_MAX_NO_VALUES})")
    pp = [float(p) for p in percents]
    if any(not 0 <= p <= 100 for p in pp):
        raise ValueError("Percentiles must be in the range [0, 100]")
    return values, pp


def display_range(arr, mask=None, no_values=None, nodata=None, percents=(0.5, 99.5), ctx: Context | None = None) -> DisplayRange:
    """The display range of OverviewPlot._plot_image (report/overview_plot.py:134-194) of a 2-D uint8 / uint16 / int16 / float32
    raster: np.percentile(valid, p) for every p of `percents`, valid = the pixels that are finite, not zero and not invalid;
    invalid = `mask == 0` (optional uint8 mask of the raster's shape) | np.isin(arr, no_values) (at most 16 DN values) |
    arr == nodata.  Without a valid pixel the range is np.nanmin / np.nanmax of the raster (two percents).  Raster and mask are both
    numpy arrays or both torch tensors on the context's device (rows contiguous; windows of wider buffers are fine, each with its own
    pitch).  A Python-number `nodata` compares with a float32 raster in float32 as numpy's does, an np.float64 in float64."""
    values, pp = _display_range_lists(no_values, percents)
    dev, img_arg, dt, H, W, stride, device = _raster_arg(arr, "display_range")
    mask_arg, mstride = _mask_arg(mask, dev, H, W, "display_range")
    what = "km_display_range_dev" if dev else "km_display_range"
    if dt not in PREP_DTYPES:
        raise KariosHipError(f"display_range: unsupported pixel type {dt} (uint8, uint16, int16, float32)")
    if H < 1 or W < 1:
        raise ValueError("display_range: empty raster")
    c = _ctx(ctx)
    if dev:
        import torch
        torch.cuda.synchronize(device)
    return _display_range_call(c, what, img_arg, dt, H, W, stride, mask_arg, mstride, values, nodata, pp)


def _display_range_call(c, what, img_arg, dt, H, W, stride, mask_arg, mstride, values, nodata, pp):
    """The library call behind `display_range` and `ResidentPair.display_ranges`: checked arguments in, a `DisplayRange` out."""
    if nodata is not None:
        with np.errstate(over="ignore"):
            nodata = float(np.float32(nodata)) if dt == np.float32 and type(nodata) in (int, float) else float(nodata)
    # the quantile as np.percentile forms it: in float32 for a float32 raster
    with np.errstate(all="ignore"):
        q = np.array([float(np.true_divide(p, np.float32(100) if dt == np.float32 else 100)) for p in pp], np.float64)
    res = _lib.DisplayRangeResult()
    v0, v1, vi = np.full(q.size, np.nan), np.full(q.size, np.nan), np.full(q.size, np.nan)
    nv = np.array(values, np.float64)
    pd = C.POINTER(C.c_double)
    c.check(getattr(c.lib, what)(c.handle, img_arg, _lib._DTYPES[dt], H, W, stride, mask_arg, mstride,
                                 C.byref(C.c_double(nodata)) if nodata is not None else None, nv.ctypes.data_as(pd) if nv.size else None, nv.size,
                                 q.size, q.ctypes.data_as(pd), C.byref(res), v0.ctypes.data_as(pd), v1.ctypes.data_as(pd), vi.ctypes.data_as(pd)), what)
    with np.errstate(all="ignore"):
        rmin, rmax = dt.type(res.raster_min), dt.type(res.raster_max)
    n = int(res.n_valid)
    if n > 0:
        out = _lerp_as_numpy(v0, v1, vi, n, dt)
    else:
        out = [rmin, rmax] if q.size == 2 else [dt.type(np.nan) if dt.kind == "f" else None] * q.size
    return DisplayRange(out, n, int(res.n_invalid), rmin, rmax)


class ProfileColumns:
    """One profile of `mean_profiles`: `key` (float32, the groups' np.floor_divide(positions, bin_size), ascending), `position`
    (int32, the reference's groups_positions), `count` (int32 rows whose value is not NaN), `mean` and `std` (float32); numpy arrays,
    or device tensors for device input."""

    def __init__(self, key, position, count, mean, std):
        self.key, self.position, self.count, self.mean, self.std = key, position, count, mean, std


def mean_profiles(profiles, ctx: Context | None = None):
    """`mean_profile` (report/commons.py:49-71) of 1 .. 8 profiles in one call: `profiles` is a sequence of (values, positions,
    bin_size) with float32 columns of one length (at most 2^20 rows; all numpy or all device tensors) and 1 <= bin_size <= 2^24
    -> a list of `ProfileColumns`.  ValueError when a group's position lies outside int32, where numpy's cast is not defined."""
    profiles = [tuple(p) for p in profiles]
    if not 1 <= len(profiles) <= PROFILE_MAX:
        raise ValueError(f"mean_profiles: {len(profiles)} profiles (1 .. {PROFILE_MAX} per call)")
    cols = []
    for values, positions, _bin in profiles:
        cols += [values, positions]
    dev, cols, n = _f32_columns(tuple(cols), "mean_profiles", "values and positions")
    if n > PROFILE_MAX_ROWS:
        raise ValueError(f"mean_profiles: {n} rows (at most 2^20)")
    bins = []
    for _v, _p, b in profiles:
        if int(b) != b or not 1 <= int(b) <= PROFILE_MAX_BIN:
            raise ValueError(f"mean_profiles: bin size {b} (an integer, 1 .. 2^24)")
        bins.append(int(b))
    c = _ctx(ctx)
    k = len(profiles)
    recs = (_lib.Profile * k)()
    outs = []
    if dev:
        import torch
        torch.cuda.synchronize(cols[0].device)
    for i in range(k):
        o = [_empty(n, t, cols[0].device if dev else None) for t in (np.float32, np.int32, np.int32, np.float32, np.float32)]
        outs.append(o)
        args = _col_args(dev, (cols[2 * i], cols[2 * i + 1]) + tuple(o), n)
        r = recs[i]
        r.values, r.positions, r.key, r.position, r.count, r.mean, r.std = [C.cast(a, C.c_void_p).value if a is not None else None for a in args]
        r.bin_size = bins[i]
    groups, oor = (C.c_int32 * k)(), (C.c_int32 * k)()
    what = "km_mean_profiles_dev" if dev else "km_mean_profiles"
    c.check(getattr(c.lib, what)(c.handle, n, k, recs, groups, oor), what)
    if any(oor):
        raise ValueError(f"mean_profiles: {sum(oor)} group position(s) outside int32")
    return [ProfileColumns(*(a[:groups[i]] for a in outs[i])) for i in range(k)]


# ---- the report's products and the altitude figure's numbers (csrc/api_report.hip km_point_rasters, km_sample_points, km_box_stats,
# k_products.hip) --------------------------------------------------------------------------------------------------------------------
BOX_STAT_NAMES = ("q1", "med", "q3", "iqr", "cilo", "cihi", "whislo", "whishi")     # the columns of km_box_stats, in its order


def _raster_shape(shape, what):
    H, W = (int(v) for v in shape)
    if H < 1 or W < 1 or H * W >= 2 ** 32 - 1:
        raise ValueError(f"{what}: a raster of {H} x {W} (at least 1 x 1, fewer than 2^32 - 1 pixels)")
    return H, W


def _out_plane(out, shape, np_dtype, dev, device, what):
    """The caller's buffer for one output - a window of a wider buffer is fine - or a fresh one."""
    if out is None:
        return _empty(shape, np_dtype, device)
    if _on_device(out) != dev:
        raise ValueError(f"{what}: the output must live where the columns live")
    dt = _torch_np_dtype(out) if dev else out.dtype
    strides = tuple(out.stride()) if dev else tuple(s // out.itemsize for s in out.strides)
    if dt != np.dtype(np_dtype) or tuple(out.shape) != tuple(shape) or (shape[-1] > 1 and strides[-1] != 1) or (not dev and not out.flags.writeable):
        raise ValueError(f"{what}: the output must be a writable {np.dtype(np_dtype).name} buffer of shape {tuple(shape)} with contiguous rows")
    return out


def point_rasters(x0, y0, dx=None, dy=None, shape=None, mask=True, delta=True, out_mask=None, out_delta=None, ctx: Context | None = None):
    """ProductGenerator._create_mask / _create_intermediate_raster (report/product_generator.py:138-218) minus the file: for float32
    key-point columns and a raster `shape` (H, W) -> (`mask`, `delta`): the uint8 H x W raster with 1 at every key point and the
    float32 2 x H x W raster of NaN with dx / dy at the key points (None for the one not asked for; `dx = dy = None` gives the mask
    alone).  Pixels are `x0.astype(int)`, `y0.astype(int)`; columns wrap as numpy's assignment into a row buffer does, rows do not;
    of several rows on one pixel the last wins.  numpy columns give numpy rasters, device tensors device tensors; `out_mask` /
    `out_delta` may name the buffers to fill (windows of wider buffers included).  IndexError, as from the reference, when a row lies
    outside the raster or has a NaN or infinite coordinate."""
    delta = bool(delta) and dx is not None
    mask = bool(mask)
    if (dx is None) != (dy is None):
        raise ValueError("point_rasters: dx and dy come together")
    if shape is None:
        raise ValueError("point_rasters: the raster's shape is needed")
    H, W = _raster_shape(shape, "point_rasters")
    dev, cols, n = _f32_columns((x0, y0) + ((dx, dy) if delta else ()), "point_rasters", "x0, y0, dx and dy")
    if n > PROFILE_MAX_ROWS:
        raise ValueError(f"point_rasters: {n} rows (at most 2^20)")
    device = cols[0].device if dev else None
    m = _out_plane(out_mask, (H, W), np.uint8, dev, device, "point_rasters") if mask else None
    d = _out_plane(out_delta, (2, H, W), np.float32, dev, device, "point_rasters") if delta else None
    c = _ctx(ctx)
    if dev:
        import torch
        torch.cuda.synchronize(device)
    args = _col_args(dev, cols, n) + [None] * (4 - len(cols))

    def plane(a):
        return None if a is None else (C.c_void_p(a.data_ptr()) if dev else ptr(a))

    def strides(a):
        return tuple(int(s) for s in a.stride()) if dev else tuple(s // a.itemsize for s in a.strides)
    ms = (strides(m)[0] if H > 1 else W) if mask else 0
    bs, rs = ((strides(d)[0], strides(d)[1] if H > 1 else W) if delta else (0, 0))
    bad = C.c_int32()
    what = "km_point_rasters_dev" if dev else "km_point_rasters"
    c.check(getattr(c.lib, what)(c.handle, n, *args, H, W, plane(m), ms, plane(d), bs, rs, C.byref(bad)), what)
    if bad.value:
        raise IndexError(f"point_rasters: {bad.value} row(s) out of bounds for a raster of {H} x {W}")
    return m, d


def sample_points(raster, x0, y0, dtype=None, ctx: Context | None = None):
    """`raster[y0.astype(int), x0.astype(int)]` (the altitude column, api/core.py:1049-1053) of a 2-D uint8 / uint16 / int16 /
    float32 raster for float32 columns: numpy's fancy indexing, negative indices counted from the end, in the raster's type.
    Raster and columns are all numpy arrays or all tensors on the context's device (rows contiguous; a window of a wider buffer is
    fine).  `dtype` names the pixel type of a tensor that only stores its bit pattern (uint16 in int16 storage); the result keeps
    the storage type.  IndexError where numpy raises it, and for a NaN or infinite coordinate."""
    dev, cols, n = _f32_columns((x0, y0), "sample_points", "x0 and y0")
    if _on_device(raster) != dev:
        raise ValueError("sample_points: raster and columns must all be numpy arrays or all be device tensors")
    _, img_arg, dt, H, W, stride, device = _raster_arg(raster, "sample_points", dtype)
    if dt not in PREP_DTYPES:
        raise KariosHipError(f"sample_points: unsupported pixel type {dt} (uint8, uint16, int16, float32)")
    if H < 1 or W < 1:
        raise ValueError("sample_points: empty raster")
    if n > PROFILE_MAX_ROWS:
        raise ValueError(f"sample_points: {n} rows (at most 2^20)")
    c = _ctx(ctx)
    if dev:
        import torch
        torch.cuda.synchronize(device)
    out = _empty(n, _torch_np_dtype(raster) if dev else dt, device)      # (a tensor's storage type)
    bad = C.c_int32()
    what = "km_sample_points_dev" if dev else "km_sample_points"
    c.check(getattr(c.lib, what)(c.handle, img_arg, _lib._DTYPES[dt], H, W, stride, n, *_col_args(dev, cols + (out,), n), C.byref(bad)), what)
    if bad.value:
        raise IndexError(f"sample_points: {bad.value} row(s) out of bounds for a raster of {H} x {W}")
    return out


class BoxStats:
    """Result of `box_stats`: per group `key` (float32, ascending), `count` (int32, NaN values included), `mean` (float32) and the
    float64 columns `q1`, `med`, `q3`, `iqr`, `cilo`, `cihi`, `whislo`, `whishi`; `cls` (int8) per ROW: 0 inside the whiskers, 1
    below, 2 above, -1 for a row without a group.  numpy arrays, or device tensors for device input."""

    def __init__(self, key, count, mean, stats, cls):
        self.key, self.count, self.mean, self.cls = key, count, mean, cls
        for name, col in zip(BOX_STAT_NAMES, stats):
            setattr(self, name, col)


def box_stats(values, positions, bin_size, ctx: Context | None = None) -> BoxStats:
    """matplotlib.cbook.boxplot_stats(x, whis=1.5) of every group of `mean_profile` (np.floor_divide(positions, bin_size), the
    groups ascending), x the group's values in row order: float32 columns of one length (at most 2^20 rows; numpy or device
    tensors), 1 <= bin_size <= 2^24 -> `BoxStats`.  The fliers of a group are its rows of class 1 in row order, then those of
    class 2 (`box_fliers`)."""
    dev, cols, n = _f32_columns((values, positions), "box_stats", "values and positions")
    if n > PROFILE_MAX_ROWS:
        raise ValueError(f"box_stats: {n} rows (at most 2^20)")
    if int(bin_size) != bin_size or not 1 <= int(bin_size) <= PROFILE_MAX_BIN:
        raise ValueError(f"box_stats: bin size {bin_size} (an integer, 1 .. 2^24)")
    c = _ctx(ctx)
    k = _lib.BOX_STATS
    device = cols[0].device if dev else None
    if dev:
        import torch
        torch.cuda.synchronize(device)
    key, count, mean = (_empty(n, t, device) for t in (np.float32, np.int32, np.float32))
    stats, cls = _empty((k, n), np.float64, device), _empty(n, np.int8, device)
    groups = C.c_int32()
    a = _col_args(dev, cols + (key, count, mean, stats, cls), n)
    what = "km_box_stats_dev" if dev else "km_box_stats"
    c.check(getattr(c.lib, what)(c.handle, n, a[0], a[1], int(bin_size), *a[2:], C.byref(groups)), what)
    g = groups.value
    return BoxStats(key[:g], count[:g], mean[:g], [stats[j, :g] for j in range(k)], cls)


# ---- the circular-error figure's numbers (csrc/api_report.hip km_ce_figure, k_ce.hip) ------------------------------------------------
CE_MAX_BINS = _lib.CE_MAX_BINS      # bins of one axis histogram the device counts; beyond it numpy on a host copy
CE_FIELDS = ("hist_x", "bins_x", "hist_y", "bins_y", "mu_x", "sigma_x", "mu_y", "sigma_y", "scatter_x", "scatter_y", "scatter_z", "counts2d",
             "x_edges", "y_edges", "radial", "plot_limit", "ce90", "ce95", "sample")


class CeFigure:
    """Result of `ce_figure`, what `CircularErrorPlot._plot` hands to matplotlib: `hist_x` (int64) on `bins_x` (float32 edges) and
    the same for y; `mu_*`, `sigma_*` of the scaled columns (np.float32); `scatter_x`, `scatter_y`, `scatter_z` in drawing order
    and `radial` ascending (float32, `sample` rows; device tensors for device input); `counts2d` (float64, 10 x 10) on `x_edges`,
    `y_edges`; `plot_limit`, `ce90`, `ce95` (np.float32).  `path` is "device" or "host"; `host_hist_x` / `host_hist_y` tell that
    numpy counted that axis on a host copy (more than CE_MAX_BINS bins); `n_outside` points lie outside the grid of bin centres
    (NaN density, drawn last)."""

    def __init__(self, **kw):
        self.path, self.host_hist_x, self.host_hist_y, self.n_outside = "device", False, False, 0
        self.__dict__.update(kw)


def _ce_histogram_host(vect, img_res):
    """`_compute_histogram`'s numpy expression (circular_error_plot.py:185-207)."""
    v_max = np.max([np.abs(np.max(vect)), np.abs(np.min(vect))])
    return np.histogram(vect * img_res, bins="sqrt", range=(-v_max * img_res, v_max * img_res))


def _ce_host(dx, dy, score, threshold, img_res, carto):
    """The reference's own numpy / scipy expressions (circular_error_plot.py:181-228, 254-303, 359-368) on host arrays of any dtype;
    only the drawing order is this project's: stable."""
    from scipy.interpolate import interpn
    dx, dy, score = np.asarray(dx), np.asarray(dy), np.asarray(score)
    keep = score > threshold
    vx, vy = dx[keep], (-dy if carto else dy)[keep]
    r = CeFigure(path="host", sample=int(vx.size))
    (r.hist_x, r.bins_x), (r.hist_y, r.bins_y) = _ce_histogram_host(vx, img_res), _ce_histogram_host(vy, img_res)
    x, y = vx * img_res, vy * img_res
    with np.errstate(invalid="ignore"):
        r.mu_x, r.sigma_x, r.mu_y, r.sigma_y = np.mean(x), np.std(x), np.mean(y), np.std(y)
        r.plot_limit = np.max([np.max(np.abs(x)), np.max(np.abs(y))])
        r.counts2d, r.x_edges, r.y_edges = np.histogram2d(x, y, bins=10)
        z = interpn((0.5 * (r.x_edges[1:] + r.x_edges[:-1]), 0.5 * (r.y_edges[1:] + r.y_edges[:-1])), r.counts2d, np.vstack([x, y]).T,
                    method="splinef2d", bounds_error=False)
        idx = np.argsort(z, kind="stable")
        r.scatter_x, r.scatter_y, r.scatter_z = x[idx], y[idx], z[idx]
        r.radial = np.sort(np.sqrt(x * x + y * y))
    r.n_outside = int(np.count_nonzero(np.isnan(z)))
    r.ce90, r.ce95 = _accuracy_host(dx, dy, score, threshold, carto, img_res, (0.9, 0.95)).ce
    return r


def _ce_axis_edges(lo, hi, v_min, v_max, n, res32):
    """np.histogram(bins="sqrt", range=...)'s edges (numpy/lib/_histograms_impl.py `_get_bin_edges`) from the extremes of the unscaled
    (lo, hi) and the scaled (v_min, v_max) column of n rows -> float32 edges."""
    bound = max(np.float32(abs(hi)), np.float32(abs(lo)))
    last = np.float32(bound * res32)
    first = np.float32(-last)
    if first == last:
        first, last = np.float32(first - np.float32(0.5)), np.float32(last + np.float32(0.5))
    width = np.float32(v_max - v_min) / np.sqrt(n)
    n_bins = int(np.ceil(np.float32(last - first) / width)) if width else 1
    edges = np.linspace(first, last, n_bins + 1, endpoint=True, dtype=np.float32)
    if np.any(edges[:-1] >= edges[1:]):
        raise ValueError(f"Too many bins for data range. Cannot create {n_bins} finite-sized bins.")
    return edges


def _ce_grid_edges(lo, hi):
    """np.histogramdd's edges of one axis: 11 float32 edges over [min, max], widened by 0.5 when they are equal."""
    if lo == hi:
        lo, hi = np.float32(lo - np.float32(0.5)), np.float32(hi + np.float32(0.5))
    return np.linspace(lo, hi, 11)


def ce_figure(dx, dy, score, threshold, img_res, carto: bool = False, ctx: Context | None = None) -> CeFigure:
    """Every array and scalar `CircularErrorPlot._plot` (karios/report/circular_error_plot.py) hands to matplotlib, for the columns dx,
    dy, score of a frame, the confidence threshold (compared as `accuracy_statistics` compares it), the resolution `img_res` (a
    Python float: the products are float32) and `carto` -> `CeFigure`.  float32 numpy arrays, or float32 torch tensors on the
    context's device: then no column crosses to the host - 64 bytes of extremes and sizes, the counts of the three histograms and
    32 bytes of final scalars do; numpy builds the bin edges and scipy fits the 10 x 10 spline from those, the GPU counts, evaluates
    the spline per point, sorts and gathers.  The drawing order is the stable one (np.argsort(z, kind="stable")).  ValueError for
    an empty sample, as the reference's np.max raises.  numpy / scipy on the host take the call where the GPU form is not
    defined: columns that are not float32, more than 2^24 rows, an np.float64 `img_res`, a NaN in dx or dy of the sample; and ONE
    axis histogram of more than CE_MAX_BINS bins (`host_hist_x` / `host_hist_y`)."""
    dev = _on_device(dx)
    if dev != _on_device(dy) or dev != _on_device(score):
        raise ValueError("ce_figure: dx, dy and score must all be numpy arrays or all be device tensors")

    def to_host(a):
        return a.detach().cpu().numpy() if dev else np.asarray(a)

    cols = (dx, dy, score)
    if dev:
        import torch
        f32_cols = all(a.dtype == torch.float32 and a.dim() == 1 and a.is_contiguous() for a in cols)
    else:
        cols = tuple(np.asarray(a) for a in cols)
        f32_cols = all(a.dtype == np.float32 and a.ndim == 1 for a in cols)
    if any(len(a.shape) != 1 for a in cols) or any(int(a.shape[0]) != int(cols[0].shape[0]) for a in cols):
        raise ValueError("ce_figure: dx, dy and score must be 1-D columns of one length")
    n = int(cols[0].shape[0])
    if isinstance(img_res, (bool, str)) or not isinstance(img_res, (float, int, np.floating, np.integer)):
        raise ValueError(f"ce_figure: img_res {img_res!r} is not a number")
    scalar_thr = isinstance(threshold, (float, int, np.floating, np.integer))
    if not f32_cols or n > ACCURACY_MAX_ROWS or isinstance(img_res, np.float64) or not scalar_thr or not np.isfinite(np.float32(img_res)):
        return _ce_host(*(to_host(a) for a in cols), threshold, img_res, carto)
    if n == 0:
        raise ValueError("ce_figure: zero-size sample: no row lies above the threshold")
    thr = float(threshold) if isinstance(threshold, np.float64) else float(np.float32(threshold))
    res32 = np.float32(img_res)
    c = _ctx(ctx)
    device = cols[0].device if dev else None
    if dev:
        torch.cuda.synchronize(device)
    else:
        cols = tuple(np.ascontiguousarray(a) for a in cols)
    what = "km_ce_figure_dev" if dev else "km_ce_figure"
    fn = getattr(c.lib, what)
    job, blk, tail = _lib.CeJob(), _lib.CeBlock(), _lib.CeTail()
    job.n, job.carto, job.thr, job.res = n, int(bool(carto)), thr, float(res32)
    job.dx, job.dy, job.score = (C.cast(a, C.c_void_p).value for a in _col_args(dev, cols, n))
    job.block, job.tail = C.pointer(blk), C.pointer(tail)

    job.stage = _lib.CE_SAMPLE
    c.check(fn(c.handle, C.byref(job)), what)
    if blk.n_nan:
        return _ce_host(*(to_host(a) for a in cols), threshold, img_res, carto)
    sample = int(blk.sample)
    if sample == 0:
        raise ValueError("ce_figure: zero-size sample: no row lies above the threshold")
    ext = np.array(blk.ext, np.float32)
    r = CeFigure(sample=sample, mu_x=np.float32(blk.mu_x), sigma_x=np.float32(blk.sigma_x), mu_y=np.float32(blk.mu_y), sigma_y=np.float32(blk.sigma_y))
    r.plot_limit = np.max(np.abs(ext[4:8]))

    # the edges: numpy's own linspace on the extremes
    r.bins_x = _ce_axis_edges(ext[0], ext[1], ext[4], ext[5], sample, res32)
    r.bins_y = _ce_axis_edges(ext[2], ext[3], ext[6], ext[7], sample, res32)
    r.x_edges, r.y_edges = _ce_grid_edges(ext[4], ext[5]), _ce_grid_edges(ext[6], ext[7])
    r.host_hist_x, r.host_hist_y = r.bins_x.size - 1 > CE_MAX_BINS, r.bins_y.size - 1 > CE_MAX_BINS
    grid = np.ascontiguousarray(np.concatenate([r.x_edges, r.y_edges]), np.float32)
    hx = np.zeros(0 if r.host_hist_x else r.bins_x.size - 1, np.uint32)
    hy = np.zeros(0 if r.host_hist_y else r.bins_y.size - 1, np.uint32)
    counts = np.zeros(100, np.uint32)
    job.stage = _lib.CE_COUNTS
    job.edges_x, job.edges_y, job.edges_grid = r.bins_x.ctypes.data, r.bins_y.ctypes.data, grid.ctypes.data
    job.bins_x, job.bins_y = hx.size, hy.size
    job.hist_x, job.hist_y, job.counts_grid = hx.ctypes.data, hy.ctypes.data, counts.ctypes.data
    c.check(fn(c.handle, C.byref(job)), what)
    r.hist_x, r.hist_y = hx.astype(np.int64), hy.astype(np.int64)
    if r.host_hist_x or r.host_hist_y:
        h_dx, h_dy, h_score = (to_host(a) for a in cols)
        keep = h_score.astype(np.float64) > thr
        if r.host_hist_x:
            r.hist_x = _ce_histogram_host(h_dx[keep], img_res)[0]
        if r.host_hist_y:
            r.hist_y = _ce_histogram_host((-h_dy if carto else h_dy)[keep], img_res)[0]
    r.counts2d = counts.astype(np.float64).reshape(10, 10)

    # the fit: scipy's own, on 100 numbers
    from scipy.interpolate import RectBivariateSpline
    cx, cy = 0.5 * (r.x_edges[1:] + r.x_edges[:-1]), 0.5 * (r.y_edges[1:] + r.y_edges[:-1])
    tx, ty, coef = (np.ascontiguousarray(a, np.float64) for a in RectBivariateSpline(cx, cy, r.counts2d).tck[:3])
    if (tx.size, ty.size, coef.size) != (14, 14, 100):
        raise KariosHipError(f"ce_figure: a spline of {tx.size} x {ty.size} knots and {coef.size} coefficients (14 x 14, 100)")
    box = np.array([cx[0], cx[-1], cy[0], cy[-1]], np.float32)
    outs = [_empty(n, np.float32, device) for _ in range(4)]
    job.stage = _lib.CE_CURVES
    job.tx, job.ty, job.coef, job.box = tx.ctypes.data, ty.ctypes.data, coef.ctypes.data, box.ctypes.data
    job.scatter_x, job.scatter_y, job.scatter_z, job.radial = (C.cast(a, C.c_void_p).value for a in _col_args(dev, outs, n))
    c.check(fn(c.handle, C.byref(job)), what)
    r.scatter_x, r.scatter_y, r.scatter_z, r.radial = (a[:sample] for a in outs)
    r.n_outside = int(tail.n_outside)
    order = np.array(tail.order, np.float32)
    ce = []
    for k, percent in enumerate((0.9, 0.95)):
        frac = _ce_ranks(percent, sample)[2]
        ce.append(order[2 * k] + (order[2 * k + 1] - order[2 * k]) * frac)       # accuracy_statistics.py:237, as `accuracy_statistics` forms it
    r.ce90, r.ce95 = ce
    return r
