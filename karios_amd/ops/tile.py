"""The tile path: the calls of matcher/klt.py (csrc/api_tile.hip), the parameters of a track and two test hooks."""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import Context, KariosHipError, KltParams, as_image, dtype_code, ptr, row_stride
from ._place import Place, _ctx, _mask_arg, _raster_arg


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


def pyrlk_initial(prev_img, next_img, prev_pts, guess_pts, winSize=(25, 25), maxLevel=1, maxCount=30, epsilon=0.03,
                  ctx: Context | None = None):
    """cv2.calcOpticalFlowPyrLK(prev, next, pts, guess, winSize=, maxLevel=, criteria=, flags=cv2.OPTFLOW_USE_INITIAL_FLOW): the search
    of every point starts at its own guess (a position in `next`), not at the point -> next points (N,1,2) float32.  The reference
    never passes the flag; a geometric prior is built on it (include/karios_hip.h: km_pyrlk_initial).  maxLevel 1, winSize <= 40 and an
    image with a pyramid level 1 only: anything else is refused, nothing runs."""
    c = _ctx(ctx)
    a = np.ascontiguousarray(prev_img, np.uint8)
    b = np.ascontiguousarray(next_img, np.uint8)
    if a.shape != b.shape or a.ndim != 2:
        raise KariosHipError("pyrlk_initial: image shape mismatch")
    if winSize[0] != winSize[1]:
        raise KariosHipError("pyrlk_initial: only square windows (KARIOS uses (w, w))")
    p = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
    g = np.ascontiguousarray(guess_pts, np.float32).reshape(-1, 2)
    if g.shape != p.shape:
        raise KariosHipError("pyrlk_initial: one guess per point")
    out = np.empty_like(p)
    c.check(c.lib.km_pyrlk_initial(c.handle, ptr(a), ptr(b), a.shape[0], a.shape[1], ptr(p), ptr(g), p.shape[0], int(winSize[0]),
                                   int(maxLevel), int(maxCount), float(epsilon), ptr(out)), "km_pyrlk_initial")
    return out.reshape(-1, 1, 2)


def prior_mask(ref, mon, prior, mask=None, nodata_ref=None, nodata_mon=None, x_off=0.0, y_off=0.0, dtype=None, ctx: Context | None = None):
    """The corner mask under a geometric prior (include/karios_hip.h: km_prior_mask): 1 where `mask` (or, without one, the reference's
    half of the automatic mask, klt.py:268-273) is set, the pixel has a guess and the guess, rounded half to even, meets a valid
    pixel of `mon` inside the box -> uint8 H x W.  `prior`: 9 float64 values (matcher.prior); `x_off, y_off`: origin of the boxes in the
    coordinates the prior maps.  numpy arrays in, a numpy array out; device tensors (contiguous rows) in, a device tensor out."""
    what = "prior_mask"
    place = Place((ref, mon, mask), what, "ref, mon and the mask")
    pr, dr, H, W, sr = _raster_arg(place, ref, what, dtype)
    pm, dm, Hm, Wm, sm = _raster_arg(place, mon, what, dtype)
    if (H, W) != (Hm, Wm) or dr != dm:
        raise KariosHipError("prior_mask: ref/mon shape or dtype mismatch")
    pk, sk = _mask_arg(place, mask, H, W, what)
    P = np.ascontiguousarray(np.asarray(prior, np.float64).reshape(-1))
    if P.size != 9:
        raise KariosHipError("prior_mask: a prior has 9 values")
    out = place.empty((H, W), np.uint8)
    nr = C.byref(C.c_double(float(nodata_ref))) if nodata_ref is not None else None
    nm = C.byref(C.c_double(float(nodata_mon))) if nodata_mon is not None else None
    place.call(_ctx(ctx), "km_prior_mask", pr, pm, _lib._DTYPES[dr], H, W, sr, sm, pk, sk, nr, nm, P.ctypes.data_as(C.POINTER(C.c_double)),
               float(x_off), float(y_off), place.pointer(out))
    return out


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
    from .. import frames
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
