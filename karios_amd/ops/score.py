"""The scores of the key points and the large-offset search (csrc/api_score.hip)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from .. import _lib
from .._lib import Context, KariosHipError, as_image, dtype_code, ptr, row_stride
from ._place import Place, _col_args, _ctx, _f32_columns, _raster_arg


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


ZnccSearch = namedtuple("ZnccSearch", "offset peak shift status surface")
ZNCC_SKIPPED, ZNCC_NO_VALUE, ZNCC_RIM_X, ZNCC_RIM_Y = 1, 2, 4, 8          # bits of ZnccSearch.status


def _check_search(what, n, radius):
    if int(radius) != radius or not 1 <= radius <= _lib.ZNCC_SEARCH_MAX_RADIUS:
        raise ValueError(f"{what}: radius {radius!r} (an integer, 1 .. {_lib.ZNCC_SEARCH_MAX_RADIUS})")
    if n > _lib.ZNCC_SEARCH_MAX_ROWS:
        raise ValueError(f"{what}: {n} rows (at most 2^20)")


def zncc_search(ref, mon, x0, y0, dx, dy, radius: int = 4, surface: bool = False, ctx: Context | None = None):
    """The ZNCC search around each key point: for oy, ox in -radius .. radius the value `_zncc2(ref, mon, Y0, X0, Y1 + oy, X1 + ox, 21)`
    (zncc_service.py:45-126) around the centres `compute_zncc` scores (X0 = int(x0), X1 = round(x0 + dx) on the float32 sum), its
    peak and the peak's sub-pixel position; the reference's call graph has no such search (include/karios_hip.h: km_zncc_search).
    The rasters (one pixel type of uint8 / uint16 / int16 / float32) and the float32 columns are all numpy arrays or all device tensors.
    -> ZnccSearch(offset int32[n, 2] = (bx, by), peak float64[n], shift float64[n, 2] = (x, y), status uint8[n] (ZNCC_* bits),
    surface float64[n, S, S] or None), living where the inputs live."""
    what = "zncc_search"
    place = Place([ref, mon], what, "ref and mon")
    place.require([x0, y0, dx, dy], what, "the rasters and x0, y0, dx, dy")
    _, cols, n = _f32_columns((x0, y0, dx, dy), what, "x0, y0, dx, dy")
    _check_search(what, n, radius)
    radius, S = int(radius), 2 * int(radius) + 1
    pr, dr, Hr, Wr, sr = _raster_arg(place, ref, what)
    pm, dm, Hm, Wm, sm = _raster_arg(place, mon, what)
    if dr != dm or dr not in _lib._DTYPES:
        raise ValueError(f"{what}: rasters of {dr} / {dm} (one pixel type of uint8, uint16, int16, float32)")
    out = ZnccSearch(place.empty((n, 2), np.int32), place.empty((n,), np.float64), place.empty((n, 2), np.float64), place.empty((n,), np.uint8),
                     place.empty((n, S, S), np.float64) if surface else None)
    if n:
        place.call(_ctx(ctx), "km_zncc_search", pr, pm, _lib._DTYPES[dr], Hr, Wr, Hm, Wm, sr, sm, *_col_args(place, cols, n), n, radius,
                   *(place.pointer(a) for a in out))
        if place.dev:
            _ctx(ctx).sync()
    return out


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


MiSearch = namedtuple("MiSearch", "offset peak peak_mi shift status surface")      # status: the ZNCC_* bits


def mi_search(ref, mon, x0, y0, dx, dy, radius: int = 4, surface: bool = False, ctx: Context | None = None):
    """The mutual-information search around each key point, `zncc_search`'s counterpart for pairs whose contrast is non-linear or
    inverted: for oy, ox in -radius .. radius Studholme's NMI (`MutualInfoService._mutual_info`, mutual_info_service.py:32-63) of the
    57 x 57 chips at (X0, Y0) in `ref` and (X1 + ox, Y1 + oy) in `mon`, around the centres `compute_mutual_info` scores, its peak and
    the peak's sub-pixel position (include/karios_hip.h: km_mi_search; exact from the counts, the same bits on every device).
    The rasters (one pixel type of uint8 / uint16 / int16 / float32) and the float32 columns are all numpy arrays or all device tensors.
    -> MiSearch(offset int32[n, 2] = (bx, by), peak float64[n], peak_mi float64[n] (the `mi_score` formula at the peak's offset),
    shift float64[n, 2] = (x, y), status uint8[n] (ZNCC_* bits), surface float64[n, S, S] or None), living where the inputs live."""
    what = "mi_search"
    place = Place([ref, mon], what, "ref and mon")
    place.require([x0, y0, dx, dy], what, "the rasters and x0, y0, dx, dy")
    _, cols, n = _f32_columns((x0, y0, dx, dy), what, "x0, y0, dx, dy")
    _check_search(what, n, radius)
    radius, S = int(radius), 2 * int(radius) + 1
    pr, dr, Hr, Wr, sr = _raster_arg(place, ref, what)
    pm, dm, Hm, Wm, sm = _raster_arg(place, mon, what)
    if dr != dm or dr not in _lib._DTYPES:
        raise ValueError(f"{what}: rasters of {dr} / {dm} (one pixel type of uint8, uint16, int16, float32)")
    out = MiSearch(place.empty((n, 2), np.int32), place.empty((n,), np.float64), place.empty((n,), np.float64), place.empty((n, 2), np.float64),
                   place.empty((n,), np.uint8), place.empty((n, S, S), np.float64) if surface else None)
    if n:
        place.call(_ctx(ctx), "km_mi_search", pr, pm, _lib._DTYPES[dr], Hr, Wr, Hm, Wm, sr, sm, *_col_args(place, cols, n), n, radius,
                   *(place.pointer(a) for a in out))
        if place.dev:
            _ctx(ctx).sync()
    return out


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
