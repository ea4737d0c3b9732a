"""The scores of the key points and the large-offset search (csrc/api_score.hip)."""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import Context, KariosHipError, as_image, dtype_code, ptr, row_stride
from ._place import _ctx


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
