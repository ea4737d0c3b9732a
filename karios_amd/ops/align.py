"""The global align step (karios/matcher/global_align.py; csrc/api_align.hip): warps, Sobel magnitude and ECC."""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import Context, KariosHipError, as_image, dtype_code, ptr, row_stride
from ._place import _ctx

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
