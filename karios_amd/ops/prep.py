"""Preprocessing of the align step, the quality check's percentiles and the report's display range (csrc/api_prep.hip)."""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import Context, KariosHipError, as_image, dtype_code, ptr, row_stride
from ._place import Place, _ctx, _mask_arg, _raster_arg

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


# ---- the report's display range (km_display_range) ------------------------------------------------------------------------------------
DISPLAY_MAX_NO_VALUES = _lib.DISPLAY_MAX_NO_VALUES


class DisplayRange:
    """Result of `display_range`: `values` one per percent (`v_min` the first, `v_max` the last) with the value and type
    np.percentile returns - or, when no pixel is valid, np.nanmin / np.nanmax of the raster; `n_valid`, `n_invalid`; `raster_min` /
    `raster_max` in the raster's type (a zero as +0.0, NaN for a raster of nothing but NaN)."""

    def __init__(self, values, n_valid, n_invalid, raster_min, raster_max):
        self.values, self.n_valid, self.n_invalid, self.raster_min, self.raster_max = values, n_valid, n_invalid, raster_min, raster_max
        self.v_min, self.v_max = (values[0], values[-1]) if len(values) else (None, None)


def lerp_as_numpy(v0, v1, vi, n, dtype):
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


def display_range_lists(no_values, percents):
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
    values, pp = display_range_lists(no_values, percents)
    place = Place((arr,))
    img_arg, dt, H, W, stride = _raster_arg(place, arr, "display_range")
    mask_arg, mstride = _mask_arg(place, mask, H, W, "display_range")
    if dt not in PREP_DTYPES:
        raise KariosHipError(f"display_range: unsupported pixel type {dt} (uint8, uint16, int16, float32)")
    if H < 1 or W < 1:
        raise ValueError("display_range: empty raster")
    c = _ctx(ctx)
    _, what = place.function(c, "km_display_range")
    return display_range_call(c, what, img_arg, dt, H, W, stride, mask_arg, mstride, values, nodata, pp)


def display_range_call(c, what, img_arg, dt, H, W, stride, mask_arg, mstride, values, nodata, pp):
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
        out = lerp_as_numpy(v0, v1, vi, n, dt)
    else:
        out = [rmin, rmax] if q.size == 2 else [dt.type(np.nan) if dt.kind == "f" else None] * q.size
    return DisplayRange(out, n, int(res.n_invalid), rmin, rmax)
