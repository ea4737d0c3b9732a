"""KariosAPI.analyze_accuracy (csrc/api_accuracy.hip, k_accuracy.hip) and the tracker's outlier clip (km_sigma_clip_dev, k_clip.hip)."""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import Context, KariosHipError, ptr
from ._place import Place, _col_args, _ctx, _float32_columns, _mask_arg, _raster_arg
from .prep import PREP_DTYPES

ACCURACY_STAT_NAMES = tuple(f"{k}_{col}" for col in "xyc" for k in ("min", "max", "median", "mean", "std"))
ACCURACY_MAX_ROWS = 1 << 24          # beyond it float32(n) is not n: numpy on the host


def count_valid_pixels(arr, mask=None, ctx: Context | None = None) -> int:
    """np.count_nonzero of `arr` with the pixels under mask == 0 set to 0 (core.py:284-290): a 2-D uint8 / uint16 / int16 /
    float32 raster and an optional uint8 mask of its shape, both numpy arrays or both torch tensors on the context's device (rows
    contiguous, a row stride is fine).  float32 counts by its bits: NaN and denormals are non-zero, -0.0 is zero."""
    place = Place((arr,))
    img_arg, dt, H, W, stride = _raster_arg(place, arr, "count_valid_pixels")
    mask_arg, mstride = _mask_arg(place, mask, H, W, "count_valid_pixels")
    if dt not in PREP_DTYPES:
        raise KariosHipError(f"count_valid_pixels: unsupported pixel type {dt} (uint8, uint16, int16, float32)")
    if H < 1 or W < 1:
        return 0
    n = C.c_int64()
    place.call(_ctx(ctx), "km_count_valid_pixels", img_arg, _lib._DTYPES[dt], H, W, stride, mask_arg, mstride, C.byref(n))
    return int(n.value)


class AccuracyStatistics:
    """Result of `accuracy_statistics`: `sample` rows above the threshold, `n_nan` of them with a NaN in dx or dy, `stats` a dict of
    np.float32 by ACCURACY_STAT_NAMES (None for an empty sample), `ce` one np.float32 per percent (None where the reference's
    index expression raises IndexError), `path` "device" or "host"."""

    def __init__(self, sample, n_nan, stats, ce, path):
        self.sample, self.n_nan, self.stats, self.ce, self.path = sample, n_nan, stats, ce, path


def ce_ranks(percent, n):
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
            r = ce_ranks(percent, n)
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
    place = Place((dx, dy, score), "accuracy_statistics", "dx, dy and score")
    cols, f32_cols = _float32_columns(place, (dx, dy, score))
    n = int(cols[0].shape[0]) if place.dev or cols[0].ndim else 0
    if any(int(a.shape[0]) != n for a in cols if len(a.shape)):
        raise ValueError("accuracy_statistics: dx, dy and score differ in length")
    if len(percents) > _lib.ACC_MAX_PERCENTS or any(not p >= 0 for p in percents):
        raise ValueError(f"accuracy_statistics: at most {_lib.ACC_MAX_PERCENTS} percents, none negative")
    if not f32_cols or n > ACCURACY_MAX_ROWS or isinstance(factor, np.float64) or not isinstance(confidence, (float, int, np.floating, np.integer)):
        return _accuracy_host(*(place.to_host(a) for a in cols), confidence, carto, factor, percents)
    thr = float(confidence) if isinstance(confidence, np.float64) else float(np.float32(confidence))
    res = _lib.AccuracyResult()
    q = (C.c_double * max(len(percents), 1))(*percents)
    place.call(_ctx(ctx), "km_accuracy_stats", *_col_args(place, cols, n), n, thr, int(bool(carto)), float(np.float32(factor)), len(percents), q, C.byref(res))
    if res.n_nan:
        return _accuracy_host(*(place.to_host(a) for a in cols), confidence, carto, factor, percents)
    sample = int(res.sample)
    stats = dict(zip(ACCURACY_STAT_NAMES, np.array(res.stats, np.float32))) if sample else None
    order = np.array(res.order, np.float32)
    ce = []
    for k, percent in enumerate(percents):
        r = ce_ranks(percent, sample)
        # the interpolation of accuracy_statistics.py:237 on the two float32 order statistics (the fraction is a Python float)
        ce.append(None if r is None else order[2 * k] + (order[2 * k + 1] - order[2 * k]) * r[2])
    return AccuracyStatistics(sample, 0, stats, tuple(ce), "device")


# ---- the tracker's outlier clip ----------------------------------------------------------------------------------------------------
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
    place = Place([a for pair in units for a in pair], "sigma_clip_batch", refusal="all columns must be numpy arrays or all be device tensors")
    k = len(units)
    tab = lambda: (C.c_void_p * k)()
    t_dx, t_dy, t_keep, ns = tab(), tab(), tab(), (C.c_int * k)()
    res = np.zeros((k, 2), np.int32)
    if place.dev:
        for dx, dy in units:
            if not _float32_columns(place, (dx, dy))[1] or dx.shape != dy.shape:
                raise ValueError("sigma_clip_batch: expected two contiguous 1-D float32 tensors of equal length")
            if dx.shape[0] > CLIP_MAX_ROWS:
                raise KariosHipError(f"sigma_clip_batch: {dx.shape[0]} rows (the device form holds {CLIP_MAX_ROWS})")
        keeps = [place.empty(max(int(dx.shape[0]), 1), np.int32) for dx, _ in units]
        d_res = place.empty((k, 2), np.int32)
        d_res[...] = 0
        for i, (dx, dy) in enumerate(units):
            ns[i] = int(dx.shape[0])
            t_dx[i], t_dy[i], t_keep[i] = place.address(dx), place.address(dy), place.address(keeps[i])
        c = _ctx(ctx)
        place.call(c, "km_sigma_clip", t_dx, t_dy, ns, k, t_keep, place.pointer(d_res))
        c.sync()
        res = place.to_host(d_res)
        return [(keeps[i][:int(res[i, 0])].long(), int(res[i, 1])) for i in range(k)]
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
