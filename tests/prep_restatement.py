"""numpy restatement of the align step's preprocessing (karios/matcher/global_align.py:87-108: _to_uint8, _preprocess) and of the
percentiles behind it and behind the quality check (karios/api/core.py:491-506), as libkarios_hip.so computes them (k_prep.hip).

This is the DEFINITION the GPU kernels are held to, bit for bit (tests/test_gpu_prep.py).  OpenCV is absent, so parity of `clahe`
with cv2 itself is unpinned; tests/test_prep_host.py compares the two when cv2 imports.  Points marked [cv4.8]
come from knowledge of OpenCV 4.8's sources (clahe.cpp), [np2] from numpy 2.x's (lib/_function_base_impl.py), not from the
reference tree; points marked [def] are choices of this project where the reference's result is not one fixed number.

Test infrastructure only: karios_amd never imports this module.
"""
from __future__ import annotations

import numpy as np


# ---- order statistics and numpy's 'linear' percentile -----------------------------------------------------------------------------
def kept_values(arr, exclude=0):
    """The values a selection ranks: every pixel as it is; for floating point, without NaN (exclude 0) or without every
    non-finite value (exclude 1)."""
    a = np.asarray(arr).reshape(-1)
    if a.dtype.kind == "f":
        a = a[np.isfinite(a) if exclude else ~np.isnan(a)]
    return a


def order_statistics(arr, q, exclude=0):
    """-> (n, v0, v1, vi): n values kept; with vi = (n - 1) * q in float64 [np2: get_virtual_index of 'linear'], v0 = the value of
    rank floor(vi) and v1 the value of rank min(floor(vi) + 1, n - 1) in ascending order, as float64 (exact for uint8, uint16,
    int16, float32).  n = 0 -> (0, None, None, None)."""
    kept = kept_values(arr, exclude)
    n = kept.size
    if n == 0:
        return 0, None, None, None
    q = np.atleast_1d(np.asarray(q, np.float64))
    vi = np.float64(n - 1) * q
    r0 = np.clip(np.floor(vi), 0, n - 1).astype(np.int64)
    r1 = np.minimum(r0 + 1, n - 1)
    part = np.partition(kept, np.unique(np.concatenate([r0, r1])))
    return n, part[r0].astype(np.float64), part[r1].astype(np.float64), vi


def lerp(v0, v1, vi, n, dtype):
    """numpy's interpolation between the two neighbours of a 'linear' quantile [np2: _get_indexes, _get_gamma, _lerp], on arrays
    of the SOURCE dtype: `b - a` is a float32 subtraction for float32 input and wraps for int16, exactly as numpy's does.
    v0, v1: the neighbours (any float type holding them exactly), vi: virtual indexes (float64), n: values ranked.  -> float64."""
    dtype = np.dtype(dtype)
    a = np.atleast_1d(np.asarray(v0)).astype(dtype)
    b = np.atleast_1d(np.asarray(v1)).astype(dtype)
    vi = np.atleast_1d(np.asarray(vi, np.float64))
    prev = np.floor(vi)
    prev[vi >= n - 1] = -1            # [np2] at or above the last index numpy indexes the LAST element as -1 ... and gamma is taken from it
    gamma = vi - prev.astype(np.intp)
    diff = np.subtract(b, a)
    out = np.asanyarray(np.add(a, diff * gamma))
    np.subtract(b, diff * (1 - gamma), out=out, where=gamma >= 0.5, casting="unsafe", dtype=type(out.dtype))
    return out


def percentile(arr, q, exclude=0):
    """np.nanpercentile(arr, q) (exclude 0) / np.percentile(arr[isfinite(arr)], q) (exclude 1) for q a float64 sequence in [0, 100]."""
    a = np.asarray(arr)
    qq = np.true_divide(np.atleast_1d(np.asarray(q, np.float64)), 100)
    n, v0, v1, vi = order_statistics(a, qq, exclude)
    if n == 0:
        return np.full(qq.shape, np.nan)
    return lerp(v0, v1, vi, n, a.dtype)


# ---- the stretch ----------------------------------------------------------------------------------------------------------------
def stretch_u8(arr, lo, hi):
    """((a - lo) / (hi - lo)) * 255 in float64, every operation rounded on its own, clipped to [0, 255], truncated.  numpy >= 2
    evaluates the reference's expression this way (the percentiles are float64 scalars); the casts are explicit here so that the
    definition does not move with the numpy version.  NaN -> 0 [def: the C cast is undefined; x86 numpy gives 0], +inf -> 255,
    -inf -> 0.  Not (hi > lo) -> zeros."""
    a = np.asarray(arr)
    if not (hi > lo):
        return np.zeros(a.shape, np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        v = a.astype(np.float32).astype(np.float64)
        t = ((v - np.float64(lo)) / (np.float64(hi) - np.float64(lo))) * np.float64(255.0)
        t = np.clip(t, 0.0, 255.0)
    t = np.where(np.isnan(t), 0.0, t)
    return t.astype(np.uint8)


def to_uint8_percentile(arr, q=(2.0, 98.0)):
    """_to_uint8 (global_align.py:87-101): uint8 passes through; nothing finite -> zeros; percentiles of the finite values."""
    a = np.asarray(arr)
    if a.dtype == np.uint8:
        return a
    a32 = a.astype(np.float32)
    # the reference ranks the float32 copy: the interpolation is float32 arithmetic whatever the source type was
    n, v0, v1, vi = order_statistics(a32, np.asarray(q, np.float64) / 100, exclude=1)
    if n == 0:
        return np.zeros(a.shape, np.uint8)
    lo, hi = lerp(v0, v1, vi, n, np.float32)
    return stretch_u8(a32, lo, hi)


# ---- CLAHE ----------------------------------------------------------------------------------------------------------------------
def _reflect101(p, n):
    p = np.asarray(p)
    return np.where(p >= n, 2 * n - 2 - p, p)   # (one reflection: the extension is at most n - 1)


def clahe_geometry(H, W, clip_limit, tiles_x, tiles_y):
    """-> (extended H, extended W, tile_h, tile_w, clip, lut_scale) [cv4.8: CLAHE_Impl::apply]; ValueError where the library refuses."""
    if tiles_x < 1 or tiles_y < 1 or tiles_x * tiles_y * 256 > 65536:
        raise ValueError("tile grid")                                  # [def] all LUTs fit 64 KB
    if W % tiles_x == 0 and H % tiles_y == 0:
        eh, ew = H, W
    else:
        # [cv4.8] copyMakeBorder(0, tilesY - H % tilesY, 0, tilesX - W % tilesX, BORDER_REFLECT_101): a divisible dimension grows by a
        # whole tilesX / tilesY
        eh, ew = H + (tiles_y - H % tiles_y), W + (tiles_x - W % tiles_x)
    if ew - W > W - 1 or eh - H > H - 1:
        raise ValueError("the reflection does not define this border")  # [def]
    th, tw = eh // tiles_y, ew // tiles_x
    area = th * tw
    clip = 0
    if clip_limit > 0.0:
        clip = max(int(float(clip_limit) * area / 256), 1)              # [cv4.8] static_cast<int>(clipLimit * tileSizeTotal / histSize), double
    lut_scale = np.float32(255.0) / np.float32(area)                    # [cv4.8] static_cast<float>(histSize - 1) / tileSizeTotal
    return eh, ew, th, tw, clip, lut_scale


def clahe_luts(img, clip_limit=2.0, tile_grid=(8, 8)):
    """The per-tile LUTs, uint8 (tiles_y, tiles_x, 256) [cv4.8: CLAHE_CalcLut_Body]."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    tiles_x, tiles_y = int(tile_grid[0]), int(tile_grid[1])
    eh, ew, th, tw, clip, lut_scale = clahe_geometry(H, W, clip_limit, tiles_x, tiles_y)
    ys, xs = _reflect101(np.arange(eh), H), _reflect101(np.arange(ew), W)
    luts = np.empty((tiles_y, tiles_x, 256), np.uint8)
    for ty in range(tiles_y):
        rows = img[ys[ty * th:(ty + 1) * th]]
        for tx in range(tiles_x):
            hist = np.bincount(rows[:, xs[tx * tw:(tx + 1) * tw]].reshape(-1), minlength=256).astype(np.int64)
            if clip > 0:
                clipped = int(np.maximum(hist - clip, 0).sum())
                hist = np.minimum(hist, clip)
                batch = clipped // 256
                residual = clipped - batch * 256
                hist = hist + batch
                if residual != 0:
                    step = max(256 // residual, 1)
                    i = 0
                    while i < 256 and residual > 0:     # [cv4.8] for (i = 0; i < histSize && residual > 0; i += step, residual--)
                        hist[i] += 1
                        i += step
                        residual -= 1
            cum = np.cumsum(hist).astype(np.int32)
            # [cv4.8] saturate_cast<uchar>(sum * lutScale): int -> float32, one float32 multiply, cvRound (half to even), saturate
            luts[ty, tx] = np.clip(np.rint(cum.astype(np.float32) * lut_scale), 0, 255).astype(np.uint8)
    return luts


def clahe(img, clip_limit=2.0, tile_grid=(8, 8), rows_per_block=512):
    """cv2.createCLAHE(clip_limit, tile_grid).apply(img) for uint8 [cv4.8: CLAHE_Interpolation_Body]: every operation a float32
    rounding of its own, in OpenCV's order (no fused multiply-add)."""
    img = np.asarray(img)
    H, W = img.shape
    tiles_x, tiles_y = int(tile_grid[0]), int(tile_grid[1])
    _eh, _ew, th, tw, _clip, _s = clahe_geometry(H, W, clip_limit, tiles_x, tiles_y)
    luts = clahe_luts(img, clip_limit, tile_grid).astype(np.float32)
    f32 = np.float32

    def axis(n, tile, tiles):
        inv = f32(1.0) / f32(tile)
        tf = np.arange(n, dtype=np.int32).astype(f32) * inv - f32(0.5)
        t1 = np.floor(tf).astype(np.int32)
        t2 = t1 + 1
        a = tf - t1.astype(f32)
        a1 = f32(1.0) - a
        return np.maximum(t1, 0), np.minimum(t2, tiles - 1), a, a1

    tx1, tx2, xa, xa1 = axis(W, tw, tiles_x)
    ty1, ty2, ya, ya1 = axis(H, th, tiles_y)
    out = np.empty((H, W), np.uint8)
    for y0 in range(0, H, rows_per_block):
        y1 = min(y0 + rows_per_block, H)
        v = img[y0:y1].astype(np.intp)
        r1, r2 = ty1[y0:y1, None], ty2[y0:y1, None]
        top = (luts[r1, tx1[None, :], v] * xa1[None, :] + luts[r1, tx2[None, :], v] * xa[None, :]) * ya1[y0:y1, None]
        bot = (luts[r2, tx1[None, :], v] * xa1[None, :] + luts[r2, tx2[None, :], v] * xa[None, :]) * ya[y0:y1, None]
        res = top + bot
        assert res.dtype == np.float32
        out[y0:y1] = np.clip(np.rint(res), 0, 255).astype(np.uint8)
    return out


def preprocess(arr):
    """_preprocess (global_align.py:104-108)."""
    return clahe(to_uint8_percentile(arr), 2.0, (8, 8))
