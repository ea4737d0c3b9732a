"""numpy restatement of ChipService.generate_chips (karios/report/chip_service.py): the key-point selection of
CenterAndQuarterCellPointSelector (:46-306), the chip windows of `_to_chips_gdal_dataset` (:567-593) and the uint8 / Laplacian
images of a chip (:37-43, :642), as libkarios_hip.so computes them (csrc/chips_math.hpp, k_chips.hip).

This is the DEFINITION the library is held to, bit for bit (tests/test_gpu_chips.py); tests/test_chips_host.py holds it to the
installed pandas and to the recorded results of the reference (tests/golden/chips.npz).  The frame's columns are float32 and meet
Python floats, so under numpy 2 / pandas 2 every intermediate of the selection is float32; every operation is spelled out one
rounding at a time.  [ref] marks the reference's expressions, [def] choices of this project where the reference raises or its
result is not one fixed value.

Test infrastructure only: karios_amd never imports this module.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
CHIP = 57
MARGIN = 28
COORD_LIMIT = float(1 << 30)      # [def] a window centre beyond it is treated like a non-finite one


def threshold_as_double(t):
    """The float64 the library compares (double)score against: a Python float compares in float32, an np.float64 in float64
    (as ops.accuracy_statistics treats its threshold)."""
    if isinstance(t, np.float64):
        return float(t)
    return float(f32(t))


# ---- selection ---------------------------------------------------------------------------------------------------------------------
def cell_bounds(cell, width, height, rows, cols):
    """[ref :140-171] float64 bounds and centre of a cell."""
    cw, ch = width / cols, height / rows
    r, c = divmod(cell, cols)
    x_start = c * cw
    x_end = (c + 1) * cw if c < cols - 1 else width
    y_start = r * ch
    y_end = (r + 1) * ch if r < rows - 1 else height
    return x_start, x_end, y_start, y_end, (x_start + x_end) / 2, (y_start + y_end) / 2


def cells_of(x0, y0, width, height, rows, cols):
    """[ref :102-115] clip(floor(x0 / float32(cell width)), 0, cols - 1), likewise for rows."""
    with np.errstate(all="ignore"):
        cx = np.floor(x0 / f32(width / cols))
        cy = np.floor(y0 / f32(height / rows))
    col = np.clip(np.nan_to_num(cx, nan=0.0), 0, cols - 1).astype(np.int64)
    row = np.clip(np.nan_to_num(cy, nan=0.0), 0, rows - 1).astype(np.int64)
    return row * cols + col


def distance(x0, y0, cx, cy):
    """[ref :173-180] sqrt((x0 - float32(cx))^2 + (y0 - float32(cy))^2), every step rounded to float32."""
    with np.errstate(all="ignore"):
        ddx, ddy = x0 - f32(cx), y0 - f32(cy)
        return np.sqrt(ddx * ddx + ddy * ddy)


def pick(key, score, rows):
    """Minimum key, then maximum score, then the first row [ref :182-198, :251-259] -> the chosen element of `rows`."""
    best = key == key.min()
    s = np.where(best, score, -np.inf)
    return int(rows[int(np.argmax(best & (s == s.max())))])


def median_f32(d):
    """np.median of a float32 array: the middle element, or float32(float32(lo + hi) / 2)."""
    s = np.sort(d)
    n = s.size
    if n & 1:
        return s[n // 2]
    with np.errstate(all="ignore"):
        return f32(f32(s[n // 2 - 1] + s[n // 2]) / f32(2))


def quarter_masks(x0, y0, bounds):
    """[ref :217-284] membership of the four quarters; the right quarters also take x0 == x_end, the bottom ones y0 == y_end."""
    x_start, x_end, y_start, y_end = bounds[:4]
    x_mid = x_start + (x_end - x_start) / 2
    y_mid = y_start + (y_end - y_start) / 2
    out = []
    for q, (xl, xh, yl, yh) in enumerate(((x_start, x_mid, y_start, y_mid), (x_mid, x_end, y_start, y_mid),
                                          (x_start, x_mid, y_mid, y_end), (x_mid, x_end, y_mid, y_end))):
        m = (x0 >= f32(xl)) & (x0 < f32(xh)) & (y0 >= f32(yl)) & (y0 < f32(yh))
        if q in (1, 3):
            m |= x0 == f32(xh)
        if q in (2, 3):
            m |= y0 == f32(yh)
        out.append(m)
    return out


def select(x0, y0, score, width, height, threshold, grid=(5, 5)):
    """Row indices into the input in the reference's output order: cells 0 .. rows * cols - 1, in a cell the centre, then quarters
    0 .. 3; empty cells and quarters are left out.  The filter is score >= threshold."""
    x0, y0, score = (np.ascontiguousarray(a, f32) for a in (x0, y0, score))
    rows, cols = int(grid[0]), int(grid[1])
    keep = np.flatnonzero(score.astype(np.float64) >= threshold_as_double(threshold))
    x, y = x0[keep], y0[keep]
    s = score[keep] + f32(0)                  # (-0 and +0 are one score)
    cell = cells_of(x, y, width, height, rows, cols)
    out = []
    for cid in range(rows * cols):
        idx = np.flatnonzero(cell == cid)
        if idx.size == 0:
            continue
        b = cell_bounds(cid, width, height, rows, cols)
        d = distance(x[idx], y[idx], b[4], b[5])
        centre = pick(d, s[idx], idx)
        out.append(centre)
        rest = idx != centre
        idx, d = idx[rest], d[rest]
        if idx.size == 0:
            continue
        for m in quarter_masks(x[idx], y[idx], b):
            if not m.any():
                continue
            dq = d[m]
            with np.errstate(all="ignore"):
                dev = np.abs(dq - median_f32(dq))
            out.append(pick(dev, s[idx][m], idx[m]))
    return keep[np.array(out, np.int64)] if out else np.zeros(0, np.int64)


# ---- windows -----------------------------------------------------------------------------------------------------------------------
def windows(x0, y0, dx, dy, ref_shape, mon_shape):
    """[ref :567-593] X0 = int(x0), X1 = round(float64(x0) + float64(dx)) (Python's round: half to even) -> X0, Y0, X1, Y1, ok.
    ok is false when a 57 x 57 window leaves its image, and [def] for a centre that is not finite or beyond 2^30 (reported as 0;
    the reference raises)."""
    cols = [np.asarray(a).astype(np.float64) for a in (x0, y0, dx, dy)]
    n = cols[0].size
    c0 = [cols[0], cols[1]]
    c1 = [cols[0] + cols[2], cols[1] + cols[3]]
    out = np.zeros((4, n), np.int64)
    ok = np.ones(n, bool)
    for k, v in enumerate(c0 + c1):
        with np.errstate(all="ignore"):
            good = np.isfinite(v) & (np.abs(v) <= COORD_LIMIT)
            r = np.trunc(v) if k < 2 else np.rint(v)
        out[k, good] = r[good].astype(np.int64)
        ok &= good
    for (X, Y), (H, W) in (((out[0], out[1]), ref_shape), ((out[2], out[3]), mon_shape)):
        ok &= (X - MARGIN >= 0) & (Y - MARGIN >= 0) & (X - MARGIN + CHIP <= W) & (Y - MARGIN + CHIP <= H)
    return out[0], out[1], out[2], out[3], ok


# ---- images ------------------------------------------------------------------------------------------------------------------------
def to_uint8(a):
    """[ref :37-43] = oracle.to_uint8: integers in float64, float32 in float32, truncation; a degenerate or all-NaN chip gives
    zeros, a NaN pixel 0."""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a.copy()
    with np.errstate(all="ignore"):
        if a.dtype == np.float32:
            fin = a[~np.isnan(a)]
            if fin.size == 0:
                return np.zeros(a.shape, np.uint8)
            mn, mx = float(fin.min()), float(fin.max())
            if not mx > mn:
                return np.zeros(a.shape, np.uint8)
            t = (a - f32(mn)) / f32(mx - mn) * f32(255)
            return np.where(np.isnan(t), f32(0), t).astype(np.int32).astype(np.uint8)
        mn, mx = float(a.min()), float(a.max())
        if not mx > mn:
            return np.zeros(a.shape, np.uint8)
        return ((a.astype(np.float64) - mn) / (mx - mn) * 255.0).astype(np.int32).astype(np.uint8)


def sobel_kernel(ksize, order):
    """OpenCV's getSobelKernels taps (order 0 or 2) as integers; ksize 1 is the 3-tap [1, -2, 1] / [0, 1, 0]."""
    if ksize == 1:
        return np.array([1, -2, 1] if order == 2 else [0, 1, 0], np.int64)
    if ksize == 3:
        return np.array([1, -2, 1] if order == 2 else [1, 2, 1], np.int64)
    ker = np.zeros(ksize + 1, np.int64)
    ker[0] = 1
    for _ in range(ksize - order - 1):
        old = ker[0]
        for j in range(1, ksize + 1):
            new = ker[j] + ker[j - 1]
            ker[j - 1] = old
            old = new
    for _ in range(order):
        old = -ker[0]
        for j in range(1, ksize + 1):
            new = ker[j - 1] - ker[j]
            ker[j - 1] = old
            old = new
    return ker[:ksize].copy()


def laplacian_u8(u8, ksize):
    """= oracle.laplacian_u8: sum of the two separable second derivatives in integers, BORDER_REFLECT_101, saturated to 0 .. 255."""
    if ksize not in (1, 3, 5, 7, 9, 11):
        raise ValueError(f"bad Laplacian ksize {ksize}")
    kd, ks = sobel_kernel(ksize, 2), sobel_kernel(ksize, 0)
    r = kd.size // 2
    p = np.pad(np.asarray(u8).astype(np.int64), r, mode="reflect")
    H, W = np.asarray(u8).shape
    hd = sum(kd[j] * p[:, j:j + W] for j in range(2 * r + 1))
    hs = sum(ks[j] * p[:, j:j + W] for j in range(2 * r + 1))
    lap = sum(ks[j] * hd[j:j + H] + kd[j] * hs[j:j + H] for j in range(2 * r + 1))
    return np.clip(lap, 0, 255).astype(np.uint8)


def images(chip, ksize):
    """-> u8, lap (None without a kernel size) of one 57 x 57 chip."""
    u8 = to_uint8(chip)
    return u8, (laplacian_u8(u8, ksize) if ksize else None)


def kernel_sizes(laplacian_ksize):
    """[ref :619-621] -> (ref, mon) kernel sizes, (0, 0) for None; an int stands for both."""
    if laplacian_ksize is None:
        return 0, 0
    if isinstance(laplacian_ksize, (int, np.integer)):
        return int(laplacian_ksize), int(laplacian_ksize)
    d = laplacian_ksize
    return int(d.get("ref", d.get("mon", 1))), int(d.get("mon", d.get("ref", 1)))


def chips(ref, mon, x0, y0, dx, dy, laplacian_ksize=None):
    """All of it for the rows of a selected frame -> dict with written, names, ref_raw, mon_raw, ref_u8, mon_u8, ref_lap, mon_lap
    (rows that are not written are zero)."""
    ref, mon = np.asarray(ref), np.asarray(mon)
    X0, Y0, X1, Y1, ok = windows(x0, y0, dx, dy, ref.shape, mon.shape)
    kr, km = kernel_sizes(laplacian_ksize)
    n = ok.size
    out = {"written": ok, "windows": np.stack([X0, Y0, X1, Y1], 1).astype(np.int32),
           "names": [(f"REF_{X0[i]}_{Y0[i]}", f"MON_{X0[i]}_{Y0[i]}") for i in range(n)],
           "ref_raw": np.zeros((n, CHIP, CHIP), ref.dtype), "mon_raw": np.zeros((n, CHIP, CHIP), mon.dtype),
           "ref_u8": np.zeros((n, CHIP, CHIP), np.uint8), "mon_u8": np.zeros((n, CHIP, CHIP), np.uint8),
           "ref_lap": np.zeros((n, CHIP, CHIP), np.uint8) if kr else None, "mon_lap": np.zeros((n, CHIP, CHIP), np.uint8) if km else None}
    for i in np.flatnonzero(ok):
        for tag, img, X, Y, k in (("ref", ref, X0[i], Y0[i], kr), ("mon", mon, X1[i], Y1[i], km)):
            chip = img[Y - MARGIN:Y - MARGIN + CHIP, X - MARGIN:X - MARGIN + CHIP]
            u8, lap = images(chip, k)
            out[f"{tag}_raw"][i], out[f"{tag}_u8"][i] = chip, u8
            if k:
                out[f"{tag}_lap"][i] = lap
    return out
