"""A geometric prior of the tracker: 9 float64 values, row-major, that map reference pixel coordinates to monitored pixel coordinates
(include/karios_hip.h).  Where the reference resamples the monitored raster once the pre-aligner
(`LargeOffsetMatcher`) or the align step (`detect_global_alignment`) has found the coarse geometry - `shift_image`, or `warpPerspective`
- and matches against the copy, a prior starts every key point of the tracker at its own guess on the rasters as they are:
`dx, dy` come out as total displacements and the scores are computed on the raw pixels.

`guesses` and `prior_columns` are the host's transcription of csrc/prior_math.hpp (numpy never fuses a multiplication into an addition,
so every float64 operation rounds on its own, as the definition asks)."""
from __future__ import annotations

import numpy as np

IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
PRIOR_COLUMNS = ["dx_prior", "dy_prior"]


def as_prior(prior) -> np.ndarray:
    """Nine finite float64 values (a flat sequence or a 3 x 3 matrix) -> the contiguous array the library takes."""
    p = np.ascontiguousarray(np.asarray(prior, np.float64).reshape(-1))
    if p.size != 9 or not np.isfinite(p).all():
        raise ValueError("prior: expected 9 finite values (a 3 x 3 matrix, row-major)")
    return p


def from_shift(row_off, col_off) -> np.ndarray:
    """The prior of an offset pair as `LargeOffsetMatcher.match()` returns it (row, column).  The reference shifts the monitored raster
    by it - shifted[y, x] = mon[y + row_off, x + col_off] - and adds the pair back to dx / dy (core.py:248-249): a reference pixel
    (x, y) is looked for at (x + col_off, y + row_off) of the monitored raster, and the frame's dx, dy are those totals."""
    return as_prior([1.0, 0.0, float(col_off), 0.0, 1.0, float(row_off), 0.0, 0.0, 1.0])


def from_alignment(alignment) -> np.ndarray:
    """The prior of a `GlobalAlignment` (or of its 3 x 3 `matrix`): that matrix maps monitored to reference pixel coordinates
    (global_align.py:427), the prior is its float64 `np.linalg.inv`, taken here; the 9 doubles handed down are the definition's input."""
    m = np.asarray(getattr(alignment, "matrix", alignment), np.float64).reshape(3, 3)
    return as_prior(np.linalg.inv(m))


def guesses(prior, x, y, x_off=0.0, y_off=0.0):
    """Key points (x, y) of a tile at (x_off, y_off), in the tile's coordinates -> (gx, gy, has_guess): the float32 start positions of the
    tracker, in the tile's coordinates too; rows without a guess (w not finite or <= 0) keep the key point."""
    P = as_prior(prior)
    x32, y32 = np.asarray(x, np.float32), np.asarray(y, np.float32)
    xs, ys = x32.astype(np.float64) + float(x_off), y32.astype(np.float64) + float(y_off)
    with np.errstate(all="ignore"):
        w = (P[6] * xs + P[7] * ys) + P[8]
        ok = (w > 0.0) & (w < np.inf)
        ws = np.where(ok, w, 1.0)
        qx = ((P[0] * xs + P[1] * ys) + P[2]) / ws - float(x_off)
        qy = ((P[3] * xs + P[4] * ys) + P[5]) / ws - float(y_off)
        gx = np.where(ok, qx.astype(np.float32), x32).astype(np.float32)
        gy = np.where(ok, qy.astype(np.float32), y32).astype(np.float32)
    return gx, gy, ok


def prior_columns(frame, prior, x_off=0.0, y_off=0.0):
    """`dx_prior, dy_prior` of a tile's frame (its x0, y0 carry the tile origin): the float32 g - p0 of every row, in the tile's
    coordinates - what the prior alone says the displacement is."""
    x = frame["x0"].to_numpy().astype(np.float32) - np.float32(x_off)
    y = frame["y0"].to_numpy().astype(np.float32) - np.float32(y_off)
    gx, gy, _ = guesses(prior, x, y, x_off, y_off)
    return gx - x, gy - y


def clip_residuals(frame, ctx=None):
    """The tracker's outlier clip (klt.py:52-71) under a prior: on the residuals dx - dx_prior, dy - dy_prior - what the tracker found
    beyond the prior - through `ops.sigma_clip`, in corner order (the frame's labels), as the tracker's own clip runs in front of the
    ordering.  -> the surviving rows in the frame's (x0, y0) order, labelled by their position among the survivors.  Clipping dx, dy
    themselves would measure the prior's geometry (a rotation spreads them by design), not the tracks."""
    from .. import ops
    if not len(frame):
        return frame
    labels = frame.index.to_numpy()
    corner_order = np.argsort(labels, kind="stable")
    res_dx = np.ascontiguousarray((frame["dx"].to_numpy() - frame["dx_prior"].to_numpy())[corner_order], np.float32)
    res_dy = np.ascontiguousarray((frame["dy"].to_numpy() - frame["dy_prior"].to_numpy())[corner_order], np.float32)
    keep = np.asarray(ops.sigma_clip(res_dx, res_dy, ctx=ctx))
    rows = np.sort(corner_order[keep])
    out = frame.iloc[rows].copy()
    out.index = np.argsort(np.argsort(labels[rows], kind="stable"), kind="stable")
    out.attrs = dict(frame.attrs)
    return out
