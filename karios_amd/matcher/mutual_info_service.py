"""Studholme normalised mutual information of the matched key points on MI355X, behind
`karios.matcher.mutual_info_service.MutualInfoService` (reference `mutual_info_service.py:32-130`): per key point the 57x57
chips around `(int(x0), int(y0))` / `(round(x0 + dx), round(y0 + dy))`, a 32x32 joint histogram, (H(X) + H(Y)) / H(X, Y) in
[1, 2]; NaN where a chip leaves its image or the joint entropy vanishes.  The reference spends ~0.7 ms per key point in a
pandas `apply`; here one kernel launch builds every key point's histogram in LDS (k_mi.hip), shared with
`ZNCCService.compute_mi`.
"""
from __future__ import annotations

import logging

import numpy as np
from pandas import DataFrame, Series

from .. import ops
from ..resident import MI_SEARCH_COLUMNS, keep_shared_across, mi_search_columns, shared_pair
from .zncc_service import CHIP_SIZE, _chip_centres, _common_pixel_type, _kernel_ready, _mi_scores, surface_peaks

logger = logging.getLogger(__name__)


class MutualInfoService:
    """Scores the key points of a frame against the raw (full-resolution) images."""

    def __init__(self, ctx=None):
        self._chip_size = CHIP_SIZE
        self._chip_margin = (CHIP_SIZE - 1) // 2
        self._ctx = ctx

    def compute_mutual_info(self, df: DataFrame, monitored, reference) -> Series:
        """Score per row of `df` (columns x0, y0, dx, dy) on the frame's index; NaN where the reference skips the row."""
        try:
            values = np.empty(0, np.float64)
            if len(df):
                ref, mon = np.asarray(reference.array), np.asarray(monitored.array)
                if not _kernel_ready(df, ref, mon):
                    ref, mon = _common_pixel_type(ref, mon)
                values = _mi_scores(df, ref, mon, self._ctx, rasters=(monitored, reference))[0]
        finally:
            from ..resident import keep_shared_across
            with keep_shared_across(monitored, reference):      # (the service's own closing call: nothing was edited since the upload)
                monitored.clear_cache()
                reference.clear_cache()
        logger.info("mutual information: %d key points scored", len(df))
        return Series(values, index=df.index, dtype=np.float64)

    def search(self, df: DataFrame, monitored, reference, radius: int = 4) -> DataFrame:
        """The mutual-information search around every row of `df`: Studholme's NMI of the 57 x 57 chips at the offsets -radius .. radius
        around the centre `compute_mutual_info` scores, the peak of that surface and its sub-pixel position (`ops.mi_search`; the
        reference has no such call).  -> a frame on `df.index`: mi_dx, mi_dy (the displacement the peak stands for, comparable with dx,
        dy), mi_peak (Studholme's NMI there), mi_peak_mi (the `mi_score` formula at the same offset), mi_off_x, mi_off_y (the peak's
        whole-pixel offset from the rounded KLT position), mi_status (bit 1: row skipped, 2: no offset has a value, 4 / 8: the peak lies
        on the rim of the square, or beside an offset without a value, in x / y).
        The kernel serves one device pixel type and a float32 frame, exact from the counts.  Anything else (a float64 frame, mixed or
        other pixel types with a common type the device reads) falls back to `ops.mi_batch` over the (2 radius + 1)^2 fabricated rows
        of every key point, with the peak from the numpy form `zncc_service.surface_peaks`: that fallback is held to 1e-9 of the
        kernel's values, not to the bit."""
        ops.score._check_search("MutualInfoService.search", len(df), radius)
        radius = int(radius)
        try:
            if len(df):
                ref, mon = np.asarray(reference.array), np.asarray(monitored.array)
                columns = self._search_columns(df, ref, mon, radius, (monitored, reference))
            else:
                empty = ops.MiSearch(np.empty((0, 2), np.int32), np.empty(0), np.empty(0), np.empty((0, 2)), np.empty(0, np.uint8), None)
                columns = mi_search_columns(empty)
        finally:
            with keep_shared_across(monitored, reference):
                monitored.clear_cache()
                reference.clear_cache()
        logger.info("mutual-information search: %d key points, radius %d", len(df), radius)
        return DataFrame(dict(zip(MI_SEARCH_COLUMNS, columns)), index=df.index)

    def _search_columns(self, df, ref, mon, radius, rasters):
        if _kernel_ready(df, ref, mon):
            cols = [df[c].to_numpy(dtype=np.float32, copy=False) for c in ("x0", "y0", "dx", "dy")]
            if ref.shape == mon.shape:
                return mi_search_columns(shared_pair(mon, ref, self._ctx, rasters=rasters).mi_search(*cols, radius=radius))
            return mi_search_columns(ops.mi_search(ref, mon, *cols, radius=radius, ctx=self._ctx))
        # float64 frames / cross-sensor pixel types: centres on the host, one fabricated row per offset whose float32 sum x0' + dx' is the
        # offset's centre exactly (x0' = X0, dx' = X1 + ox - X0: integers far below 2^24), both scores of all of them in one call
        ref, mon = _common_pixel_type(ref, mon)
        u0, v0, u1, v1, inside = _chip_centres(df, self._chip_margin, ref.shape, mon.shape)
        S = 2 * radius + 1
        surface = np.full((len(df), S, S), np.nan)
        other = np.full((len(df), S, S), np.nan)
        if inside.any():
            o = np.arange(-radius, radius + 1)
            m = int(inside.sum())
            x0 = np.broadcast_to(v0[inside, None, None], (m, S, S)).astype(np.float32).ravel()
            y0 = np.broadcast_to(u0[inside, None, None], (m, S, S)).astype(np.float32).ravel()
            dx = np.broadcast_to((v1 - v0)[inside, None, None] + o[None, None, :], (m, S, S)).astype(np.float32).ravel()
            dy = np.broadcast_to((u1 - u0)[inside, None, None] + o[None, :, None], (m, S, S)).astype(np.float32).ravel()
            st, nmi = ops.mi_batch(ref, mon, x0, y0, dx, dy, ctx=self._ctx)
            surface[inside], other[inside] = st.reshape(m, S, S), nmi.reshape(m, S, S)
        found = surface_peaks(surface, radius, (v0, u0, v1, u1), inside)
        iy, ix = found.offset[:, 1] + radius, found.offset[:, 0] + radius
        peak_mi = np.where((found.status & 3) == 0, other[np.arange(len(df)), iy, ix], np.nan)
        return mi_search_columns(ops.MiSearch(found.offset, found.peak, peak_mi, found.shift, found.status, None))
