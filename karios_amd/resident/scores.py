"""The score entry points on a resident pair: `ScoreCalls` (ZNCC, its search, mutual information, its search, `score_frame`)."""
from __future__ import annotations

import ctypes as C

import numpy as np
from pandas import DataFrame

from .. import frames
from .._lib import KariosHipError, pinned_empty
from ..ops.score import MiSearch, ZnccSearch, _check_search
from .calls import Scope

ZNCC_SEARCH_COLUMNS = ["zncc_dx", "zncc_dy", "zncc_peak", "zncc_off_x", "zncc_off_y", "zncc_status"]
MI_SEARCH_COLUMNS = ["mi_dx", "mi_dy", "mi_peak", "mi_peak_mi", "mi_off_x", "mi_off_y", "mi_status"]


def search_columns(found: ZnccSearch):
    """The six frame columns of a search result (ZNCC_SEARCH_COLUMNS), as arrays."""
    return found.shift[:, 0], found.shift[:, 1], found.peak, found.offset[:, 0], found.offset[:, 1], found.status


def mi_search_columns(found: MiSearch):
    """The seven frame columns of a mutual-information search result (MI_SEARCH_COLUMNS), as arrays."""
    return found.shift[:, 0], found.shift[:, 1], found.peak, found.peak_mi, found.offset[:, 0], found.offset[:, 1], found.status


def _columns(x0, y0, dx, dy):
    return [np.ascontiguousarray(v, np.float32) for v in (x0, y0, dx, dy)]


class ScoreCalls:
    """Scores of key points given in image coordinates (mixed into `ResidentPair`)."""

    def _stage(self, cols, n_outputs: int):
        """Stage the four key-point columns for a call with `n_outputs` float64 slots per row, in page-locked memory the kernels read /
        write DIRECTLY over PCIe (a few hundred KB), so neither direction queues a copy behind an image upload that is in flight on the
        DMA engine -> (the arguments the score entry points start with: context, both rasters with their sizes and strides, the four
        column addresses, n; the float64 view of the n_outputs * n outputs; its address)."""
        n = len(cols[0])
        need = n * (4 * 4 + n_outputs * 8)
        # one grow-only buffer per CONTEXT: releasing page-locked memory synchronises with every copy in flight, so a pair
        # that owned its staging would stall the pipeline whenever it is dropped while the next pair's upload travels
        raw = self.ctx._kp_staging
        if raw is None or raw.nbytes < need:
            raw = self.ctx._kp_staging = pinned_empty(need + need // 2 + 64, np.uint8, self.ctx)
        out = raw[:n_outputs * n * 8].view(np.float64)
        np.concatenate(cols, out=raw[n_outputs * n * 8:n_outputs * n * 8 + 16 * n].view(np.float32))
        o, y, x = out.ctypes.data, self.y_size, self.x_size
        f = o + n_outputs * n * 8
        return (self.ctx.handle, C.c_void_p(self.ref_ptr), C.c_void_p(self.mon_ptr), self.code, y, x, y, x, x, x,
                C.c_void_p(f), C.c_void_p(f + 4 * n), C.c_void_p(f + 8 * n), C.c_void_p(f + 12 * n), n), out, o

    def zncc(self, x0, y0, dx, dy) -> np.ndarray:
        """ZNCCService.compute_zncc values (zncc_service.py:186-238) for key points given in image coordinates."""
        self._ready()
        c = self.ctx
        cols = _columns(x0, y0, dx, dy)
        if len(cols[0]) == 0:
            return np.empty(0, np.float64)
        args, scores, o = self._stage(cols, 1)
        with Scope(c, self.window):
            c.check(c.lib.km_zncc_batch_dev(*args, C.c_void_p(o)), "km_zncc_batch_dev")
        c.sync()
        return scores.copy()

    def zncc_search(self, x0, y0, dx, dy, radius: int = 4, surface: bool = False) -> ZnccSearch:
        """`ops.zncc_search` on the resident rasters: the ZNCC surface over the offsets -radius .. radius around the centre `zncc`
        scores, its peak and the peak's sub-pixel position, for key points given in image coordinates -> ZnccSearch of numpy arrays.
        A windowed pair (row-band mode) raises KariosHipError: the search reads whole rasters."""
        if self.window is not None:
            raise KariosHipError("zncc_search: the pair holds a window of its rasters (row-band mode); a windowed search is not supported")
        cols = _columns(x0, y0, dx, dy)
        n = len(cols[0])
        _check_search("zncc_search", n, radius)
        radius = int(radius)
        SS = (2 * radius + 1) ** 2
        if n == 0:
            return ZnccSearch(np.empty((0, 2), np.int32), np.empty(0, np.float64), np.empty((0, 2), np.float64), np.empty(0, np.uint8),
                              np.empty((0, 2 * radius + 1, 2 * radius + 1), np.float64) if surface else None)
        self._ready()
        c = self.ctx
        # one float64 slot per row for each of: peak | shift x, y | offset (2 x int32) | status (bytes, in the fifth) | the surface
        args, out, o = self._stage(cols, 5 + (SS if surface else 0))
        c.check(c.lib.km_zncc_search_dev(*args, radius, C.c_void_p(o + 24 * n), C.c_void_p(o), C.c_void_p(o + 8 * n), C.c_void_p(o + 32 * n),
                                         C.c_void_p(o + 40 * n) if surface else None), "km_zncc_search_dev")
        c.sync()
        return ZnccSearch(out[3 * n:4 * n].view(np.int32).reshape(n, 2).copy(), out[:n].copy(), out[n:3 * n].reshape(n, 2).copy(),
                          out[4 * n:5 * n].view(np.uint8)[:n].copy(),
                          out[5 * n:].reshape(n, 2 * radius + 1, 2 * radius + 1).copy() if surface else None)

    def mutual_info(self, x0, y0, dx, dy):
        """(mutual_info_score, mi_score) per key point on the resident images: `MutualInfoService.compute_mutual_info`
        (mutual_info_service.py:73-130) and `ZNCCService.compute_mi` (zncc_service.py:240-287)."""
        self._ready()
        c = self.ctx
        cols = _columns(x0, y0, dx, dy)
        n = len(cols[0])
        if n == 0:
            return np.empty(0, np.float64), np.empty(0, np.float64)
        # the two scores come out of ONE kernel run; the reference asks for them in two separate service calls on the same
        # key points (core.py:894-907), so the last result is remembered
        digest = b"".join(v.tobytes() for v in cols)          # the key points themselves (16 B each), compared byte for byte
        memo = self._mi_memo
        if memo is not None and memo[0] == digest:
            return memo[1].copy(), memo[2].copy()
        args, scores, o = self._stage(cols, 2)
        with Scope(c, self.window):
            c.check(c.lib.km_mi_batch_dev(*args, C.c_void_p(o), C.c_void_p(o + 8 * n)), "km_mi_batch_dev")
        c.sync()
        st, nmi = scores[:n].copy(), scores[n:].copy()
        self._mi_memo = (digest, st, nmi)
        return st.copy(), nmi.copy()

    def mi_search(self, x0, y0, dx, dy, radius: int = 4, surface: bool = False) -> MiSearch:
        """`ops.mi_search` on the resident rasters: the surface of Studholme's NMI over the offsets -radius .. radius around the centre
        `mutual_info` scores, its peak, the `mi_score` formula there and the peak's sub-pixel position, for key points given in image
        coordinates -> MiSearch of numpy arrays.  A windowed pair (row-band mode) raises KariosHipError: the search reads whole rasters."""
        if self.window is not None:
            raise KariosHipError("mi_search: the pair holds a window of its rasters (row-band mode); a windowed search is not supported")
        cols = _columns(x0, y0, dx, dy)
        n = len(cols[0])
        _check_search("mi_search", n, radius)
        radius = int(radius)
        S = 2 * radius + 1
        if n == 0:
            return MiSearch(np.empty((0, 2), np.int32), np.empty(0, np.float64), np.empty(0, np.float64), np.empty((0, 2), np.float64),
                            np.empty(0, np.uint8), np.empty((0, S, S), np.float64) if surface else None)
        self._ready()
        c = self.ctx
        # one float64 slot per row for each of: peak | peak_mi | shift x, y | offset (2 x int32) | status (bytes, in the sixth) | the surface
        args, out, o = self._stage(cols, 6 + (S * S if surface else 0))
        c.check(c.lib.km_mi_search_dev(*args, radius, C.c_void_p(o + 32 * n), C.c_void_p(o), C.c_void_p(o + 8 * n), C.c_void_p(o + 16 * n),
                                       C.c_void_p(o + 40 * n), C.c_void_p(o + 48 * n) if surface else None), "km_mi_search_dev")
        c.sync()
        return MiSearch(out[4 * n:5 * n].view(np.int32).reshape(n, 2).copy(), out[:n].copy(), out[n:2 * n].copy(), out[2 * n:4 * n].reshape(n, 2).copy(),
                        out[5 * n:6 * n].view(np.uint8)[:n].copy(), out[6 * n:].reshape(n, S, S).copy() if surface else None)

    def score_frame(self, frame: DataFrame, confidence_threshold: float = 0.4, mutual_info: bool = False,
                    zncc_search_radius: int | None = None, mi_search_radius: int | None = None) -> DataFrame:
        """`_handle_klt_results` numeric columns (core.py:872-907): radial error, angle, the ZNCC of the rows with
        score >= confidence_threshold (NaN elsewhere) and, with `mutual_info`, the `mutual_info_score` / `mi_score`
        columns of the same rows.  With `zncc_search_radius` the same rows also get the columns of `zncc_search`
        (ZNCC_SEARCH_COLUMNS; NaN elsewhere) and with `mi_search_radius` those of `mi_search` (MI_SEARCH_COLUMNS, behind them); None,
        the default of both, adds nothing."""
        frame = frames.radial_angle_columns(frame)
        dx, dy, score = frame["dx"].to_numpy(), frame["dy"].to_numpy(), frame["score"].to_numpy()
        keep = score >= confidence_threshold
        if "zncc_score" not in frame.columns:   # else: already scored on the device (match_tile(..., zncc_threshold=...))
            z = np.full(len(frame), np.nan, np.float64)
            if keep.any():
                z[keep] = self.zncc(frame["x0"].to_numpy()[keep], frame["y0"].to_numpy()[keep], dx[keep], dy[keep])
            frame["zncc_score"] = z
        if mutual_info and "mutual_info_score" not in frame.columns:     # else: scored by the device call that produced the frame
            st = np.full(len(frame), np.nan, np.float64)
            nmi = np.full(len(frame), np.nan, np.float64)
            if keep.any():
                st[keep], nmi[keep] = self.mutual_info(frame["x0"].to_numpy()[keep], frame["y0"].to_numpy()[keep], dx[keep], dy[keep])
            frame["mutual_info_score"] = st
            frame["mi_score"] = nmi
        if zncc_search_radius is not None:
            found = self.zncc_search(frame["x0"].to_numpy()[keep], frame["y0"].to_numpy()[keep], dx[keep], dy[keep], zncc_search_radius)
            for name, values in zip(ZNCC_SEARCH_COLUMNS, search_columns(found)):
                column = np.full(len(frame), np.nan, np.float64)
                column[keep] = values
                frame[name] = column
        if mi_search_radius is not None:
            found = self.mi_search(frame["x0"].to_numpy()[keep], frame["y0"].to_numpy()[keep], dx[keep], dy[keep], mi_search_radius)
            for name, values in zip(MI_SEARCH_COLUMNS, mi_search_columns(found)):
                column = np.full(len(frame), np.nan, np.float64)
                column[keep] = values
                frame[name] = column
        return frame
