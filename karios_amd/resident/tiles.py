"""The tile entry points on a resident pair: `TileCalls` (the methods of `ResidentPair` that run KLT on a box) and `submit_units`.

Every tile call is `_tile_args`' head, the parameters and the call's own tail, made inside one `calls.Scope`."""
from __future__ import annotations

import ctypes as C
import os
from functools import partial

import numpy as np
from pandas import DataFrame

from .. import _lib, frames, tiling
from .._lib import KariosHipError
from ..ops import make_params
from .buffers import DeviceBuffer
from .calls import Scope, clips, frame_capacity, no_data_pointers, score_columns
from .pending import PendingBatch, PendingFrame, PriorSteps, RawFrame


def _origin(origin, box):
    return origin if origin is not None else ((box[0], box[1]) if box is not None else (0, 0))


class TileCalls:
    """KLT on a box of the pair (mixed into `ResidentPair`, which brings `_box`, the pointers and the sizes)."""

    def _outputs(self, cap: int):
        need = 3 * cap * 2 * 4 + 16
        if self._out is None or self._out.nbytes < need:
            self._out = DeviceBuffer(self.ctx, need)
        base = self._out.ptr
        return base, base + cap * 8, base + 2 * cap * 8, base + 3 * cap * 8

    def _tile_args(self, box):
        """ctypes arguments of a tile call on a validated box (`_box`) -> (head, whole, x_size, y_size of the box): the head every tile
        entry point starts with (context, ref, mon, pixel type, H, W, strides, mask, mask stride, no-data pointers), and the
        whole-raster group the scores read (ref, mon, H, W, strides)."""
        _, _, bx, by, off = self._box(box)
        es, s = self.dtype.itemsize, self.x_size
        head = (self.ctx.handle, C.c_void_p(self.ref_ptr + off * es), C.c_void_p(self.mon_ptr + off * es), self.code, by, bx, s, s,
                C.c_void_p(self.mask_ptr + off) if self.mask_ptr else None, s) + no_data_pointers(self)
        return head, (C.c_void_p(self.ref_ptr), C.c_void_p(self.mon_ptr), self.y_size, s, s, s), bx, by

    def _frame_clip(self, on: bool) -> Scope:
        """Context manager: frames produced inside are clipped on the device (`Scope`)."""
        return Scope(self.ctx, clip=on)

    @staticmethod
    def _params(conf, ksizes=None, invert_mon=None):
        mon_k, ref_k = ksizes if ksizes is not None else tiling.kernel_sizes(conf.laplacian_kernel_size)
        invert = bool(conf.laplacian_invert_polarity) if invert_mon is None else bool(invert_mon)
        return make_params(conf, mon_k, ref_k, invert)

    def _frame_capacity(self, conf, box) -> int:
        """`frame_capacity` of a box of this pair (None: the whole pair) under `conf`."""
        bx, by = (box[2], box[3]) if box is not None else (self.x_size, self.y_size)
        return frame_capacity(conf.maxCorners, bx, by)

    def track_tile(self, conf, box=None, mon_ksize=None, ref_ksize=None, invert_mon=False, out_ptrs=None):
        """km_klt_tile_dev on one box (x_off, y_off, x_size, y_size) of the resident pair.
        -> (status, (p0, p1, p0r) | None) like `ops.klt_tile`; with `out_ptrs` (p0, p1, p0r, n device
        pointers, capacity) the results stay on the device and only (status, n) is returned."""
        c = self.ctx
        head, _, bx, by = self._tile_args(box)
        prm = self._params(conf, None if mon_ksize is None or ref_ksize is None else (mon_ksize, ref_ksize), invert_mon)
        cap = frame_capacity(prm.max_corners, bx, by)
        if out_ptrs is not None:
            d0, d1, d2, dn, ocap = out_ptrs
            if ocap < cap:
                raise KariosHipError("track_tile: output capacity below maxCorners")
        else:
            d0, d1, d2, dn = self._outputs(cap)
        c.check(c.lib.km_klt_tile_dev(*head, C.byref(prm), C.c_void_p(d0), C.c_void_p(d1), C.c_void_p(d2), cap, C.c_void_p(dn)), "km_klt_tile_dev")
        st = c.stats()  # valid_pixels is known on the host as soon as the call returns
        if st.valid_pixels == 0:
            return "no_valid_pixels", None
        nbuf = np.empty(1, np.int32)
        c.check(c.lib.km_d2h(c.handle, nbuf.ctypes.data_as(C.c_void_p), C.c_void_p(dn), 4), "km_d2h")
        n = int(nbuf[0])
        if n == 0:
            return "no_features", None
        if out_ptrs is not None:
            return "ok", n
        pts = np.empty((3, n, 2), np.float32)
        for i, d in enumerate((d0, d1, d2)):
            c.check(c.lib.km_d2h(c.handle, pts[i].ctypes.data_as(C.c_void_p), C.c_void_p(d), n * 8), "km_d2h")
        return "ok", tuple(p.reshape(-1, 1, 2) for p in pts)

    def match_tile(self, conf, box=None, zncc_threshold=None, ksizes=None, invert_mon=None, origin=None, mutual_info: bool = False,
                   prior=None) -> DataFrame | None:
        """One tile of `KLT.match` (reference klt.py:236-349) on resident data with fixed Laplacian kernel sizes and
        polarity: `ksizes` (mon, ref) / `invert_mon` default to the configuration's (its 'auto' values are the caller's
        business: `karios_amd.matcher.KLT`).  `origin` (x, y) is added to the key points (default: the box offset).
        With `zncc_threshold` the frame also carries the `zncc_score` column of `_handle_klt_results` (core.py:876-893)
        computed in the same device call.
        `prior` (9 float64 values that map reference to monitored pixel coordinates, `karios_amd.matcher.prior`; the coordinates are
        those of the key points, `origin` included): every key point is tracked from its guess on the rasters as they are
        (km_klt_tile_frame_prior_dev), the frame carries `dx_prior, dy_prior` behind its columns, and the outlier clip of
        `conf.outliers_filtering` runs on the residuals dx - dx_prior, dy - dy_prior.  None, the default, changes nothing."""
        if ksizes is None and conf.laplacian_kernel_size == "auto" or invert_mon is None and conf.laplacian_invert_polarity == "auto":
            raise KariosHipError("ResidentPair.match_tile: 'auto' modes are resolved by karios_amd.matcher.KLT")
        x_off, y_off = _origin(origin, box)
        if prior is not None:
            return self._match_tile_prior(conf, box, x_off, y_off, prior, zncc_threshold, ksizes, invert_mon, mutual_info)
        if clips(conf) and self._frame_capacity(conf, box) > _lib.CLIP_MAX_ROWS:
            # more rows than the device clip holds (maxCorners 0 on a large tile): FB test, clip and ordering on the host
            return self._match_tile_host_clip(conf, box, x_off, y_off, zncc_threshold, ksizes, invert_mon)
        return self._match_tile_device_frame(conf, box, x_off, y_off, zncc_threshold, ksizes=ksizes, invert_mon=invert_mon, mutual_info=mutual_info)

    def _match_tile_host_clip(self, conf, box, x_off, y_off, zncc_threshold=None, ksizes=None, invert_mon=None) -> DataFrame | None:
        """`match_tile` with the outlier filter on the host: the tracks come back as three point lists, FB test, `frames.sigma_clip`
        (numpy) and the ordering run here, a second device call scores the survivors.  The path of a frame of more than 32768 rows,
        and the tests' second opinion on the device clip."""
        mon_k, ref_k = ksizes if ksizes is not None else tiling.kernel_sizes(conf.laplacian_kernel_size)
        invert = bool(conf.laplacian_invert_polarity) if invert_mon is None else bool(invert_mon)
        status, tracks = self.track_tile(conf, box, mon_k, ref_k, invert)
        if status != "ok":
            return None
        cols, n_init = frames.track_columns(*tracks)
        points = frames.assemble(cols, x_off, y_off, clip_outliers=True)
        points.attrs["Ninit"] = n_init
        if zncc_threshold is not None:
            keep = points["score"].to_numpy() >= zncc_threshold
            z = np.full(len(points), np.nan)
            if keep.any():
                z[keep] = self.zncc(*(points[c].to_numpy()[keep] for c in ("x0", "y0", "dx", "dy")))
            points["zncc_score"] = z
        return points

    def _match_tile_device_frame(self, conf, box, x_off, y_off, zncc_threshold=None, build_frame=True, ksizes=None,
                                 invert_mon=None, mutual_info: bool = False) -> DataFrame | None:
        """Tile pipeline + FB test + score + (x0, y0) ordering (+ the outlier clip of `conf.outliers_filtering`) (+ ZNCC [+ MI / NMI] of
        the confident rows) on the device, one D2H copy of the finished frame."""
        c = self.ctx
        n_scores = score_columns(zncc_threshold, mutual_info)
        head, whole, bx, by = self._tile_args(box)
        prm = self._params(conf, ksizes, invert_mon)
        cap = frame_capacity(prm.max_corners, bx, by)
        if self._host_frame is None or self._host_frame.size < frames.block_words(cap, 3):
            self._host_frame = np.empty(frames.block_words(cap, 3), np.float32)
        buf = self._host_frame
        if zncc_threshold is None:
            with Scope(c, clip=clips(conf)):
                c.check(c.lib.km_klt_tile_frame_dev(*head, C.byref(prm), float(x_off), float(y_off), buf.ctypes.data_as(C.c_void_p), cap),
                        "km_klt_tile_frame_dev")
        else:
            with Scope(c, self.window, n_scores == 3, clips(conf)):
                c.check(c.lib.km_klt_tile_frame_zncc_dev(*head, C.byref(prm), float(x_off), float(y_off), *whole, float(zncc_threshold),
                                                         buf.ctypes.data_as(C.c_void_p), cap), "km_klt_tile_frame_zncc_dev")
        if not build_frame:
            return None
        frame = frames.block_to_frame(buf, cap, n_scores)
        if frame is not None:
            frame.attrs["Ninit"] = int(buf[:2].view(np.int32)[1])
        return frame

    def _match_tile_prior(self, conf, box, x_off, y_off, prior, zncc_threshold=None, ksizes=None, invert_mon=None, mutual_info: bool = False):
        """`match_tile` under a geometric prior: one device call (mask under the prior, seeded tracker, frame, scores), then on the
        host the two prior columns and - with `conf.outliers_filtering` - the clip of the residuals through `ops.sigma_clip`, in corner
        order as the tracker's own clip runs (the device call keeps "frame_clip" off: that stage clips dx, dy themselves)."""
        from ..matcher import prior as _prior
        P = _prior.as_prior(prior)
        raw = self._prior_tile_raw(conf, box, x_off, y_off, P, zncc_threshold, ksizes, invert_mon, mutual_info)
        frame = frames.block_to_frame(raw.block, raw.cap, raw.with_zncc)
        if frame is None:
            return None
        frame = PriorSteps(P, x_off, y_off, clips(conf)).apply(frame, self.ctx)
        frame.attrs["Ninit"] = int(raw.block[:2].view(np.int32)[1])
        return frame

    def _prior_tile_raw(self, conf, box, x_off, y_off, P, zncc_threshold=None, ksizes=None, invert_mon=None, mutual_info: bool = False) -> "RawFrame":
        """GPU half of `match_tile(prior=)`: km_klt_tile_frame_prior_dev on a box, the raw block as a private copy.  The call repeats a
        flagged tile itself, so this is also the repeat of a flagged unit of a batch under priors (`submit_units`); the frame sink is
        lifted around it as for `_exact_repeat`."""
        c = self.ctx
        if self.window is not None:
            raise KariosHipError("ResidentPair.match_tile: a prior on a windowed pair is not supported")
        n_scores = score_columns(zncc_threshold, mutual_info)
        head, whole, bx, by = self._tile_args(box)
        prm = self._params(conf, ksizes, invert_mon)
        cap = frame_capacity(prm.max_corners, bx, by)
        buf = np.empty(frames.block_words(cap, 3), np.float32)
        # (without a threshold no row is scored: a score never exceeds 1)
        thr = 2.0 if zncc_threshold is None else float(zncc_threshold)
        sink = c.frame_sink
        if sink[0]:
            c.set_frame_sink(None)
        try:
            with Scope(c, mi=n_scores == 3):
                c.check(c.lib.km_klt_tile_frame_prior_dev(*head, C.byref(prm), float(x_off), float(y_off), *whole, thr,
                                                          P.ctypes.data_as(C.POINTER(C.c_double)), buf.ctypes.data_as(C.c_void_p), cap),
                        "km_klt_tile_frame_prior_dev")
        finally:
            if sink[0]:
                c.set_frame_sink(*sink)
        return RawFrame(buf[:frames.block_words(cap, n_scores)], cap, n_scores)

    def match_tile_prior_raw(self, conf, box=None, zncc_threshold=None, origin=None, mutual_info: bool = False, prior=None) -> "RawFrame":
        """`match_tile_raw` under a prior (blocking): the raw block; `PriorSteps` are its host half."""
        from ..matcher import prior as _prior
        if conf.laplacian_kernel_size == "auto" or conf.laplacian_invert_polarity == "auto":
            raise KariosHipError("ResidentPair.match_tile_prior_raw: 'auto' modes need ResidentPair.match_tile / matcher.KLT")
        x_off, y_off = _origin(origin, box)
        return self._prior_tile_raw(conf, box, x_off, y_off, _prior.as_prior(prior), zncc_threshold, mutual_info=mutual_info)

    def match_tile_auto_ksize(self, conf, box=None, invert_mon: bool = False, candidates=tiling.AUTO_KSIZE_CANDIDATES, origin=None):
        """The Laplacian kernel-size search of the reference (klt.py:465-545) for one tile of the resident pair in ONE
        device call: every Laplacian, pyramid and corner list is built once on the device and shared by the
        len(candidates)^2 tracker runs; the winner is the (mon, ref) pair with the highest inlier ratio, first in
        (mon outer, ref inner) order on ties.
        -> (frame | None, {(mon_k, ref_k): inlier ratio}, (mon_k, ref_k) | None, Ninit).  No outlier filtering."""
        if clips(conf):
            raise KariosHipError("match_tile_auto_ksize: the sigma clip changes the inlier counts - use karios_amd.matcher.KLT")
        c = self.ctx
        head, _, bx, by = self._tile_args(box)
        prm = make_params(conf, 1, 1, bool(invert_mon))
        cap = frame_capacity(prm.max_corners, bx, by)
        buf = np.empty(frames.block_words(cap), np.float32)
        ks = np.ascontiguousarray(candidates, np.int32)
        nk = len(ks)
        ratios = np.zeros(nk * nk, np.float64)
        best = np.zeros(2, np.int32)
        x_off, y_off = _origin(origin, box)
        c.check(c.lib.km_klt_auto_ksize_frame_dev(*head, C.byref(prm), ks.ctypes.data_as(C.c_void_p), nk, float(x_off), float(y_off),
                                                  buf.ctypes.data_as(C.c_void_p), cap, ratios.ctypes.data_as(C.c_void_p),
                                                  best.ctypes.data_as(C.c_void_p)), "km_klt_auto_ksize_frame_dev")
        scores = {(int(ks[i]), int(ks[j])): float(ratios[i * nk + j]) for i in range(nk) for j in range(nk)}
        if best[0] < 0:
            return None, scores, None, 0
        n_init = int(buf[:2].view(np.int32)[1])
        return frames.block_to_frame(buf, cap), scores, (int(best[0]), int(best[1])), n_init

    def _check_raw(self, what: str, conf, box):
        """The raw forms take fixed kernel size / polarity, and clip on the device: frames of at most 32768 rows."""
        if conf.laplacian_kernel_size == "auto" or conf.laplacian_invert_polarity == "auto":
            raise KariosHipError(f"ResidentPair.{what}: 'auto' modes need ResidentPair.match_tile / matcher.KLT")
        if clips(conf) and self._frame_capacity(conf, box) > _lib.CLIP_MAX_ROWS:
            raise KariosHipError(f"ResidentPair.{what}: outlier filtering of more than 32768 rows needs ResidentPair.match_tile")

    def match_tile_raw(self, conf, box=None, zncc_threshold=None, origin=None, mutual_info: bool = False) -> "RawFrame":
        """GPU half of `match_tile`: runs the device pipeline and returns the raw frame block (a private copy), leaving
        the pandas half to `RawFrame.to_frame()` - which may run in another thread while this thread already drives the
        next tile (ctypes releases the GIL inside the library).  Fixed kernel size / polarity; the outlier filter on the device, for
        frames of at most 32768 rows."""
        self._check_raw("match_tile_raw", conf, box)
        x_off, y_off = _origin(origin, box)
        n_scores = score_columns(zncc_threshold, mutual_info)
        # host blocks rotate through a ring of three: the previous block may still be read by the host half of the pipeline
        ring, slot = self._raw_ring, self._raw_slot
        self._raw_slot = (slot + 1) % len(ring)
        self._host_frame = ring[slot]
        self._match_tile_device_frame(conf, box, x_off, y_off, zncc_threshold, build_frame=False, mutual_info=mutual_info)
        cap = self._frame_capacity(conf, box)
        block, ring[slot], self._host_frame = self._host_frame, self._host_frame, None
        return RawFrame(block[:frames.block_words(cap, n_scores)], cap, n_scores)

    def _exact_repeat(self, conf, box, zncc_threshold, origin, mutual_info) -> "RawFrame":
        """The exact repeat of a unit the synchronisation-free corner path flagged (`PendingFrame.redo`, `PendingBatch.redo`):
        `match_tile_raw` with speculation off, as a private copy."""
        c = self.ctx
        before = c.get_option("speculative", int(os.environ.get("KARIOS_HIP_SPECULATIVE", "1") or 0))
        c.set_option("speculative", 0)
        # the frame sink (km_set_frame_sink) now points at the slot of a NEWER unit: the repeat must not overwrite that block
        # (the all-gather then shipped the redone block of step s - D in the place of step s's own); the caller
        # takes the repeated block from the returned RawFrame
        sink = c.frame_sink
        if sink[0]:
            c.set_frame_sink(None)
        try:
            raw = self.match_tile_raw(conf, box, zncc_threshold, origin=origin, mutual_info=mutual_info)
            return RawFrame(raw.block.copy(), raw.cap, raw.with_zncc)      # (match_tile_raw's blocks rotate through a ring of three)
        finally:
            c.set_option("speculative", before)
            if sink[0]:
                c.set_frame_sink(*sink)

    def submit_tile(self, conf, box=None, zncc_threshold=None, origin=None, mutual_info: bool = False) -> PendingFrame:
        """Asynchronous `match_tile_raw` (km_klt_tile_frame_submit): returns when the tile's last kernel and the copy of
        its frame block are enqueued, so the next `submit_tile` queues its dense stages right behind them - no GPU idle
        time between tiles.  Up to three tiles may be pending; `PendingFrame.wait()` may run in another thread."""
        self._check_raw("submit_tile", conf, box)
        c = self.ctx
        head, whole, bx, by = self._tile_args(box)
        prm = self._params(conf)
        cap = frame_capacity(prm.max_corners, bx, by)
        n_scores = score_columns(zncc_threshold, mutual_info)
        if not n_scores:
            whole = (None, None) + whole[2:]
        ticket = C.c_int(-1)
        x_off, y_off = _origin(origin, box)
        with Scope(c, self.window, n_scores == 3, clips(conf)):
            c.check(c.lib.km_klt_tile_frame_submit(*head, C.byref(prm), float(x_off), float(y_off), *whole, float(zncc_threshold or 0.0), cap,
                                                   C.byref(ticket)), "km_klt_tile_frame_submit")
        return PendingFrame(c, ticket.value, cap, n_scores, redo=partial(self._exact_repeat, conf, box, zncc_threshold, (x_off, y_off), mutual_info))

    def match_pipelined(self, conf, boxes=None, zncc_threshold=None, host_stage=None, with_empty: bool = False, split_small_grids: bool = True,
                        prior=None):
        """`match` as a pipeline (`karios_amd.stream.FrameStream`): tile i+1 is submitted to the device (`submit_tile`) while a
        worker thread waits for tile i and builds its DataFrame.  `host_stage(frame)` (e.g. `score_frame`) runs on the CALLING
        thread when the frame is collected: a context is not thread-safe, and a stage that calls back into the library (ZNCC /
        MI of rows the device call did not score) must not run beside `submit_tile`.  Yields the frames in tile order, like
        `KLT.match`.  `prior` (`karios_amd.matcher.prior`): every tile under it, as `match_tile(prior=)` tile by tile - the batches go
        through km_klt_units_frame_prior_submit, the frames carry `dx_prior, dy_prior` and are clipped on the residuals."""
        from ..stream import FrameStream
        if boxes is None:
            boxes = tiling.tile_grid(self.x_size, self.y_size, conf.tile_size, conf.xStart)
        stage = None if host_stage is None else (lambda frame, _pair: host_stage(frame))
        with FrameStream(zncc_threshold, depth=1, host_stage=stage, score_columns=False) as stream:
            # the tiles travel as batched submissions (one set of device launches per <= 16 tiles) where the batch form covers them.  A grid
            # of 8 .. 16 tiles goes as TWO submissions: the device pipelines them (csrc/api_units.hip) and the first half's DataFrames are
            # built while the second half is on the device - as one submission every frame waited for the last tile (tools/investigations/e2e_shape_probe.py:
            # 16 tiles of 3000^2 15.0 -> 14.45 ms per pair; four tiles gain nothing: 2.45 against 2.52)
            units = [(self, box, None) for box in boxes]
            halves = [units[:len(units) // 2], units[len(units) // 2:]] if split_small_grids and 8 <= len(units) <= 16 else [units]
            for part in halves:
                for done in stream.submit_many(part, conf, priors=prior):
                    if done.frame is not None or with_empty:          # (with_empty: None for a tile without valid pixels / corners)
                        yield done.frame
            for done in stream.drain():
                if done.frame is not None or with_empty:
                    yield done.frame

    def match(self, conf):
        """All tiles in the reference order (x outer, y inner; klt.py:220-232)."""
        for box in tiling.tile_grid(self.x_size, self.y_size, conf.tile_size, conf.xStart):
            frame = self.match_tile(conf, box)
            if frame is not None:
                yield frame


def _unit_priors(priors, n: int):
    """None, one prior for all units (nine values: shape (9,) or (3, 3)), or one per unit (a sequence of n such) -> None | n arrays of
    9 float64 (`matcher.prior.as_prior`).  The shape decides, not the number of values: `[P]` is one prior per unit of a one-unit list."""
    from ..matcher import prior as _prior
    if priors is None:
        return None
    try:
        shape = np.shape(priors)
    except ValueError:                      # (a ragged sequence: 3 x 3 matrices beside flat ones)
        shape = None
    if shape in ((9,), (3, 3)):
        return [_prior.as_prior(priors)] * n
    if len(priors) != n:
        raise ValueError(f"priors: {len(priors)} for {n} units")
    return [_prior.as_prior(p) for p in priors]


def submit_units(units, conf, zncc_threshold=None, mutual_info: bool = False, priors=None) -> "PendingBatch | None":
    """`ResidentPair.submit_tile` for up to 16 independent units at once - `units` = [(pair, box | None, origin | None), ...], all on
    ONE context, one pixel type, all with a user mask or none: the tiles of `KLT.match` (klt.py:220-253), of one pair or of several bands.  Every
    dense kernel, the corner-selection chain, LK, the frame stage and the scores are launched ONCE for all units
    (csrc/api_units.hip); the frames are the unit-by-unit frames bit for bit.  Returns None when the batch form does not cover the
    case (the library answers KM_E_UNSUPPORTED: maxCorners 0, a unit narrower than 512 columns ...) or the
    units do not share a context / pixel type, or only some carry a user mask - submit them one by one then.  With
    `conf.outliers_filtering` every unit's frame is clipped on the device (km_set_option "frame_clip") in front of its scores.
    `priors` (None, one prior for all units, or one per unit; `karios_amd.matcher.prior`): km_klt_units_frame_prior_submit - every unit is
    tracked from its guesses as `match_tile(prior=)` tracks it alone, bit for bit; the device clip stays off (the clip under a prior runs
    on the residuals: `PendingBatch.prior_steps`), a flagged unit is repeated under its prior, and a windowed pair is not covered."""
    if not units or len(units) > _lib.UNITS_PER_SUBMISSION:
        return None
    if conf.laplacian_kernel_size == "auto" or conf.laplacian_invert_polarity == "auto" or conf.maxCorners <= 0:
        return None
    first = units[0][0]
    c = first.ctx
    if any(p.ctx is not c or p.code != first.code or bool(p.mask_ptr) != bool(first.mask_ptr) or p.no_data_mon != first.no_data_mon
           or p.no_data_ref != first.no_data_ref for p, _, _ in units):
        return None
    n_scores = score_columns(zncc_threshold, mutual_info)
    prm = TileCalls._params(conf)
    cap = prm.max_corners
    arr = (_lib.KmUnit * len(units))()
    redos, steps = [], []
    P = _unit_priors(priors, len(units))
    for k, (pair, box, origin) in enumerate(units):
        bx_off, by_off, bx, by, off = pair._box(box)
        x_off, y_off = origin if origin is not None else (bx_off, by_off)
        es = pair.dtype.itemsize
        u = arr[k]
        u.d_ref, u.d_mon, u.sref, u.smon, u.H, u.W = pair.ref_ptr + off * es, pair.mon_ptr + off * es, pair.x_size, pair.x_size, by, bx
        u.x_off, u.y_off = float(x_off), float(y_off)
        if n_scores:
            u.d_ref_full, u.d_mon_full, u.sref_f, u.smon_f, u.Hf, u.Wf = pair.ref_ptr, pair.mon_ptr, pair.x_size, pair.x_size, pair.y_size, pair.x_size
        if pair.window is not None:
            u.win_ox, u.win_oy, u.win_H, u.win_W = (int(v) for v in pair.window)
        if pair.mask_ptr:                     # the user mask of the box (klt.py:258-266): a uint8 raster of the pair's shape
            u.d_mask, u.smask = pair.mask_ptr + off, pair.x_size
        if P is None:
            redos.append(partial(pair._exact_repeat, conf, box, zncc_threshold, (x_off, y_off), mutual_info))
        else:
            redos.append(partial(pair._prior_tile_raw, conf, box, x_off, y_off, P[k], zncc_threshold, None, None, mutual_info))
            steps.append(PriorSteps(P[k], x_off, y_off, clips(conf)))
    nr, nm = no_data_pointers(first)
    ticket = C.c_int(-1)
    if P is None:
        with Scope(c, mi=n_scores == 3, clip=clips(conf)):        # (every unit carries its own window)
            rc = c.lib.km_klt_units_frame_submit(c.handle, arr, len(units), first.code, nr, nm, C.byref(prm), float(zncc_threshold or 0.0), cap, C.byref(ticket))
        name = "km_klt_units_frame_submit"
    else:
        table = np.ascontiguousarray(np.stack(P), np.float64)     # n x 9, unit order
        with Scope(c, mi=n_scores == 3, clip=False):
            rc = c.lib.km_klt_units_frame_prior_submit(c.handle, arr, len(units), first.code, nr, nm, C.byref(prm), float(zncc_threshold or 0.0), cap,
                                                       table.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ticket))
        name = "km_klt_units_frame_prior_submit"
    if rc == _lib.E_UNSUPPORTED:
        return None
    c.check(rc, name)
    return PendingBatch(c, ticket.value, cap, n_scores, redos, steps or None)
