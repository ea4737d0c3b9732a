"""Frame blocks and the tickets of submitted tiles: `RawFrame`, `PendingFrame`, `PendingBatch`; `PriorSteps`, the host half of a frame
tracked under a geometric prior."""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np
from pandas import DataFrame

from .. import frames
from .._lib import Context, KariosHipError


class RawFrame:
    """One tile's frame block as the device pipeline delivers it (layout of km_klt_tile_frame[_zncc]_dev): 4 int32
    {n_rows, n_init, flags, candidates} + 6*cap float32 (x0 | y0 | dx | dy | score | index bits) + `with_zncc` x cap float64
    (the number of score columns, `calls.score_columns`; a bool counts as 0 / 1)."""
    __slots__ = ("block", "cap", "with_zncc")

    def __init__(self, block: np.ndarray, cap: int, with_zncc: int):
        self.block, self.cap, self.with_zncc = block, cap, with_zncc

    @property
    def n_rows(self) -> int:
        return int(self.block[:1].view(np.int32)[0])

    @property
    def flags(self) -> int:
        """Non-zero: the tile did not fit the fixed capacities of the synchronisation-free corner path (KM_FLAG_* of
        csrc/common.hpp) and its rows are NOT the result - repeat it through the exact path (`PendingFrame.redo`)."""
        return int(self.block[2:3].view(np.int32)[0])

    @property
    def n_candidates(self) -> int:
        return int(self.block[3:4].view(np.int32)[0])

    def to_frame(self, radial: bool = False) -> DataFrame | None:
        """The tile's DataFrame; `radial`: with the `radial error` / `angle` columns of `score_frame` already in place."""
        return frames.block_to_frame(self.block, self.cap, self.with_zncc, radial, own=True)   # (the block is this frame's private copy)


class PriorSteps:
    """What the host adds to a frame that was tracked under a prior (`ResidentPair.match_tile(prior=)`, `submit_units(priors=)`): the
    `dx_prior, dy_prior` columns of the prior at the unit's origin and - `clip`: with `conf.outliers_filtering` - the outlier clip on the
    residuals.  `apply` makes a library call when it clips: submitting thread only."""
    __slots__ = ("P", "x_off", "y_off", "clip")

    def __init__(self, P, x_off, y_off, clip: bool):
        self.P, self.x_off, self.y_off, self.clip = P, x_off, y_off, bool(clip)

    def apply(self, frame: DataFrame, ctx=None) -> DataFrame:
        from ..matcher import prior as _prior
        frame["dx_prior"], frame["dy_prior"] = _prior.prior_columns(frame, self.P, self.x_off, self.y_off)
        return _prior.clip_residuals(frame, ctx=ctx) if self.clip else frame


class _Ticket:
    """A submission the device is still working on: its frame slot (`ticket`) and the shape of the blocks it delivers."""

    def __init__(self, ctx: Context, ticket: int, cap: int, with_zncc: int):
        self.ctx, self.ticket, self.cap, self.with_zncc = ctx, ticket, cap, with_zncc

    def _collect(self, n: int) -> "list[RawFrame]":
        """km_frame_wait (any thread), then the slot's `n` blocks as one private copy."""
        c = self.ctx
        blk, nbytes = C.c_void_p(), C.c_size_t()
        rc = c.lib.km_frame_wait(c.handle, self.ticket, C.byref(blk), C.byref(nbytes))
        if rc != 0:
            raise KariosHipError(f"km_frame_wait(ticket {self.ticket}) failed with status {rc}")
        n32 = frames.block_words(self.cap, self.with_zncc)
        pinned = np.ctypeslib.as_array(C.cast(blk, C.POINTER(C.c_float)), shape=(n * n32,))
        own = pinned.copy()                                   # the pinned slot is reused 3 submissions later
        return [RawFrame(own[k * n32:(k + 1) * n32], self.cap, self.with_zncc) for k in range(n)]

    def stage_ms(self) -> dict:
        """Stage spans of this submission (after `wait`, with `Context.set_profiling(True)`)."""
        c = self.ctx
        buf, n = (C.c_float * 16)(), C.c_int()
        rc = c.lib.km_frame_stage_ms(c.handle, self.ticket, buf, 16, C.byref(n))
        if rc != 0:
            raise KariosHipError(f"km_frame_stage_ms failed with status {rc}")
        return {c.lib.km_stage_name(i).decode(): float(buf[i]) for i in range(n.value)}


class PendingFrame(_Ticket):
    """A tile submitted with `ResidentPair.submit_tile`: the device is still working on its tail (LK, FB test, ZNCC, copy)
    while the caller already submits the next tile.  `wait()` (any thread) -> `RawFrame`."""

    def __init__(self, ctx: Context, ticket: int, cap: int, with_zncc: int, redo=None):
        super().__init__(ctx, ticket, cap, with_zncc)
        self._raw = None
        self._redo = redo

    def redo(self) -> "RawFrame":
        """The same tile through the exact (synchronising) corner path, for a frame whose `flags` are set.  Runs device work on
        the context: call it on the thread that submits, not on a worker that only waits."""
        if self._redo is None:
            raise KariosHipError("this frame cannot be repeated")
        self._raw = self._redo()
        return self._raw

    def result(self) -> "RawFrame":
        """`wait()`, and `redo()` when the speculative path flagged the tile (submitting thread only)."""
        raw = self.wait()
        return self.redo() if raw.flags else raw

    def wait(self) -> "RawFrame":
        if self._raw is None:
            self._raw = self._collect(1)[0]
        return self._raw


class PendingBatch(_Ticket):
    """Units submitted together with `submit_units` (km_klt_units_frame_submit): ONE device pipeline for all of them.
    `wait()` (any thread) -> the units' `RawFrame`s in submission order; `redo(i)` repeats unit i alone through the exact path - under
    its prior when the batch was submitted with priors (km_klt_units_frame_prior_submit); `frame(i)` is then unit i's DataFrame with
    `dx_prior, dy_prior`, clipped on the residuals."""

    def __init__(self, ctx: Context, ticket: int, cap: int, with_zncc: int, redos, prior_steps=None):
        super().__init__(ctx, ticket, cap, with_zncc)
        self._redos = redos
        self.prior_steps = prior_steps          # a submission under priors: unit i's `PriorSteps`; None otherwise
        self._raws = None
        self._submitter = threading.get_ident()

    def __len__(self):
        return len(self._redos)

    def wait(self) -> "list[RawFrame]":
        if self._raws is None:
            if threading.get_ident() == self._submitter:
                self.ctx.flush(self.ticket)     # ("units_pipeline": the submitting thread waits and no further submission came - the deferred tail goes now;
                                                #  a worker thread just waits: the submitting thread submits the next batch or flushes - FrameStream does)
            self._raws = self._collect(len(self._redos))
        return self._raws

    def redo(self, i: int) -> "RawFrame":
        """Unit i through the exact (synchronising) corner path (submitting thread only)."""
        self._raws[i] = self._redos[i]()
        return self._raws[i]

    def frame(self, i: int) -> DataFrame | None:
        """Unit i's DataFrame (submitting thread): `wait`, the repeat of a flagged unit, and the host half of its prior, if any."""
        raw = self.wait()[i]
        if raw.flags:
            raw = self.redo(i)
        frame = raw.to_frame()
        if frame is not None and self.prior_steps is not None:
            frame = self.prior_steps[i].apply(frame, self.ctx)
        return frame
