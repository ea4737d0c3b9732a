"""`ResidentPair`: construction, uploads, `_ready` / `_box`, and the calls that are neither tiles nor scores."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .._lib import Context, KariosHipError, default_context, dtype_code
from .buffers import DeviceBuffer
from .scores import ScoreCalls
from .tiles import TileCalls


class ResidentPair(TileCalls, ScoreCalls):
    """A monitored / reference image pair (plus optional user mask) resident in HBM."""

    def __init__(self, ctx: Context | None, mon_ptr: int, ref_ptr: int, dtype, y_size: int, x_size: int,
                 mask_ptr: int | None = None, no_data_mon=None, no_data_ref=None, owned=()):
        self._upload_ticket = -1          # (first: `__del__` reads it, also of a pair whose construction failed below)
        self.ctx = ctx if ctx is not None else default_context()
        self.mon_ptr, self.ref_ptr, self.mask_ptr = int(mon_ptr), int(ref_ptr), (int(mask_ptr) if mask_ptr else None)
        self.dtype = np.dtype(dtype)
        self.code = dtype_code(np.empty(0, self.dtype))
        self.y_size, self.x_size = int(y_size), int(x_size)
        self.no_data_mon, self.no_data_ref = no_data_mon, no_data_ref
        self._owned = list(owned)
        # (ox, oy, image y_size, image x_size) when the buffers are only a window of a larger image (km_set_image_window):
        # key points are then image coordinates everywhere (tile `origin`s, zncc / mutual_info arguments)
        self.window = None
        self._out = None                  # device outputs of `track_tile`
        self._host_frame = None           # host block of the frame calls; `match_tile_raw` rotates it through `_raw_ring`
        self._raw_ring, self._raw_slot = [None, None, None], 0
        self._mi_memo = None              # (key points, mutual_info_score, mi_score) of the last `mutual_info`
        self._upload_sources = None       # host arrays of an upload that may still travel

    def __del__(self):
        # a pair that was uploaded (e.g. prefetched) but never used still holds an upload ticket: give its slot and event back
        # (never from the finalizer's thread unless it is the context's own: km_upload_join mutates the context)
        try:
            t, self._upload_ticket = self._upload_ticket, -1
            ctx = self.ctx
            if t >= 0 and getattr(ctx, "handle", None):
                ctx.run_or_defer(lambda: ctx.handle and ctx.lib.km_upload_join(ctx.handle, t))
        except Exception:  # pragma: no cover - interpreter shutdown
            pass

    @classmethod
    def upload(cls, mon: np.ndarray, ref: np.ndarray, mask: np.ndarray | None = None, ctx: Context | None = None,
               no_data_mon=None, no_data_ref=None) -> "ResidentPair":
        ctx = ctx if ctx is not None else default_context()
        mon, ref = np.asarray(mon), np.asarray(ref)
        if mon.shape != ref.shape or mon.dtype != ref.dtype or mon.ndim != 2:
            raise KariosHipError("ResidentPair: mon/ref must be 2-D arrays of equal shape and dtype")
        dtype_code(mon)                                   # unsupported pixel types fail before anything is allocated
        bm, br = DeviceBuffer(ctx, mon.nbytes), DeviceBuffer(ctx, ref.nbytes)
        # the copies travel on the context's copy stream; the pair's first device call waits for them ON THE DEVICE, so a
        # pair uploaded from page-locked memory while the previous one is being matched costs no time
        keep = [br.upload_image_async(ref), bm.upload_image_async(mon)]
        owned, mptr = [bm, br], None
        if mask is not None:
            mk = np.asarray(mask)
            if mk.dtype != np.uint8:
                mk = mk.astype(np.uint8)
            if mk.shape != mon.shape:
                raise KariosHipError("ResidentPair: mask shape differs from the images'")
            bk = DeviceBuffer(ctx, mk.nbytes)
            keep.append(bk.upload_image_async(mk))
            owned.append(bk)
            mptr = bk.ptr
        pair = cls(ctx, bm.ptr, br.ptr, mon.dtype, mon.shape[0], mon.shape[1], mptr, no_data_mon, no_data_ref, owned)
        pair._upload_sources = keep
        ticket = C.c_int(-1)
        ctx.check(ctx.lib.km_upload_mark(ctx.handle, C.byref(ticket)), "km_upload_mark")
        pair._upload_ticket = ticket.value      # joined by the pair's first device call: work queued for OTHER pairs meanwhile does not wait
        return pair

    @classmethod
    def from_windows(cls, mon, ref, mask=None, ctx: Context | None = None, no_data_mon=None, no_data_ref=None) -> "ResidentPair":
        """Pair from boxes that already live in HBM (`karios_amd.core.DeviceWindow`, what `DeviceRasterImage.read` returns):
        dense device copies (device-to-device, nothing crosses PCIe) owned by the pair."""
        import torch
        m, r = mon.view.contiguous(), ref.view.contiguous()
        if m.data_ptr() == mon.view.data_ptr():
            m = m.clone()                                   # the pair owns its pixels like an uploaded one
        if r.data_ptr() == ref.view.data_ptr():
            r = r.clone()
        k = None
        if mask is not None:
            from ..core.image import DeviceWindow
            k = mask.view.contiguous() if isinstance(mask, DeviceWindow) else torch.as_tensor(np.ascontiguousarray(mask, np.uint8), device=m.device)
        torch.cuda.synchronize(m.device)                    # the library runs on its own stream
        return cls(ctx, m.data_ptr(), r.data_ptr(), mon.dtype, m.shape[0], m.shape[1], None if k is None else k.data_ptr(),
                   no_data_mon, no_data_ref, owned=[m, r, k])

    @classmethod
    def from_device_pointers(cls, mon_ptr: int, ref_ptr: int, dtype, y_size: int, x_size: int, ctx: Context | None = None,
                             mask_ptr: int | None = None, no_data_mon=None, no_data_ref=None, keepalive=()) -> "ResidentPair":
        """Wrap existing device memory (row-major, dense rows), e.g. torch tensors' data_ptr().
        The library works on its own HIP stream: the producer of these buffers must have completed
        (e.g. `torch.cuda.synchronize()`) before the first call."""
        return cls(ctx, mon_ptr, ref_ptr, dtype, y_size, x_size, mask_ptr, no_data_mon, no_data_ref, keepalive)

    def _ready(self):
        """Before the first kernel on this pair: its uploads (and only its uploads) must have landed."""
        self.ctx.drain()
        t = self._upload_ticket
        if t >= 0:
            self._upload_ticket = -1
            self.ctx.check(self.ctx.lib.km_upload_join(self.ctx.handle, t), "km_upload_join")
            for buf in self._owned:          # from here on the compute stream is ordered behind the copies: a context sync covers them
                if isinstance(buf, DeviceBuffer):
                    buf.upload_in_flight = False

    def _box(self, box):
        """-> (x_off, y_off, x_size, y_size, element offset of the box origin) of a validated box (None = whole pair)."""
        self._ready()
        x_off, y_off, bx, by = box if box is not None else (0, 0, self.x_size, self.y_size)
        if x_off < 0 or y_off < 0 or x_off + bx > self.x_size or y_off + by > self.y_size or bx <= 0 or by <= 0:
            raise KariosHipError(f"box {box} outside the {self.x_size}x{self.y_size} image")
        return x_off, y_off, bx, by, y_off * self.x_size + x_off

    def chips(self, points, confidence_threshold: float = 0.4, laplacian_ksize=None):
        """`ChipService.generate_chips` on the resident rasters (report/chip_service.py:397-493): the key points with
        score >= confidence_threshold, per cell of a 5 x 5 grid the centre point and one per quarter, and their 57 x 57 chips of
        both images - raw, stretched to uint8 and, with `laplacian_ksize` (an int or {"mon": k, "ref": k}), their Laplacian.
        `points`: a DataFrame or a mapping of float32 device columns.  -> `karios_amd.report.Chips`, None when no row passes."""
        from ..report.chip_service import pair_chips
        return pair_chips(self, points, confidence_threshold, laplacian_ksize)

    def display_ranges(self, no_values=None, percents=(0.5, 99.5)):
        """The display ranges of the overview figure (report/overview_plot.py:115-118, 153-178) on the resident rasters ->
        (mon, ref) `ops.DisplayRange`: the monitored raster under the pair's mask, `no_values` and `no_data_mon`; the reference
        raster without mask under `no_values` and `no_data_ref`."""
        from .. import ops
        values, pp = ops.display_range_lists(no_values, percents)
        self._ready()
        c = self.ctx
        H, W = self.y_size, self.x_size
        mask = C.c_void_p(self.mask_ptr) if self.mask_ptr else None
        mon = ops.display_range_call(c, "km_display_range_dev", C.c_void_p(self.mon_ptr), self.dtype, H, W, W, mask, W if mask else 0, values,
                                     self.no_data_mon, pp)
        ref = ops.display_range_call(c, "km_display_range_dev", C.c_void_p(self.ref_ptr), self.dtype, H, W, W, None, 0, values, self.no_data_ref, pp)
        return mon, ref

    def point_rasters(self, points, mask: bool = True, delta: bool = True):
        """The rasters behind `kp_mask.tif` and `kp_delta.tif` (report/product_generator.py:138-218) in the reference raster's shape
        -> (mask, delta): uint8 y_size x x_size with 1 at every key point, float32 2 x y_size x x_size of NaN with dx / dy at the
        key points; None for the one not asked for.  `points`: a DataFrame (numpy rasters) or a mapping of float32 device columns
        (device tensors)."""
        from .. import ops
        from ..report.product_generator import point_columns
        cols = point_columns(points, ("x0", "y0", "dx", "dy") if delta else ("x0", "y0"))
        return ops.point_rasters(*cols, shape=(self.y_size, self.x_size), mask=mask, delta=delta, ctx=self.ctx)

    def phase_offset(self) -> np.ndarray:
        """LargeOffsetMatcher.match() on resident data (large_offset.py:39): [row, col]."""
        self._ready()
        c = self.ctx
        out = (C.c_double * 2)()
        c.check(c.lib.km_phase_shift_dev(c.handle, C.c_void_p(self.mon_ptr), C.c_void_p(self.ref_ptr), self.code, self.y_size, self.x_size,
                                         self.x_size, self.x_size, out), "km_phase_shift_dev")
        return np.array([out[0], out[1]], np.float64)

    def shifted_monitored(self, y_off: int, x_off: int) -> "ResidentPair":
        """shift_image(mon, y_off, x_off) on the device (image.py:70-101); returns a new pair sharing ref."""
        self._ready()
        c = self.ctx
        buf = DeviceBuffer(c, self.y_size * self.x_size * self.dtype.itemsize)
        c.check(c.lib.km_shift_image_dev(c.handle, C.c_void_p(self.mon_ptr), self.dtype.itemsize, self.y_size, self.x_size, self.x_size,
                                         int(y_off), int(x_off), C.c_void_p(buf.ptr)), "km_shift_image_dev")
        return ResidentPair(c, buf.ptr, self.ref_ptr, self.dtype, self.y_size, self.x_size, self.mask_ptr, self.no_data_mon,
                            self.no_data_ref, owned=[buf, self])
