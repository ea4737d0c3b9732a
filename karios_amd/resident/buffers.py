"""Device buffers of the resident pairs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .._lib import Context, as_image


class DeviceBuffer:
    """Device buffer drawn from the context's pool (`Context.dev_alloc`)."""

    def __init__(self, ctx: Context, nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        self.ptr, self._cap = ctx.dev_alloc(self.nbytes)
        self.upload_in_flight = False       # an asynchronous upload into this buffer has not been joined / waited for yet

    def free(self):
        if self.ptr:
            ptr_, self.ptr = self.ptr, None
            ctx, cap, flying = self.ctx, self._cap, self.upload_in_flight
            # (a finalizer may run on another thread than the context's: the release is then left for the owning thread)
            ctx.run_or_defer(lambda: ctx.dev_release(ptr_, cap, flying))

    def __del__(self):
        try:
            self.free()
        except Exception:  # pragma: no cover
            pass

    def upload(self, arr: np.ndarray):
        """Blocking upload of a whole array."""
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        self.ctx.check(self.ctx.lib.km_h2d(self.ctx.handle, C.c_void_p(self.ptr), a.ctypes.data_as(C.c_void_p), a.nbytes), "km_h2d")

    def upload_image_async(self, img: np.ndarray) -> np.ndarray:
        """Queue the upload of a 2-D image (rows may be strided views of a larger array) on the context's copy stream and
        return the array that must stay alive until the context's next call: from page-locked memory (`pinned_empty`) this
        returns at once and the copy overlaps whatever the device is computing; from pageable memory the library completes the copy
        before it returns (km_upload_async)."""
        a = as_image(img)
        assert a.shape[0] * a.shape[1] * a.itemsize <= self.nbytes
        w = a.shape[1] * a.itemsize
        self.ctx.check(self.ctx.lib.km_upload_async(self.ctx.handle, C.c_void_p(self.ptr), w, a.ctypes.data_as(C.c_void_p),
                                                    a.strides[0] if a.shape[0] > 1 else w, w, a.shape[0]), "km_upload_async")
        self.upload_in_flight = True
        return a

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        self.ctx.check(self.ctx.lib.km_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), out.nbytes), "km_d2h")
        return out
