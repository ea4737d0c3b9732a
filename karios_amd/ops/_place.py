"""Where the arrays of one call live - numpy arrays on the host or torch tensors on the context's device - and the argument
helpers built on that answer.  The only module of the package that touches torch."""
import ctypes as C

import numpy as np

from .._lib import as_image, default_context, ptr, row_stride


def _ctx(ctx):
    return ctx if ctx is not None else default_context()


def tensor_np_dtype(t):
    return np.dtype(str(t.dtype).replace("torch.", ""))


def _torch_dtype(np_dtype):
    import torch
    return getattr(torch, np.dtype(np_dtype).name)


class Place:
    """The side the arrays of one call live on: `dev` False for numpy arrays, True for torch tensors (then on `device`).  Built from
    the arrays that decide it (None entries are skipped); a mix is refused with the wrapper's name and its wording of the arguments."""

    def __init__(self, arrays, what="", names="", refusal=None):
        arrays = [a for a in arrays if a is not None]
        self.dev = bool(arrays) and hasattr(arrays[0], "data_ptr")
        self.device = arrays[0].device if self.dev else None
        self.require(arrays, what, names, refusal)

    def holds(self, a):
        return hasattr(a, "data_ptr") == self.dev

    def require(self, arrays, what, names, refusal=None):
        if not all(self.holds(a) for a in arrays):
            raise ValueError(f"{what}: " + (refusal or f"{names} must all be numpy arrays or all be device tensors"))

    def empty(self, shape, np_dtype):
        if not self.dev:
            return np.empty(shape, np_dtype)
        import torch
        return torch.empty(shape, dtype=_torch_dtype(np_dtype), device=self.device)

    def pointer(self, a):
        """The c_void_p argument of an array; None for None."""
        return C.c_void_p(a.data_ptr()) if self.dev and a is not None else ptr(a)

    def address(self, a):
        """The address as an integer, for a structure's field; None for None."""
        return None if a is None else a.data_ptr() if self.dev else a.ctypes.data

    def strides(self, a):                     # in elements
        return tuple(int(s) for s in a.stride()) if self.dev else tuple(s // a.itemsize for s in a.strides)

    def dtype(self, a):
        return tensor_np_dtype(a) if self.dev else a.dtype

    def view(self, a, np_dtype):              # the same bits as another type of the same size
        return a.view(_torch_dtype(np_dtype) if self.dev else np_dtype)

    def to_host(self, a):
        return a.detach().cpu().numpy() if self.dev else np.asarray(a)

    def function(self, c, base):
        """-> (`base` or `base`_dev of the library, its name), the tensors' device synchronised: the library runs on its own stream."""
        what = base + "_dev" if self.dev else base
        if self.dev:
            import torch
            torch.cuda.synchronize(self.device)
        return getattr(c.lib, what), what

    def call(self, c, base, *args):
        fn, what = self.function(c, base)
        c.check(fn(c.handle, *args), what)


def _raster_arg(place, a, what, dtype=None):
    """A 2-D raster with contiguous rows -> (pointer argument, numpy dtype, H, W, row stride).  `dtype` names the pixel type of a
    tensor that only stores its bit pattern."""
    if not place.dev:
        a = as_image(a)
        return ptr(a), a.dtype, a.shape[0], a.shape[1], row_stride(a)
    if a.dim() != 2 or (a.shape[1] > 1 and a.stride(1) != 1):
        raise ValueError(f"{what}: expected a 2-D tensor with contiguous rows")
    dt = tensor_np_dtype(a)
    if dtype is not None:
        if np.dtype(dtype).itemsize != dt.itemsize:
            raise ValueError(f"{what}: pixel type {np.dtype(dtype)} in {dt} storage")
        dt = np.dtype(dtype)
    H, W = int(a.shape[0]), int(a.shape[1])
    return place.pointer(a), dt, H, W, (int(a.stride(0)) if H > 1 else W)


def _mask_arg(place, mask, H, W, what):
    """The optional uint8 mask of an H x W raster, living where the raster lives -> (pointer argument or None, row stride)."""
    if mask is None:
        return None, 0
    if place.dev:
        if not place.holds(mask) or tensor_np_dtype(mask) != np.uint8 or tuple(mask.shape) != (H, W) or (W > 1 and mask.stride(1) != 1):
            raise ValueError(f"{what}: the mask must be a uint8 tensor of the raster's shape with contiguous rows")
        return place.pointer(mask), (int(mask.stride(0)) if H > 1 else W)
    m = np.asarray(mask)
    if m.shape != (H, W):
        raise ValueError(f"{what}: mask shape differs from the raster's")
    m = as_image(m if m.dtype == np.uint8 else (m != 0).astype(np.uint8))
    return ptr(m), row_stride(m)


def _float32_columns(place, cols):
    """-> (the columns; whether all of them are 1-D float32 columns the library can read: numpy's are then contiguous arrays)"""
    if place.dev:
        return tuple(cols), all(tensor_np_dtype(a) == np.float32 and a.dim() == 1 and a.is_contiguous() for a in cols)
    cols = tuple(np.asarray(a) for a in cols)
    f32 = all(a.dtype == np.float32 and a.ndim == 1 for a in cols)
    return (tuple(np.ascontiguousarray(a) for a in cols) if f32 else cols), f32


def _f32_columns(cols, what, names):
    """The columns of one call, all numpy or all device tensors -> (their place, columns as the library reads them, rows)."""
    place = Place(cols, what, names)
    cols, f32 = _float32_columns(place, cols)
    if not f32:
        raise ValueError(f"{what}: {names} must be " + ("contiguous 1-D float32 tensors" if place.dev else "1-D float32 arrays"))
    n = int(cols[0].shape[0])
    if any(int(a.shape[0]) != n for a in cols):
        raise ValueError(f"{what}: {names} differ in length")
    return place, cols, n


def _col_args(place, cols, n):
    return [place.pointer(a) if n else None for a in cols]


def _out_plane(place, out, shape, np_dtype, what):
    """The caller's buffer for one output - a window of a wider buffer is fine - or a fresh one."""
    if out is None:
        return place.empty(shape, np_dtype)
    if not place.holds(out):
        raise ValueError(f"{what}: the output must live where the columns live")
    if (place.dtype(out) != np.dtype(np_dtype) or tuple(out.shape) != tuple(shape) or (shape[-1] > 1 and place.strides(out)[-1] != 1)
            or (not place.dev and not out.flags.writeable)):
        raise ValueError(f"{what}: the output must be a writable {np.dtype(np_dtype).name} buffer of shape {tuple(shape)} with contiguous rows")
    return out
