"""Mirror of `karios.report.product_generator.ProductGenerator._create_mask` / `_create_intermediate_raster`
(report/product_generator.py:138-218) minus the file: the key-point mask behind `kp_mask.tif` and the dx / dy raster behind
`kp_delta.tif`, built on the device.  Opening the GeoTIFF, its grid, compression and the GeoJSON stay with the integrator."""
from __future__ import annotations

import numpy as np

from .. import ops

COLUMNS = ("x0", "y0", "dx", "dy")


def _host_column(col, index: bool):
    a = col.to_numpy() if hasattr(col, "to_numpy") else np.asarray(col)
    if a.dtype == np.float32:
        return a
    # the reference's own conversions: `.astype(int)` for a coordinate (an index float32 holds exactly), `.astype(np.float32)` else
    return a.astype(int).astype(np.float32) if index else a.astype(np.float32)


def point_columns(points, names=COLUMNS):
    """The float32 columns `names` of a frame: a DataFrame (or mapping of numpy columns) gives numpy arrays, a mapping of device
    tensors gives those tensors."""
    missing = [k for k in names if k not in points]
    if missing:
        raise ValueError(f"Missing required columns: {missing}")
    cols = [points[k] for k in names]
    if all(hasattr(c, "data_ptr") for c in cols):
        return cols
    return [_host_column(c, k in ("x0", "y0")) for k, c in zip(names, cols)]


def _shape(pair_or_shape):
    if hasattr(pair_or_shape, "y_size"):
        return int(pair_or_shape.y_size), int(pair_or_shape.x_size)
    H, W = pair_or_shape
    return int(H), int(W)


def _ctx(pair_or_shape, ctx):
    return ctx if ctx is not None else getattr(pair_or_shape, "ctx", None)


def kp_mask(points, pair_or_shape, out=None, ctx=None):
    """`_create_mask`: the uint8 raster of the reference image's shape - a `ResidentPair` or (y_size, x_size) - with 1 at every key
    point; a numpy array for a DataFrame, a device tensor for device columns."""
    x0, y0 = point_columns(points, ("x0", "y0"))
    return ops.point_rasters(x0, y0, shape=_shape(pair_or_shape), delta=False, out_mask=out, ctx=_ctx(pair_or_shape, ctx))[0]


def kp_delta(points, pair_or_shape, out=None, ctx=None):
    """`_create_intermediate_raster`: the float32 raster of two bands, NaN with dx (band 0) and dy (band 1) at the key points."""
    x0, y0, dx, dy = point_columns(points)
    return ops.point_rasters(x0, y0, dx, dy, shape=_shape(pair_or_shape), mask=False, out_delta=out, ctx=_ctx(pair_or_shape, ctx))[1]
