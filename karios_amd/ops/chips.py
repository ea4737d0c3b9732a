"""ChipService.generate_chips (csrc/api_chips.hip km_chip_select / km_chips, k_chips.hip)."""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import Context, KariosHipError
from ._place import _col_args, _ctx, _f32_columns, _raster_arg
from .prep import PREP_DTYPES

CHIP_SIZE = _lib.CHIP_SIZE
CHIP_KSIZES = (1, 3, 5, 7, 9, 11)


def select_chip_points(x0, y0, score, width, height, threshold, grid=(5, 5), ctx: Context | None = None):
    """CenterAndQuarterCellPointSelector.select_points (report/chip_service.py:46-306) on the rows with score >= threshold, for
    float32 columns: the row indices (int32) in the reference's output order - per cell of the `grid` (rows, cols) over a
    width x height image the row nearest to the centre, then one row per quarter.  A Python-float threshold compares in float32
    like the reference's frame does, an np.float64 in float64.  numpy columns give a numpy array, device tensors a device tensor."""
    place, cols, n = _f32_columns((x0, y0, score), "select_chip_points", "x0, y0 and score")
    rows, ncols = (int(v) for v in grid)
    if not (1 <= rows <= _lib.CHIP_MAX_GRID and 1 <= ncols <= _lib.CHIP_MAX_GRID):
        raise ValueError(f"select_chip_points: grid {grid} (1 .. {_lib.CHIP_MAX_GRID} cells per axis)")
    if n > _lib.CHIP_SELECT_MAX_ROWS:
        raise ValueError(f"select_chip_points: {n} rows (at most 2^24)")
    cap = rows * ncols * _lib.CHIP_PICKS
    count = C.c_int32()
    tail = (n, int(width), int(height), float(threshold), int(isinstance(threshold, np.float64)), rows, ncols)
    out = place.empty(cap, np.int32)
    place.call(_ctx(ctx), "km_chip_select", *_col_args(place, cols, n), *tail, *_col_args(place, (out,), cap), C.byref(count))
    return out[:count.value]


class ChipImages:
    """Result of `extract_chips` for n rows: `ok` (n, bool), `windows` (n, 4: X0, Y0 of ref and X1, Y1 of mon, the chip centres),
    `ref_raw` / `mon_raw` (n, 57, 57 in the rasters' type), `ref_u8` / `mon_u8`, `ref_lap` / `mon_lap` (uint8; None without a
    kernel size).  Rows that are not ok are zero in every image."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def chip_ksize(k):
    """Kernel size argument of the library: None -> 0 (no Laplacian), else one of CHIP_KSIZES."""
    if k is None:
        return 0
    if int(k) != k or int(k) not in CHIP_KSIZES:
        raise ValueError(f"Laplacian kernel size {k} (one of {CHIP_KSIZES} or None)")
    return int(k)


def extract_chips(ref, mon, x0, y0, dx, dy, ksize_ref=None, ksize_mon=None, ctx: Context | None = None) -> ChipImages:
    """The chips of `_to_chips_gdal_dataset` (report/chip_service.py:544-648) for the rows x0, y0, dx, dy (float32): the 57 x 57
    windows of `ref` around (int(x0), int(y0)) and of `mon` around (round(x0 + dx), round(y0 + dy)), their uint8 stretch by each
    chip's own minimum and maximum and, with a kernel size, cv2.Laplacian(u8, CV_8U, ksize) of each chip.  Rasters: 2-D uint8 /
    uint16 / int16 / float32 of one type, each at least 57 x 57 (windows of wider buffers are fine); numpy in gives numpy out,
    device tensors in give device tensors out."""
    kr, km = chip_ksize(ksize_ref), chip_ksize(ksize_mon)
    place, cols, n = _f32_columns((x0, y0, dx, dy), "extract_chips", "x0, y0, dx and dy")
    place.require((ref, mon), "extract_chips", "rasters and columns")
    if n > _lib.CHIP_MAX_ROWS:
        raise ValueError(f"extract_chips: {n} rows (at most 2^20)")
    if place.dev and any(a.dim() != 2 or (a.shape[1] > 1 and a.stride(1) != 1) for a in (ref, mon)):
        raise ValueError("extract_chips: expected 2-D tensors with contiguous rows")
    ref_arg, dt, Hr, Wr, sref = _raster_arg(place, ref, "extract_chips")
    mon_arg, dt_m, Hm, Wm, smon = _raster_arg(place, mon, "extract_chips")
    if dt != dt_m or dt not in PREP_DTYPES:
        raise KariosHipError(f"extract_chips: rasters of {dt} and {dt_m} (one of uint8, uint16, int16, float32 for both)")
    if min(Hr, Wr, Hm, Wm) < CHIP_SIZE:
        raise ValueError(f"extract_chips: rasters of {(Hr, Wr)} and {(Hm, Wm)} (at least {CHIP_SIZE} x {CHIP_SIZE})")
    shape = (n, CHIP_SIZE, CHIP_SIZE)
    empty = place.empty
    res = ChipImages(ok=empty((n,), np.uint8), windows=empty((n, 4), np.int32), ref_raw=empty(shape, dt), mon_raw=empty(shape, dt), ref_u8=empty(shape, np.uint8),
                     mon_u8=empty(shape, np.uint8), ref_lap=empty(shape, np.uint8) if kr else None, mon_lap=empty(shape, np.uint8) if km else None)
    if n:
        c = _ctx(ctx)
        out = _lib.ChipOutputs(*(place.address(a) for a in (res.ref_raw, res.mon_raw, res.ref_u8, res.mon_u8, res.ref_lap, res.mon_lap, res.ok, res.windows)))
        place.call(c, "km_chips", ref_arg, mon_arg, _lib._DTYPES[dt], Hr, Wr, Hm, Wm, sref, smon, *_col_args(place, cols, n), n, kr, km, C.byref(out))
        if place.dev:
            c.sync()
    res.ok = res.ok != 0
    return res
