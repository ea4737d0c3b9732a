"""Mirror of `karios.report.chip_service`: the key-point chips of a matched pair, selected and cut on the GPU.

`CenterAndQuarterCellPointSelector.select_points` and `ChipService.generate_chips` keep the reference's names and arguments
(chip_service.py:46-306, :384-493).  The selection, the 57 x 57 windows, their uint8 stretch and their Laplacian are computed by
libkarios_hip.so (`ops.select_chip_points`, `ops.extract_chips`) on rasters that may already live in HBM (`pair=`); the result is
a `Chips` object and, with `output_dir`, `chips/chips.csv`.  Writing the GeoTIFF / PNG / VRT files stays with the integrator, who
has GDAL and OpenCV.  Columns are read as float32, the type the matcher's frames have.
"""
from __future__ import annotations

import logging
import os
import shutil
from pathlib import Path

import numpy as np
import pandas as pd

from .. import ops
from .._lib import KariosHipError

logger = logging.getLogger(__name__)

COLUMNS = ("x0", "y0", "dx", "dy", "score")


class Chips:
    """What `generate_chips` produced for the selected key points, row i of every member belonging to row i of `points`:
    `points` the selected frame (float64, every input column; the rows of chips.csv, skipped rows included), `written` whether the
    row's chips lie inside both rasters, `names` its (REF_{x0}_{y0}, MON_{x0}_{y0}) file stems, `windows` the chip centres
    (X0, Y0, X1, Y1), `ref_raw` / `mon_raw` the chips in the rasters' type, `ref_u8` / `mon_u8` their uint8 stretch, `ref_lap` /
    `mon_lap` their Laplacian (None without `laplacian_ksize`); all n x 57 x 57 numpy arrays, zero where the row is not written."""

    def __init__(self, points, images):
        self.points = points
        self.written = np.asarray(images.ok, bool)
        self.windows = np.asarray(images.windows)
        self.names = [(f"REF_{int(x)}_{int(y)}", f"MON_{int(x)}_{int(y)}") for x, y in zip(self.windows[:, 0], self.windows[:, 1])]
        for key in ("ref_raw", "mon_raw", "ref_u8", "mon_u8", "ref_lap", "mon_lap"):
            setattr(self, key, getattr(images, key))

    def __len__(self):
        return len(self.points)


def kernel_sizes(laplacian_ksize):
    """-> (ref, mon) kernel sizes as the reference looks them up (:619-621), (None, None) without; an int stands for both."""
    if laplacian_ksize is None:
        return None, None
    if isinstance(laplacian_ksize, (int, np.integer)):
        return int(laplacian_ksize), int(laplacian_ksize)
    d = laplacian_ksize
    return d.get("ref", d.get("mon", 1)), d.get("mon", d.get("ref", 1))


def _selected_frame(df, index):
    out = df.iloc[np.asarray(index, np.int64)].reset_index(drop=True)
    return out.astype({k: np.float64 for k in out.columns if pd.api.types.is_numeric_dtype(out[k])})


def _f32(df, names):
    return [np.ascontiguousarray(df[k].to_numpy(), np.float32) for k in names]


def _require(df, names):
    missing = [k for k in names if k not in df.columns]
    if missing:
        raise ValueError(f"Missing required columns: {missing}")


class CenterAndQuarterCellPointSelector:
    """Select points from image cells: the point closest to the cell's centre, then per quarter the point whose distance to the
    centre is closest to the quarter's median distance (chip_service.py:46-306)."""

    def __init__(self, image_width, image_height, grid_size=(5, 5), ctx=None):
        self.image_width, self.image_height = image_width, image_height
        self.grid_rows, self.grid_cols = grid_size
        self._ctx = ctx

    def select_index(self, df, threshold=-np.inf) -> np.ndarray:
        """Positions of the selected rows of `df` (columns x0, y0, score) among the rows with score >= threshold."""
        _require(df, ("x0", "y0", "score"))
        if len(df) == 0:
            return np.zeros(0, np.int32)
        return ops.select_chip_points(*_f32(df, ("x0", "y0", "score")), self.image_width, self.image_height, threshold,
                                      (self.grid_rows, self.grid_cols), ctx=self._ctx)

    def select_points(self, df):
        """-> the selected rows as a float64 frame with every input column and the index reset; an empty frame for an empty one."""
        if df.empty:
            return pd.DataFrame()
        index = self.select_index(df)
        return _selected_frame(df, index) if len(index) else pd.DataFrame()


def pair_chips(pair, points, confidence_threshold=0.4, laplacian_ksize=None):
    """`ResidentPair.chips`: selection and chips on the pair's resident rasters -> Chips, or None when no row passes.  `points`: a
    DataFrame, or a mapping of float32 device tensors (x0, y0, dx, dy, score and whatever else the frame carries)."""
    import ctypes as C

    from .. import _lib
    from ..resident import DeviceBuffer
    if pair.window is not None:
        raise KariosHipError("chips: the pair holds a window of its image only")
    kr, km = (ops.chip_ksize(k) for k in kernel_sizes(laplacian_ksize))
    c = pair.ctx
    if isinstance(points, pd.DataFrame):
        _require(points, COLUMNS)
        if len(points) == 0:
            return None
        selector = CenterAndQuarterCellPointSelector(pair.x_size, pair.y_size, ctx=c)
        index = selector.select_index(points, confidence_threshold)
        if len(index) == 0:
            return None
        frame = _selected_frame(points, index)
    else:
        missing = [k for k in COLUMNS if k not in points]
        if missing:
            raise ValueError(f"Missing required columns: {missing}")
        if int(points["score"].shape[0]) == 0:
            return None
        index = ops.select_chip_points(points["x0"], points["y0"], points["score"], pair.x_size, pair.y_size, confidence_threshold, ctx=c)
        if int(index.shape[0]) == 0:
            return None
        rows = index.long()
        frame = pd.DataFrame({k: v[rows].detach().cpu().numpy().astype(np.float64) for k, v in points.items()})
    n = len(frame)
    cols = np.concatenate(_f32(frame, ("x0", "y0", "dx", "dy")))
    pair._ready()
    px, es = n * ops.CHIP_SIZE * ops.CHIP_SIZE, pair.dtype.itemsize
    sizes = [("ref_raw", px * es), ("mon_raw", px * es), ("ref_u8", px), ("mon_u8", px), ("ref_lap", px if kr else 0), ("mon_lap", px if km else 0),
             ("ok", n), ("windows", 16 * n), ("cols", 16 * n)]          # (the first eight in km_chip_outputs' order)
    offsets, total = {}, 0
    for key, size in sizes:
        offsets[key] = total
        total += (size + 255) & ~255
    buf = DeviceBuffer(c, total)
    c.check(c.lib.km_h2d(c.handle, C.c_void_p(buf.ptr + offsets["cols"]), cols.ctypes.data_as(C.c_void_p), cols.nbytes), "km_h2d")
    out = _lib.ChipOutputs(*(buf.ptr + offsets[k] if size else None for k, size in sizes[:8]))
    f = buf.ptr + offsets["cols"]
    c.check(c.lib.km_chips_dev(c.handle, C.c_void_p(pair.ref_ptr), C.c_void_p(pair.mon_ptr), pair.code, pair.y_size, pair.x_size, pair.y_size,
                               pair.x_size, pair.x_size, pair.x_size, C.c_void_p(f), C.c_void_p(f + 4 * n), C.c_void_p(f + 8 * n),
                               C.c_void_p(f + 12 * n), n, kr, km, C.byref(out)), "km_chips_dev")
    raw = buf.download((total,), np.uint8)
    buf.free()
    shape = (n, ops.CHIP_SIZE, ops.CHIP_SIZE)

    def part(key, dtype, shp):
        size = dict(sizes)[key]
        return raw[offsets[key]:offsets[key] + size].view(dtype).reshape(shp).copy() if size else None

    images = ops.ChipImages(ok=part("ok", np.uint8, (n,)) != 0, windows=part("windows", np.int32, (n, 4)), ref_raw=part("ref_raw", pair.dtype, shape),
                            mon_raw=part("mon_raw", pair.dtype, shape), ref_u8=part("ref_u8", np.uint8, shape), mon_u8=part("mon_u8", np.uint8, shape),
                            ref_lap=part("ref_lap", np.uint8, shape), mon_lap=part("mon_lap", np.uint8, shape))
    return Chips(frame, images)


class ChipService:
    """Generates the key-point chips (57 x 57 px) of the monitored and reference images."""

    def __init__(self):
        self._ouput_dir_name = "chips"
        self._laplacian_output_dir_name = "chips_laplacian"
        self._chip_size = ops.CHIP_SIZE

    def generate_chips(self, monitored, reference, points, confident_threshold, output_dir=None, laplacian_ksize=None, pair=None, ctx=None):
        """At most 125 chips of the key points with score >= confident_threshold: per cell of a 5 x 5 grid over the monitored image
        the centre point and one per quarter; reference chips centred on (x0, y0), monitored ones on round(x0 + dx), round(y0 + dy)
        (chip_service.py:397-493).  With `pair` (a ResidentPair of the two rasters) nothing is read from the image objects except
        their names; without, their arrays go through `resident.shared_pair` (rasters of one shape and type) or are staged for the
        call.  -> Chips, or None (with the reference's warning) when no key point passes.  With `output_dir`, `chips/chips.csv`
        is written (sep=";", no index) into a cleaned `chips` directory, beside the empty directories the chip files go to."""
        logger.info("Generate chips")
        _require(points, COLUMNS)
        ksizes = kernel_sizes(laplacian_ksize)
        for k in ksizes:
            ops.chip_ksize(k)
        if len(points) == 0 or not (points["score"] >= confident_threshold).any():
            logger.warning("No KP found having score gte to confident threshold %s to extract chip", confident_threshold)
            return None
        chips = None
        if pair is None:
            mon, ref = np.asarray(monitored.array), np.asarray(reference.array)
            if mon.shape == ref.shape and mon.dtype == ref.dtype:
                from ..resident import shared_pair
                pair = shared_pair(mon, ref, ctx, rasters=(monitored, reference))
            else:
                selector = CenterAndQuarterCellPointSelector(monitored.x_size, monitored.y_size, ctx=ctx)
                frame = _selected_frame(points, selector.select_index(points, confident_threshold))
                chips = Chips(frame, ops.extract_chips(ref, mon, *_f32(frame, ("x0", "y0", "dx", "dy")), *ksizes, ctx=ctx))
        if chips is None:
            chips = pair_chips(pair, points, confident_threshold, laplacian_ksize)
        logger.info("Select %s/%s points (%.2f%%) based on confident threshold %s", len(chips), points.size, 100 * len(chips) / len(points),
                    confident_threshold)
        for _ in range(int((~chips.written).sum())):
            logger.warning("Chip to close to image boundaries, skip it")
        if output_dir is not None:
            self._write(chips, monitored, reference, Path(output_dir), laplacian_ksize is not None)
        return chips

    def _write(self, chips, monitored, reference, output_dir, with_laplacian):
        names = [(self._ouput_dir_name, "Chips")] + ([(self._laplacian_output_dir_name, "Laplacian chips")] if with_laplacian else [])
        for name, what in names:
            path = output_dir / name
            if os.path.exists(path):
                logger.warning("%s output dir already exists, clean it", what)
                shutil.rmtree(path)
            os.mkdir(path)
            for image in (monitored, reference):
                os.makedirs(path / image.file_name, exist_ok=True)
        chips.points.to_csv(output_dir / self._ouput_dir_name / "chips.csv", sep=";", index=False)
        logger.info("Chips generated in %s", output_dir / self._ouput_dir_name)
