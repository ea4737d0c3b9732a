"""Post-matching step of the reference's API layer on resident data:

  * `handle_klt_results`   - `KariosAPI._handle_klt_results` (karios/api/core.py:848-921): radial error / angle columns,
                              ZNCC + both mutual-information scores of the rows with score >= confidence threshold,
                              CSV written tile by tile (`sep=";"`, header once, no index), frames concatenated;
  * `filter_by_dn_values`  - `KariosAPI._filter_by_dn_values` (core.py:650-737): drop the key points under which the
                              reference or monitored image holds one of the excluded DN values / its no-data value;
  * `_check_quality`       - `KariosAPI._check_quality` (core.py:491-506): the dynamic range between the 2nd and 98th percentile
                              of both rasters, a warning when it is 10 or less;
  * `analyze_accuracy`     - `KariosAPI.analyze_accuracy` (core.py:268-328): valid pixels of the monitored raster under the mask,
                              `GeometricStat`'s statistics, CE90 / CE95 and the line of `correl_res.txt`;
  * `load_mask`            - `KariosAPI._load_mask` (core.py:538-620): the raster mask, the vector mask burnt on the monitored image's
                              grid (`core.image.rasterize_vector_mask`), or their AND with the three logged counts.

The pixel work (ZNCC, MI / NMI, DN gather) runs on the device through `ResidentPair`; the column arithmetic and the
CSV formatting are the reference's own numpy / pandas expressions.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path
from typing import Iterable

import logging

import numpy as np
import pandas as pd

from . import ops
from ._lib import KariosHipError
from .accuracy_analysis import GeometricStat
from .core.configuration import AccuracyAnalysisConfiguration
from .frames import radial_angle_columns
from .resident import MI_SEARCH_COLUMNS, ZNCC_SEARCH_COLUMNS, ResidentPair

logger = logging.getLogger(__name__)

CSV_COLUMNS = ["x0", "y0", "dx", "dy", "score", "radial error", "angle", "zncc_score", "mutual_info_score", "mi_score"]


def handle_klt_results(results: Iterable[pd.DataFrame], csv_file, pair: ResidentPair, confidence_threshold: float = 0.4,
                       large_shift_applied: bool = False, zncc_search_radius: int | None = None, prior=None,
                       outliers_filtering: bool = False, mi_search_radius: int | None = None) -> pd.DataFrame:
    """`KariosAPI._handle_klt_results` (core.py:848-921) for the frames of `KLT.match` / `ResidentPair.match*`.
    With `large_shift_applied` the scores are skipped like in the reference (core.py:909-910) and the CSV has 7 columns.
    With `zncc_search_radius` the scored rows also carry the columns of the ZNCC search (`ResidentPair.zncc_search`,
    ZNCC_SEARCH_COLUMNS) behind the reference's, and with `mi_search_radius` those of the mutual-information search
    (`ResidentPair.mi_search`, MI_SEARCH_COLUMNS) behind both; None, the default, leaves the frame and the CSV as the reference writes them.
    With `prior` (the frames of `KLT.match(..., prior=)`, `karios_amd.matcher.prior`) the rasters were never shifted or resampled: the
    scores are computed although a large shift is in play (`large_shift_applied` is ignored), and `dx_prior, dy_prior` - the float32
    displacement the prior alone predicts - follow the reference's columns; `outliers_filtering` then clips the rows on the residuals
    dx - dx_prior, dy - dy_prior (`ops.sigma_clip`; frames that `KLT.match` already clipped lose nothing)."""
    from .matcher import prior as _prior
    csv_file = Path(csv_file)
    searched = (ZNCC_SEARCH_COLUMNS if zncc_search_radius is not None else []) + (MI_SEARCH_COLUMNS if mi_search_radius is not None else [])
    more = {} if mi_search_radius is None else {"mi_search_radius": mi_search_radius}      # (the default call is the one made before the argument existed)
    all_frame = pd.DataFrame()
    for frame in results:
        if prior is not None:
            if "dx_prior" not in frame.columns:
                frame = frame.copy()
                frame["dx_prior"], frame["dy_prior"] = _prior.prior_columns(frame, prior)
            if outliers_filtering:
                frame = _prior.clip_residuals(frame, ctx=pair.ctx)
            frame = pair.score_frame(frame, confidence_threshold, mutual_info=True, zncc_search_radius=zncc_search_radius, **more)
            frame = frame[CSV_COLUMNS + _prior.PRIOR_COLUMNS + searched]
        elif large_shift_applied:
            frame = radial_angle_columns(frame)
            if "zncc_score" in frame.columns:
                frame = frame.drop(columns=["zncc_score"])
        else:
            frame = pair.score_frame(frame, confidence_threshold, mutual_info=True, zncc_search_radius=zncc_search_radius, **more)
            frame = frame[CSV_COLUMNS + searched]      # the reference's column order, whatever produced zncc_score first
        if not csv_file.exists():
            frame.to_csv(csv_file, sep=";", index=False)
        else:
            frame.to_csv(csv_file, mode="a", sep=";", index=False, header=False)
        all_frame = pd.concat([all_frame, frame])
    return all_frame


def filter_by_dn_values(points: pd.DataFrame, pair: ResidentPair, no_values=None) -> pd.DataFrame:
    """`KariosAPI._filter_by_dn_values` (core.py:650-737) with the DN gather on the device.  `no_values` apply to both
    images; each image's own no-data value (pair.no_data_ref / no_data_mon) applies to that image only."""
    ref_nd, mon_nd = pair.no_data_ref, pair.no_data_mon
    if not no_values and ref_nd is None and mon_nd is None:
        return points
    n = len(points)
    if n == 0:
        return points[np.ones(0, bool)].copy()
    c = pair.ctx
    pair._ready()
    x0 = np.ascontiguousarray(points["x0"].to_numpy(), np.float32)
    y0 = np.ascontiguousarray(points["y0"].to_numpy(), np.float32)
    nv = np.ascontiguousarray([float(v) for v in (no_values or [])], np.float64)
    keep = np.empty(n, np.uint8)
    nr = C.byref(C.c_double(float(ref_nd))) if ref_nd is not None else None
    nm = C.byref(C.c_double(float(mon_nd))) if mon_nd is not None else None
    rc = c.lib.km_dn_keep_dev(c.handle, C.c_void_p(pair.ref_ptr), C.c_void_p(pair.mon_ptr), pair.code, pair.y_size, pair.x_size,
                              pair.x_size, pair.x_size, x0.ctypes.data_as(C.c_void_p), y0.ctypes.data_as(C.c_void_p), n,
                              nv.ctypes.data_as(C.c_void_p) if len(nv) else None, len(nv), nr, nm, keep.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raw = c.lib.km_last_error(c.handle)
        msg = raw.decode() if raw else ""
        if "outside" in msg:
            raise IndexError(msg)                # numpy's fancy indexing raises for an out-of-bounds key point
        raise KariosHipError(f"km_dn_keep_dev: {msg}")
    return points[keep.astype(bool)].copy()


def _dynamic_range(image) -> np.ndarray:
    """np.nanpercentile(image.array, [2, 98]) (core.py:500, 504): on the GPU for 2-D uint8 / uint16 / int16 / float32 rasters, numpy
    for anything else (float64 and 32-bit integer rasters: a float32 key would not order them exactly)."""
    arr = image.array if hasattr(image, "array") else np.asarray(image)
    if arr.ndim == 2 and arr.dtype in ops.PREP_DTYPES:
        return ops.nanpercentile(arr, [2, 98])
    return np.nanpercentile(arr, [2, 98])


def _check_quality(monitored_image, reference_image) -> tuple:
    """`KariosAPI._check_quality` (core.py:491-506): warn about a low dynamic range (98th - 2nd percentile <= 10) of either image.
    -> the two percentile pairs (monitored, reference), which the reference discards."""
    min_max_mon = _dynamic_range(monitored_image)
    if min_max_mon[1] - min_max_mon[0] <= 10:
        logger.warning("Low dynamic range detected for monitored, you could get poor results")
    min_max_ref = _dynamic_range(reference_image)
    if min_max_ref[1] - min_max_ref[0] <= 10:
        logger.warning("Low dynamic range detected for reference, you could get poor results")
    return min_max_mon, min_max_ref


def _mask_pixels(image):
    """The pixels of a mask image: a device tensor for a `DeviceRasterImage`, else its array."""
    return image.tensor if hasattr(image, "tensor") else image.array if hasattr(image, "array") else np.asarray(image)


def load_mask(monitored, raster_mask=None, vector=None, geo_transform=None):
    """`KariosAPI._load_mask` (core.py:538-620) minus the files: `raster_mask` (a raster image of the monitored image's shape, or
    None) and `vector` (what `core.image.rasterize_vector_mask` takes, or None) -> None, the one mask given, or their AND - a pixel
    is valid only if it is valid in BOTH - with the reference's log line and its three counts.  The vector mask is burnt, and the AND
    taken, where the monitored image lives: for a `DeviceRasterImage` nothing but the polygon's vertices (and a raster mask that
    is still on the host) crosses PCIe.  ValueError for a raster mask of another shape (the reference's geo-information check
    stays with the integrator, who holds the geo information)."""
    from .core.image import DeviceRasterImage, NumpyRasterImage, rasterize_vector_mask
    shape = (int(monitored.y_size), int(monitored.x_size))
    if raster_mask is not None:
        if (int(raster_mask.y_size), int(raster_mask.x_size)) != shape:
            raise ValueError(f"Mask shape {(raster_mask.y_size, raster_mask.x_size)} not compatible with monitored image {shape}")
        logger.info("Raster mask loaded")
    vector_mask = None
    if vector is not None:
        vector_mask = rasterize_vector_mask(vector, monitored, geo_transform)
        logger.info("Vector mask rasterized and loaded")
    if raster_mask is None and vector_mask is None:
        logger.info("No mask provided")
        return None
    if raster_mask is None:
        return vector_mask
    if vector_mask is None:
        return raster_mask
    logger.info("Combining raster and vector masks with AND logic")
    a, b = _mask_pixels(raster_mask), _mask_pixels(vector_mask)
    on_device = hasattr(b, "data_ptr")
    if on_device and not hasattr(a, "data_ptr"):
        import torch
        a = torch.as_tensor(np.ascontiguousarray((np.asarray(a) > 0).astype(np.uint8)), device=b.device)
    elif not on_device and hasattr(a, "data_ptr"):
        a = a.detach().cpu().numpy()
    combined, (raster_valid, vector_valid, combined_valid) = ops.combine_masks(a, b)
    logger.info("Mask combination: raster=%d valid pixels, vector=%d valid pixels, combined=%d valid pixels (AND logic)",
                raster_valid, vector_valid, combined_valid)
    return DeviceRasterImage(combined, filepath="combined_mask.tif") if on_device else NumpyRasterImage(combined, filepath="combined_mask.tif")


@dataclass
class AccuracyAnalysis:
    """Result of `analyze_accuracy` (the reference's dataclass of the same name, core.py:79-90)."""

    statistics: GeometricStat
    mean_x: float
    mean_y: float
    std_x: float
    std_y: float
    ce90: float
    ce95: float
    valid_pixels: int
    total_pixels: int


def analyze_accuracy(points, pair: ResidentPair, confidence_threshold: float = 0.4, carto: bool = False, pixel_size=None,
                     stats_file=None, ref_name: str = "ref", mon_name: str = "mon") -> AccuracyAnalysis:
    """`KariosAPI.analyze_accuracy` (core.py:268-328) for the points of `match_images` and the pair they came from: the valid
    pixels of the monitored raster under the pair's mask are counted where the raster lives (`ops` / km_count_valid_pixels_dev on
    pair.mon_ptr / pair.mask_ptr), the statistics and CE90 / CE95 come from `GeometricStat` on the GPU.  `carto`: the monitored
    image has a pixel resolution (`have_pixel_resolution()`); `pixel_size`: the resolution CE is scaled by (None: 1.0, core.py:314);
    `stats_file`: where the line of `correl_res.txt` goes (None: not written)."""
    c = pair.ctx
    pair._ready()
    stats = GeometricStat(AccuracyAnalysisConfiguration(confidence_threshold=confidence_threshold), points, carto, ctx=c)
    n = C.c_int64()
    c.check(c.lib.km_count_valid_pixels_dev(c.handle, C.c_void_p(pair.mon_ptr), pair.code, pair.y_size, pair.x_size, pair.x_size,
                                            C.c_void_p(pair.mask_ptr) if pair.mask_ptr else None, pair.x_size, C.byref(n)),
            "km_count_valid_pixels_dev")
    nb_valid_pixel = int(n.value)
    total_pixels = pair.x_size * pair.y_size
    stats.compute_stats(nb_valid_pixel)
    if stats_file is not None:
        stats.update_statistic_file(ref_name, mon_name, str(stats_file))
    img_res = pixel_size if pixel_size is not None else 1.0
    ce90 = stats.compute_percentile(0.9, img_res)
    ce95 = stats.compute_percentile(0.95, img_res)
    return AccuracyAnalysis(statistics=stats, mean_x=stats.mean_x, mean_y=stats.mean_y, std_x=stats.std_x, std_y=stats.std_y, ce90=ce90,
                            ce95=ce95, valid_pixels=nb_valid_pixel, total_pixels=total_pixels)
