"""The masks a pair is matched under (csrc/api_prep.hip km_rasterize_polygons, km_mask_and; k_mask.hip): a vector mask burnt on the
raster's grid as `gdal.RasterizeLayer(..., options=['BURN=1', 'ALL_TOUCHED=TRUE'])` burns polygons (core/image.py:104-191) and its AND
with a raster mask (api/core.py:593-612).  tests/rasterize_restatement.py is the definition; GDAL itself was never run against it."""
import ctypes as C
import json as _json
import math as _math
import os as _os

import numpy as np

from .. import _lib
from .._lib import Context, ptr
from ._place import Place, _ctx, _out_plane, tensor_np_dtype
from .report import _raster_shape

MASK_MAX_VERTICES, MASK_MAX_COORD = _lib.MASK_MAX_VERTICES, _lib.MASK_MAX_COORD


def geo_to_pixel(xy, geo_transform):
    """World coordinates -> pixel / line, as GDALInvGeoTransform then GDALApplyGeoTransform compute them in float64: a sequence of
    (X, Y) -> a list of (pixel, line).  Reprojection between a layer's CRS and the raster's is not done here."""
    gt = [float(v) for v in geo_transform]
    if len(gt) != 6:
        raise ValueError("geo_to_pixel: a geotransform has six coefficients")
    if gt[2] == 0.0 and gt[4] == 0.0 and gt[1] != 0.0 and gt[5] != 0.0:
        inv = (-gt[0] / gt[1], 1.0 / gt[1], 0.0, -gt[3] / gt[5], 0.0, 1.0 / gt[5])
    else:
        det = gt[1] * gt[5] - gt[2] * gt[4]
        if det == 0.0:
            raise ValueError("geo_to_pixel: the geotransform is not invertible")
        inv_det = 1.0 / det
        inv = ((gt[2] * gt[3] - gt[0] * gt[5]) * inv_det, gt[5] * inv_det, -gt[2] * inv_det,
               (-gt[1] * gt[3] + gt[0] * gt[4]) * inv_det, -gt[4] * inv_det, gt[1] * inv_det)
    return [(inv[0] + float(p[0]) * inv[1] + float(p[1]) * inv[2], inv[3] + float(p[0]) * inv[4] + float(p[1]) * inv[5]) for p in xy]


def _geometry_rings(geometry, what):
    """Every ring of a Polygon, a MultiPolygon or a GeometryCollection of those: one feature, as GDAL collects the rings of a shape."""
    kind = geometry.get("type") if isinstance(geometry, dict) else None
    if kind == "Polygon":
        return [list(ring) for ring in geometry["coordinates"]]
    if kind == "MultiPolygon":
        return [list(ring) for polygon in geometry["coordinates"] for ring in polygon]
    if kind == "GeometryCollection":
        return [ring for member in geometry["geometries"] for ring in _geometry_rings(member, what)]
    raise NotImplementedError(f"{what}: geometry type {kind!r} (Polygon, MultiPolygon and GeometryCollection of those only)")


def geojson_features(doc, what="geojson_features"):
    """A parsed GeoJSON document - FeatureCollection, Feature, Polygon, MultiPolygon or GeometryCollection of those - -> the list of
    features `rasterize_polygons` takes, in the document's coordinates: per OGR feature the rings of all its polygons (the members
    of a MultiPolygon share a feature, so where they overlap they cancel).  A Feature without a geometry burns nothing."""
    kind = doc.get("type") if isinstance(doc, dict) else None
    if kind == "FeatureCollection":
        members = doc["features"]
    elif kind == "Feature":
        members = [doc]
    else:
        return [_geometry_rings(doc, what)]
    out = []
    for member in members:
        if not isinstance(member, dict) or member.get("type") != "Feature":
            raise NotImplementedError(f"{what}: a FeatureCollection holds {member.get('type') if isinstance(member, dict) else member!r}")
        if member.get("geometry") is not None:
            out.append(_geometry_rings(member["geometry"], what))
    return out


def read_vector_features(vector, what="read_vector_features"):
    """A GeoJSON path or a parsed GeoJSON dict -> its features in the file's coordinates.  Other file formats need OGR, which this
    project does not have: NotImplementedError naming the format."""
    if isinstance(vector, dict):
        return geojson_features(vector, what)
    path = _os.fspath(vector)
    ext = _os.path.splitext(path)[1].lower()
    if ext not in (".geojson", ".json"):
        raise NotImplementedError(f"{what}: vector format {ext or path!r} (GeoJSON only: convert other formats with OGR first)")
    with open(path, "r", encoding="utf-8") as f:
        return geojson_features(_json.load(f), what)


def _polygon_tables(features, what):
    """The three host tables of km_rasterize_polygons; rings are closed here, rings of fewer than 2 points dropped."""
    xy, ring_sizes, feature_rings = [], [], []
    for feature in features:
        rings = 0
        for ring in feature:
            pts = [(float(p[0]), float(p[1])) for p in ring]
            for x, y in pts:
                if not (_math.isfinite(x) and _math.isfinite(y)):
                    raise ValueError(f"{what}: a vertex is not finite")
                if abs(x) > MASK_MAX_COORD or abs(y) > MASK_MAX_COORD:
                    raise ValueError(f"{what}: a vertex lies beyond 2^30")
            if len(pts) < 2:
                continue
            if pts[0] != pts[-1]:
                pts.append(pts[0])
            xy.extend(pts)
            ring_sizes.append(len(pts))
            rings += 1
        feature_rings.append(rings)
    if len(xy) > MASK_MAX_VERTICES:
        raise ValueError(f"{what}: {len(xy)} vertices (at most 2^20)")
    return (np.ascontiguousarray(np.array(xy, np.float64).reshape(-1, 2)), np.array(ring_sizes, np.int32), np.array(feature_rings, np.int32))


def rasterize_polygons(features, shape, out=None, device=None, ctx: Context | None = None):
    """`gdal.RasterizeLayer(..., options=['BURN=1', 'ALL_TOUCHED=TRUE'])` of polygon features on an H x W grid of zeros -> the uint8
    raster, 1 where a feature's fill (even-odd at pixel centres, GDAL's half-open rules) or the all-touched pass over its rings
    burns.  `features`: a list of features, each a list of rings, each a list of (x, y) in pixel / line space (see `geo_to_pixel`);
    all rings of a MultiPolygon are ONE feature.  Open rings are closed, rings of fewer than 2 points dropped.  The result is a numpy
    array unless `out` (a uint8 H x W buffer, numpy or device tensor; a window of a wider buffer is fine) or `device` (a torch
    device) puts it on the device.  ValueError for a vertex that is not finite or lies beyond 2^30, and for more than 2^20
    vertices."""
    what = "rasterize_polygons"
    H, W = _raster_shape(shape, what)
    xy, ring_sizes, feature_rings = _polygon_tables(features, what)
    if out is None and device is not None:
        import torch
        out = torch.empty((H, W), dtype=torch.uint8, device=device)
    place = Place((out,), what, "the output")
    out = _out_plane(place, out, (H, W), np.uint8, what)
    stride = place.strides(out)[0] if H > 1 else W
    place.call(_ctx(ctx), "km_rasterize_polygons", ptr(xy), int(xy.shape[0]), ptr(ring_sizes), int(ring_sizes.size), ptr(feature_rings),
               int(feature_rings.size), H, W, place.pointer(out), stride)
    return out


def combine_masks(raster_mask, vector_mask, ctx: Context | None = None):
    """`np.logical_and(raster_mask > 0, vector_mask > 0).astype(np.uint8)` of two masks of one shape (api/core.py:595-598) and the
    three counts `_load_mask` logs -> (mask, (raster_valid, vector_valid, combined_valid)).  Both numpy arrays or both uint8 device
    tensors with contiguous rows (windows are fine)."""
    what = "combine_masks"
    place = Place((raster_mask, vector_mask), what, "the two masks")
    if place.dev:
        masks = (raster_mask, vector_mask)
        if any(m.dim() != 2 or tensor_np_dtype(m) != np.uint8 or (m.shape[1] > 1 and m.stride(1) != 1) for m in masks):
            raise ValueError(f"{what}: the masks must be 2-D uint8 tensors with contiguous rows")
    else:
        masks = tuple(np.asarray(m) for m in (raster_mask, vector_mask))
        if any(m.ndim != 2 for m in masks):
            raise ValueError(f"{what}: the masks must be 2-D")
        masks = tuple(_lib.as_image(m if m.dtype == np.uint8 else (m > 0).astype(np.uint8)) for m in masks)
    if tuple(masks[0].shape) != tuple(masks[1].shape):
        raise ValueError(f"{what}: mask shapes differ: {tuple(masks[0].shape)} and {tuple(masks[1].shape)}")
    H, W = _raster_shape(masks[0].shape, what)
    out = place.empty((H, W), np.uint8)
    strides = [place.strides(m)[0] if H > 1 else W for m in masks]
    counts = (C.c_int64 * 3)()
    place.call(_ctx(ctx), "km_mask_and", place.pointer(masks[0]), strides[0], place.pointer(masks[1]), strides[1], H, W, place.pointer(out), W, counts)
    return out, (int(counts[0]), int(counts[1]), int(counts[2]))
