"""Mirror of the numbers of `karios.report.shift_by_alt_plot.MeanShiftByAltitudeGroupPlot._plot_alt`
(report/shift_by_alt_plot.py:127-171) and of the altitude column it reads (api/core.py:1049-1053): the key points' altitudes out of
the DEM, the mean profile of a displacement over altitude groups and the statistics `boxplot` computes of those groups - what
`Axes.bxp` takes.  The figure itself stays with the integrator."""
from __future__ import annotations

import numpy as np

from .. import ops
from . import commons
from .product_generator import point_columns

f32 = np.float32


def _dem_raster(dem):
    """-> (numpy array or device tensor, pixel type)."""
    if hasattr(dem, "tensor"):                      # DeviceRasterImage
        return dem.tensor, np.dtype(dem.dtype)
    if hasattr(dem, "data_ptr"):
        return dem, ops.tensor_np_dtype(dem)
    a = np.asarray(dem.array if hasattr(dem, "array") else dem)
    return a, a.dtype


def altitudes(points, dem, ctx=None):
    """`points["alt"] = dem.array[y_index, x_index]`: the DEM's pixel under every key point, in the DEM's type.  `dem`: a numpy
    raster, a device tensor or a `DeviceRasterImage`; the columns are moved to where the DEM lives.  A device DEM gives a device
    tensor (uint16 in the storage type of the tensor)."""
    raster, dt = _dem_raster(dem)
    x0, y0 = point_columns(points, ("x0", "y0"))
    on_device = hasattr(raster, "data_ptr")
    if on_device and not hasattr(x0, "data_ptr"):
        import torch
        x0, y0 = (torch.from_numpy(np.ascontiguousarray(a)).to(raster.device) for a in (x0, y0))
    elif not on_device and hasattr(x0, "data_ptr"):
        x0, y0 = x0.cpu().numpy(), y0.cpu().numpy()
    return ops.sample_points(raster, x0, y0, dtype=dt if on_device else None, ctx=ctx)


def _as_float32(alt, dt):
    """The altitudes as the float32 column the device groups on: exact for the integer types."""
    if not hasattr(alt, "data_ptr"):
        return np.asarray(alt).astype(f32)
    import torch
    if dt == np.uint16:                            # (stored as int16, or as torch's uint16, which few operators take)
        return (alt.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float32)
    return alt.to(torch.float32)


def _host_altitudes(alt, dt):
    if not hasattr(alt, "data_ptr"):
        return np.asarray(alt)
    import torch
    return alt.view(torch.int16).cpu().numpy().view(np.uint16) if dt == np.uint16 else alt.cpu().numpy()


def _relabel(profile, dt, bin_size):
    """Keys and positions of an integer DEM as pandas forms them: in the DEM's own type, wrap included."""
    from pandas import Index, Series
    key = profile.mean_values.index.to_numpy().astype(np.int64).astype(dt)
    with np.errstate(over="ignore"):
        pos = (key * bin_size + bin_size // 2).astype(np.int32)
    index = Index(key, name="po")
    out = commons.MeanProfile(Series(pos, index=index, name="po"), Series(profile.mean_values.to_numpy(), index=index, name="val"),
                              Series(profile.nb_pos.to_numpy(), index=index, name="val"),
                              Series(profile.values_std.to_numpy(), index=index, name="val"), columns=profile._columns)
    return out


def _bxp_stats(box, values, alt32, bin_size):
    """The list of dicts `Axes.bxp` takes, from the device's columns: the fliers are the rows of class 1 of a group in row order,
    then those of class 2."""
    host = commons._host
    cls, v = host(box.cls), host(values)
    cols = {k: host(getattr(box, k)) for k in ("mean",) + ops.BOX_STAT_NAMES}
    rows = np.flatnonzero(cls > 0)
    with np.errstate(all="ignore"):
        key = np.floor_divide(host(alt32)[rows], f32(bin_size)) + f32(0)
    group = np.searchsorted(host(box.key), key)
    out = []
    for g in range(cols["mean"].size):
        mine = rows[group == g]
        st = {k: c[g] for k, c in cols.items()}
        st["fliers"] = np.concatenate([v[mine[cls[mine] == 1]], v[mine[cls[mine] == 2]]])
        out.append(st)
    return out


class AltitudeProfile:
    """`profile`: the `MeanProfile` of the displacement over altitude groups; `box_stats`: per group, in the profile's order, the dict
    of mean, med, q1, q3, iqr, cilo, cihi, whislo, whishi and fliers that `Axes.bxp(box_stats, positions=profile.groups_positions)`
    draws - `boxplot` without its statistics step."""

    def __init__(self, profile, box_stats):
        self.profile, self.box_stats = profile, box_stats


def altitude_profile(points, dem, dimension, x_res, bin_size, ctx=None) -> AltitudeProfile:
    """`_plot_alt`'s numbers: mean_profile(points[dimension] * x_res, points["alt"], bin_size) with the altitudes read out of `dem`,
    and the box statistics of the same groups.  The product is the reference's own expression on a host column - a float32 Series
    times a number stays float32 in pandas - and a float32 product on a device column times a Python number; a float32 product is
    grouped on the device, one of another type (a float64 column, a numpy column times an np.float64) takes the host expressions
    of pandas and matplotlib, as `mean_profile` does."""
    raster, dt = _dem_raster(dem)
    if dt.kind in "ui":
        np.floor_divide(np.zeros(0, dt), bin_size)           # a bin size the DEM's type cannot hold: numpy's OverflowError
    alt = altitudes(points, dem, ctx)
    col = points[dimension]
    if hasattr(col, "data_ptr"):
        # a device column: torch multiplies a float32 tensor by a Python number in float32, as pandas does; anything else goes to the host
        weak = ops.tensor_np_dtype(col) == f32 and (type(x_res) in (int, float) or isinstance(x_res, f32))
        values = col * float(f32(x_res)) if weak else col.cpu().numpy() * x_res
    else:
        values = col * x_res                                   # the reference's expression, with pandas' or numpy's own result type
        values = values.to_numpy() if hasattr(values, "to_numpy") else np.asarray(values)
    if (not hasattr(values, "data_ptr") and values.dtype != f32) or int(bin_size) != bin_size:
        from matplotlib.cbook import boxplot_stats
        from pandas import Series
        profile = commons._pandas_profile(Series(commons._host(values)), Series(_host_altitudes(alt, dt)), bin_size)
        return AltitudeProfile(profile, boxplot_stats([g[1].to_numpy() for g in profile.grouped_values]))
    alt32 = _as_float32(alt, dt)
    if hasattr(alt32, "data_ptr") and not hasattr(values, "data_ptr"):
        import torch
        values = torch.from_numpy(np.ascontiguousarray(values)).to(alt32.device)
    elif hasattr(values, "data_ptr") and not hasattr(alt32, "data_ptr"):
        values = values.cpu().numpy()
    profile = commons.mean_profiles([(values, alt32, int(bin_size))], ctx)[0]
    box = ops.box_stats(values, alt32, int(bin_size), ctx)
    if dt.kind in "ui":
        profile = _relabel(profile, dt, int(bin_size))
    return AltitudeProfile(profile, _bxp_stats(box, values, alt32, int(bin_size)))
