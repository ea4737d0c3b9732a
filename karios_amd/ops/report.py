"""The report's numbers and products (csrc/api_report.hip km_mean_profiles, km_point_rasters, km_sample_points, km_box_stats;
k_report.hip, k_products.hip) and the circular-error figure's (km_ce_figure, k_ce.hip)."""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import Context, KariosHipError
from ._place import Place, _col_args, _ctx, _f32_columns, _float32_columns, _out_plane, _raster_arg
from .accuracy import ACCURACY_MAX_ROWS, _accuracy_host, ce_ranks
from .prep import PREP_DTYPES

PROFILE_MAX, PROFILE_MAX_ROWS, PROFILE_MAX_BIN = _lib.PROFILE_MAX, _lib.PROFILE_MAX_ROWS, _lib.PROFILE_MAX_BIN


class ProfileColumns:
    """One profile of `mean_profiles`: `key` (float32, the groups' np.floor_divide(positions, bin_size), ascending), `position`
    (int32, the reference's groups_positions), `count` (int32 rows whose value is not NaN), `mean` and `std` (float32); numpy arrays,
    or device tensors for device input."""

    def __init__(self, key, position, count, mean, std):
        self.key, self.position, self.count, self.mean, self.std = key, position, count, mean, std


def mean_profiles(profiles, ctx: Context | None = None):
    """`mean_profile` (report/commons.py:49-71) of 1 .. 8 profiles in one call: `profiles` is a sequence of (values, positions,
    bin_size) with float32 columns of one length (at most 2^20 rows; all numpy or all device tensors) and 1 <= bin_size <= 2^24
    -> a list of `ProfileColumns`.  ValueError when a group's position lies outside int32, where numpy's cast is not defined."""
    profiles = [tuple(p) for p in profiles]
    if not 1 <= len(profiles) <= PROFILE_MAX:
        raise ValueError(f"mean_profiles: {len(profiles)} profiles (1 .. {PROFILE_MAX} per call)")
    cols = []
    for values, positions, _bin in profiles:
        cols += [values, positions]
    place, cols, n = _f32_columns(tuple(cols), "mean_profiles", "values and positions")
    if n > PROFILE_MAX_ROWS:
        raise ValueError(f"mean_profiles: {n} rows (at most 2^20)")
    bins = []
    for _v, _p, b in profiles:
        if int(b) != b or not 1 <= int(b) <= PROFILE_MAX_BIN:
            raise ValueError(f"mean_profiles: bin size {b} (an integer, 1 .. 2^24)")
        bins.append(int(b))
    k = len(profiles)
    recs = (_lib.Profile * k)()
    outs = []
    for i in range(k):
        o = [place.empty(n, t) for t in (np.float32, np.int32, np.int32, np.float32, np.float32)]
        outs.append(o)
        r = recs[i]
        r.values, r.positions, r.key, r.position, r.count, r.mean, r.std = [place.address(a) if n else None for a in (cols[2 * i], cols[2 * i + 1], *o)]
        r.bin_size = bins[i]
    groups, oor = (C.c_int32 * k)(), (C.c_int32 * k)()
    place.call(_ctx(ctx), "km_mean_profiles", n, k, recs, groups, oor)
    if any(oor):
        raise ValueError(f"mean_profiles: {sum(oor)} group position(s) outside int32")
    return [ProfileColumns(*(a[:groups[i]] for a in outs[i])) for i in range(k)]


BOX_STAT_NAMES = ("q1", "med", "q3", "iqr", "cilo", "cihi", "whislo", "whishi")     # the columns of km_box_stats, in its order


def _raster_shape(shape, what):
    H, W = (int(v) for v in shape)
    if H < 1 or W < 1 or H * W >= 2 ** 32 - 1:
        raise ValueError(f"{what}: a raster of {H} x {W} (at least 1 x 1, fewer than 2^32 - 1 pixels)")
    return H, W


def point_rasters(x0, y0, dx=None, dy=None, shape=None, mask=True, delta=True, out_mask=None, out_delta=None, ctx: Context | None = None):
    """ProductGenerator._create_mask / _create_intermediate_raster (report/product_generator.py:138-218) minus the file: for float32
    key-point columns and a raster `shape` (H, W) -> (`mask`, `delta`): the uint8 H x W raster with 1 at every key point and the
    float32 2 x H x W raster of NaN with dx / dy at the key points (None for the one not asked for; `dx = dy = None` gives the mask
    alone).  Pixels are `x0.astype(int)`, `y0.astype(int)`; columns wrap as numpy's assignment into a row buffer does, rows do not;
    of several rows on one pixel the last wins.  numpy columns give numpy rasters, device tensors device tensors; `out_mask` /
    `out_delta` may name the buffers to fill (windows of wider buffers included).  IndexError, as from the reference, when a row lies
    outside the raster or has a NaN or infinite coordinate."""
    delta = bool(delta) and dx is not None
    mask = bool(mask)
    if (dx is None) != (dy is None):
        raise ValueError("point_rasters: dx and dy come together")
    if shape is None:
        raise ValueError("point_rasters: the raster's shape is needed")
    H, W = _raster_shape(shape, "point_rasters")
    place, cols, n = _f32_columns((x0, y0) + ((dx, dy) if delta else ()), "point_rasters", "x0, y0, dx and dy")
    if n > PROFILE_MAX_ROWS:
        raise ValueError(f"point_rasters: {n} rows (at most 2^20)")
    m = _out_plane(place, out_mask, (H, W), np.uint8, "point_rasters") if mask else None
    d = _out_plane(place, out_delta, (2, H, W), np.float32, "point_rasters") if delta else None
    args = _col_args(place, cols, n) + [None] * (4 - len(cols))
    ms = (place.strides(m)[0] if H > 1 else W) if mask else 0
    bs, rs = ((place.strides(d)[0], place.strides(d)[1] if H > 1 else W) if delta else (0, 0))
    bad = C.c_int32()
    place.call(_ctx(ctx), "km_point_rasters", n, *args, H, W, place.pointer(m), ms, place.pointer(d), bs, rs, C.byref(bad))
    if bad.value:
        raise IndexError(f"point_rasters: {bad.value} row(s) out of bounds for a raster of {H} x {W}")
    return m, d


def sample_points(raster, x0, y0, dtype=None, ctx: Context | None = None):
    """`raster[y0.astype(int), x0.astype(int)]` (the altitude column, api/core.py:1049-1053) of a 2-D uint8 / uint16 / int16 /
    float32 raster for float32 columns: numpy's fancy indexing, negative indices counted from the end, in the raster's type.
    Raster and columns are all numpy arrays or all tensors on the context's device (rows contiguous; a window of a wider buffer is
    fine).  `dtype` names the pixel type of a tensor that only stores its bit pattern (uint16 in int16 storage); the result keeps
    the storage type.  IndexError where numpy raises it, and for a NaN or infinite coordinate."""
    place, cols, n = _f32_columns((x0, y0), "sample_points", "x0 and y0")
    place.require((raster,), "sample_points", "raster and columns")
    img_arg, dt, H, W, stride = _raster_arg(place, raster, "sample_points", dtype)
    if dt not in PREP_DTYPES:
        raise KariosHipError(f"sample_points: unsupported pixel type {dt} (uint8, uint16, int16, float32)")
    if H < 1 or W < 1:
        raise ValueError("sample_points: empty raster")
    if n > PROFILE_MAX_ROWS:
        raise ValueError(f"sample_points: {n} rows (at most 2^20)")
    out = place.empty(n, place.dtype(raster) if place.dev else dt)      # (a tensor's storage type)
    bad = C.c_int32()
    place.call(_ctx(ctx), "km_sample_points", img_arg, _lib._DTYPES[dt], H, W, stride, n, *_col_args(place, cols + (out,), n), C.byref(bad))
    if bad.value:
        raise IndexError(f"sample_points: {bad.value} row(s) out of bounds for a raster of {H} x {W}")
    return out


class BoxStats:
    """Result of `box_stats`: per group `key` (float32, ascending), `count` (int32, NaN values included), `mean` (float32) and the
    float64 columns `q1`, `med`, `q3`, `iqr`, `cilo`, `cihi`, `whislo`, `whishi`; `cls` (int8) per ROW: 0 inside the whiskers, 1
    below, 2 above, -1 for a row without a group.  numpy arrays, or device tensors for device input."""

    def __init__(self, key, count, mean, stats, cls):
        self.key, self.count, self.mean, self.cls = key, count, mean, cls
        for name, col in zip(BOX_STAT_NAMES, stats):
            setattr(self, name, col)


def box_stats(values, positions, bin_size, ctx: Context | None = None) -> BoxStats:
    """matplotlib.cbook.boxplot_stats(x, whis=1.5) of every group of `mean_profile` (np.floor_divide(positions, bin_size), the
    groups ascending), x the group's values in row order: float32 columns of one length (at most 2^20 rows; numpy or device
    tensors), 1 <= bin_size <= 2^24 -> `BoxStats`.  The fliers of a group are its rows of class 1 in row order, then those of
    class 2 (`box_fliers`)."""
    place, cols, n = _f32_columns((values, positions), "box_stats", "values and positions")
    if n > PROFILE_MAX_ROWS:
        raise ValueError(f"box_stats: {n} rows (at most 2^20)")
    if int(bin_size) != bin_size or not 1 <= int(bin_size) <= PROFILE_MAX_BIN:
        raise ValueError(f"box_stats: bin size {bin_size} (an integer, 1 .. 2^24)")
    k = _lib.BOX_STATS
    key, count, mean = (place.empty(n, t) for t in (np.float32, np.int32, np.float32))
    stats, cls = place.empty((k, n), np.float64), place.empty(n, np.int8)
    groups = C.c_int32()
    a = _col_args(place, cols + (key, count, mean, stats, cls), n)
    place.call(_ctx(ctx), "km_box_stats", n, a[0], a[1], int(bin_size), *a[2:], C.byref(groups))
    g = groups.value
    return BoxStats(key[:g], count[:g], mean[:g], [stats[j, :g] for j in range(k)], cls)


# ---- the circular-error figure's numbers (km_ce_figure, k_ce.hip) ---------------------------------------------------------------------
CE_MAX_BINS = _lib.CE_MAX_BINS      # bins of one axis histogram the device counts; beyond it numpy on a host copy
CE_FIELDS = ("hist_x", "bins_x", "hist_y", "bins_y", "mu_x", "sigma_x", "mu_y", "sigma_y", "scatter_x", "scatter_y", "scatter_z", "counts2d",
             "x_edges", "y_edges", "radial", "plot_limit", "ce90", "ce95", "sample")


class CeFigure:
    """Result of `ce_figure`, what `CircularErrorPlot._plot` hands to matplotlib: `hist_x` (int64) on `bins_x` (float32 edges) and
    the same for y; `mu_*`, `sigma_*` of the scaled columns (np.float32); `scatter_x`, `scatter_y`, `scatter_z` in drawing order
    and `radial` ascending (float32, `sample` rows; device tensors for device input); `counts2d` (float64, 10 x 10) on `x_edges`,
    `y_edges`; `plot_limit`, `ce90`, `ce95` (np.float32).  `path` is "device" or "host"; `host_hist_x` / `host_hist_y` tell that
    numpy counted that axis on a host copy (more than CE_MAX_BINS bins); `n_outside` points lie outside the grid of bin centres
    (NaN density, drawn last)."""

    def __init__(self, **kw):
        self.path, self.host_hist_x, self.host_hist_y, self.n_outside = "device", False, False, 0
        self.__dict__.update(kw)


def _ce_histogram_host(vect, img_res):
    """`_compute_histogram`'s numpy expression (circular_error_plot.py:185-207)."""
    v_max = np.max([np.abs(np.max(vect)), np.abs(np.min(vect))])
    return np.histogram(vect * img_res, bins="sqrt", range=(-v_max * img_res, v_max * img_res))


def _ce_host(dx, dy, score, threshold, img_res, carto):
    """The reference's own numpy / scipy expressions (circular_error_plot.py:181-228, 254-303, 359-368) on host arrays of any dtype;
    only the drawing order is this project's: stable."""
    from scipy.interpolate import interpn
    dx, dy, score = np.asarray(dx), np.asarray(dy), np.asarray(score)
    keep = score > threshold
    vx, vy = dx[keep], (-dy if carto else dy)[keep]
    r = CeFigure(path="host", sample=int(vx.size))
    (r.hist_x, r.bins_x), (r.hist_y, r.bins_y) = _ce_histogram_host(vx, img_res), _ce_histogram_host(vy, img_res)
    x, y = vx * img_res, vy * img_res
    with np.errstate(invalid="ignore"):
        r.mu_x, r.sigma_x, r.mu_y, r.sigma_y = np.mean(x), np.std(x), np.mean(y), np.std(y)
        r.plot_limit = np.max([np.max(np.abs(x)), np.max(np.abs(y))])
        r.counts2d, r.x_edges, r.y_edges = np.histogram2d(x, y, bins=10)
        z = interpn((0.5 * (r.x_edges[1:] + r.x_edges[:-1]), 0.5 * (r.y_edges[1:] + r.y_edges[:-1])), r.counts2d, np.vstack([x, y]).T,
                    method="splinef2d", bounds_error=False)
        idx = np.argsort(z, kind="stable")
        r.scatter_x, r.scatter_y, r.scatter_z = x[idx], y[idx], z[idx]
        r.radial = np.sort(np.sqrt(x * x + y * y))
    r.n_outside = int(np.count_nonzero(np.isnan(z)))
    r.ce90, r.ce95 = _accuracy_host(dx, dy, score, threshold, carto, img_res, (0.9, 0.95)).ce
    return r


def ce_axis_edges(lo, hi, v_min, v_max, n, res32):
    """np.histogram(bins="sqrt", range=...)'s edges (numpy/lib/_histograms_impl.py `_get_bin_edges`) from the extremes of the unscaled
    (lo, hi) and the scaled (v_min, v_max) column of n rows -> float32 edges."""
    bound = max(np.float32(abs(hi)), np.float32(abs(lo)))
    last = np.float32(bound * res32)
    first = np.float32(-last)
    if first == last:
        first, last = np.float32(first - np.float32(0.5)), np.float32(last + np.float32(0.5))
    width = np.float32(v_max - v_min) / np.sqrt(n)
    n_bins = int(np.ceil(np.float32(last - first) / width)) if width else 1
    edges = np.linspace(first, last, n_bins + 1, endpoint=True, dtype=np.float32)
    if np.any(edges[:-1] >= edges[1:]):
        raise ValueError(f"Too many bins for data range. Cannot create {n_bins} finite-sized bins.")
    return edges


def ce_grid_edges(lo, hi):
    """np.histogramdd's edges of one axis: 11 float32 edges over [min, max], widened by 0.5 when they are equal."""
    if lo == hi:
        lo, hi = np.float32(lo - np.float32(0.5)), np.float32(hi + np.float32(0.5))
    return np.linspace(lo, hi, 11)


def ce_figure(dx, dy, score, threshold, img_res, carto: bool = False, ctx: Context | None = None) -> CeFigure:
    """Every array and scalar `CircularErrorPlot._plot` (karios/report/circular_error_plot.py) hands to matplotlib, for the columns dx,
    dy, score of a frame, the confidence threshold (compared as `accuracy_statistics` compares it), the resolution `img_res` (a
    Python float: the products are float32) and `carto` -> `CeFigure`.  float32 numpy arrays, or float32 torch tensors on the
    context's device: then no column crosses to the host - 64 bytes of extremes and sizes, the counts of the three histograms and
    32 bytes of final scalars do; numpy builds the bin edges and scipy fits the 10 x 10 spline from those, the GPU counts, evaluates
    the spline per point, sorts and gathers.  The drawing order is the stable one (np.argsort(z, kind="stable")).  ValueError for
    an empty sample, as the reference's np.max raises.  numpy / scipy on the host take the call where the GPU form is not
    defined: columns that are not float32, more than 2^24 rows, an np.float64 `img_res`, a NaN in dx or dy of the sample; and ONE
    axis histogram of more than CE_MAX_BINS bins (`host_hist_x` / `host_hist_y`)."""
    place = Place((dx, dy, score), "ce_figure", "dx, dy and score")
    cols, f32_cols = _float32_columns(place, (dx, dy, score))
    if any(len(a.shape) != 1 for a in cols) or any(int(a.shape[0]) != int(cols[0].shape[0]) for a in cols):
        raise ValueError("ce_figure: dx, dy and score must be 1-D columns of one length")
    n = int(cols[0].shape[0])
    if isinstance(img_res, (bool, str)) or not isinstance(img_res, (float, int, np.floating, np.integer)):
        raise ValueError(f"ce_figure: img_res {img_res!r} is not a number")
    scalar_thr = isinstance(threshold, (float, int, np.floating, np.integer))
    if not f32_cols or n > ACCURACY_MAX_ROWS or isinstance(img_res, np.float64) or not scalar_thr or not np.isfinite(np.float32(img_res)):
        return _ce_host(*(place.to_host(a) for a in cols), threshold, img_res, carto)
    if n == 0:
        raise ValueError("ce_figure: zero-size sample: no row lies above the threshold")
    thr = float(threshold) if isinstance(threshold, np.float64) else float(np.float32(threshold))
    res32 = np.float32(img_res)
    c = _ctx(ctx)
    fn, what = place.function(c, "km_ce_figure")
    job, blk, tail = _lib.CeJob(), _lib.CeBlock(), _lib.CeTail()
    job.n, job.carto, job.thr, job.res = n, int(bool(carto)), thr, float(res32)
    job.dx, job.dy, job.score = (place.address(a) for a in cols)
    job.block, job.tail = C.pointer(blk), C.pointer(tail)

    job.stage = _lib.CE_SAMPLE
    c.check(fn(c.handle, C.byref(job)), what)
    if blk.n_nan:
        return _ce_host(*(place.to_host(a) for a in cols), threshold, img_res, carto)
    sample = int(blk.sample)
    if sample == 0:
        raise ValueError("ce_figure: zero-size sample: no row lies above the threshold")
    ext = np.array(blk.ext, np.float32)
    r = CeFigure(sample=sample, mu_x=np.float32(blk.mu_x), sigma_x=np.float32(blk.sigma_x), mu_y=np.float32(blk.mu_y), sigma_y=np.float32(blk.sigma_y))
    r.plot_limit = np.max(np.abs(ext[4:8]))

    # the edges: numpy's own linspace on the extremes
    r.bins_x = ce_axis_edges(ext[0], ext[1], ext[4], ext[5], sample, res32)
    r.bins_y = ce_axis_edges(ext[2], ext[3], ext[6], ext[7], sample, res32)
    r.x_edges, r.y_edges = ce_grid_edges(ext[4], ext[5]), ce_grid_edges(ext[6], ext[7])
    r.host_hist_x, r.host_hist_y = r.bins_x.size - 1 > CE_MAX_BINS, r.bins_y.size - 1 > CE_MAX_BINS
    grid = np.ascontiguousarray(np.concatenate([r.x_edges, r.y_edges]), np.float32)
    hx = np.zeros(0 if r.host_hist_x else r.bins_x.size - 1, np.uint32)
    hy = np.zeros(0 if r.host_hist_y else r.bins_y.size - 1, np.uint32)
    counts = np.zeros(100, np.uint32)
    job.stage = _lib.CE_COUNTS
    job.edges_x, job.edges_y, job.edges_grid = r.bins_x.ctypes.data, r.bins_y.ctypes.data, grid.ctypes.data
    job.bins_x, job.bins_y = hx.size, hy.size
    job.hist_x, job.hist_y, job.counts_grid = hx.ctypes.data, hy.ctypes.data, counts.ctypes.data
    c.check(fn(c.handle, C.byref(job)), what)
    r.hist_x, r.hist_y = hx.astype(np.int64), hy.astype(np.int64)
    if r.host_hist_x or r.host_hist_y:
        h_dx, h_dy, h_score = (place.to_host(a) for a in cols)
        keep = h_score.astype(np.float64) > thr
        if r.host_hist_x:
            r.hist_x = _ce_histogram_host(h_dx[keep], img_res)[0]
        if r.host_hist_y:
            r.hist_y = _ce_histogram_host((-h_dy if carto else h_dy)[keep], img_res)[0]
    r.counts2d = counts.astype(np.float64).reshape(10, 10)

    # the fit: scipy's own, on 100 numbers
    from scipy.interpolate import RectBivariateSpline
    cx, cy = 0.5 * (r.x_edges[1:] + r.x_edges[:-1]), 0.5 * (r.y_edges[1:] + r.y_edges[:-1])
    tx, ty, coef = (np.ascontiguousarray(a, np.float64) for a in RectBivariateSpline(cx, cy, r.counts2d).tck[:3])
    if (tx.size, ty.size, coef.size) != (14, 14, 100):
        raise KariosHipError(f"ce_figure: a spline of {tx.size} x {ty.size} knots and {coef.size} coefficients (14 x 14, 100)")
    box = np.array([cx[0], cx[-1], cy[0], cy[-1]], np.float32)
    outs = [place.empty(n, np.float32) for _ in range(4)]
    job.stage = _lib.CE_CURVES
    job.tx, job.ty, job.coef, job.box = tx.ctypes.data, ty.ctypes.data, coef.ctypes.data, box.ctypes.data
    job.scatter_x, job.scatter_y, job.scatter_z, job.radial = (place.address(a) for a in outs)
    c.check(fn(c.handle, C.byref(job)), what)
    r.scatter_x, r.scatter_y, r.scatter_z, r.radial = (a[:sample] for a in outs)
    r.n_outside = int(tail.n_outside)
    order = np.array(tail.order, np.float32)
    ce = []
    for k, percent in enumerate((0.9, 0.95)):
        frac = ce_ranks(percent, sample)[2]
        ce.append(order[2 * k] + (order[2 * k + 1] - order[2 * k]) * frac)       # accuracy_statistics.py:237, as `accuracy_statistics` forms it
    r.ce90, r.ce95 = ce
    return r
