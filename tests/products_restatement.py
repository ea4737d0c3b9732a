"""The report's products and the altitude figure's numbers restated in numpy: the definition csrc/products_math.hpp,
csrc/k_products.hip and the Python layer are held to.

`point_rasters`: ProductGenerator._create_mask / _create_intermediate_raster (karios/report/product_generator.py:138-218) minus the
file - the uint8 raster with 1 at every key point, the two float32 bands of NaN with dx / dy at the key points.
`sample_points`: the altitude column, `dem.array[y_index, x_index]` (karios/api/core.py:1049-1053).
`box_stats`: what `boxplot` computes of the altitude groups (karios/report/shift_by_alt_plot.py:127-171):
matplotlib.cbook.boxplot_stats(x, whis=1.5) of every group of `mean_profile`, as explicit arithmetic.
`integer_labels`: the group keys and positions pandas gives an integer DEM, in the DEM's own type.

tests/test_products_host.py checks all of it against numpy, pandas, matplotlib and the recorded results of the reference.
"""
import numpy as np

from accuracy_restatement import mean_f32
from report_restatement import MAX_BIN_SIZE, MAX_PROFILE_ROWS

f32 = np.float32
f64 = np.float64
NAN_FILL_BITS = 0x7FC00000     # float(np.float32(np.nan)) stored into a float32 row
MAX_ROWS = MAX_PROFILE_ROWS
STAT_NAMES = ("q1", "med", "q3", "iqr", "cilo", "cihi", "whislo", "whishi")
ZERO_FOLDED = ("q1", "med", "q3", "whislo", "whishi")   # a zero is +0.0 here; numpy's sign depends on where partition left the zeros


def truncated_index(v):
    """float32 -> (astype(int) where that is defined, defined): truncation toward zero; NaN, infinities and what int64 cannot hold
    are not defined (numpy gives them an arbitrary value with a warning) and count as out of range."""
    v = np.asarray(v, f32)
    ok = np.isfinite(v) & (np.abs(v) < f32(2.0 ** 63))
    out = np.zeros(v.shape, np.int64)
    out[ok] = v[ok].astype(np.int64)
    return out, ok


def point_rasters(x0, y0, dx, dy, H, W):
    """-> (mask uint8 H x W, delta float32 2 x H x W or None, rows out of range).  Columns wrap as numpy's fancy assignment into
    a row buffer does (x in [-W, W)); rows are GDAL's (y in [0, H)); several rows on one pixel: the last in input order."""
    x, okx = truncated_index(x0)
    y, oky = truncated_index(y0)
    ok = okx & oky & (x >= -W) & (x < W) & (y >= 0) & (y < H)
    xw = np.where(x < 0, x + W, x)
    mask = np.zeros((H, W), np.uint8)
    delta = None
    if dx is not None:
        delta = np.full((2, H, W), NAN_FILL_BITS, np.uint32)
        bx, by = np.asarray(dx, f32).view(np.uint32), np.asarray(dy, f32).view(np.uint32)
    for i in np.flatnonzero(ok):
        mask[y[i], xw[i]] = 1
        if delta is not None:
            delta[0, y[i], xw[i]] = bx[i]
            delta[1, y[i], xw[i]] = by[i]
    return mask, None if delta is None else delta.view(f32), int((~ok).sum())


def sample_points(raster, x0, y0):
    """-> (raster[y_index, x_index] with numpy's wrap of both indices, rows out of range); an out-of-range row reads as 0."""
    raster = np.asarray(raster)
    H, W = raster.shape
    x, okx = truncated_index(x0)
    y, oky = truncated_index(y0)
    ok = okx & oky & (x >= -W) & (x < W) & (y >= -H) & (y < H)
    out = np.zeros(x.shape, raster.dtype)
    for i in np.flatnonzero(ok):
        out[i] = raster[y[i] + (H if y[i] < 0 else 0), x[i] + (W if x[i] < 0 else 0)]
    return out, int((~ok).sum())


# ---- box statistics ---------------------------------------------------------------------------------------------------------------
def _plus_zero(v):
    return v + v.dtype.type(0) if v == 0 else v


def percentiles_f64(s, quantiles=(0.25, 0.5, 0.75)):
    """np.percentile(x, [25, 50, 75]) of a float32 array, given `s` = x sorted ascending without a NaN: numpy 2.2's _quantile with
    the linear method and a float64 array of quantiles.  The virtual index (n - 1) * q, its floor and gamma are float64; at or
    above n - 1 both neighbours are the last element and gamma is index + 1.  _lerp: the neighbours' difference is formed in
    FLOAT32, everything after it in float64 - a + diff * gamma below one half, b - diff * (1 - gamma) from there."""
    n = s.size
    out = []
    with np.errstate(all="ignore"):
        for q in quantiles:
            vi = f64(n - 1) * f64(q)
            if vi >= n - 1:
                lo = hi = n - 1
                gamma = vi - f64(-1)
            else:
                lo = int(np.floor(vi))
                hi = lo + 1
                gamma = vi - f64(lo)
            a, b = _plus_zero(s[lo]), _plus_zero(s[hi])
            diff = f64(f32(b - a))
            out.append(f64(b) - diff * (f64(1) - gamma) if gamma >= 0.5 else f64(a) + diff * gamma)
    return out


def group_stats(x):
    """matplotlib.cbook.boxplot_stats(x, whis=1.5, bootstrap=None, autorange=False) of one float32 array with at least one element
    -> (dict of n, mean (float32) and STAT_NAMES (float64), classes int8 per element: 0 inside, 1 below whislo, 2 above whishi)."""
    x = np.asarray(x, f32)
    n = x.size
    st = {"n": n, "mean": mean_f32(x)}
    cls = np.zeros(n, np.int8)
    nan = f64(np.nan)
    if np.isnan(x).any():                      # the percentiles are NaN, every comparison with them is false: no fliers
        st.update({k: nan for k in STAT_NAMES})
        return st, cls
    s = np.sort(x)
    xd = x.astype(f64)
    with np.errstate(all="ignore"):
        q1, med, q3 = percentiles_f64(s)
        iqr = q3 - q1
        half = f64(1.57) * iqr / np.sqrt(f64(n))
        cilo, cihi = med - half, med + half
        loval, hival = q1 - f64(1.5) * iqr, q3 + f64(1.5) * iqr
        below = xd[xd <= hival]
        whishi = q3 if below.size == 0 or below.max() < q3 else _plus_zero(below.max())
        above = xd[xd >= loval]
        whislo = q1 if above.size == 0 or above.min() > q1 else _plus_zero(above.min())
        cls[xd < whislo] = 1
        cls[xd > whishi] = 2
    st.update(q1=q1, med=med, q3=q3, iqr=iqr, cilo=cilo, cihi=cihi, whislo=whislo, whishi=whishi)
    return st, cls


class BoxStats:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def box_stats(values, positions, bin_size):
    """The groups of `mean_profile` (np.floor_divide(positions, float32(bin)), NaN keys dropped, -0.0 and 0.0 one group), ascending;
    per group `group_stats` of its values in row order, NaN values included.  `cls` per row, -1 for a dropped row."""
    values, positions = np.asarray(values), np.asarray(positions)
    assert values.dtype == f32 and positions.dtype == f32 and values.shape == positions.shape and values.ndim == 1
    assert 1 <= bin_size <= MAX_BIN_SIZE and values.size <= MAX_ROWS
    with np.errstate(all="ignore"):
        key = np.floor_divide(positions, f32(bin_size))
    key = key + f32(0)
    rows = np.flatnonzero(~np.isnan(key))
    order = rows[np.argsort(key[rows], kind="stable")]
    cls = np.full(values.size, -1, np.int8)
    keys, count, mean = [], [], []
    cols = {k: [] for k in STAT_NAMES}
    at = 0
    while at < order.size:
        k = key[order[at]]
        end = at
        while end < order.size and key[order[end]] == k:
            end += 1
        idx = order[at:end]
        st, c = group_stats(values[idx])
        cls[idx] = c
        keys.append(k), count.append(st["n"]), mean.append(st["mean"])
        for name in STAT_NAMES:
            cols[name].append(st[name])
        at = end
    return BoxStats(key=np.array(keys, f32), count=np.array(count, np.int32), mean=np.array(mean, f32), cls=cls,
                    **{k: np.array(v, f64) for k, v in cols.items()})


def fliers(x, cls):
    """matplotlib's order: the low ones in row order, then the high ones in row order."""
    x, cls = np.asarray(x), np.asarray(cls)
    return np.concatenate([x[cls == 1], x[cls == 2]])


def groups_of(values, positions, bin_size):
    """-> list of row-index arrays, one per group of `box_stats`, in its order (for the tests' per-group comparisons)."""
    with np.errstate(all="ignore"):
        key = np.floor_divide(np.asarray(positions, f32), f32(bin_size)) + f32(0)
    rows = np.flatnonzero(~np.isnan(key))
    order = rows[np.argsort(key[rows], kind="stable")]
    cut = np.flatnonzero(np.diff(key[order]) != 0) + 1
    return [g for g in np.split(order, cut) if g.size]


# ---- altitude labels ----------------------------------------------------------------------------------------------------------------
def integer_labels(float_keys, dtype, bin_size):
    """Group keys and `groups_positions` of an integer DEM (uint8, uint16, int16), from the float32 keys the device grouped on:
    key = np.floor_divide(alt, bin) in the DEM's type - float32(alt) // float32(bin) is that integer exactly - and the position
    (key * bin + bin // 2).astype(int32) computed in that type, wrap included.  A bin size the type cannot hold: OverflowError,
    as numpy raises it."""
    dtype = np.dtype(dtype)
    assert dtype.kind in "ui"
    key = np.asarray(float_keys, f32).astype(np.int64).astype(dtype)
    with np.errstate(over="ignore"):
        pos = key * bin_size + bin_size // 2          # numpy 2: a Python integer out of the type's range raises OverflowError
    return key, pos.astype(np.int32)
