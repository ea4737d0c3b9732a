"""The report's numbers restated in numpy: the definition csrc/report_math.hpp, csrc/k_report.hip and the Python layer are held to.

`display_range`: the display range of OverviewPlot._plot_image (karios/report/overview_plot.py:134-194) - the invalid mask of
_build_invalid_mask, the percentiles of the finite, non-zero, not invalid pixels, the nanmin / nanmax fallback.
`mean_profile`: karios/report/commons.py:49-71 - the pandas group-by of a float32 column over np.floor_divide(positions, bin_size)
as explicit recurrences (pandas' group_mean: Kahan in float32; group_var: Welford in float64).

tests/test_report_host.py checks both against numpy's and pandas' own evaluation and the recorded results of the reference.
"""
import numpy as np

f32 = np.float32
f64 = np.float64
MAX_NO_VALUES = 16            # KM_DISPLAY_MAX_NO_VALUES
MAX_PROFILE_ROWS = 1 << 20
MAX_BIN_SIZE = 1 << 24


class DisplayRange:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def _positive_zero(v):
    """numpy's sign of a zero minimum / maximum depends on the order of the elements (-0.0 == 0.0): a zero extreme is +0.0 here."""
    return v + v.dtype.type(0) if v == 0 else v


def invalid_mask(arr, mask=None, no_values=None, nodata=None):
    """_build_invalid_mask without its `.any()` shortcut: always an array."""
    arr = np.asarray(arr)
    invalid = np.zeros(arr.shape, bool)
    if mask is not None:
        invalid |= np.asarray(mask) == 0
    with np.errstate(all="ignore"):
        if no_values is not None and len(no_values):
            invalid |= np.isin(arr, no_values)    # by value: (double)pixel == (double)v
        if nodata is not None:
            invalid |= arr == nodata              # by value too, but see nodata_as_compared
    return invalid


def nodata_as_compared(dtype, nodata):
    """The float64 a pixel is compared with by value.  numpy compares a float32 raster with a Python number in float32 (the scalar is
    'weak'), with an np.float64 in float64."""
    if nodata is None:
        return None
    if np.dtype(dtype) == f32 and type(nodata) in (int, float):
        with np.errstate(over="ignore"):
            return float(f32(nodata))
    return float(nodata)


def display_range(arr, mask=None, no_values=None, nodata=None, percents=(0.5, 99.5)):
    arr = np.asarray(arr)
    invalid = invalid_mask(arr, mask, no_values, nodata)
    valid = arr[np.isfinite(arr) & (arr != 0) & ~invalid]
    with np.errstate(all="ignore"):
        nan_free = arr[~np.isnan(arr)] if arr.dtype.kind == "f" else arr.ravel()
        if nan_free.size:
            raster_min, raster_max = _positive_zero(nan_free.min()), _positive_zero(nan_free.max())
        else:
            raster_min = raster_max = arr.dtype.type(np.nan)
    if valid.size:
        v = [np.percentile(valid, p) for p in percents]
    else:
        v = [raster_min, raster_max] if len(percents) == 2 else [arr.dtype.type(np.nan)] * len(percents)
    return DisplayRange(values=v, v_min=v[0] if v else None, v_max=v[-1] if v else None, n_valid=int(valid.size), n_invalid=int(invalid.sum()),
                        raster_min=raster_min, raster_max=raster_max)


def representable(v, dtype):
    """The DN value as the pixel type holds it, or None where no pixel can equal it (np.isin compares by value)."""
    dtype = np.dtype(dtype)
    v = f64(v)
    if np.isnan(v):
        return None
    if dtype.kind == "f":
        with np.errstate(over="ignore"):
            c = dtype.type(v)
        return c if f64(c) == v else None
    info = np.iinfo(dtype)
    if v != np.floor(v) or v < info.min or v > info.max:
        return None
    return dtype.type(int(v))


# ---- mean profiles ------------------------------------------------------------------------------------------------------------------
def floor_divide_f32(a, b):
    """np.floor_divide of float32 by float32 as numpy's npy_divmodf computes it, one value."""
    a, b = f32(a), f32(b)
    with np.errstate(all="ignore"):
        mod = np.fmod(a, b)
        div = f32(f32(a - mod) / b)
        if mod != 0:                                   # (a NaN is "non-zero" and takes neither branch's correction)
            if (b < 0) != (mod < 0):
                div = f32(div - f32(1))
        if div != 0:
            fl = np.floor(div)
            if f32(div - fl) > f32(0.5):
                fl = f32(fl + f32(1))
            return f32(fl)
        return np.copysign(f32(0), f32(a / b))


def group_position(key, bin_size):
    """int32(float32(float32(key * bin) + float32(bin // 2))) -> (position, in range)."""
    p = f32(f32(f32(key) * f32(bin_size)) + f32(bin_size // 2))
    ok = f32(-2147483648.0) <= p < f32(2147483648.0)
    return (np.int32(p) if ok else np.int32(0)), bool(ok)


class Profile:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def mean_profile(values, positions, bin_size=20):
    values, positions = np.asarray(values), np.asarray(positions)
    assert values.dtype == f32 and positions.dtype == f32 and values.shape == positions.shape and values.ndim == 1
    assert 1 <= bin_size <= MAX_BIN_SIZE and values.size <= MAX_PROFILE_ROWS
    with np.errstate(all="ignore"):
        key = np.floor_divide(positions, f32(bin_size))
    key = key + f32(0)                                 # -0.0 and 0.0 are one group
    rows = np.flatnonzero(~np.isnan(key))
    order = rows[np.argsort(key[rows], kind="stable")]
    keys, pos, cnt, mean, std = [], [], [], [], []
    out_of_range = 0
    at = 0
    with np.errstate(all="ignore"):
        while at < order.size:
            k = key[order[at]]
            end = at
            while end < order.size and key[order[end]] == k:
                end += 1
            s = c = f32(0)
            n, m, m2 = 0, f64(0), f64(0)
            for i in order[at:end]:
                x = values[i]
                if np.isnan(x):
                    continue
                y = f32(x - c)
                t = f32(s + y)
                c = f32(f32(t - s) - y)
                if np.isnan(c):
                    c = f32(0)
                s = t
                n += 1
                old = m
                m = m + (f64(x) - old) / f64(n)
                m2 = m2 + (f64(x) - m) * (f64(x) - old)
            p, ok = group_position(k, bin_size)
            out_of_range += not ok
            keys.append(k), pos.append(p), cnt.append(n)
            mean.append(f32(s / f32(n)) if n else f32(np.nan))
            std.append(f32(np.sqrt(m2 / f64(n - 1))) if n >= 2 else f32(np.nan))
            at = end
    return Profile(key=np.array(keys, f32), position=np.array(pos, np.int32), count=np.array(cnt, np.int64), mean=np.array(mean, f32),
                   std=np.array(std, f32), out_of_range=out_of_range)
