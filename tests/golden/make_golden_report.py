#!/usr/bin/env python3
"""Golden vectors for the report's numbers, produced by the REFERENCE's own `OverviewPlot._build_invalid_mask` / `_plot_image`
(karios/report/overview_plot.py) and `mean_profile` (karios/report/commons.py), imported from the reference tree (build container
only).

Run here, never on the GPU box:   python tests/golden/make_golden_report.py      -> tests/golden/report_numbers.npz
Only DATA is written: checksums of the inputs (rebuilt by `range_cases` / `profile_cases` below, integer arithmetic only), the
`vmin` / `vmax` the reference hands to imshow, the number of pixels its invalid mask marks, and the four series of every profile.
No reference source is copied.

`_plot_image` runs as it is on stand-ins: an object with `array` / `no_data_value` / `filepath` for GdalRasterImage, an axes object
that records `imshow`'s arguments; `osgeo` is a mock.

`range_cases`, `profile_cases` and `crc` are imported by the tests; nothing at module level touches the reference.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_accuracy import _hash, _unit  # noqa: E402
from make_golden_chips import crc  # noqa: E402,F401

f32 = np.float32
DTYPES = ("uint8", "uint16", "int16", "float32")
H, W = 37, 53


def _raster(dtype, seed, h=H, w=W):
    n = h * w
    k = _hash(n, 11 * seed + 1)
    if dtype == "uint8":
        a = (k % np.uint64(256)).astype(np.uint8)
    elif dtype == "uint16":
        a = (k % np.uint64(12000)).astype(np.uint16)
        a[k % np.uint64(17) == 0] = 0
    elif dtype == "int16":
        a = ((k % np.uint64(9000)).astype(np.int64) - 3000).astype(np.int16)
        a[k % np.uint64(19) == 0] = 0
    else:
        a = (_unit(n, 11 * seed + 2) * 7 - 2).astype(f32)
        a[k % np.uint64(23) == 0] = 0
        a[k % np.uint64(29) == 1] = f32(-0.0)
        a[k % np.uint64(31) == 2] = np.nan
        a[k % np.uint64(37) == 3] = np.inf
        a[k % np.uint64(41) == 4] = -np.inf
    return a.reshape(h, w)


def _mask(seed, h=H, w=W):
    return (_hash(h * w, 13 * seed + 5) % np.uint64(4) != 0).astype(np.uint8).reshape(h, w) * np.uint8(255)


def range_cases():
    """-> list of (name, raster, mask or None, no_values or None, nodata or None)."""
    out = []
    for k, dt in enumerate(DTYPES):
        a = _raster(dt, k)
        present = a[3, 5].item()
        out.append((f"plain_{dt}", a, None, None, None))
        out.append((f"mask_{dt}", a, _mask(k), None, None))
        out.append((f"list_{dt}", a, None, [present, 0, -1, 70000, 0.5, float("nan")], None))
        out.append((f"nodata_{dt}", a, None, None, a[7, 11].item()))
        out.append((f"all_{dt}", a, _mask(k + 9), [present, a[20, 20].item(), 300], a[7, 11].item()))
        out.append((f"fallback_{dt}", a, np.zeros((H, W), np.uint8), None, None))
    u16 = _raster("uint16", 7)
    out.append(("nodata0_uint16", u16, None, None, 0.0))
    out.append(("list16_uint16", u16, None, [int(v) for v in np.unique(u16)[1:17]], None))
    fl = _raster("float32", 8)
    out.append(("nodata_nan_float32", fl, None, None, float("nan")))
    out.append(("nodata_weak_float32", fl, None, None, float(fl[4, 4])))      # a Python float: numpy compares it in float32
    out.append(("list0_float32", fl, None, [0], None))                        # matches -0.0 too
    for n_valid in (1, 2):
        a = np.zeros((5, 9), np.int16)
        a.ravel()[[7, 30][:n_valid]] = [-5, 12][:n_valid]
        out.append((f"valid{n_valid}_int16", a, None, None, None))
        b = np.full((5, 9), np.nan, f32)
        b.ravel()[[7, 30][:n_valid]] = [f32(-5.5), f32(12.25)][:n_valid]
        out.append((f"valid{n_valid}_float32", b, None, None, None))
    out.append(("all_nan_float32", np.full((4, 6), np.nan, f32), None, None, None))
    out.append(("one_pixel_uint8", np.array([[9]], np.uint8), None, None, None))
    return out


def profile_cases():
    """-> list of (name, values, positions, bin_size): float32 columns."""
    out = []
    n = 20000
    x = (np.floor(_unit(n, 201) * 10980)).astype(f32)
    out.append(("frame_20000", (_unit(n, 202) - 0.5).astype(f32), x, 20))
    n = 600
    v = ((_unit(n, 203) - 0.5) * 1000).astype(f32)
    p = ((_unit(n, 204) - 0.4) * 300).astype(f32)
    k = _hash(n, 205)
    v[k % np.uint64(7) == 0] = np.nan
    v[k % np.uint64(53) == 1] = np.inf
    p[k % np.uint64(11) == 2] = np.nan
    p[k % np.uint64(13) == 3] = np.inf
    p[k % np.uint64(17) == 4] = f32(-0.0)
    p[k % np.uint64(19) == 5] = f32(0.0)
    p[k % np.uint64(23) == 6] = f32(-0.25)
    for b in (1, 7, 20, 100):
        out.append((f"odd_bin{b}", v, p, b))
    out.append(("single_rows", np.arange(40, dtype=f32) * f32(0.1), np.arange(40, dtype=f32) * f32(20), 20))
    out.append(("one_group", (_unit(300, 206) * 3).astype(f32), (_unit(300, 207) * 19).astype(f32), 20))
    out.append(("all_nan_values", np.full(12, np.nan, f32), np.arange(12, dtype=f32), 5))
    out.append(("empty", np.zeros(0, f32), np.zeros(0, f32), 20))
    return out


def main():
    import matplotlib
    matplotlib.use("Agg")
    from make_golden import import_reference
    import_reference()
    import warnings
    import pandas as pd
    import karios.report.overview_plot as rop
    import karios.report.commons as rco

    class Img:
        def __init__(self, a, nodata):
            self.array, self.no_data_value, self.filepath, self.file_name = a, nodata, "stand-in", "stand-in"

    class Axes:
        def set_title(self, _t):
            pass

        def imshow(self, _a, cmap=None, vmin=None, vmax=None):
            self.v = (vmin, vmax)

    out = {}
    for name, a, mask, no_values, nodata in range_cases():
        plot = rop.OverviewPlot.__new__(rop.OverviewPlot)
        plot._mask = None if mask is None else Img(mask, None)
        plot._no_values = no_values
        img, axes = Img(a, nodata), Axes()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            invalid = plot._build_invalid_mask(img, apply_user_mask=True)
            plot._plot_image(axes, img, "t", invalid=invalid)
        out[f"crc_{name}"] = np.array([crc(a, *([] if mask is None else [mask]))], np.uint32)
        out[f"vmin_{name}"], out[f"vmax_{name}"] = np.asarray(axes.v[0]), np.asarray(axes.v[1])
        out[f"invalid_{name}"] = np.array([0 if invalid is None else int(invalid.sum())], np.int64)
    for name, v, p, b in profile_cases():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = rco.mean_profile(pd.Series(v), pd.Series(p), b)
        out[f"crc_{name}"] = np.array([crc(v, p)], np.uint32)
        out[f"key_{name}"] = m.mean_values.index.to_numpy()
        out[f"pos_{name}"] = m.groups_positions.to_numpy()
        out[f"count_{name}"] = m.nb_pos.to_numpy()
        out[f"mean_{name}"] = m.mean_values.to_numpy()
        out[f"std_{name}"] = m.values_std.to_numpy()
        assert (m.groups_positions.dtype, m.nb_pos.dtype, m.mean_values.dtype, m.values_std.dtype) == (np.int32, np.int64, f32, f32), name
    path =os.path.join(HERE, "report_numbers.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
