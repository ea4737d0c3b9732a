#!/usr/bin/env python3
"""Golden vectors for the report's products and the altitude figure's box statistics, produced by the REFERENCE's own
`ProductGenerator._create_mask` / `_create_intermediate_raster` (karios/report/product_generator.py) and
`MeanShiftByAltitudeGroupPlot._plot_alt` (karios/report/shift_by_alt_plot.py), imported from the reference tree (build container
only).

Run here, never on the GPU box:   python tests/golden/make_golden_products.py      -> tests/golden/products.npz
Only DATA is written: checksums of the inputs (rebuilt by `raster_cases` / `altitude_cases` below, integer arithmetic only), the
rasters the reference's methods write, and per altitude group what matplotlib.cbook.boxplot_stats makes of the arrays the
reference hands to `boxplot`.  No reference source is copied.

The two `_create_*` methods run as they are on a stand-in `gdal` whose bands collect `Fill` / `WriteArray` into numpy arrays;
`_plot_alt` runs on a recording axes object that keeps `boxplot`'s `arr` and `positions`.

`raster_cases`, `altitude_cases` and `crc` are imported by the tests; nothing at module level touches the reference.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_accuracy import _hash, _unit  # noqa: E402
from make_golden_chips import crc  # noqa: E402,F401

f32 = np.float32
H, W = 37, 53
STATS = ("mean", "med", "q1", "q3", "iqr", "cilo", "cihi", "whislo", "whishi")


def _points(n, seed, h, w):
    """x0, y0 inside the raster with fractions, dx, dy (float32)."""
    x = (_unit(n, 7 * seed + 1) * w).astype(f32)
    y = (_unit(n, 7 * seed + 2) * h).astype(f32)
    x = np.minimum(x, f32(w) - f32(0.25))          # (float32 rounding of u * w may reach w)
    y = np.minimum(y, f32(h) - f32(0.25))
    dx = ((_unit(n, 7 * seed + 3) - 0.5) * 4).astype(f32)
    dy = ((_unit(n, 7 * seed + 4) - 0.5) * 4).astype(f32)
    return x, y, dx, dy


def raster_cases():
    """-> list of (name, x0, y0, dx, dy, H, W): every row inside the ranges the reference accepts."""
    out = []
    x, y, dx, dy = _points(300, 1, H, W)
    x[10:13], y[10:13] = f32(7.5), f32(3.25)                      # three rows on one pixel, different dx
    x[40], y[40] = x[200], y[200]                                 # ... and two far apart in the input
    x[50], x[51], y[50], y[51] = f32(-1), f32(W - 1), f32(5), f32(5)     # the same pixel through the wrap
    x[60], y[60] = f32(-0.9), f32(-0.9)                           # truncation toward zero: pixel (0, 0)
    x[61], y[61] = f32(-W), f32(H - 1)
    dx[70], dy[70] = f32(np.nan), f32(-0.0)
    dx[71], dy[71] = f32(np.inf), f32(-np.inf)
    out.append(("frame_300", x, y, dx, dy, H, W))
    out.append(("small_5x9", *_points(20, 2, 5, 9), 5, 9))
    out.append(("one_row", *_points(1, 3, H, W), H, W))
    out.append(("empty", *_points(0, 4, H, W), H, W))
    out.append(("dense_2000", *_points(2000, 5, H, W), H, W))    # more rows than pixels
    return out


def altitude_cases():
    """-> list of (name, values, alt, x_res, bin_size): float32 values, altitudes in a DEM's type."""
    out = []
    n = 600
    v = ((_unit(n, 301) - 0.5) * 3).astype(f32)
    k = _hash(n, 302)
    v[k % np.uint64(41) == 0] *= f32(9)                            # fliers on both sides
    out.append(("int16_dem", v, ((_unit(n, 303) * 900) - 100).astype(np.int16), 10, 20))
    out.append(("uint16_dem", v, (_unit(n, 304) * 3000).astype(np.uint16), 10, 100))
    out.append(("uint8_dem", v, (_unit(n, 305) * 256).astype(np.uint8), 1, 3))
    a = ((_unit(n, 306) * 700) - 50).astype(f32)
    a[k % np.uint64(53) == 1] = np.nan
    a[k % np.uint64(59) == 2] = f32(-0.0)
    out.append(("float32_dem", v, a, 10, 20))
    w = v.copy()
    w[k % np.uint64(97) == 3] = np.nan                             # groups with a NaN value
    out.append(("nan_values", w, (_unit(n, 307) * 200).astype(np.int16), 10, 20))
    sizes = (1, 2, 3, 4, 5, 127, 128, 129)
    alt = np.concatenate([np.full(s, 20 * i + 7, np.int16) for i, s in enumerate(sizes)])
    out.append(("group_sizes", ((_unit(alt.size, 308) - 0.5) * 2).astype(f32), alt, 10, 20))
    out.append(("equal_values", np.full(40, f32(1.5)), (np.arange(40) // 10 * 20).astype(np.int16), 10, 20))
    out.append(("wrap_int16", v[:30], np.where(np.arange(30) % 2 == 0, 32767, -32768).astype(np.int16), 10, 20))
    return out


class _Band:
    def __init__(self, h, w, dtype):
        self.a = np.zeros((h, w), dtype)

    def SetNoDataValue(self, _v):
        pass

    def Fill(self, v):
        self.a.fill(v)

    def WriteArray(self, buf, xoff, yoff):
        assert yoff >= 0 and xoff == 0
        self.a[yoff:yoff + buf.shape[0], xoff:xoff + buf.shape[1]] = buf


class _Dataset:
    def __init__(self, h, w, bands, dtype):
        self.bands = [_Band(h, w, dtype) for _ in range(bands)]

    def GetRasterBand(self, i):
        return self.bands[i - 1]

    def SetProjection(self, _p):
        pass

    def SetGeoTransform(self, _t):
        pass

    def FlushCache(self):
        pass


class _Gdal:
    GDT_Byte, GDT_Float32 = "uint8", "float32"

    def __init__(self):
        self.made = []

    def GetDriverByName(self, _name):
        return self

    def Create(self, _path, xsize, ysize, bands, eType, options=None):
        self.made.append(_Dataset(ysize, xsize, bands, np.dtype(eType)))
        return self.made[-1]


def main():
    import types
    import warnings
    from unittest import mock

    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.cbook as cbook
    import pandas as pd
    from make_golden import import_reference
    import_reference()
    import karios.report.product_generator as rpg
    import karios.report.shift_by_alt_plot as rsa

    out = {}
    for name, x, y, dx, dy, h, w in raster_cases():
        gdal = _Gdal()
        rpg.gdal = gdal
        gen = rpg.ProductGenerator.__new__(rpg.ProductGenerator)
        gen._config = types.SimpleNamespace(output_directory="stand-in")
        gen._points = pd.DataFrame({"x0": x, "y0": y, "dx": dx, "dy": dy})
        gen._reference_image = types.SimpleNamespace(x_size=w, y_size=h, projection=None, x_min=0.0, x_res=1.0, y_max=0.0, y_res=-1.0)
        gen._create_mask()
        gen._create_intermediate_raster()
        mask, delta = gdal.made
        out[f"crc_{name}"] = np.array([crc(x, y, dx, dy)], np.uint32)
        out[f"mask_{name}"] = mask.bands[0].a
        out[f"delta_{name}"] = np.stack([b.a for b in delta.bands]).view(np.uint32)       # (by bits: the fill's NaN, dx's NaN)
    for name, v, alt, x_res, b in altitude_cases():
        plot = rsa.MeanShiftByAltitudeGroupPlot.__new__(rsa.MeanShiftByAltitudeGroupPlot)
        plot._direction, plot._x_img_res, plot._mini, plot._maxi = "dx", x_res, -1, 1
        plot._points = pd.DataFrame({"dx": v, "alt": alt})
        plot._config = types.SimpleNamespace(histo_mean_bin_size=b, show_fliers=True)
        axis = mock.MagicMock()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plot._plot_alt(axis)
            (arr,), kw = axis.twinx.return_value.boxplot.call_args
            stats = cbook.boxplot_stats(arr, whis=1.5, bootstrap=None, autorange=False)
        assert all(a.dtype == f32 for a in arr), name
        out[f"crc_{name}"] = np.array([crc(v, alt)], np.uint32)
        pos = kw["positions"]
        out[f"pos_{name}"] = pos.to_numpy()
        out[f"key_{name}"] = pos.index.to_numpy()
        out[f"count_{name}"] = np.array([len(a) for a in arr], np.int32)
        for k in STATS:
            col = [s[k] for s in stats]
            assert all(type(c) is (f32 if k == "mean" else np.float64) or (k in ("whislo", "whishi") and type(c) is f32) for c in col), (name, k)
            out[f"{k}_{name}"] = np.array(col, f32 if k == "mean" else np.float64)
        fl = [s["fliers"] for s in stats]
        out[f"fliers_{name}"] = np.concatenate(fl).astype(f32) if fl else np.zeros(0, f32)
        out[f"nfliers_{name}"] = np.array([len(a) for a in fl], np.int32)
    path = os.path.join(HERE, "products.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
