#!/usr/bin/env python3
"""Golden vectors for the circular-error figure's numbers, produced by the REFERENCE's own `CircularErrorPlot._compute_histogram`,
`_ce_scatter`, `_hist_vector` and `_radial_error_plot` (karios/report/circular_error_plot.py) on the reference's own `GeometricStat`,
imported from the reference tree (build container only).

Run here, never on the GPU box:   python tests/golden/make_golden_ce_figure.py      -> tests/golden/ce_figure.npz
Only DATA is written: checksums of the inputs (rebuilt by `cases` below, integer arithmetic only) and what the four methods hand to
`axes.hist`, `axes.scatter` and `axes.plot`, plus the text of `get_string_block`.  No reference source is copied.

The methods run as they are on stand-ins: an axes object that records the arguments of `hist`, `scatter` and `plot`, a configuration
with a colour-map name; `osgeo` is a mock and `normaltest` (out of scope: it only feeds a log line, and refuses fewer than 8 bins)
is a stand-in as well.

`cases` and `crc` are imported by the tests; nothing at module level touches the reference.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_accuracy import _hash, _unit  # noqa: E402
from make_golden_chips import crc  # noqa: E402,F401

f32 = np.float32
THRESHOLD = 0.4
VALID_PIXELS = 123456          # the `nb_pixels` of compute_stats: only the text block shows it


def _bell(n, seed):
    """Roughly normal in (-1, 1): four uniform draws."""
    return (_unit(n, seed) + _unit(n, seed + 1) + _unit(n, seed + 2) + _unit(n, seed + 3)) / 2.0 - 1.0


def _score(n, seed, every=4):
    """Scores on a grid of 1 / 64; one row in `every` lies below the threshold."""
    k = _hash(n, seed)
    s = ((k % np.uint64(38)) + np.uint64(27)).astype(f32) / f32(64)
    s[k % np.uint64(every) == 0] = f32(0.25)
    return s


def cases():
    """-> list of (name, dx, dy, score, img_res, carto): float32 columns, a Python-float resolution."""
    out = []
    n = 3000
    out.append(("frame_3000", (_bell(n, 11) * 1.5 + 0.2).astype(f32), (_bell(n, 21) * 0.8 - 0.1).astype(f32), _score(n, 31), 10.0, False))
    n = 1500
    out.append(("carto_1500", (_bell(n, 12) * 0.6).astype(f32), (_bell(n, 22) * 2.5 + 0.7).astype(f32), _score(n, 32), 30.0, True))
    n = 900
    q = lambda a: (np.round(a * 8) / 8).astype(f32)                                                   # noqa: E731  points exactly on edges
    out.append(("quantised_900", q(_bell(n, 13) * 2), q(_bell(n, 23) * 3), _score(n, 33), 1.0, False))
    n = 500
    out.append(("far_500", (20 + _bell(n, 14) * 0.05).astype(f32), (-7 + _bell(n, 24) * 0.02).astype(f32), _score(n, 34), 0.1, False))
    n = 40
    out.append(("equal_40", np.full(n, 0.25, f32), np.full(n, -0.5, f32), _score(n, 35), 10.0, False))
    out.append(("zeros_12", np.zeros(12, f32), np.zeros(12, f32), _score(12, 36), 30.0, True))
    for n in (1, 2, 3, 65):
        s = _score(n + 2, 37 + n)
        s[:n] = f32(0.75)
        s[n:] = f32(0.25)
        out.append((f"sample_{n}", (_bell(n + 2, 15 + n) * 1.1).astype(f32), (_bell(n + 2, 25 + n) * 0.9).astype(f32), s, 0.1, n == 3))
    return out


class _Axes:
    """Records what the figure's methods hand to matplotlib."""

    def __init__(self):
        self.hists, self.scatters, self.plots = [], [], []

    def hist(self, x, bins, weights=None, **_kw):
        self.hists.append((np.asarray(x), np.asarray(bins), np.asarray(weights)))

    def scatter(self, x, y, c=None, **_kw):
        self.scatters.append((np.asarray(x), np.asarray(y), np.asarray(c)))
        return object()

    def plot(self, x, y, *_a, **_kw):
        self.plots.append((np.asarray(x), np.asarray(y)))

    def __getattr__(self, _name):
        return lambda *a, **k: None


def main():
    import types
    import warnings
    import matplotlib
    matplotlib.use("Agg")
    from make_golden import import_reference
    import_reference()
    import pandas as pd
    import karios.report.circular_error_plot as rcp
    from karios.accuracy_analysis.accuracy_statistics import GeometricStat

    rcp.sp_stats = types.SimpleNamespace(normaltest=lambda _h: (0.0, 1.0))
    out = {}
    for name, dx, dy, score, res, carto in cases():
        stats = GeometricStat(types.SimpleNamespace(confidence_threshold=THRESHOLD), pd.DataFrame({"dx": dx, "dy": dy, "score": score}), carto=carto)
        stats.compute_stats(VALID_PIXELS)
        plot = rcp.CircularErrorPlot.__new__(rcp.CircularErrorPlot)
        plot._stats, plot._img_res, plot._short_unit = stats, res, "m"
        plot._conf = types.SimpleNamespace(ce_scatter_colormap="viridis")
        plot._x_scatter_label = plot._y_scatter_label = "stand-in"
        out[f"crc_{name}"] = np.array([crc(dx, dy, score)], np.uint32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a = _Axes()
            plot._ce_scatter(a)
            (out[f"scatter_x_{name}"], out[f"scatter_y_{name}"], out[f"scatter_z_{name}"]), = a.scatters
            for axis, vect in (("x", stats.v_x_th), ("y", stats.v_y_th)):
                a = _Axes()
                plot._hist_vector(a, vect, axis)
                (first, bins, weights), (curve_x, curve_y) = a.hists[0], a.plots[0]
                assert np.array_equal(first, bins[:-1]) and np.array_equal(curve_x, bins)
                out[f"bins_{axis}_{name}"], out[f"hist_{axis}_{name}"], out[f"curve_{axis}_{name}"] = bins, weights, curve_y
                out[f"text_{axis}_{name}"] = np.array(stats.get_string_block(res, direction=axis))
            a = _Axes()
            plot._radial_error_plot(a)
            (_pct, out[f"radial_{name}"]), (_p90, ce90), (_p95, ce95) = a.plots
            out[f"ce_{name}"] = np.array([ce90, ce95])
    path = os.path.join(HERE, "ce_figure.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
