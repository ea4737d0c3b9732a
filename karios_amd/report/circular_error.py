"""Mirror of the numbers of `karios.report.circular_error_plot.CircularErrorPlot._plot` (report/circular_error_plot.py:112-175): what
its `_hist_vector`, `_ce_scatter`, `_radial_error_plot` and `_text_box` hand to `axes.hist`, `axes.scatter`, `axes.plot` and
`axes.text`, computed by `ops.ce_figure` where the frame's columns live.  With a frame of device tensors no column crosses to the
host; the scatter's and the radial curve's arrays are device tensors until matplotlib asks for them (`host()`).  The figure itself,
its layout and `scipy.stats.normaltest` stay with the integrator."""
from __future__ import annotations

import numpy as np

from .. import ops


def host(a):
    """A device tensor as the numpy array matplotlib takes; numpy arrays pass."""
    return a.detach().cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def rmse(mean, std, img_res=None):
    """`_rmse` (circular_error_plot.py:38-46)."""
    if img_res is not None:
        mean, std = mean * img_res, std * img_res
    return np.sqrt(mean * mean + std * std)


class CircularErrorNumbers:
    """The numbers of the circular-error figure of `stats` (a `karios_amd.accuracy_analysis.GeometricStat`) at the resolution
    `img_res` (None: pixels, factor 1.0), computed once, on first use."""

    def __init__(self, stats, img_res, ctx=None):
        self._stats = stats
        self.pixel_units = img_res is None
        self.img_res = 1.0 if img_res is None else img_res
        self.short_unit = "px" if self.pixel_units else "m"
        self._ctx = ctx
        self._fig = None

    @property
    def figure(self) -> ops.CeFigure:
        if self._fig is None:
            dx, dy, score, threshold, carto = self._stats.columns
            self._fig = ops.ce_figure(dx, dy, score, threshold, self.img_res, carto=carto, ctx=self._ctx or getattr(self._stats, "_ctx", None))
        return self._fig

    def compute_histogram(self, direction):
        """`_compute_histogram` -> (hist, bins): `axes.hist(bins[:-1], bins, weights=hist, ...)`."""
        f = self.figure
        return (f.hist_x, f.bins_x) if direction == "x" else (f.hist_y, f.bins_y)

    def gaussian(self, direction):
        """The overlay of `_hist_vector` -> (bins, curve, mu, sigma): `axes.plot(bins, curve)` (swapped for the horizontal
        histogram), the label from mu and sigma.  n_bins + 1 points: the reference's numpy expression."""
        f = self.figure
        hist, bins = self.compute_histogram(direction)
        mu, sigma = (f.mu_x, f.sigma_x) if direction == "x" else (f.mu_y, f.sigma_y)
        with np.errstate(all="ignore"):
            n = 1 / (sigma * np.sqrt(2 * np.pi)) * np.exp(-((bins - mu) ** 2) / (2 * sigma**2))
            curve = n / (np.sum(n)) * np.sum(hist)
        return bins, curve, mu, sigma

    def ce_scatter(self):
        """`_ce_scatter` -> (x, y, z, plot_limit, ce90): `axes.scatter(x, y, c=z)` in drawing order, the axis limits, the circle's
        radius."""
        f = self.figure
        return host(f.scatter_x), host(f.scatter_y), host(f.scatter_z), f.plot_limit, f.ce90

    def radial_error(self):
        """`_radial_error_plot` -> (percent, radial, ce90, ce95): `axes.plot(percent, radial)` and the two marks."""
        f = self.figure
        v = host(f.radial)
        return np.linspace(0, 100, v.shape[0]), v, f.ce90, f.ce95

    def text_lines(self, x_label=None, y_label=None, pixel_size_line=None):
        """The lines of `_text_box` (circular_error_plot.py:379-418), tabs not yet expanded; `pixel_size_line`, if given, goes in
        fourth place as the reference's "Pixel size" line does."""
        s, res, u, f = self._stats, self.img_res, self.short_unit, self.figure
        x_label = x_label or ("Row displacement (pixel)" if self.pixel_units else "Easting displacement (meter)")
        y_label = y_label or ("Line displacement (pixel)" if self.pixel_units else "Northing displacement (meter)")
        x_rmse, y_rmse = rmse(s.mean_x, s.std_x, res), rmse(s.mean_y, s.std_y, res)
        lines = [f"Total Number of Key Point : {s.sample_pixel}", f"Confidence value : {s.confidence:.2f}",
                 f"Percentage of Confident Pixels : {s.percentage_of_pixel:.2f}%", ""]
        for label, axis, r in ((x_label, "x", x_rmse), (y_label, "y", y_rmse)):
            lines += [f"{label}:"] + [f"\t{title} : {getattr(s, f'{name}_{axis}') * res:.2f} {u}"
                                     for title, name in (("Min", "min"), ("Max", "max"), ("Mean", "mean"), ("Sigma", "std"))]
            lines += [f"\tRMSE : {r:.2f} {u}", ""]
        lines += [f"Global RMSE : {rmse(x_rmse, y_rmse):.2f} {u}", f"CE @90 the percentile : {f.ce90:.2f} {u}", f"CE @95 the percentile : {f.ce95:.2f} {u}"]
        if pixel_size_line is not None:
            lines.insert(3, pixel_size_line)
        return lines


def text_lines(stats, img_res, **kw):
    """The lines of the figure's text box for `stats` at `img_res` (`CircularErrorNumbers.text_lines`)."""
    return CircularErrorNumbers(stats, img_res).text_lines(**kw)
