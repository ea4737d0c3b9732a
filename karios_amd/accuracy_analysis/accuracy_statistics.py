"""`GeometricStat` of karios/accuracy_analysis/accuracy_statistics.py with the numbers computed by `ops.accuracy_statistics`
(csrc/k_accuracy.hip): the sample above the confidence threshold, minimum / maximum / median / mean / standard deviation of
dx, dy and the score, and the CE percentiles of the radial error.  The attribute names and the text written to `correl_res.txt`
are the reference's; the statistics are np.float32 scalars, so `str()` of them reads the same.  `get_string_block` gives the
reference's text block; `display_results` (log text) is not mirrored.  `columns` and `device_sample` hand the sample on where it
lives (karios_amd.report.circular_error)."""
from __future__ import annotations

import os

import numpy as np

from .. import ops

_STATS = tuple(f"{k}_{axis}" for axis in "xy" for k in ("min", "max", "median", "mean", "std"))
TITLES = ("refImg", "secImg", "total_valid_pixel", "sample_pixel", "confidence_th") + _STATS


def _column(points, name):
    col = points[name]
    return col.to_numpy() if hasattr(col, "to_numpy") else col


class GeometricStat:
    """Statistics of the displacements of a frame with the columns dx, dy and score (a pandas DataFrame, or any mapping of
    float32 numpy arrays / device tensors with a `columns`-free interface: `points[name]`)."""

    def __init__(self, config, points, carto=False, pixel_size=1, ctx=None):
        self.valid = False
        self.confidence = config.confidence_threshold
        self.total_pixel = ""      # valid pixels of the monitored image
        self.sample_pixel = ""     # rows the statistics are taken over
        for name in _STATS:
            setattr(self, name, "")
        names = list(points.columns) if hasattr(points, "columns") else list(points.keys())
        missing = [col for col in ("dx", "dy", "score") if col not in names]
        if missing:
            raise ValueError(f"Missing required columns in points DataFrame: {missing}. Available columns: {names}. ")
        self._ctx = ctx
        self._carto = bool(carto)
        self._dx, self._dy, self.v_c = _column(points, "dx"), _column(points, "dy"), _column(points, "score")
        self.v_x = self._dx
        self.v_y = -self._dy if carto else self._dy          # y (line / northing) reversed for an image with an SRS
        self.total_match = int(self.v_x.shape[0])
        self.pixel_size = pixel_size
        self.apply_confidence(self.confidence)

    def _run(self, factor=1.0, percents=()):
        return ops.accuracy_statistics(self._dx, self._dy, self.v_c, self.confidence, carto=self._carto, factor=factor,
                                       percents=percents, ctx=self._ctx)

    def apply_confidence(self, confidence_threshold):
        """Keep the rows whose score is above the threshold (strictly, compared like `Series.gt`)."""
        self.confidence = confidence_threshold
        self._result = self._run()
        self._sample = None
        self.sample_pixel = self._result.sample
        with np.errstate(divide="ignore", invalid="ignore"):
            self.percentage_of_match = 100 * np.double(self.sample_pixel) / np.double(self.total_match)

    def _host_sample(self):
        if self._sample is None:
            def host(a):
                return a.detach().cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
            c = host(self.v_c)
            keep = c > self.confidence
            self._sample = (host(self.v_x)[keep], host(self.v_y)[keep], c[keep])
        return self._sample

    # the sample's columns as host arrays, like the reference's attributes (built on first use: the statistics do not need them)
    v_x_th = property(lambda self: self._host_sample()[0])
    v_y_th = property(lambda self: self._host_sample()[1])
    v_c_th = property(lambda self: self._host_sample()[2])

    @property
    def columns(self):
        """(dx, dy, score, threshold, carto) as they were given: what `ops.accuracy_statistics` and `ops.ce_figure` take."""
        return self._dx, self._dy, self.v_c, self.confidence, self._carto

    def device_sample(self):
        """The sample's columns (x, y, score) where the frame's columns live: device tensors stay on the device, compacted there in
        row order with the comparison `ops.accuracy_statistics` makes; numpy columns give `v_x_th`, `v_y_th`, `v_c_th`."""
        if not hasattr(self.v_c, "data_ptr"):
            return self._host_sample()
        import torch
        t = self.confidence
        thr = float(t) if isinstance(t, np.float64) else float(np.float32(t))
        keep = self.v_c.to(torch.float64) > thr
        return self.v_x[keep], self.v_y[keep], self.v_c[keep]

    def get_string_block(self, scale_factor, direction="x"):
        """The text block of one direction as the reference writes it (after `compute_stats`)."""
        pick = {name: getattr(self, f"{name}_{direction}") for name in ("min", "max", "mean", "std", "median")}
        head = f" Conf_Value : {self.confidence:.2f}" if direction == "x" else f" Conf_Value :{self.confidence:.2f}"
        lines = [head, f" %Conf Px   :{self.percentage_of_pixel:.2f}%", f"Minimum    : {(pick['min'] * scale_factor):.2f}",
                 f"Maximum   : {(pick['max'] * scale_factor):.2f}", f"Mean          : {(pick['mean'] * scale_factor):.2f}",
                 f"Std Dev      : {(pick['std'] * scale_factor):.2f}", f"Median       : {(pick['median'] * scale_factor):.2f}"]
        return "\n ".join(lines)

    def compute_stats(self, nb_pixels, confidence_threshold=None):
        if confidence_threshold is not None:
            self.apply_confidence(confidence_threshold)
        res = self._result
        self.total_pixel = nb_pixels
        self.sample_pixel = res.sample
        with np.errstate(divide="ignore", invalid="ignore"):
            self.percentage_of_pixel = 100 * np.double(self.sample_pixel) / np.double(self.total_pixel)
        self.valid = res.sample > 0
        if self.valid:
            for name, value in res.stats.items():
                setattr(self, name, value)

    def compute_percentile(self, percent, factor):
        """CE at `percent` of the radial errors scaled by `factor` (IndexError for an empty sample, like the reference's indexing)."""
        ce = self._run(factor, (percent,)).ce[0]
        if ce is None:
            raise IndexError(f"compute_percentile: {percent} of {self.sample_pixel} rows is no index")
        return ce

    def result_line(self, ref: str, mon: str) -> str:
        values = [self.total_pixel, self.sample_pixel, self.confidence] + [getattr(self, name) for name in _STATS]
        return f"{ref} {mon} {' '.join(str(v) for v in values)}\n"

    def update_statistic_file(self, ref: str, mon: str, out_file_path: str = None):
        """Append the line of this pair to `out_file_path` (default: correl_res.txt in the current directory), titles first."""
        if out_file_path is None:
            out_file_path = os.path.join(os.getcwd(), "correl_res.txt")
        if not os.path.exists(out_file_path):
            with open(out_file_path, "w", encoding="utf-8") as txt_file:
                txt_file.write(" ".join(TITLES) + "\n")
        with open(out_file_path, "a", encoding="utf-8") as txt_file:
            txt_file.write(self.result_line(ref, mon))
