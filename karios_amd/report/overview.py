"""The numbers of `karios.report.overview_plot.OverviewPlot` that need the full rasters (report/overview_plot.py:134-194): the
invalid-pixel rule and the 0.5 % - 99.5 % display range of the monitored and the reference image, on the rasters a `ResidentPair`
holds.  The figure itself - imshow with `vmin` / `vmax`, the colour maps, the scatter plots - stays with the integrator."""
from __future__ import annotations

from .. import ops

PERCENTS = (0.5, 99.5)


def display_ranges(pair, no_values=None):
    """-> (mon, ref) `ops.DisplayRange`; `v_min` / `v_max` are what `_plot_image` hands to imshow.  The monitored image goes under
    the pair's user mask, both go under `no_values` and their own no-data value (`_plot`: apply_user_mask for the monitored image)."""
    return pair.display_ranges(no_values, PERCENTS)


def display_range(image, mask=None, no_values=None, nodata=None, ctx=None):
    """One raster that is not part of a pair (numpy array or device tensor), like `ops.display_range`."""
    return ops.display_range(image, mask, no_values, nodata, PERCENTS, ctx)
