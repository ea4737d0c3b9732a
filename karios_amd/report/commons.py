"""Mirror of `karios.report.commons.mean_profile` (report/commons.py:49-71): the grouped count, mean and standard deviation behind
the row / column / altitude profile figures, computed on the device for float32 columns."""
from __future__ import annotations

import numpy as np

from .. import ops


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def _group(values, positions, bin_size):
    from pandas import DataFrame
    return DataFrame.from_dict({"val": values, "po": np.floor_divide(positions, bin_size)}).groupby("po")


class MeanProfile:
    """The reference's MeanProfile, field for field.  `grouped_values`, the pandas SeriesGroupBy only the altitude box plot reads,
    is built from host copies of the columns on first use."""

    def __init__(self, groups_positions, mean_values, nb_pos, values_std, grouped_values=None, columns=None):
        self.groups_positions, self.mean_values, self.nb_pos, self.values_std = groups_positions, mean_values, nb_pos, values_std
        self._grouped, self._columns = grouped_values, columns

    @property
    def grouped_values(self):
        if self._grouped is None:
            values, positions, bin_size = self._columns
            self._grouped = _group(_host(values), _host(positions), bin_size)["val"]
        return self._grouped

    def compute_std_min_max(self):
        y_err = self.values_std * np.sqrt(
            1 / len(self.groups_positions)
            + (self.groups_positions - self.groups_positions.mean()) ** 2
            / np.sum((self.groups_positions - self.groups_positions.mean()) ** 2)
        )
        return (self.mean_values - y_err, self.mean_values + y_err)


def _pandas_profile(values, positions, bin_size):
    group = _group(values, positions, bin_size)
    return MeanProfile((group["po"].first() * bin_size + bin_size // 2).astype(np.int32), group["val"].mean(), group["val"].count(),
                       group["val"].std(), grouped_values=group["val"])


def mean_profiles(requests, ctx=None):
    """Several float32 profiles over the same rows in one device call (the report asks for dx and dy over x0 and y0 at once):
    `requests` is a sequence of (values, positions, bin_size) of numpy arrays or device tensors -> a list of MeanProfile."""
    from pandas import Index, Series
    requests = [tuple(r) for r in requests]
    out = []
    for request, cols in zip(requests, ops.mean_profiles(requests, ctx)):
        index = Index(_host(cols.key), name="po")
        out.append(MeanProfile(Series(_host(cols.position), index=index, name="po"), Series(_host(cols.mean), index=index, name="val"),
                               Series(_host(cols.count).astype(np.int64), index=index, name="val"),
                               Series(_host(cols.std), index=index, name="val"), columns=request))
    return out


def mean_profile(values, positions, bin_size: int = 20, ctx=None) -> MeanProfile:
    """`mean_profile(values, positions, bin_size)` of the reference: count, mean and sample standard deviation of `values` per group
    of np.floor_divide(positions, bin_size), bit for bit what pandas 2.3 gives.  `groups_positions`, `mean_values`, `nb_pos` and
    `values_std` are pandas Series indexed by `po` (int32, float32, int64, float32).

    float32 columns - pandas Series, numpy arrays or device tensors, which is what the matcher's frame holds - are grouped on the
    device.  Columns of another type, for instance dx times a float64 resolution, take the pandas expression on the host."""
    v = values.to_numpy() if hasattr(values, "to_numpy") else values
    p = positions.to_numpy() if hasattr(positions, "to_numpy") else positions
    if not (hasattr(v, "data_ptr") and hasattr(p, "data_ptr")):
        v, p = np.asarray(v), np.asarray(p)
        if v.dtype != np.float32 or p.dtype != np.float32 or int(bin_size) != bin_size:
            return _pandas_profile(values, positions, bin_size)
    return mean_profiles([(v, p, int(bin_size))], ctx)[0]
