"""GPU suite: the numbers of the circular-error figure on resident data (csrc/k_ce.hip, ops.ce_figure,
karios_amd.report.circular_error) against their definition, tests/ce_figure_restatement.py, by bits; end to end against the
reference's expressions on numpy / scipy with host copies of a frame that was tracked on the device."""
import functools
import os
import re
import sys

import numpy as np
import pytest

import ce_figure_cases as K
import ce_figure_restatement as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_ce_figure as G  # noqa: E402

from karios_amd import ops, synth  # noqa: E402
from karios_amd.accuracy_analysis import GeometricStat  # noqa: E402
from karios_amd.core.configuration import AccuracyAnalysisConfiguration, KLTConfiguration  # noqa: E402
from karios_amd.report.circular_error import CircularErrorNumbers  # noqa: E402
from karios_amd.resident import ResidentPair  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = (1, 2, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 70001)      # the sort's tile is 2048 keys, the block sum 8192 elements
FLAGS = ("path", "host_hist_x", "host_hist_y")


def to_dev(a, pad=0):
    """The column as a device tensor; pad > 0: inside a longer buffer whose other elements would change every number if read."""
    import torch
    if not pad:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    buf = np.concatenate([np.full(pad, 0.96875, f32), a, np.full(pad + 3, 0.984375, f32)])
    return torch.from_numpy(buf).cuda()[pad:pad + a.size]


@functools.lru_cache(maxsize=None)
def restated_golden():
    return {name: R.figure(dx, dy, score, G.THRESHOLD, res, carto) for name, dx, dy, score, res, carto in G.cases()}


@functools.lru_cache(maxsize=None)
def restated_fresh(kind, n, res):
    dx, dy, score, carto = K.fresh(kind, n, seed=2)
    return (dx, dy, score, carto), R.figure(dx, dy, score, K.THRESHOLD, res, carto)


def check(got, want, tag, path="device", host_x=False):
    assert not K.differing(got, want), (tag, K.differing(got, want))
    assert (got.path, got.host_hist_x, got.host_hist_y) == (path, host_x, False), (tag, [getattr(got, f) for f in FLAGS])
    assert got.n_outside == int(np.isnan(want.scatter_z).sum()), tag


def test_golden_cases_in_both_call_forms():
    want = restated_golden()
    for name, dx, dy, score, res, carto in G.cases():
        check(ops.ce_figure(dx, dy, score, G.THRESHOLD, res, carto=carto), want[name], name + " host arrays")
        got = ops.ce_figure(to_dev(dx), to_dev(dy), to_dev(score), G.THRESHOLD, res, carto=carto)
        assert hasattr(got.scatter_x, "data_ptr") and hasattr(got.radial, "data_ptr") and not hasattr(got.hist_x, "data_ptr")
        check(got, want[name], name + " device tensors")


@pytest.mark.parametrize("n", SIZES)
def test_sample_sizes_inside_poisoned_buffers(n):
    (dx, dy, score, carto), want = restated_fresh("normal", n, 10.0)
    check(ops.ce_figure(to_dev(dx, 7), to_dev(dy, 5), to_dev(score, 9), K.THRESHOLD, 10.0, carto=carto), want, n)


def test_an_empty_sample_raises():
    dx, dy, score, _ = K.fresh("normal", 300)
    low = np.minimum(score, f32(0.25))
    for cols in ((dx, dy, low), (to_dev(dx), to_dev(dy), to_dev(low))):
        with pytest.raises(ValueError, match="zero-size"):
            ops.ce_figure(*cols, K.THRESHOLD, 10.0)
    check(ops.ce_figure(dx, dy, score, K.THRESHOLD, 10.0), R.figure(dx, dy, score, K.THRESHOLD, 10.0), "the call after a refused one")


@pytest.mark.parametrize("res", [1.0, 0.1, 30.0])
def test_content_cases(res):
    for kind, n in (("equal", 64), ("quantised", 2500), ("far", 700), ("carto", 3000)):
        (dx, dy, score, carto), want = restated_fresh(kind, n, res)
        check(ops.ce_figure(to_dev(dx), to_dev(dy), to_dev(score), K.THRESHOLD, res, carto=carto), want, (kind, res))
        if kind == "equal":
            assert want.bins_x.size == 2 and want.x_edges[0] == want.scatter_x[0] - f32(0.5)
        if kind == "far":
            assert want.bins_x.size - 1 > R.LDS_BINS and want.bins_y.size - 1 > R.LDS_BINS          # the global-atomics form, both axes
        if kind in ("quantised", "carto"):                                                           # points in the outer half-bins: NaN, drawn last
            k = int(np.isnan(want.scatter_z).sum())
            assert 0 < k < n and np.isnan(want.scatter_z[n - k:]).all()
    z = np.zeros(40, f32)                                                                            # all zero: one bin over [-0.5, 0.5]
    want = R.figure(z, z, np.ones(40, f32), K.THRESHOLD, res)
    assert list(want.bins_x) == [-0.5, 0.5]
    check(ops.ce_figure(to_dev(z), to_dev(z), to_dev(np.ones(40, f32)), K.THRESHOLD, res), want, ("zeros", res))
    # an LDS axis beside a global one, in one launch
    dx, dy, score, _ = K.fresh("far", 700, seed=4)
    dy = (dy + f32(7)).astype(f32)
    want = R.figure(dx, dy, score, K.THRESHOLD, res)
    assert want.bins_x.size - 1 > R.LDS_BINS >= want.bins_y.size - 1
    check(ops.ce_figure(to_dev(dx), to_dev(dy), to_dev(score), K.THRESHOLD, res), want, ("mixed", res))


def test_more_bins_than_the_cap_take_numpy_for_that_axis_and_say_so():
    dx, dy, score, carto = K.beyond_the_cap()
    want = R.figure(dx, dy, score, K.THRESHOLD, 1.0, carto)
    assert want.bins_x.size - 1 > ops.CE_MAX_BINS >= 65536
    for cols in ((dx, dy, score), (to_dev(dx), to_dev(dy), to_dev(score))):
        check(ops.ce_figure(*cols, K.THRESHOLD, 1.0, carto=carto), want, "beyond the cap", host_x=True)


def test_a_nan_in_the_sample_takes_the_host_expressions():
    (dx, dy, score, carto), _ = restated_fresh("normal", 2047, 10.0)
    dx = dx.copy()
    dx[np.flatnonzero(score > K.THRESHOLD)[5]] = np.nan
    with np.errstate(all="ignore"):
        try:
            want = K.numpy_figure(dx, dy, score, K.THRESHOLD, 10.0, carto)
        except ValueError as e:                                   # numpy refuses a range that is not finite: so must the call
            with pytest.raises(ValueError, match=re.escape(str(e)[:20])):
                ops.ce_figure(to_dev(dx), to_dev(dy), to_dev(score), K.THRESHOLD, 10.0, carto=carto)
            return
    got = ops.ce_figure(to_dev(dx), to_dev(dy), to_dev(score), K.THRESHOLD, 10.0, carto=carto)
    assert got.path == "host" and not K.differing(got, want)


def test_two_runs_give_the_same_bytes():
    (dx, dy, score, carto), _ = restated_fresh("normal", 70001, 10.0)
    cols = (to_dev(dx), to_dev(dy), to_dev(score))
    a, b = (ops.ce_figure(*cols, K.THRESHOLD, 10.0, carto=carto) for _ in range(2))
    for f in R.FIELDS:
        assert K.host(getattr(a, f)).tobytes() == K.host(getattr(b, f)).tobytes(), f


def test_end_to_end_on_a_resident_frame():
    mon, ref = synth.make_pair(403, 640, 0.5, 0.0)
    frame = ResidentPair.upload(mon, ref).match_tile(KLTConfiguration())
    assert frame is not None and len(frame) > 300
    host = {k: frame[k].to_numpy() for k in ("dx", "dy", "score")}
    assert all(a.dtype == f32 for a in host.values())
    t = float(np.median(host["score"]))                          # half of the rows
    for res, carto in ((10.0, True), (None, False)):
        stats = GeometricStat(AccuracyAnalysisConfiguration(confidence_threshold=t), {k: to_dev(a) for k, a in host.items()}, carto=carto)
        stats.compute_stats(403 * 640)
        num = CircularErrorNumbers(stats, res)
        want = K.numpy_figure(host["dx"], host["dy"], host["score"], t, 1.0 if res is None else res, carto)
        assert num.figure.path == "device" and hasattr(num.figure.scatter_x, "data_ptr") and want.sample == stats.sample_pixel > 100
        assert not K.differing(num.figure, want), K.differing(num.figure, want)
        for axis in "xy":
            hist, bins = num.compute_histogram(axis)
            assert K.same(hist, getattr(want, f"hist_{axis}")) and K.same(bins, getattr(want, f"bins_{axis}"))
            assert num.gaussian(axis)[1].shape == bins.shape
        x, y, z, limit, ce90 = num.ce_scatter()
        assert K.same(x, want.scatter_x) and K.same(y, want.scatter_y) and K.same(z, want.scatter_z) and K.same(limit, want.plot_limit)
        assert K.same(num.radial_error()[1], want.radial) and K.same(ce90, want.ce90) and K.same(num.radial_error()[3], want.ce95)
        assert K.same(ce90, stats.compute_percentile(0.9, num.img_res)) and len(num.text_lines()) == 21
        sx, sy, sc = stats.device_sample()
        assert hasattr(sx, "data_ptr") and K.same(sx, stats.v_x_th) and K.same(sy, stats.v_y_th) and K.same(sc, stats.v_c_th)
