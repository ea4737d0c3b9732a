"""GPU suite: KariosAPI.analyze_accuracy on resident data (csrc/k_accuracy.hip) against its definition, tests/accuracy_restatement.py,
and the recorded results of the reference (tests/golden/accuracy.npz): the valid-pixel count exactly, the statistics by bits
(minimum / maximum / median by value: the sign of a zero is not pinned), CE by bits."""
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

import accuracy_restatement as A

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_accuracy as G  # noqa: E402

from karios_amd import synth  # noqa: E402
from karios_amd.accuracy_analysis import GeometricStat  # noqa: E402
from karios_amd.core.configuration import AccuracyAnalysisConfiguration  # noqa: E402
from karios_amd.ops import accuracy_statistics, count_valid_pixels  # noqa: E402
from karios_amd.resident import ResidentPair  # noqa: E402
from karios_amd.results import analyze_accuracy  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "accuracy.npz"))
f32 = np.float32
SIZES = G.SIZES + (70001,)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def random_raster(dt, H, W, rng):
    dt = np.dtype(dt)
    a = (rng.integers(0, 4, (H, W)) * rng.integers(1, 100, (H, W))).astype(dt)      # one pixel in four is zero
    if dt == np.int16:
        a = np.where(rng.random((H, W)) < 0.5, a, -a).astype(dt)
    if dt == np.float32:
        special = np.array([0x7FC00000, 0x80000000, 0x00000001, 0x807FFFFF, 0xFFC00001, 0x00000000], np.uint32).view(f32)
        where = rng.random((H, W)) < 0.2
        a[where] = rng.choice(special, int(where.sum()))
    return a


# ---- the count --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", G.DTYPES)
def test_count_small_shapes_host_and_device_form(dt):
    rng = np.random.default_rng(1)
    for H, W in ((1, 1), (3, 5), (64, 64), (97, 131)):
        a = random_raster(dt, H, W, rng)
        for mask in (None, (rng.random((H, W)) < 0.6).astype(np.uint8) * 200, np.zeros((H, W), np.uint8)):
            want = A.count_valid_pixels(a, mask)
            assert count_valid_pixels(a, mask) == want, (dt, H, W)
            assert count_valid_pixels(to_dev(a), None if mask is None else to_dev(mask)) == want, (dt, H, W)
    a, mask = G.raster(dt)
    assert [count_valid_pixels(a), count_valid_pixels(a, mask)] == list(GOLD[f"count_{dt}"])


@pytest.mark.parametrize("dt", G.DTYPES)
def test_count_window_of_a_wider_buffer_with_poisoned_padding(dt):
    """257 x 1030 at (5, 7) of a 270 x 1100 buffer, the mask at (3, 1) of a 265 x 1111 one: rows start off the 16-byte grid, everything
    around the window is non-zero."""
    rng = np.random.default_rng(2)
    H, W = 257, 1030
    a = random_raster(dt, H, W, rng)
    mask = (rng.random((H, W)) < 0.7).astype(np.uint8)
    big = np.full((270, 1100), 7, a.dtype)
    if a.dtype == np.float32:
        big.view(np.uint32)[:] = 0x7FC00000
    big[5:5 + H, 7:7 + W] = a
    mbig = np.full((265, 1111), 255, np.uint8)
    mbig[3:3 + H, 1:1 + W] = mask
    want = A.count_valid_pixels(a, mask)
    assert 0 < want < A.count_valid_pixels(a) < H * W
    d_big, d_mbig = to_dev(big), to_dev(mbig)
    assert count_valid_pixels(d_big[5:5 + H, 7:7 + W], d_mbig[3:3 + H, 1:1 + W]) == want
    assert count_valid_pixels(d_big[5:5 + H, 7:7 + W]) == A.count_valid_pixels(a)
    assert count_valid_pixels(big[5:5 + H, 7:7 + W], mbig[3:3 + H, 1:1 + W]) == want        # host form: strided rows through the staging ring


def test_count_many_workgroups():
    rng = np.random.default_rng(3)
    a = random_raster("uint16", 2048, 2048, rng)
    mask = (rng.random(a.shape) < 0.5).astype(np.uint8)
    d_a, d_m = to_dev(a), to_dev(mask)
    assert count_valid_pixels(d_a, d_m) == A.count_valid_pixels(a, mask)
    assert count_valid_pixels(d_a) == A.count_valid_pixels(a)
    assert count_valid_pixels(d_a, to_dev(np.zeros_like(mask))) == 0


# ---- the statistics ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frame(n):
    if n in G.SIZES:
        return G.frame(n, G.SIZES.index(n))
    return G.frame(n, 99)


@functools.lru_cache(maxsize=None)
def expected(n, f64_threshold, carto):
    dx, dy, score = frame(n)
    thr = np.float64(G.THRESHOLD) if f64_threshold else G.THRESHOLD
    sample, stats = A.statistics(dx, dy, score, thr, carto)
    x, y, _c = A.sample(dx, dy, score, thr, carto)
    return sample, stats, {f: [A.ce(x, y, p, f) for p in G.PERCENTS] for f in G.FACTORS}


def check(res, want, factor):
    sample, stats, ce = want
    assert res.path == "device" and res.sample == sample and res.n_nan == 0
    got = np.array([res.stats[k] for k in A.STAT_NAMES], f32)
    by_value = list(A.BY_VALUE)
    rest = [i for i in range(15) if i not in by_value]
    assert np.array_equal(got[by_value], stats[by_value]), (got, stats)
    assert np.array_equal(bits(got[rest]), bits(stats[rest])), (got, stats)
    assert all(type(v) is f32 for v in res.ce) and np.array_equal(bits(res.ce), bits(ce[factor]))


@pytest.mark.parametrize("n", SIZES)
def test_statistics_by_bits(n):
    dx, dy, score = frame(n)
    for f64_threshold in (False, True):
        thr = np.float64(G.THRESHOLD) if f64_threshold else G.THRESHOLD
        for carto in (False, True):
            want = expected(n, f64_threshold, carto)
            assert want[0] == n + int(f64_threshold)                       # the row AT float32(0.4) passes the float64 comparison only
            for factor in G.FACTORS:
                check(accuracy_statistics(dx, dy, score, thr, carto=carto, factor=factor, percents=G.PERCENTS), want, factor)
            if n in G.SIZES:                                              # ... and the reference's own numbers
                key = f"{n}_{'f64' if f64_threshold else 'py'}_{int(carto)}"
                assert np.array_equal(bits(want[1][[3, 4, 8, 9, 13, 14]]), bits(GOLD[f"stats_{key}"][[3, 4, 8, 9, 13, 14]]))
                assert np.array_equal(bits([v for f in G.FACTORS for v in want[2][f]]), bits(GOLD[f"ce_{key}"]))
    check(accuracy_statistics(dx, dy, score, f32(G.THRESHOLD), factor=f32(0.3)), expected(n, False, False), 0.3)


def test_statistics_of_device_tensors_twice_in_a_row():
    for n in (20000, 129, 20000):                                          # the workspace shrinks and grows again
        cols = [to_dev(a) for a in frame(n)]
        for _ in range(2):
            check(accuracy_statistics(*cols, G.THRESHOLD, carto=True, factor=10.0), expected(n, False, True), 10.0)


def test_nothing_above_the_threshold():
    dx, dy, score = frame(9)
    res = accuracy_statistics(dx, dy, score, 2.0)
    assert res.path == "device" and res.sample == 0 and res.stats is None and res.ce == (None, None)
    res = accuracy_statistics(dx[:0], dy[:0], score[:0], 0.4)
    assert res.sample == 0 and res.stats is None
    st = GeometricStat(AccuracyAnalysisConfiguration(confidence_threshold=2.0), pd.DataFrame({"dx": dx, "dy": dy, "score": score}))
    st.compute_stats(5)
    assert st.sample_pixel == 0 and st.valid is False and st.mean_x == ""
    with pytest.raises(IndexError):
        st.compute_percentile(0.9, 1.0)


def test_nan_in_dx_comes_back_as_numpy_gives_it():
    dx, dy, score = (a.copy() for a in frame(1000))
    dx[np.flatnonzero(score > f32(0.4))[17]] = np.nan
    res = accuracy_statistics(dx, dy, score, G.THRESHOLD)
    keep = score > f32(0.4)
    assert res.path == "host" and res.sample == 1000 and res.n_nan == 1
    for k in ("min_x", "max_x", "median_x", "mean_x", "std_x"):
        assert np.isnan(res.stats[k])
    assert bits(res.stats["mean_y"]) == bits(np.mean(dy[keep])) and bits(res.stats["std_c"]) == bits(np.std(score[keep]))
    # a NaN outside the sample is nobody's business
    dx, dy, score = (a.copy() for a in frame(1000))
    dx[np.flatnonzero(~(score > f32(0.4)))[0]] = np.nan
    check(accuracy_statistics(dx, dy, score, G.THRESHOLD), expected(1000, False, False), 1.0)


# ---- the whole step ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask", [False, True])
def test_analyze_accuracy_on_a_resident_pair(with_mask, tmp_path):
    mon, ref = synth.make_pair(512, 512, 0.5, -0.25, seed=5)
    mon = mon.copy()
    mon[100:140, 50:300] = 0
    mask = None
    if with_mask:
        mask = np.ones(mon.shape, np.uint8)
        mask[:, 400:] = 0
    pair = ResidentPair.upload(mon, ref, mask)
    dx, dy, score = frame(8193)
    points = pd.DataFrame({"x0": np.zeros(dx.size, f32), "y0": np.zeros(dx.size, f32), "dx": dx, "dy": dy, "score": score})
    stats_file = tmp_path / "correl_res.txt"
    res = analyze_accuracy(points, pair, confidence_threshold=0.4, carto=True, pixel_size=10.0, stats_file=stats_file)
    sample, stats, ce = expected(8193, False, True)
    assert res.valid_pixels == A.count_valid_pixels(mon, mask) and res.total_pixels == 512 * 512
    assert res.valid_pixels < (512 * 512 if not with_mask else 512 * 400)
    assert res.statistics.valid and res.statistics.sample_pixel == sample and res.statistics.total_pixel == res.valid_pixels
    named = dict(zip(A.STAT_NAMES, stats))
    for k in ("mean_x", "mean_y", "std_x", "std_y"):
        assert type(getattr(res, k)) is f32 and bits(getattr(res, k)) == bits(named[k])
    assert [bits(res.ce90), bits(res.ce95)] == [bits(v) for v in ce[10.0]]
    title, line = stats_file.read_text().splitlines()
    assert title.split()[:5] == ["refImg", "secImg", "total_valid_pixel", "sample_pixel", "confidence_th"]
    assert line.split()[2:5] == [str(res.valid_pixels), str(sample), "0.4"] and line.split()[8] == str(named["mean_x"])
