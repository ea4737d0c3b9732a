"""GPU suite: the report's products and the altitude figure's numbers on resident data (csrc/k_products.hip) - the key-point rasters,
the altitude column and the box statistics - against their definition, tests/products_restatement.py, the recorded results of the
reference (tests/golden/products.npz) and numpy / pandas / matplotlib on the host copies.  Every comparison is by bits (NaN equals
NaN; the sign of a zero folded for the order statistics and whisker ends only)."""
import functools
import os
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

import products_restatement as P

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_products as G  # noqa: E402

from karios_amd import ops, synth  # noqa: E402
from karios_amd.core import KLTConfiguration  # noqa: E402
from karios_amd.core.image import DeviceRasterImage  # noqa: E402
from karios_amd.report import product_generator, shift_by_alt  # noqa: E402
from karios_amd.resident import ResidentPair  # noqa: E402
from test_gpu_report import same, to_dev, to_host  # noqa: E402
from test_products_host import OUT_OF_RANGE, box_cases, same_box, same_stat  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "products.npz"))
f32 = np.float32
f64 = np.float64
FORMS = ("host", "dev")


def device_rasters(form, x, y, dx, dy, h, w, **kw):
    if form == "dev":
        cols = [None if a is None else to_dev(a) for a in (x, y, dx, dy)]
        m, d = ops.point_rasters(*cols, shape=(h, w), **kw)
        return (None if m is None else to_host(m)), (None if d is None else to_host(d))
    return ops.point_rasters(x, y, dx, dy, shape=(h, w), **kw)


def check_rasters(form, x, y, dx, dy, h, w, tag):
    want_mask, want_delta, bad = P.point_rasters(x, y, dx, dy, h, w)
    assert bad == 0, tag
    mask, delta = device_rasters(form, x, y, dx, dy, h, w)
    assert same(mask, want_mask) and same(delta.view(np.uint32), want_delta.view(np.uint32)), tag
    only, none = device_rasters(form, x, y, None, None, h, w)
    assert none is None and same(only, want_mask), tag
    none, only = device_rasters(form, x, y, dx, dy, h, w, mask=False)
    assert none is None and same(only.view(np.uint32), want_delta.view(np.uint32)), tag


def frame(rng, n, h, w):
    """n rows inside an h x w raster: fractions, both halves of the column wrap, negative fractions, pixels hit more than once."""
    x = (rng.random(n) * 2 * w - w).astype(f32)
    y = (rng.random(n) * h).astype(f32)
    x, y = np.clip(x, -w, f32(w) - f32(0.5)), np.minimum(y, f32(h) - f32(0.5))
    if n > 8:
        x[3:6], y[3:6] = f32(2.5), f32(1.25)               # three rows on one pixel, different dx
        x[6], x[7], y[6], y[7] = f32(-1), f32(w - 1), f32(0), f32(0)
        x[8], y[8] = f32(-0.9), f32(-0.9)
    return x, y, rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)


# ---- point rasters ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_golden_rasters(form):
    for name, x, y, dx, dy, h, w in G.raster_cases():
        mask, delta = device_rasters(form, x, y, dx, dy, h, w)
        assert same(mask, GOLD[f"mask_{name}"]) and same(delta.view(np.uint32), GOLD[f"delta_{name}"]), name


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 2049, 70001])
def test_raster_sizes(form, n):
    """Around the wavefront, the sort's 2048-key tile, more than one sweep; 37 x 53 and 5 x 9."""
    rng = np.random.default_rng(n + 11)
    for h, w in ((37, 53), (5, 9)):
        check_rasters(form, *frame(rng, n, h, w), h, w, (n, h, w))


def test_window_of_a_poisoned_buffer():
    """A 64 x 100 window inside wider buffers: row strides above the width, bases off the 16-byte grid; nothing outside may change."""
    import torch
    rng = np.random.default_rng(21)
    h, w = 64, 100
    x, y, dx, dy = frame(rng, 3000, h, w)
    want_mask, want_delta, _ = P.point_rasters(x, y, dx, dy, h, w)
    mbuf = torch.full((h + 2, 131), 0xAB, dtype=torch.uint8, device="cuda")
    dbuf = torch.full((2, h + 3, 109), -7.0, dtype=torch.float32, device="cuda")
    mwin, dwin = mbuf[1:1 + h, 3:3 + w], dbuf[:, 2:2 + h, 5:5 + w]
    assert mwin.data_ptr() % 16 and dwin.data_ptr() % 16
    m, d = ops.point_rasters(*(to_dev(a) for a in (x, y, dx, dy)), shape=(h, w), out_mask=mwin, out_delta=dwin)
    assert m is mwin and d is dwin
    mhost, dhost = mbuf.cpu().numpy(), dbuf.cpu().numpy()
    assert same(mhost[1:1 + h, 3:3 + w], want_mask) and same(dhost[:, 2:2 + h, 5:5 + w].view(np.uint32), want_delta.view(np.uint32))
    mhost[1:1 + h, 3:3 + w] = 0xAB
    dhost[:, 2:2 + h, 5:5 + w] = -7
    assert (mhost == 0xAB).all() and (dhost == -7).all()
    # the host form into strided numpy windows
    mnp, dnp = np.full((h + 2, 131), 0xAB, np.uint8), np.full((2, h + 3, 109), -7, f32)
    ops.point_rasters(x, y, dx, dy, shape=(h, w), out_mask=mnp[1:1 + h, 3:3 + w], out_delta=dnp[:, 2:2 + h, 5:5 + w])
    assert same(mnp[1:1 + h, 3:3 + w], want_mask) and same(dnp[:, 2:2 + h, 5:5 + w].view(np.uint32), want_delta.view(np.uint32))
    mnp[1:1 + h, 3:3 + w] = 0xAB
    dnp[:, 2:2 + h, 5:5 + w] = -7
    assert (mnp == 0xAB).all() and (dnp == -7).all()


@pytest.mark.parametrize("form", FORMS)
def test_rows_out_of_range_raise(form):
    h, w = 37, 53
    for x, y in ((np.nan, 1), (np.inf, 1), (1, -1), (1, h), (w, 1), (-w - 1, 1)):
        xs, ys, d = np.array([2, x, 3], f32), np.array([2, y, 3], f32), np.ones(3, f32)
        for kw in ({}, {"delta": False}, {"mask": False}):
            with pytest.raises(IndexError, match="1 row"):
                device_rasters(form, xs, ys, d, d, h, w, **kw)
    xs, ys = np.array([p[0] for p in OUT_OF_RANGE] + [1], f32), np.array([p[1] for p in OUT_OF_RANGE] + [1], f32)
    with pytest.raises(IndexError, match=f"{len(OUT_OF_RANGE)} row"):
        device_rasters(form, xs, ys, xs, ys, h, w)


# ---- sampling ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16", "float32"])
def test_sampling(form, dtype):
    rng = np.random.default_rng(31)
    h, w = 37, 53
    buf = (rng.random((h + 2, w + 9)) * 250 - (100 if dtype in ("int16", "float32") else 0)).astype(dtype)
    raster = buf[1:1 + h, 4:4 + w]                           # a strided window
    for n in (0, 1, 65, 3000):
        x = np.clip((rng.random(n) * 2 * w - w).astype(f32), -w, f32(w) - f32(0.5))
        y = np.clip((rng.random(n) * 2 * h - h).astype(f32), -h, f32(h) - f32(0.5))
        if n > 2:
            x[:3], y[:3] = np.array([-w, -1, -0.9], f32), np.array([-h, -1, -0.9], f32)      # both indices negative
        want = raster[y.astype(int), x.astype(int)]
        if form == "dev":
            got = to_host(ops.sample_points(to_dev(buf)[1:1 + h, 4:4 + w], to_dev(x), to_dev(y)))
        else:
            got = ops.sample_points(raster, x, y)
        assert same(got, want) and same(got, P.sample_points(raster, x, y)[0]), n
    for x, y in ((np.nan, 1), (np.inf, 1), (1, -h - 1), (1, h), (w, 1), (-w - 1, 1)):
        xs, ys = np.array([2, x], f32), np.array([2, y], f32)
        with pytest.raises(IndexError, match="1 row"):
            ops.sample_points(to_dev(np.ascontiguousarray(raster)), to_dev(xs), to_dev(ys)) if form == "dev" else ops.sample_points(raster, xs, ys)


# ---- box statistics ---------------------------------------------------------------------------------------------------------------------
def device_box(form, v, p, b):
    if form == "host":
        return ops.box_stats(v, p, b)
    got = ops.box_stats(to_dev(v), to_dev(p), b)
    return P.BoxStats(**{k: to_host(getattr(got, k)) for k in ("key", "count", "mean", "cls") + P.STAT_NAMES})


@pytest.mark.parametrize("form", FORMS)
def test_box_cases(form):
    """Group sizes 1 .. 5, 127 .. 129 and 8193, every row its own group, a NaN value, equal values, values on and beyond the fences,
    signed-zero, NaN and infinite positions, infinite values."""
    for name, v, p, b in box_cases():
        assert same_box(device_box(form, v, p, b), P.box_stats(v, p, b)), name


@pytest.mark.parametrize("form", FORMS)
def test_box_one_group_of_70001_rows(form):
    rng = np.random.default_rng(41)
    v = (rng.standard_normal(70001) * 5).astype(f32)
    p = (rng.random(v.size) * 19).astype(f32)
    got = device_box(form, v, p, 20)
    assert same_box(got, P.box_stats(v, p, 20)) and got.key.size == 1
    assert same(got.mean[0], np.mean(v)) and same(got.q1[0], np.percentile(v, [25, 50, 75])[0])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2049, 20000])
def test_box_sizes(n):
    rng = np.random.default_rng(n + 5)
    v = (rng.standard_normal(n) * rng.choice([1, 1, 1, 8], n)).astype(f32)
    p = (rng.random(n) * 900 - 100).astype(f32)
    for b in (7, 20):
        assert same_box(device_box("dev", v, p, b), P.box_stats(v, p, b)), (n, b)


def test_golden_box_stats():
    for name, v, alt, x_res, b in G.altitude_cases():
        values = v * f32(x_res)
        got = device_box("dev", values, alt.astype(f32), b)
        assert same(got.count, GOLD[f"count_{name}"]) and same(got.mean, GOLD[f"mean_{name}"]), name
        for k in P.STAT_NAMES:
            assert same_stat(k, getattr(got, k), GOLD[f"{k}_{name}"]), (name, k)


# ---- the altitude profile -----------------------------------------------------------------------------------------------------------------
def host_altitude_numbers(frame_, dem, dimension, x_res, b):
    """The reference's own expressions on host copies: numpy's fancy indexing, pandas' group-by, matplotlib's statistics."""
    from matplotlib.cbook import boxplot_stats
    alt = dem[frame_["y0"].to_numpy().astype(int), frame_["x0"].to_numpy().astype(int)]
    points = frame_.copy()
    points["alt"] = alt                                    # (by position, as core.py assigns it: the frame's index is not 0 .. n - 1)
    values, positions = points[dimension] * x_res, points["alt"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        group = pd.DataFrame.from_dict({"val": values, "po": np.floor_divide(positions, b)}).groupby("po")
        pos = (group["po"].first() * b + b // 2).astype(np.int32)
        stats = boxplot_stats([g[1].to_numpy() for g in group["val"]])
        return alt, pos, group["val"].count(), group["val"].mean(), group["val"].std(), stats


def check_altitude_profile(got, want, tag):
    alt, pos, count, mean, std, stats = want
    m = got.profile
    assert same(m.groups_positions.to_numpy(), pos.to_numpy()) and same(m.groups_positions.index.to_numpy(), pos.index.to_numpy()), tag
    assert same(m.nb_pos.to_numpy(), count.to_numpy()) and same(m.mean_values.to_numpy(), mean.to_numpy()) and same(m.values_std.to_numpy(), std.to_numpy()), tag
    assert len(got.box_stats) == len(stats), tag
    for g, (a, b) in enumerate(zip(got.box_stats, stats)):
        assert same(a["mean"], b["mean"]) and same(a["fliers"], b["fliers"]), (tag, g)
        for k in P.STAT_NAMES:
            assert same_stat(k, f64(a[k]), f64(b[k])), (tag, g, k)


@functools.lru_cache(maxsize=None)
def matched_frame():
    mon, ref = synth.make_pair(403, 640, 0.5, 0.0)
    pair = ResidentPair.upload(mon, ref)
    frame_ = pair.match_tile(KLTConfiguration())
    assert frame_ is not None and len(frame_) > 300 and all(frame_[c].dtype == f32 for c in ("x0", "y0", "dx", "dy"))
    return pair, frame_


def dem_of(dtype, h=403, w=640):
    yy, xx = np.mgrid[0:h, 0:w]
    rough = (np.sin(xx / 37.0) + np.cos(yy / 23.0)) * 0.5 + (xx + yy) / float(h + w)         # 0 .. 2, smooth: groups of many sizes
    if dtype == "uint8":
        return (rough * 100).clip(0, 255).astype(np.uint8)
    if dtype == "uint16":
        return (rough * 20000 + 100).clip(0, 65535).astype(np.uint16)
    if dtype == "int16":
        return (rough * 900 - 400).astype(np.int16)
    dem = (rough * 900 - 400).astype(f32)
    dem[::17, ::13] = np.nan
    return dem


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16", "float32"])
def test_altitude_profile_end_to_end(dtype):
    pair, frame_ = matched_frame()
    dem = dem_of(dtype)
    b = {"uint8": 3, "uint16": 500, "int16": 20, "float32": 20}[dtype]
    want = host_altitude_numbers(frame_, dem, "dx", 10, b)
    assert same(shift_by_alt.altitudes(frame_, dem), want[0])
    check_altitude_profile(shift_by_alt.altitude_profile(frame_, dem, "dx", 10, b), want, dtype)
    # the DEM resident, as a tensor and as a DeviceRasterImage; the frame as device columns
    image = DeviceRasterImage(to_dev(dem.view(np.int16)) if dtype == "uint16" else to_dev(dem), dtype=dtype)
    assert same(to_host(shift_by_alt.altitudes(frame_, image)).view(dem.dtype), want[0])
    cols = {k: to_dev(frame_[k].to_numpy()) for k in ("x0", "y0", "dx", "dy")}
    check_altitude_profile(shift_by_alt.altitude_profile(cols, image, "dx", 10, b), want, dtype + " resident")
    check_altitude_profile(shift_by_alt.altitude_profile(frame_, to_dev(dem), "dy", 0.5, b), host_altitude_numbers(frame_, dem, "dy", 0.5, b), dtype + " dy")
    # the products of the same frame in the pair's shape
    want_mask, want_delta, bad = P.point_rasters(*(frame_[k].to_numpy() for k in ("x0", "y0", "dx", "dy")), 403, 640)
    mask, delta = pair.point_rasters(frame_)
    assert bad == 0 and same(mask, want_mask) and same(delta.view(np.uint32), want_delta.view(np.uint32))
    assert same(product_generator.kp_mask(frame_, pair), want_mask) and same(to_host(product_generator.kp_delta(cols, (403, 640))).view(np.uint32), want_delta.view(np.uint32))


def test_integer_dem_labels_wrap_as_pandas_does():
    rng = np.random.default_rng(51)
    n = 400
    frame_ = pd.DataFrame({"x0": (rng.random(n) * 9).astype(f32), "y0": (rng.random(n) * 5).astype(f32), "dx": rng.standard_normal(n).astype(f32)})
    dem = np.where(rng.random((5, 9)) < 0.5, 32767, -32768).astype(np.int16)
    dem[0, 0] = 32767
    frame_.loc[0, ["x0", "y0"]] = f32(0.5)
    got = shift_by_alt.altitude_profile(frame_, dem, "dx", 10, 20)
    check_altitude_profile(got, host_altitude_numbers(frame_, dem, "dx", 10, 20), "int16")
    assert -32766 in list(got.profile.groups_positions)                 # (32767 // 20) * 20 + 10 in int16
    dem8 = np.where(rng.random((5, 9)) < 0.5, 255, 7).astype(np.uint8)
    dem8[0, 0] = 255
    got = shift_by_alt.altitude_profile(frame_, dem8, "dx", 10, 3)
    check_altitude_profile(got, host_altitude_numbers(frame_, dem8, "dx", 10, 3), "uint8")
    assert 0 in list(got.profile.groups_positions)                      # (255 // 3) * 3 + 1 in uint8
    with pytest.raises(OverflowError):
        shift_by_alt.altitude_profile(frame_, dem, "dx", 10, 40000)
