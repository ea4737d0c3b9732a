"""GPU suite: the report's numbers on resident data (csrc/k_report.hip) - the display range of OverviewPlot._plot_image and
mean_profile - against their definition, tests/report_restatement.py, the recorded results of the reference
(tests/golden/report_numbers.npz) and numpy / pandas on the host copies.  Every comparison is by bits (NaN equals NaN)."""
import functools
import os
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

import report_restatement as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_report as G  # noqa: E402

from karios_amd import ops, synth  # noqa: E402
from karios_amd.core import KLTConfiguration  # noqa: E402
from karios_amd.report import commons, overview  # noqa: E402
from karios_amd.resident import ResidentPair  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "report_numbers.npz"))
f32 = np.float32
FORMS = ("host", "dev")


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def to_host(t):
    import torch
    if isinstance(t, np.ndarray):
        return t
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        nan = np.isnan(a)
        return bool(np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes())
    return a.tobytes() == b.tobytes()


def restated(a, mask=None, no_values=None, nodata=None, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return R.display_range(a, mask, no_values, nodata, **kw)


def device_range(form, a, mask=None, no_values=None, nodata=None, **kw):
    if form == "dev":
        return ops.display_range(to_dev(a), None if mask is None else to_dev(mask), no_values, nodata, **kw)
    return ops.display_range(a, mask, no_values, nodata, **kw)


def check_range(got, want, what=""):
    assert (got.n_valid, got.n_invalid) == (want.n_valid, want.n_invalid), (what, got.n_valid, got.n_invalid, want.n_valid, want.n_invalid)
    assert same(got.raster_min, want.raster_min) and same(got.raster_max, want.raster_max), (what, got.raster_min, got.raster_max)
    assert len(got.values) == len(want.values) and all(same(g, w) for g, w in zip(got.values, want.values)), (what, got.values, want.values)


def raster(rng, dt, shape):
    if dt == "float32":
        a = (rng.standard_normal(shape) * 100).astype(f32)
        for frac, v in ((0.05, 0.0), (0.03, -0.0), (0.03, np.nan), (0.02, np.inf), (0.02, -np.inf)):
            a[rng.random(shape) < frac] = f32(v)
        return a
    info = np.iinfo(dt)
    a = rng.integers(max(info.min, -500), min(info.max, 4000) + 1, shape).astype(dt)
    a[rng.random(shape) < 0.05] = 0
    return a


# ---- display range ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_golden_ranges(form):
    for name, a, mask, no_values, nodata in G.range_cases():
        got = device_range(form, a, mask, no_values, nodata)
        check_range(got, restated(a, mask, no_values, nodata), name)
        assert got.n_invalid == int(GOLD[f"invalid_{name}"][0]), name
        if got.n_valid:
            assert same(got.v_min, GOLD[f"vmin_{name}"]) and same(got.v_max, GOLD[f"vmax_{name}"]), name


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", G.DTYPES)
def test_shapes_and_predicate_terms(form, dt):
    """1 x 1, the flat path with a tail behind the last whole vector, widths around the row path's 256-lane chunk; each term of the
    predicate alone and all together; everything invalid (the fallback)."""
    rng = np.random.default_rng(G.DTYPES.index(dt) + 40)
    for shape in ((1, 1), (37, 53), (3, 255), (3, 256), (3, 257), (3, 513)):
        a = raster(rng, dt, shape)
        mask = (rng.random(shape) < 0.7).astype(np.uint8)
        nv = [a.ravel()[0].item(), a.ravel()[-1].item(), 0, -1, 70000, 0.5, float("nan")]
        nd = a[shape[0] // 2, shape[1] // 2].item()
        for args in ((None, None, None), (mask, None, None), (None, nv, None), (None, None, nd), (mask, nv, nd), (np.zeros(shape, np.uint8), None, None)):
            check_range(device_range(form, a, *args), restated(a, *args), (shape, args[1:]))
    a = raster(rng, dt, (37, 53))
    nv16 = [v.item() for v in np.unique(a[np.isfinite(a)])[:16]]
    check_range(device_range(form, a, None, nv16, None, percents=(0, 33.3, 50, 99.5, 100)), restated(a, None, nv16, None, percents=(0, 33.3, 50, 99.5, 100)))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", G.DTYPES)
def test_window_of_a_poisoned_buffer(form, dt):
    """A 61 x 200 window at column offset 3 of a 64 x 211 buffer, the mask a window at another pitch."""
    rng = np.random.default_rng(9)
    buf = np.full((64, 211), 7777 if dt != "uint8" else 201, dt)
    if dt == "float32":
        buf[:] = f32(1e30)
    mbuf = np.full((64, 230), 255, np.uint8)
    mbuf[:, ::2] = 0
    a = buf[2:63, 3:203]
    m = mbuf[1:62, 5:205]
    a[:] = raster(rng, dt, (61, 200))
    m[:] = (rng.random((61, 200)) < 0.7).astype(np.uint8)
    nv, nd = [a[5, 5].item(), 0], a[8, 8].item()
    want = restated(a, m, nv, nd)
    if form == "dev":
        got = ops.display_range(to_dev(buf)[2:63, 3:203], to_dev(mbuf)[1:62, 5:205], nv, nd)
    else:
        got = ops.display_range(a, m, nv, nd)
    check_range(got, want)
    assert want.n_valid > 5000 and want.n_invalid > 3000


def test_more_than_one_sweep_of_the_grid():
    """2100 x 2100 uint16: more than 2048 workgroups x 256 lanes x 8 sixteen-bit elements; dense on the device, and a window."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 12000, (2100, 2100)).astype(np.uint16)
    a[rng.random(a.shape) < 0.1] = 0
    mask = (rng.random(a.shape) < 0.8).astype(np.uint8)
    nv = [17, 4000, 11999]
    want = restated(a, mask, nv, 5)
    d, dm = to_dev(a), to_dev(mask)
    first = ops.display_range(d, dm, nv, 5)
    check_range(first, want)
    again = ops.display_range(d, dm, nv, 5)                      # the same call twice: the same bits
    assert (again.values, again.n_valid, again.n_invalid) == (first.values, first.n_valid, first.n_invalid)
    check_range(ops.display_range(d[1:, 1:], dm[1:, 1:], nv, 5), restated(a[1:, 1:], mask[1:, 1:], nv, 5))
    # km_order_statistics on the same raster is what it was: every pixel, no predicate
    n, v0, _v1, _vi = ops.order_statistics(a, [0.0, 1.0])
    assert n == a.size and (v0[0], v0[1]) == (a.min(), a.max())


@pytest.mark.parametrize("form", FORMS)
def test_few_valid_pixels_and_float_specials(form):
    for dt in G.DTYPES:
        for n_valid in (1, 2):
            a = np.zeros((5, 300), dt)
            a.ravel()[[7, 900][:n_valid]] = [3, 100][:n_valid]
            check_range(device_range(form, a), restated(a), (dt, n_valid))
    a = np.array([[np.nan, -0.0, 0.0, np.inf], [-np.inf, 2.5, -7.25, np.nan]], f32)
    check_range(device_range(form, a), restated(a))
    check_range(device_range(form, a, None, [0, 2.5], float("nan")), restated(a, None, [0, 2.5], float("nan")))
    nan = np.full((3, 70), np.nan, f32)
    got = device_range(form, nan)
    check_range(got, restated(nan))
    assert got.n_valid == 0 and np.isnan(got.v_min) and np.isnan(got.v_max)
    weak = np.full((2, 9), f32(0.1), f32)                        # a Python float compares in float32, an np.float64 in float64
    assert device_range(form, weak, nodata=0.1).n_invalid == 18 and device_range(form, weak, nodata=np.float64(0.1)).n_invalid == 0


def test_c_abi_refuses_a_longer_list():
    from karios_amd._lib import KariosHipError, default_context
    import ctypes as C
    c = default_context()
    a = np.ones((4, 4), np.uint16)
    nv = np.arange(17, dtype=np.float64)
    q = np.array([0.5])
    out = np.zeros(3)
    pd_ = C.POINTER(C.c_double)
    res = ops._lib.DisplayRangeResult()
    rc = c.lib.km_display_range(c.handle, a.ctypes.data_as(C.c_void_p), 1, 4, 4, 4, None, 0, None, nv.ctypes.data_as(pd_), 17, 1, q.ctypes.data_as(pd_),
                                C.byref(res), out[0:].ctypes.data_as(pd_), out[1:].ctypes.data_as(pd_), out[2:].ctypes.data_as(pd_))
    assert rc == ops._lib.E_ARG
    with pytest.raises(KariosHipError, match="at most 16"):
        c.check(rc, "km_display_range")


# ---- mean profiles ------------------------------------------------------------------------------------------------------------------------
def columns(rng, n, odd=True):
    v = (rng.standard_normal(n) * 10.0 ** rng.integers(-2, 4)).astype(f32)
    p = (rng.random(n) * 3000 - 700).astype(f32)
    if odd and n:
        for frac, x in ((0.1, np.nan), (0.01, np.inf)):
            v[rng.random(n) < frac] = f32(x)
        for frac, x in ((0.05, np.nan), (0.02, np.inf), (0.02, -np.inf), (0.03, -0.0), (0.03, -0.5)):
            p[rng.random(n) < frac] = f32(x)
    return v, p


def check_profile(got, want, what=""):
    assert got.key.shape == want.key.shape, (what, got.key.shape, want.key.shape)
    for k in ("key", "position", "mean", "std"):
        assert same(to_host(getattr(got, k)), getattr(want, k)), (what, k)
    assert same(to_host(got.count).astype(np.int64), want.count), what


def test_golden_profiles():
    for name, v, p, b in G.profile_cases():
        check_profile(ops.mean_profiles([(v, p, b)])[0], R.mean_profile(v, p, b), name)
        m = commons.mean_profile(pd.Series(v), pd.Series(p), b)
        assert same(m.mean_values.to_numpy(), GOLD[f"mean_{name}"]) and same(m.values_std.to_numpy(), GOLD[f"std_{name}"]), name
        assert same(m.nb_pos.to_numpy(), GOLD[f"count_{name}"]) and same(m.groups_positions.to_numpy(), GOLD[f"pos_{name}"]), name
        assert same(m.mean_values.index.to_numpy() + f32(0), GOLD[f"key_{name}"].astype(f32) + f32(0)), name


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 70001])
def test_profile_sizes(n):
    rng = np.random.default_rng(n + 1)
    v, p = columns(rng, n)
    for b in (1, 20):
        check_profile(ops.mean_profiles([(v, p, b)])[0], R.mean_profile(v, p, b), (n, b))


def test_one_group_and_every_row_its_own():
    rng = np.random.default_rng(77)
    v, p = columns(rng, 5000, odd=False)
    one = ops.mean_profiles([(v, np.abs(p) % f32(19), 20)])[0]
    check_profile(one, R.mean_profile(v, np.abs(p) % f32(19), 20))
    assert one.key.size == 1 and int(one.count[0]) == 5000
    own = np.arange(5000, dtype=f32)[rng.permutation(5000)] * f32(7)
    each = ops.mean_profiles([(v, own, 7)])[0]
    check_profile(each, R.mean_profile(v, own, 7))
    assert each.key.size == 5000 and np.isnan(each.std).all()


def test_eight_profiles_in_one_call_and_device_tensors():
    rng = np.random.default_rng(5)
    n = 3001
    reqs = [columns(rng, n) + (b,) for b in (1, 7, 20, 100, 20, 20, 3, 50)]
    batch = ops.mean_profiles(reqs)
    for r, got in zip(reqs, batch):
        want = R.mean_profile(*r)
        check_profile(got, want)
        check_profile(ops.mean_profiles([r])[0], want)
    dev = ops.mean_profiles([(to_dev(v), to_dev(p), b) for v, p, b in reqs[:3]])
    for r, got in zip(reqs, dev):
        assert got.key.is_cuda and got.mean.is_cuda
        check_profile(got, R.mean_profile(*r))


def test_group_outside_int32_raises():
    v = np.ones(4, f32)
    with pytest.raises(ValueError, match="outside int32"):
        ops.mean_profiles([(v, np.array([1, 2, 3e12, 4], f32), 20)])
    with pytest.raises(ValueError, match="outside int32"):
        ops.mean_profiles([(v, v, 20), (v, np.array([1, 2, -4e10, 4], f32), 20)])
    assert ops.mean_profiles([(v, np.array([1, 2, 1e9, 4], f32), 2)])[0].key.size == 4


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matched_pair():
    mon, ref = synth.make_pair(403, 640, 0.5, 0.0)
    mask = np.full(mon.shape, 255, np.uint8)
    mask[:40, :] = 0
    mask[200:230, 100:400] = 0
    nd_mon, nd_ref = mon[10, 10].item(), ref[300, 300].item()
    pair = ResidentPair.upload(mon, ref, mask, no_data_mon=nd_mon, no_data_ref=nd_ref)
    frame = pair.match_tile(KLTConfiguration())
    assert frame is not None and len(frame) > 300
    return mon, ref, mask, pair, frame


def numpy_plot_range(a, mask, no_values, nodata):
    """OverviewPlot._build_invalid_mask + _plot_image evaluated by numpy on the host copies."""
    invalid = np.zeros(a.shape, bool) if mask is None else mask == 0
    if no_values:
        invalid = invalid | np.isin(a, no_values)
    if nodata is not None:
        invalid = invalid | (a == nodata)
    valid = a[np.isfinite(a) & (a != 0) & ~invalid]
    assert len(valid) > 0
    return np.percentile(valid, 0.5), np.percentile(valid, 99.5), len(valid), int(invalid.sum())


def test_end_to_end_pair():
    mon, ref, mask, pair, frame = matched_pair()
    no_values = [mon[50, 50].item(), ref[60, 60].item(), 0]
    got_mon, got_ref = overview.display_ranges(pair, no_values)
    for got, a, m, nd in ((got_mon, mon, mask, pair.no_data_mon), (got_ref, ref, None, pair.no_data_ref)):
        vmin, vmax, n_valid, n_invalid = numpy_plot_range(a, m, no_values, nd)
        assert same(got.v_min, vmin) and same(got.v_max, vmax) and (got.n_valid, got.n_invalid) == (n_valid, n_invalid)
        assert same(got.raster_min, a.min()) and same(got.raster_max, a.max())
    assert got_mon.n_invalid > 40 * 640 and got_ref.n_invalid < got_mon.n_invalid
    # the four row / column profiles of the report, in one call and one by one, against pandas on the frame
    import karios_amd.report.commons as C_
    reqs = [(frame[val].to_numpy(), frame[pos].to_numpy(), 20) for val in ("dx", "dy") for pos in ("x0", "y0")]
    assert all(v.dtype == f32 and p.dtype == f32 for v, p, _b in reqs)
    batch = C_.mean_profiles(reqs)
    for (val, pos), got in zip([(val, pos) for val in ("dx", "dy") for pos in ("x0", "y0")], batch):
        group = pd.DataFrame.from_dict({"val": frame[val], "po": np.floor_divide(frame[pos], 20)}).groupby("po")
        want_pos = (group["po"].first() * 20 + 20 // 2).astype(np.int32)
        single = commons.mean_profile(frame[val], frame[pos], 20)
        for m in (got, single):
            assert same(m.groups_positions.to_numpy(), want_pos.to_numpy()) and m.groups_positions.dtype == np.int32
            assert same(m.mean_values.to_numpy(), group["val"].mean().to_numpy()) and same(m.values_std.to_numpy(), group["val"].std().to_numpy())
            assert same(m.nb_pos.to_numpy(), group["val"].count().to_numpy()) and m.nb_pos.dtype == np.int64
            assert same(m.mean_values.index.to_numpy(), want_pos.index.to_numpy().astype(f32))
        assert got.grouped_values.ngroups == len(want_pos) and len(got.compute_std_min_max()[0]) == len(want_pos)
