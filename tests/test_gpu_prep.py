"""The align step's preprocessing on the MI355X against the numpy restatement (tests/prep_restatement.py): exact order statistics,
the percentile stretch and CLAHE.  Every comparison is exact (counts and order statistics equal as numbers, images bit for bit, every
pixel); every entry point is bitwise identical run to run and its _dev form on a strided device buffer equals its host form."""
from __future__ import annotations

import ctypes as C
import logging
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_restatement as R  # noqa: E402

from karios_amd import _lib, ops, results, synth  # noqa: E402
from karios_amd.matcher import global_align  # noqa: E402
from karios_amd.ops import clahe, nanpercentile, order_statistics, percentile, to_uint8_percentile  # noqa: E402,F401  (the feature's names)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (389, 517), (1098, 1096)]
DTYPES = [np.uint8, np.uint16, np.int16, np.float32]
QUANTILES = [0.0, 0.02, 0.333, 0.5, 0.98, 0.99999, 1.0]     # seven: the library takes them four at a time
GRIDS = [(8, 8), (4, 2), (16, 16)]
CLIPS = [0.0, 2.0, 40.0]


def _strided(a, pad=(3, 7)):
    """The same values as a view into a larger array (row stride > width)."""
    big = np.zeros((a.shape[0] + pad[0], a.shape[1] + pad[1]), a.dtype)
    big[1:1 + a.shape[0], 2:2 + a.shape[1]] = a
    return big[1:1 + a.shape[0], 2:2 + a.shape[1]]


def _natural(shape, seed):
    """Smooth texture + noise around 1000 .. 5000 (neighbouring pixels fall into the same coarse bins), float64."""
    H, W = shape
    base = synth.make_base(max(H, 8), max(W, 8), seed)[:H, :W].astype(np.float64)
    return base


def _rasters(dtype, shape, seed=0):
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype) if np.dtype(dtype).kind in "iu" else None
    yield "constant", np.full(shape, 77, dtype)
    levels = np.array([3, 40, 41, 100, 101, 120], dtype) if info is not None else np.array([-2.5, -0.0, 0.0, 1e-3, 7.25, 1e9], np.float32)
    yield "six-level", rng.choice(levels, shape)
    if info is not None:
        yield "full-range", rng.integers(info.min, int(info.max) + 1, shape).astype(dtype)
        yield "natural", np.clip(_natural(shape, 5) / (16 if dtype == np.uint8 else 1) - (3000 if dtype == np.int16 else 0), info.min, info.max).astype(dtype)
    else:
        yield "full-range", rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32).view(np.float32)   # every bit pattern: NaN, inf, denormals
        a = (rng.standard_normal(shape) * 900).astype(np.float32)
        for k, v in enumerate([np.nan, np.inf, -np.inf, 1e-42, -1e-42, 0.0, -0.0, 3e38, -3e38]):
            a[rng.random(shape) < 0.04] = v
        yield "special", a
        yield "natural", _natural(shape, 6).astype(np.float32) - np.float32(2500.5)
        yield "all-nan", np.full(shape, np.nan, np.float32)


def _check_stats(a, exclude, what):
    got = ops.order_statistics(a, QUANTILES, exclude)
    n, v0, v1, vi = R.order_statistics(a, QUANTILES, exclude)
    assert got[0] == n, what
    if n == 0:
        assert np.isnan(got[1]).all() and np.isnan(got[2]).all()       # left alone
        return got
    np.testing.assert_array_equal(got[1], v0, err_msg=what)             # equal as numbers (the sign of a zero is not pinned)
    np.testing.assert_array_equal(got[2], v1, err_msg=what)
    np.testing.assert_array_equal(got[3], vi, err_msg=what)
    return got


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_order_statistics_equal_restatement(dtype, shape):
    for name, a in _rasters(dtype, shape):
        for exclude in (0, 1):
            _check_stats(a, exclude, f"{name} exclude={exclude}")
            _check_stats(_strided(a), exclude, f"{name} strided exclude={exclude}")


def test_order_statistics_more_than_eight_ranks_and_none():
    a = np.random.default_rng(2).integers(0, 65536, (300, 301)).astype(np.uint16)
    qs = np.linspace(0, 1, 23)
    got = ops.order_statistics(a, qs)
    n, v0, v1, vi = R.order_statistics(a, qs)
    assert got[0] == n
    np.testing.assert_array_equal(got[1], v0)
    np.testing.assert_array_equal(got[2], v1)
    np.testing.assert_array_equal(got[3], vi)
    assert ops.order_statistics(a, [])[0] == a.size


@pytest.mark.parametrize("dtype", DTYPES)
def test_percentiles_equal_numpy(dtype):
    """ops.percentile / ops.nanpercentile: the neighbours from the GPU, numpy's interpolation in the source dtype -> np.percentile's bits."""
    qs = [0, 2, 33.3, 50, 98, 99.999, 100]
    for shape in SHAPES:
        for name, a in _rasters(dtype, shape, seed=3):
            if name == "full-range" and dtype == np.float32:
                a = np.where(np.isinf(a), np.float32(1.0), a)              # inf - inf inside numpy's lerp only adds warnings
            with np.errstate(invalid="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                exp_nan, exp = np.nanpercentile(a, qs), np.percentile(a, qs)
                got_nan, got = ops.nanpercentile(a, qs), ops.percentile(a, qs)
            for g, e in ((got_nan, exp_nan), (got, exp)):
                assert g.dtype == np.float64
                np.testing.assert_array_equal(g == g, e == e, err_msg=f"{name} {shape}")      # NaN in the same places
                np.testing.assert_array_equal(g[g == g], np.asarray(e, np.float64)[e == e], err_msg=f"{name} {shape}")
    a = np.random.default_rng(4).integers(-30000, 30001, (64, 65)).astype(np.int16)           # numpy's b - a wraps here; the port follows
    assert float(ops.percentile(a, 50.0)) == float(np.percentile(a, np.float64(50.0)))


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("shape", SHAPES + [(512, 512), (512, 389)])
def test_to_uint8_percentile_bit_identical(shape):
    for dtype in DTYPES:
        for name, a in _rasters(dtype, shape, seed=8):
            for src in (a, _strided(a)):
                _same(ops.to_uint8_percentile(src), R.to_uint8_percentile(src))
                if dtype != np.uint8:
                    n, v0, v1, vi = R.order_statistics(src.astype(np.float32), [0.02, 0.98], 1)
                    lo, hi = R.lerp(v0, v1, vi, n, np.float32) if n else (np.nan, np.nan)
                    _same(ops.stretch_percentile_u8(src, lo, hi), R.stretch_u8(src, lo, hi))
    u8 = np.arange(6, dtype=np.uint8).reshape(2, 3)
    assert ops.to_uint8_percentile(u8) is u8                                # passes through untouched
    f = np.array([[np.nan, -np.inf, np.inf, -5.0, 0.0, 1.0, 99.99, 100.0, 1e30]], np.float32)
    _same(ops.stretch_percentile_u8(f, 0.0, 100.0), np.array([[0, 0, 255, 0, 0, 2, 254, 255, 255]], np.uint8))
    _same(ops.stretch_percentile_u8(f, 5.0, 5.0), np.zeros(f.shape, np.uint8))
    _same(global_align._to_uint8(np.arange(12.0).reshape(3, 4)), R.to_uint8_percentile(np.arange(12.0).reshape(3, 4)))   # float64: astype(float32) first
    _same(global_align._to_uint8(np.arange(12, dtype=np.int32).reshape(3, 4)), R.to_uint8_percentile(np.arange(12, dtype=np.int32).reshape(3, 4)))


def _clahe_images(shape, seed):
    rng = np.random.default_rng(seed)
    yield rng.integers(0, 256, shape, dtype=np.uint8)
    yield np.clip(_natural(shape, seed) / 16 - 60, 0, 255).astype(np.uint8)
    yield np.where(rng.random(shape) < 0.7, 0, rng.integers(0, 256, shape)).astype(np.uint8)      # a nodata plateau: heavy clipping


@pytest.mark.parametrize("shape", SHAPES + [(512, 512), (512, 389)])
def test_clahe_bit_identical(shape):
    H, W = shape
    compared = 0
    for grid in GRIDS + [(1, 1)]:
        try:
            R.clahe_geometry(H, W, 2.0, grid[0], grid[1])
        except ValueError:
            with pytest.raises(_lib.KariosHipError) as e:
                ops.clahe(np.zeros(shape, np.uint8), 2.0, grid)
            assert e.value.code == _lib.E_ARG
            continue
        for k, img in enumerate(_clahe_images(shape, 21)):
            for clip in CLIPS:
                _same(ops.clahe(img, clip, grid), R.clahe(img, clip, grid))
                compared += 1
            _same(ops.clahe(_strided(img), 2.0, grid), R.clahe(img, 2.0, grid))
    assert compared >= 9


def _dev(a, pad):
    """Device copy of `a` inside a wider buffer -> (tensor keeping it alive, pointer to its first pixel, row stride in elements)."""
    import torch
    store = {np.dtype("uint16"): np.int16}.get(a.dtype, a.dtype)          # (torch has no uint16 arithmetic; only the bits travel)
    t = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=getattr(torch, np.dtype(store).name), device="cuda")
    t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a).view(store)).cuda()
    torch.cuda.synchronize()
    return t, C.c_void_p(t.data_ptr()), a.shape[1] + pad


@pytest.mark.parametrize("dtype", DTYPES)
def test_dev_forms_equal_host_forms_and_runs_repeat(dtype):
    import torch
    c = _lib.default_context()
    H, W = 389, 517
    name, a = [r for r in _rasters(dtype, (H, W), seed=12) if r[0] in ("natural",)][0]
    if dtype == np.float32:
        a = a.copy()
        a[::7, ::5] = np.nan
        a[3, 3] = np.inf
    t, p, stride = _dev(a, 11)
    q = np.ascontiguousarray(QUANTILES[:4], np.float64)
    pd = C.POINTER(C.c_double)
    for exclude in (0, 1):
        runs = []
        for _ in range(2):
            n = C.c_int64()
            v0, v1, vi = np.zeros(4), np.zeros(4), np.zeros(4)
            c.check(c.lib.km_order_statistics_dev(c.handle, p, _lib.dtype_code(a), H, W, stride, exclude, 4, q.ctypes.data_as(pd), C.byref(n),
                                                  v0.ctypes.data_as(pd), v1.ctypes.data_as(pd), vi.ctypes.data_as(pd)), "km_order_statistics_dev")
            runs.append((n.value, v0.tobytes(), v1.tobytes(), vi.tobytes()))
        assert runs[0] == runs[1]
        host = [ops.order_statistics(a, q, exclude) for _ in range(2)]
        for h in host:
            assert (h[0], h[1].tobytes(), h[2].tobytes(), h[3].tobytes()) == runs[0]
    lo, hi = ops.percentile(np.nan_to_num(a, nan=0.0, posinf=0.0), [2, 98])
    outs = []
    for _ in range(2):
        d_out = torch.full((H, W + 5), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.check(c.lib.km_stretch_percentile_u8_dev(c.handle, p, _lib.dtype_code(a), H, W, stride, float(lo), float(hi), C.c_void_p(d_out.data_ptr()),
                                                   W + 5), "km_stretch_percentile_u8_dev")
        c.sync()
        o = d_out.cpu().numpy()
        assert (o[:, W:] == 9).all()                                       # nothing written past the row
        outs.append(o[:, :W].copy())
    _same(outs[0], outs[1])
    _same(outs[0], ops.stretch_percentile_u8(a, lo, hi))
    _same(outs[0], ops.stretch_percentile_u8(a, lo, hi))
    u8 = outs[0]
    tu, pu, su = _dev(u8, 3)
    host = ops.clahe(u8, 2.0, (8, 8))
    _same(host, ops.clahe(u8, 2.0, (8, 8)))
    for _ in range(2):
        d_out = torch.full((H, W + 6), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.check(c.lib.km_clahe_dev(c.handle, pu, H, W, su, 2.0, 8, 8, C.c_void_p(d_out.data_ptr()), W + 6), "km_clahe_dev")
        c.sync()
        o = d_out.cpu().numpy()
        assert (o[:, W:] == 9).all()
        _same(o[:, :W].copy(), host)
    del t, tu


def test_argument_errors_launch_nothing():
    c = _lib.default_context()
    img = np.zeros((16, 16), np.uint8)
    out = np.zeros((16, 16), np.uint8)

    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    # CLAHE: an extension the reflection cannot define, more than 64 KB of LUTs, an empty grid, a NaN clip limit
    assert c.lib.km_clahe(c.handle, vp(img), 3, 3, 16, 2.0, 8, 8, vp(out)) == _lib.E_ARG and b"reflected border" in c.lib.km_last_error(c.handle)
    assert c.lib.km_clahe(c.handle, vp(img), 1, 16, 16, 2.0, 2, 2, vp(out)) == _lib.E_ARG
    assert c.lib.km_clahe(c.handle, vp(img), 16, 16, 16, 2.0, 32, 16, vp(out)) == _lib.E_ARG and b"LUT" in c.lib.km_last_error(c.handle)
    assert c.lib.km_clahe(c.handle, vp(img), 16, 16, 16, 2.0, 0, 8, vp(out)) == _lib.E_ARG
    assert c.lib.km_clahe(c.handle, vp(img), 16, 16, 16, float("nan"), 8, 8, vp(out)) == _lib.E_ARG
    assert c.lib.km_clahe(c.handle, vp(img), 16, 16, 8, 2.0, 8, 8, vp(out)) == _lib.E_ARG           # stride < width
    assert (out == 0).all()
    # an unsupported dtype (4 = float64 in the library's wider code list), bad quantiles, a bad exclude
    pd = C.POINTER(C.c_double)
    q = np.array([0.5]); bad = np.array([1.5])
    n = C.c_int64(-7)
    v = np.full(3, -1.0)
    args = (C.byref(n), v[0:1].ctypes.data_as(pd), v[1:2].ctypes.data_as(pd), v[2:3].ctypes.data_as(pd))
    f64 = np.zeros((16, 16))
    assert c.lib.km_order_statistics(c.handle, vp(f64), 4, 16, 16, 16, 0, 1, q.ctypes.data_as(pd), *args) == _lib.E_ARG
    assert c.lib.km_order_statistics(c.handle, vp(img), _lib.KM_U8, 16, 16, 16, 0, 1, bad.ctypes.data_as(pd), *args) == _lib.E_ARG
    assert c.lib.km_order_statistics(c.handle, vp(img), _lib.KM_U8, 16, 16, 16, 2, 1, q.ctypes.data_as(pd), *args) == _lib.E_ARG
    assert c.lib.km_stretch_percentile_u8(c.handle, vp(f64), 4, 16, 16, 16, 0.0, 1.0, vp(out)) == _lib.E_ARG
    assert n.value == -7 and (v == -1.0).all() and (out == 0).all()
    with pytest.raises(_lib.KariosHipError):
        ops.order_statistics(f64, [0.5])
    with pytest.raises(_lib.KariosHipError):
        ops.clahe(f64)


def test_preprocess_and_check_quality_at_10980(caplog):
    """_preprocess and _check_quality through the mirrors on a Sentinel-2-size uint16 raster: percentiles equal as float64, the
    preprocessed image bit-identical, every pixel compared."""
    import torch
    S = 10980
    mon_t, ref_t = synth.make_pair_torch(S, S, 0.5, 0.25, seed=20260101, device="cuda")
    torch.cuda.synchronize()
    mon = mon_t.cpu().numpy().view(np.uint16)
    ref = ref_t.cpu().numpy().view(np.uint16)
    del mon_t, ref_t

    class Img:
        def __init__(self, a):
            self.array = a

    with caplog.at_level(logging.WARNING, logger="karios_amd.results"):
        mm_mon, mm_ref = results._check_quality(Img(mon), Img(ref))
    mine = lambda: [r.getMessage() for r in caplog.records if r.name == "karios_amd.results"]   # noqa: E731
    assert not mine()                                                   # a textured scene: no low-dynamic-range warning
    for got, a in ((mm_mon, mon), (mm_ref, ref)):
        exp = R.percentile(a, [2, 98])
        assert got.dtype == np.float64 and got.tobytes() == exp.tobytes()
    assert mm_mon.tobytes() == np.nanpercentile(mon, [2, 98]).tobytes()
    got = global_align._preprocess(mon)
    exp = R.preprocess(mon)
    _same(got, exp)
    _same(global_align._preprocess(mon), got)                           # and again: bitwise repeatable
    # the warning fires on a flat raster, and an all-NaN raster gives NaN as numpy does
    flat = np.full((64, 64), 1234, np.uint16)
    with caplog.at_level(logging.WARNING, logger="karios_amd.results"):
        results._check_quality(Img(flat), Img(ref[:64, :64]))
    assert mine() == ["Low dynamic range detected for monitored, you could get poor results"]
    assert np.isnan(results._dynamic_range(Img(np.full((8, 8), np.nan, np.float32)))).all()
    f64 = np.random.default_rng(1).random((40, 50)) * 1000                # float64: numpy's own
    assert results._dynamic_range(Img(f64)).tobytes() == np.nanpercentile(f64, [2, 98]).tobytes()
