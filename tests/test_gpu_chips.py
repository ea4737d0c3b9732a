"""GPU suite: ChipService.generate_chips on resident data (csrc/k_chips.hip) against its definition, tests/chips_restatement.py, and
the recorded results of the reference (tests/golden/chips.npz).  Every comparison is exact: row indices, written rows, names, window
centres, raw / uint8 / Laplacian chips by bytes, the text of chips.csv."""
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

import chips_restatement as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_chips as G  # noqa: E402

from karios_amd import ops, synth  # noqa: E402
from karios_amd._lib import KariosHipError, default_context  # noqa: E402
from karios_amd.core import KLTConfiguration, NumpyRasterImage  # noqa: E402
from karios_amd.report import ChipService  # noqa: E402
from karios_amd.resident import ResidentPair, forget_shared_pairs  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "chips.npz"))
f32 = np.float32
IMAGE_KEYS = ("ref_raw", "mon_raw", "ref_u8", "mon_u8", "ref_lap", "mon_lap")


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def to_host(t):
    import torch
    if t is None or isinstance(t, np.ndarray):
        return t
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def selection_cases():
    return G.selection_cases()


@functools.lru_cache(maxsize=None)
def chip_cases():
    return G.chip_cases()


def as_dict(res):
    """ops.ChipImages / report.Chips -> the restatement's dict, on the host."""
    out = {k: to_host(getattr(res, k)) for k in IMAGE_KEYS}
    out["written"] = np.asarray(to_host(res.ok if hasattr(res, "ok") else res.written), bool)
    out["windows"] = to_host(res.windows)
    return out


def same_chips(got, want, what=""):
    assert np.array_equal(got["written"], want["written"]), what
    assert np.array_equal(got["windows"], want["windows"]), what
    for key in IMAGE_KEYS:
        assert (got[key] is None) == (want[key] is None), (what, key)
        if got[key] is not None:
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (what, key)
            assert not got[key][~got["written"]].view(np.uint8).any(), (what, key)


# ---- selection -------------------------------------------------------------------------------------------------------------------------
def test_selection_golden_frames_numpy_and_device_form():
    for name, x0, y0, score, width, height in selection_cases():
        dev = [to_dev(a) for a in (x0, y0, score)]
        for tag, thr in G.THRESHOLDS:
            want = GOLD[f"sel_{name}_{tag}"]
            got = ops.select_chip_points(x0, y0, score, width, height, thr)
            assert isinstance(got, np.ndarray) and np.array_equal(got, want), (name, tag)
            got = ops.select_chip_points(*dev, width, height, thr)
            assert got.is_cuda and np.array_equal(to_host(got), want), (name, tag)


@pytest.mark.parametrize("width,height", [(640, 403), (10980, 10980)])
def test_selection_random_frames_equal_the_restatement(width, height):
    rng = np.random.default_rng(width)
    for n in (1, 2, 63, 64, 65, 1000, 70001):
        x0 = np.floor(rng.random(n) * width).astype(f32)
        y0 = (rng.random(n) * height).astype(f32)
        if n >= 63:
            x0[::5], y0[::7] = f32(width), f32(height)
            x0[3::8] = x0[2::8][:x0[3::8].size]                 # duplicate columns: ties
        score = (rng.integers(0, 65, n) / 64).astype(f32)
        for thr, grid in ((0.4, (5, 5)), (np.float64(0.4), (5, 5)), (0.4, (1, 1)), (0.25, (3, 7))):
            want = R.select(x0, y0, score, width, height, thr, grid)
            got = ops.select_chip_points(x0, y0, score, width, height, thr, grid)
            assert np.array_equal(got, want), (n, thr, grid)
            again = ops.select_chip_points(*(to_dev(a) for a in (x0, y0, score)), width, height, thr, grid)
            assert np.array_equal(to_host(again), got), (n, thr, grid)
    # nothing passes; no rows
    assert ops.select_chip_points(x0, y0, score, width, height, 2.0).size == 0
    assert ops.select_chip_points(x0[:0], y0[:0], score[:0], width, height, 0.4).size == 0


# ---- chips -----------------------------------------------------------------------------------------------------------------------------
def check_golden(got, tag):
    written = GOLD[f"written_{tag}"]
    assert np.array_equal(got["written"], written), tag
    names = [f"REF_{w[0]}_{w[1]} MON_{w[0]}_{w[1]}" for w in got["windows"]]
    assert names == list(GOLD[f"names_{tag}"]), tag
    for key in IMAGE_KEYS[2:]:
        if f"{key}_{tag}" in GOLD.files:
            assert got[key][written].tobytes() == GOLD[f"{key}_{tag}"].tobytes(), (tag, key)


@pytest.mark.parametrize("case", range(7))
def test_chips_golden_cases_numpy_and_device_form(case):
    name, ref, mon, x0, y0, dx, dy, ksizes = chip_cases()[case]
    ctx = default_context()
    for ks in ksizes:
        kr, km = R.kernel_sizes(ks)
        want = R.chips(ref, mon, x0, y0, dx, dy, ks)
        for form in ("numpy", "device"):
            args = (ref, mon, x0, y0, dx, dy) if form == "numpy" else tuple(to_dev(a) for a in (ref, mon, x0, y0, dx, dy))
            got = as_dict(ops.extract_chips(*args, kr or None, km or None))
            check_golden(got, f"{name}_{G.ktag(ks)}")
            same_chips(got, want, (name, ks, form))
        # the existing kernels agree on every written row
        for i in np.flatnonzero(got["written"]):
            for tag, k in (("ref", kr), ("mon", km)):
                u8 = ops.to_uint8(got[f"{tag}_raw"][i], ctx=ctx)
                assert np.array_equal(u8, got[f"{tag}_u8"][i])
                if k:
                    assert np.array_equal(ops.laplacian_u8(u8, k, ctx=ctx), got[f"{tag}_lap"][i])


@pytest.mark.parametrize("dt", G.DTYPES)
def test_chips_windows_of_wider_poisoned_buffers(dt):
    """97 x 131 at (5, 7) of a 110 x 150 buffer (ref) and at (2, 3) of a 101 x 141 one (mon): the padding is non-zero (NaN for float32),
    the pitches are off the 16-byte grid."""
    name, ref, mon, x0, y0, dx, dy, _ks = next(c for c in chip_cases() if c[0] == f"types_{dt}")
    bufs = []
    for a, (H, W, oy, ox) in ((ref, (110, 150, 5, 7)), (mon, (101, 141, 2, 3))):
        big = np.full((H, W), 199, a.dtype)
        if a.dtype == np.float32:
            big[:] = np.nan
        big[oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
        bufs.append((big, big[oy:oy + a.shape[0], ox:ox + a.shape[1]]))
    want = R.chips(ref, mon, x0, y0, dx, dy, {"ref": 11, "mon": 5})
    same_chips(as_dict(ops.extract_chips(bufs[0][1], bufs[1][1], x0, y0, dx, dy, 11, 5)), want, dt)
    dev = [to_dev(big)[oy:oy + 97, ox:ox + 131] for (big, _view), (oy, ox) in zip(bufs, ((5, 7), (2, 3)))]
    assert not dev[0].is_contiguous()
    same_chips(as_dict(ops.extract_chips(dev[0], dev[1], *(to_dev(a) for a in (x0, y0, dx, dy)), 11, 5)), want, dt)


@pytest.mark.parametrize("n", [0, 1, 125, 1000])
def test_chips_row_counts(n):
    _name, ref, mon, *_ = next(c for c in chip_cases() if c[0] == "types_int16")
    rng = np.random.default_rng(n)
    x0, y0 = np.floor(rng.random(n) * 131).astype(f32), np.floor(rng.random(n) * 97).astype(f32)      # most rows near a border: not written
    dx, dy = ((rng.random(n) - 0.5) * 6).astype(f32), ((rng.random(n) - 0.5) * 6).astype(f32)
    if n:
        x0[::3], y0[::3] = f32(60) + np.arange(x0[::3].size, dtype=f32) % 9, f32(45)
    want = R.chips(ref, mon, x0, y0, dx, dy, {"mon": 3})
    got = as_dict(ops.extract_chips(ref, mon, x0, y0, dx, dy, 3, 3))
    same_chips(got, want, n)
    assert got["ref_u8"].shape == (n, 57, 57) and (n < 2 or (got["written"].any() and not got["written"].all()))
    dev = ops.extract_chips(*(to_dev(a) for a in (ref, mon, x0, y0, dx, dy)), None, 3)
    assert dev.ref_lap is None
    want["ref_lap"] = None
    same_chips(as_dict(dev), want, n)


def test_chips_rasters_of_exactly_57x57_and_rows_that_are_not_finite():
    rng = np.random.default_rng(5)
    ref, mon = (rng.random((57, 57)) * 3 - 1).astype(f32), (rng.random((57, 57)) * 60000).astype(f32)
    cols = [np.array(c, f32) for c in zip((28, 28, 0.5, -0.5), (28.9, 28.2, -0.4, 0.2), (29, 28, 0, 0), (np.nan, 28, 0, 0), (28, 28, np.inf, 0),
                                          (3e9, 28, 0, 0), (28, -1e30, 0, 0))]
    want = R.chips(ref, mon, *cols, 7)
    got = as_dict(ops.extract_chips(ref, mon, *cols, 7, 7))
    same_chips(got, want)
    assert list(got["written"]) == [True, True, False, False, False, False, False]


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matched_pair():
    mon, ref = synth.make_pair(403, 640, 0.5, 0.0)
    pair = ResidentPair.upload(mon, ref)
    frame = pair.match_tile(KLTConfiguration())
    assert frame is not None and len(frame) > 500
    return mon, ref, pair, frame


def restated(frame, ref, mon, thr, ks):
    cols = {k: frame[k].to_numpy().astype(f32) for k in ("x0", "y0", "dx", "dy", "score")}
    index = R.select(cols["x0"], cols["y0"], cols["score"], ref.shape[1], ref.shape[0], thr)
    points = frame.iloc[index].astype(np.float64).reset_index(drop=True)
    return points, R.chips(ref, mon, *(cols[k][index] for k in ("x0", "y0", "dx", "dy")), ks)


def test_pair_chips_equal_the_restatement_end_to_end(tmp_path):
    mon, ref, pair, frame = matched_pair()
    ks = {"mon": 7, "ref": 5}
    points, want = restated(frame, ref, mon, 0.4, ks)
    chips = pair.chips(frame, 0.4, ks)
    assert 25 <= len(chips) <= 125 and chips.written.any()
    pd.testing.assert_frame_equal(chips.points, points, check_exact=True)
    same_chips(as_dict(chips), want)
    assert chips.names == want["names"]
    # device columns in: the same rows and chips
    import torch
    dev = pair.chips({k: torch.from_numpy(frame[k].to_numpy().astype(f32)).cuda() for k in frame.columns}, 0.4, ks)
    pd.testing.assert_frame_equal(dev.points, points, check_exact=True)
    same_chips(as_dict(dev), want)
    # the service on the resident pair: the same chips.csv as pandas writes for the restatement's frame; nothing read from the images
    class Named:
        file_name, x_size, y_size = "mon.tif", 640, 403

        @property
        def array(self):
            raise AssertionError("the image was read")
    (tmp_path / "chips").mkdir()
    (tmp_path / "chips" / "stale.txt").write_text("x")
    got = ChipService().generate_chips(Named(), Named(), frame, 0.4, output_dir=tmp_path, laplacian_ksize=ks, pair=pair)
    same_chips(as_dict(got), want)
    assert (tmp_path / "chips" / "chips.csv").read_text() == points.to_csv(sep=";", index=False)
    assert not (tmp_path / "chips" / "stale.txt").exists() and (tmp_path / "chips_laplacian" / "mon.tif").is_dir()
    # ... and without a pair, through the shared pair of the two arrays
    got = ChipService().generate_chips(NumpyRasterImage(mon), NumpyRasterImage(ref), frame, np.float64(0.4), laplacian_ksize=3)
    points, want = restated(frame, ref, mon, np.float64(0.4), 3)
    pd.testing.assert_frame_equal(got.points, points, check_exact=True)
    same_chips(as_dict(got), want)
    assert ChipService().generate_chips(NumpyRasterImage(mon), NumpyRasterImage(ref), frame, 2.0) is None
    forget_shared_pairs()


def test_argument_errors_leave_the_context_usable():
    _name, ref, mon, x0, y0, dx, dy, _ks = chip_cases()[0]
    ctx = default_context()
    import ctypes as C
    from karios_amd import _lib
    out = _lib.ChipOutputs()
    n = C.c_int32()
    idx = np.zeros(125, np.int32)

    def select(x=x0, n_rows=None, thr=0.4, rows=5, cols=5, width=131):
        return ctx.lib.km_chip_select(ctx.handle, _lib.ptr(x), _lib.ptr(y0), _lib.ptr(dx), x0.size if n_rows is None else n_rows, width, 97, thr, 0,
                                      rows, cols, _lib.ptr(idx), C.byref(n))

    def chips(r=ref, H=97, W=131, kr=3, km=3, x=x0, n_rows=None, dtype=1):
        return ctx.lib.km_chips(ctx.handle, _lib.ptr(r), _lib.ptr(mon), dtype, H, W, 97, 131, 131, 131, _lib.ptr(x), _lib.ptr(y0), _lib.ptr(dx),
                                _lib.ptr(dy), x0.size if n_rows is None else n_rows, kr, km, C.byref(out))
    for call in (lambda: select(thr=float("nan")), lambda: select(rows=0), lambda: select(cols=17), lambda: select(x=None), lambda: select(n_rows=-1),
                 lambda: select(width=0), lambda: chips(kr=2), lambda: chips(km=13), lambda: chips(H=56), lambda: chips(W=56), lambda: chips(x=None),
                 lambda: chips(n_rows=(1 << 20) + 1), lambda: chips(dtype=9), lambda: chips(r=None), lambda: chips()):       # (the last: null outputs)
        assert call() == _lib.E_ARG and ctx.lib.km_last_error(ctx.handle)
    with pytest.raises(ValueError):
        ops.extract_chips(ref[:50], mon, x0, y0, dx, dy)
    with pytest.raises(ValueError):
        ops.extract_chips(ref, mon, x0.astype(np.float64), y0, dx, dy)
    with pytest.raises(KariosHipError):
        ops.extract_chips(ref, mon.astype(np.int16), x0, y0, dx, dy)
    with pytest.raises(ValueError):
        ops.select_chip_points(x0, y0, dx, 131, 97, 0.4, grid=(0, 5))
    with pytest.raises(KariosHipError, match="NaN"):
        ops.select_chip_points(x0, y0, dx, 131, 97, float("nan"))
    # the context goes on working
    same_chips(as_dict(ops.extract_chips(ref, mon, x0, y0, dx, dy, 5, 3, ctx=ctx)), R.chips(ref, mon, x0, y0, dx, dy, {"ref": 5, "mon": 3}))
