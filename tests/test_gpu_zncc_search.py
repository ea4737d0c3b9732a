"""GPU suite: the ZNCC search around each key point (csrc/k_zncc_search.hip) held to its definition, tests/zncc_search_restatement.py, on
the shared case list (tests/zncc_search_cases.py: two raster sizes given as windows of wider buffers, radius 1 / 4 / 8, all four pixel
types, 0 / 1 / 5 / 300 rows with border crossings, skipped rows, flat windows, period-4 ties and peaks on the rim) - integer pixel
types byte for byte, float32 within the tolerances of `zncc_search_cases.assert_matches` - and to the reference's own `_zncc2` values
(tests/golden/zncc_search.npz).  What the definition itself is checked against: tests/test_zncc_search_host.py."""
import os

import numpy as np
import pandas as pd
import pytest

import zncc_search_cases as Z
import zncc_search_restatement as R

from karios_amd import results, synth  # noqa: E402
from karios_amd._lib import KariosHipError  # noqa: E402
from karios_amd.core import KLTConfiguration, NumpyRasterImage  # noqa: E402
from karios_amd.matcher import KLT, ZNCCService  # noqa: E402
from karios_amd.resident import ZNCC_SEARCH_COLUMNS, ResidentPair  # noqa: E402
from test_gpu_report import to_dev, to_host  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = Z.cases()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zncc_search.npz")


@pytest.fixture(scope="module")
def expected():
    """name -> (the case's arrays, the restatement's Result), computed once."""
    return {c.name: (Z.build(c), R.search(*Z.build(c), c.radius)) for c in CASES}


def window_to_dev(a):
    """The same window of the same wider buffer, on the device."""
    base = a.base if a.base is not None else a
    first = (a.ctypes.data - base.ctypes.data) // a.itemsize
    return to_dev(base)[:, first:first + a.shape[1]]


def search(ops, form, arrays, radius, surface=True):
    ref, mon, *cols = arrays
    if form == "device":
        import torch
        got = ops.zncc_search(window_to_dev(ref), window_to_dev(mon), *(torch.from_numpy(c).cuda() for c in cols), radius=radius, surface=surface)
        assert all(t is None or t.is_cuda for t in got)
        return R.Result(*(None if t is None else to_host(t) for t in got))
    got = ops.zncc_search(ref, mon, *cols, radius=radius, surface=surface)
    assert all(t is None or isinstance(t, np.ndarray) for t in got)
    return R.Result(*got)


@pytest.mark.parametrize("form", ("numpy", "device"))
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_equal_the_restatement(ops, expected, form, case):
    arrays, want = expected[case.name]
    assert arrays[0].strides[0] // arrays[0].itemsize % 2 == 1           # an odd row stride
    got = search(ops, form, arrays, case.radius)
    S = 2 * case.radius + 1
    assert got.surface.shape == (case.n, S, S) and got.offset.shape == (case.n, 2)
    Z.assert_matches(case, want, got)
    if case.n == 5:                                                      # without the surface: the same rows
        Z.assert_matches(case, want, search(ops, form, arrays, case.radius, surface=False), surface=False)


def test_reference_values_hold(ops):
    g = np.load(GOLDEN)
    radius = int(g["radius"])
    for tag in ("u16", "f32"):
        want = g["surface_" + tag]
        got = ops.zncc_search(g["ref_" + tag], g["mon_" + tag], *g["cols_" + tag], radius=radius, surface=True)
        assert np.array_equal(np.isnan(got.surface), np.isnan(want)), tag
        assert np.nanmax(np.abs(got.surface - want)) <= 1e-9, tag
        valued = ~np.isnan(want).all(axis=(1, 2))
        assert np.array_equal((got.status & 3) == 0, valued)
        k = np.flatnonzero(valued)
        assert np.allclose(got.peak[k], np.nanmax(want[k].reshape(len(k), -1), axis=1), rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", ["u16_128x160_r4_n300", "u8_96x120_r1_n300", "i16_128x160_r4_n300", "f32_96x120_r8_n300", "u16_extreme_r4_n5"])
def test_centre_of_the_surface_is_the_zncc_score(ops, expected, name):
    case = next(c for c in CASES if c.name == name)
    arrays, _want = expected[name]
    got = search(ops, "numpy", arrays, case.radius)
    score = ops.zncc_batch(*arrays)
    centre = got.surface[:, case.radius, case.radius]
    if np.dtype(case.dtype) != np.float32:
        assert centre.tobytes() == score.tobytes()                       # exact moments: bit for bit
    else:
        assert np.array_equal(np.isnan(centre), np.isnan(score)) and np.nanmax(np.abs(centre - score)) <= 1e-9
    assert (~np.isnan(score)).sum() > case.n // 2


def test_resident_pair_searches_and_a_windowed_pair_raises(ops, expected):
    case = next(c for c in CASES if c.name == "u16_128x160_r4_n300")
    (ref, mon, *cols), want = expected[case.name]
    pair = ResidentPair.upload(np.ascontiguousarray(mon), np.ascontiguousarray(ref))
    Z.assert_matches(case, want, R.Result(*pair.zncc_search(*cols, radius=case.radius, surface=True)))
    plain = pair.zncc_search(*cols, radius=case.radius)
    assert plain.surface is None
    Z.assert_matches(case, want, R.Result(*plain), surface=False)
    none = pair.zncc_search(*(c[:0] for c in cols), radius=2, surface=True)
    assert none.surface.shape == (0, 5, 5) and none.status.shape == (0,)
    pair.window = (0, 0, case.H, case.W)                                 # the row-band mode: the pair holds a window of its rasters
    try:
        with pytest.raises(KariosHipError, match="window"):
            pair.zncc_search(*cols, radius=case.radius)
    finally:
        pair.window = None
    ctx = ops.default_context()                                          # the entry point itself, with an image window set
    ctx.check(ctx.lib.km_set_image_window(ctx.handle, 0, 0, case.H, case.W), "km_set_image_window")
    try:
        with pytest.raises(KariosHipError) as e:
            ops.zncc_search(ref, mon, *cols, radius=case.radius)
        assert e.value.code == -4                                        # KM_E_UNSUPPORTED
    finally:
        ctx.lib.km_set_image_window(ctx.handle, 0, 0, 0, 0)


def test_service_search_after_klt_match_is_consistent_with_klt(ops):
    """Consistency only: on a synthetic pair moved by a known sub-pixel shift the correlation peak lies within half a pixel of the KLT
    displacement, away from the rim.  No accuracy claim."""
    mon, ref = synth.make_pair(256, 320, 0.4, -0.3, seed=31)
    monitored, reference = NumpyRasterImage(mon), NumpyRasterImage(ref)
    frames = list(KLT(KLTConfiguration(tile_size=512, maxCorners=300, laplacian_kernel_size=5)).match(monitored, reference, None))
    frame = pd.concat(frames)
    frame = frame[frame["score"] >= 0.4]
    assert len(frame) > 50
    service = ZNCCService()
    found = service.search(frame, monitored, reference, radius=4)
    assert list(found.columns) == ZNCC_SEARCH_COLUMNS and found.index.equals(frame.index)
    live = found["zncc_status"].to_numpy() & 3 == 0
    assert live.sum() > 40
    assert (found["zncc_status"].to_numpy()[live] == 0).all()            # rim bits clear
    assert (np.abs(found["zncc_dx"].to_numpy() - frame["dx"].to_numpy())[live] <= 0.5).all()
    assert (np.abs(found["zncc_dy"].to_numpy() - frame["dy"].to_numpy())[live] <= 0.5).all()
    # the same numbers as the entry point on the same rasters
    cols = [frame[c].to_numpy(np.float32) for c in ("x0", "y0", "dx", "dy")]
    direct = ops.zncc_search(ref, mon, *cols, radius=4)
    assert found["zncc_peak"].to_numpy().tobytes() == direct.peak.tobytes() and np.array_equal(found["zncc_status"].to_numpy(), direct.status)
    # the centre of the search is the service's own score
    score = service.compute_zncc(frame, monitored, reference).to_numpy()
    centre = ops.zncc_search(ref, mon, *cols, radius=1, surface=True).surface[:, 1, 1]
    assert centre.tobytes() == score.tobytes()


def test_handle_klt_results_adds_the_columns_only_when_asked(ops, tmp_path):
    mon, ref = synth.make_pair(256, 320, 0.4, -0.3, seed=32)
    pair = ResidentPair.upload(mon, ref)
    frames = list(KLT(KLTConfiguration(tile_size=512, maxCorners=200, laplacian_kernel_size=5)).match(NumpyRasterImage(mon), NumpyRasterImage(ref), None))
    assert frames and len(frames[0]) > 30

    def run(name, **kw):
        csv = tmp_path / name
        return results.handle_klt_results(iter(f.copy() for f in frames), csv, pair, 0.4, **kw), csv.read_bytes()

    plain, plain_csv = run("plain.csv")
    again, again_csv = run("again.csv", zncc_search_radius=None)
    assert list(plain.columns) == results.CSV_COLUMNS and plain.equals(again) and plain_csv == again_csv
    searched, searched_csv = run("searched.csv", zncc_search_radius=4)
    assert list(searched.columns) == results.CSV_COLUMNS + ZNCC_SEARCH_COLUMNS
    assert searched[results.CSV_COLUMNS].equals(plain) and searched_csv.splitlines()[0].decode().split(";") == list(searched.columns)
    keep = (plain["score"] >= 0.4).to_numpy()
    assert keep.any() and searched.loc[~keep, ZNCC_SEARCH_COLUMNS].isna().all().all() and searched.loc[keep, "zncc_status"].notna().all()
    cols = [plain[c].to_numpy(np.float32)[keep] for c in ("x0", "y0", "dx", "dy")]
    direct = pair.zncc_search(*cols, radius=4)
    assert np.array_equal(searched.loc[keep, "zncc_dx"].to_numpy(), direct.shift[:, 0], equal_nan=True)
    assert np.array_equal(searched.loc[keep, "zncc_status"].to_numpy(), direct.status.astype(np.float64))
    # the centre value of the search is the frame's zncc_score
    centre = pair.zncc_search(*cols, radius=1, surface=True).surface[:, 1, 1]
    assert np.array_equal(centre, plain["zncc_score"].to_numpy()[keep], equal_nan=True)
