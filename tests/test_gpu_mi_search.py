"""GPU suite: the mutual-information search around each key point (csrc/k_mi_search.hip) held to its definition,
tests/mi_search_restatement.py, on the shared case list (tests/mi_search_cases.py: rasters given as windows of wider buffers, radius
1 / 4 / 8, all four pixel types, up to 64 rows with rim crossings, skipped rows, constant chips, extreme pixels that enter and leave the
chip, non-finite samples, period-4 ties and peaks on the rim): every output of every row byte for byte, no tolerance, for the
host-memory and the device-memory form.  What the definition itself is checked against: tests/test_mi_search_host.py."""
import numpy as np
import pandas as pd
import pytest

import mi_search_cases as M
import mi_search_restatement as R

from karios_amd import results, synth  # noqa: E402
from karios_amd._lib import KariosHipError  # noqa: E402
from karios_amd.core import KLTConfiguration, NumpyRasterImage  # noqa: E402
from karios_amd.matcher import KLT, MutualInfoService  # noqa: E402
from karios_amd.resident import MI_SEARCH_COLUMNS, ZNCC_SEARCH_COLUMNS, ResidentPair  # noqa: E402
from test_gpu_report import to_dev, to_host  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = M.cases()


@pytest.fixture(scope="module")
def expected():
    """name -> (the case's arrays, the restatement's Result), computed once."""
    return {c.name: (M.build(c), R.search(*M.build(c), c.radius)) for c in CASES}


def window_to_dev(a):
    """The same window of the same wider buffer, on the device."""
    base = a.base if a.base is not None else a
    first = (a.ctypes.data - base.ctypes.data) // a.itemsize
    return to_dev(base)[:, first:first + a.shape[1]]


def search(ops, form, arrays, radius, surface=True):
    ref, mon, *cols = arrays
    if form == "device":
        import torch
        got = ops.mi_search(window_to_dev(ref), window_to_dev(mon), *(torch.from_numpy(c).cuda() for c in cols), radius=radius, surface=surface)
        assert all(t is None or t.is_cuda for t in got)
        return type(got)(*(None if t is None else to_host(t) for t in got))
    got = ops.mi_search(ref, mon, *cols, radius=radius, surface=surface)
    assert all(t is None or isinstance(t, np.ndarray) for t in got)
    return got


@pytest.mark.parametrize("form", ("numpy", "device"))
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_equal_the_restatement_byte_for_byte(ops, expected, form, case):
    arrays, want = expected[case.name]
    assert arrays[0].strides[0] // arrays[0].itemsize % 2 == 1           # an odd row stride
    got = search(ops, form, arrays, case.radius)
    S = 2 * case.radius + 1
    assert got.surface.shape == (case.n, S, S) and got.offset.shape == (case.n, 2)
    M.assert_matches(case, want, got)
    if case.n == 5:                                                      # without the surface: the same rows
        M.assert_matches(case, want, search(ops, form, arrays, case.radius, surface=False), surface=False)


@pytest.mark.parametrize("name", ["u16_texture_r4_n64", "u8_texture_r1_n64", "i16_texture_r4_n40", "f32_texture_r4_n40", "u16_fullrange_r4_n5", "f32_binary_r1_n5"])
def test_centre_of_the_surface_is_the_mutual_info_score(ops, expected, name):
    """The surface's centre against km_mi_batch_dev on the same rows, within 1e-9: the gate that kernel is held to."""
    import torch
    case = next(c for c in CASES if c.name == name)
    (ref, mon, *cols), want = expected[name]
    n = case.n
    st, nmi = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    d_ref, d_mon, d_cols = window_to_dev(ref), window_to_dev(mon), [torch.from_numpy(c).cuda() for c in cols]
    ctx = ops.default_context()
    torch.cuda.synchronize()
    ctx.check(ctx.lib.km_mi_batch_dev(ctx.handle, d_ref.data_ptr(), d_mon.data_ptr(), ops._lib._DTYPES[ref.dtype], *ref.shape, *mon.shape,
                                      d_ref.stride(0), d_mon.stride(0), *(c.data_ptr() for c in d_cols), n, st.data_ptr(), nmi.data_ptr()), "km_mi_batch_dev")
    ctx.sync()
    st, nmi = to_host(st), to_host(nmi)
    got = search(ops, "device", (ref, mon, *cols), case.radius)
    centre = got.surface[:, case.radius, case.radius]
    assert np.array_equal(np.isnan(centre), np.isnan(st)) and np.nanmax(np.abs(centre - st)) <= 1e-9
    assert np.array_equal(np.isnan(want.surface_mi[:, case.radius, case.radius]), np.isnan(nmi))
    assert np.nanmax(np.abs(want.surface_mi[:, case.radius, case.radius] - nmi)) <= 1e-9
    at_centre = (got.offset == 0).all(axis=1) & ((got.status & 3) == 0)
    assert np.allclose(got.peak_mi[at_centre], nmi[at_centre], rtol=0, atol=1e-9)
    assert (~np.isnan(st)).sum() >= 3


def test_resident_pair_service_and_frame_columns_on_one_pair(ops, expected, tmp_path):
    case = next(c for c in CASES if c.name == "u16_texture_r4_n64")
    (ref, mon, *cols), want = expected[case.name]
    pair = ResidentPair.upload(np.ascontiguousarray(mon), np.ascontiguousarray(ref))
    M.assert_matches(case, want, pair.mi_search(*cols, radius=case.radius, surface=True))
    plain = pair.mi_search(*cols, radius=case.radius)
    assert plain.surface is None
    M.assert_matches(case, want, plain, surface=False)
    none = pair.mi_search(*(c[:0] for c in cols), radius=2, surface=True)
    assert none.surface.shape == (0, 5, 5) and none.status.shape == (0,) and none.peak_mi.shape == (0,)
    # the service: a float32 frame on one pixel type takes the kernel, on this pair's rasters
    frame = pd.DataFrame({"x0": cols[0], "y0": cols[1], "dx": cols[2], "dy": cols[3]}, index=np.arange(case.n) * 2 + 5)
    found = MutualInfoService().search(frame, NumpyRasterImage(np.ascontiguousarray(mon)), NumpyRasterImage(np.ascontiguousarray(ref)), radius=case.radius)
    assert list(found.columns) == MI_SEARCH_COLUMNS and found.index.equals(frame.index)
    assert found["mi_peak"].to_numpy().tobytes() == want.peak.tobytes() and found["mi_peak_mi"].to_numpy().tobytes() == want.peak_mi.tobytes()
    assert found[["mi_dx", "mi_dy"]].to_numpy().tobytes() == want.shift.tobytes() and np.array_equal(found["mi_status"].to_numpy(), want.status)
    assert np.array_equal(found[["mi_off_x", "mi_off_y"]].to_numpy(), want.offset)
    # the frame columns: only when asked for, behind the reference's and the ZNCC search's
    frame["score"] = np.where(np.arange(case.n) % 3 == 0, 0.2, 0.9).astype(np.float32)
    frame = frame.astype(np.float32)

    def run(name, **kw):
        csv = tmp_path / name
        return results.handle_klt_results(iter([frame.copy()]), csv, pair, 0.4, **kw), csv.read_bytes()
    base, base_csv = run("plain.csv")
    again, again_csv = run("again.csv", mi_search_radius=None)
    assert list(base.columns) == results.CSV_COLUMNS and base.equals(again) and base_csv == again_csv
    both, both_csv = run("both.csv", zncc_search_radius=2, mi_search_radius=case.radius)
    assert list(both.columns) == results.CSV_COLUMNS + ZNCC_SEARCH_COLUMNS + MI_SEARCH_COLUMNS
    assert both[results.CSV_COLUMNS].equals(base) and both_csv.splitlines()[0].decode().split(";") == list(both.columns)
    keep = (frame["score"] >= 0.4).to_numpy()
    assert both.loc[~keep, MI_SEARCH_COLUMNS].isna().all().all()
    assert np.array_equal(both.loc[keep, "mi_peak"].to_numpy(), want.peak[keep], equal_nan=True)
    assert np.array_equal(both.loc[keep, "mi_dx"].to_numpy(), want.shift[keep, 0], equal_nan=True)
    assert np.array_equal(both.loc[keep, "mi_status"].to_numpy(), want.status[keep].astype(np.float64))
    pair.window = (0, 0, M.H, M.W)                                       # the row-band mode: the pair holds a window of its rasters
    try:
        with pytest.raises(KariosHipError, match="window"):
            pair.mi_search(*cols, radius=case.radius)
    finally:
        pair.window = None


def test_window_refusal_leaves_the_context_clean(ops, expected):
    case = next(c for c in CASES if c.name == "u16_texture_r1_n5")
    (ref, mon, *cols), _want = expected[case.name]
    before = ops.mi_batch(ref, mon, *cols)
    ctx = ops.default_context()
    ctx.check(ctx.lib.km_set_image_window(ctx.handle, 0, 0, M.H, M.W), "km_set_image_window")
    try:
        with pytest.raises(KariosHipError) as e:
            ops.mi_search(ref, mon, *cols, radius=case.radius)
        assert e.value.code == -4                                        # KM_E_UNSUPPORTED
    finally:
        ctx.lib.km_set_image_window(ctx.handle, 0, 0, 0, 0)
    ctx.sync()                                                           # nothing was queued: a clean km_ctx_sync
    after = ops.mi_batch(ref, mon, *cols)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()      # km_mi_batch with its usual bits
    assert (~np.isnan(after[0])).sum() >= 3


def test_service_search_after_klt_match_equals_the_entry_point(ops):
    """The service on the frames and rasters of a KLT match (the shared resident pair): the same bits as the entry point on the same rasters.
    No accuracy claim."""
    mon, ref = synth.make_pair(256, 320, 0.4, -0.3, seed=31)
    monitored, reference = NumpyRasterImage(mon), NumpyRasterImage(ref)
    frame = pd.concat(list(KLT(KLTConfiguration(tile_size=512, maxCorners=120, laplacian_kernel_size=5)).match(monitored, reference, None)))
    frame = frame[frame["score"] >= 0.4]
    assert len(frame) > 30
    found = MutualInfoService().search(frame, monitored, reference, radius=2)
    live = found["mi_status"].to_numpy() & 3 == 0
    assert live.sum() > 20
    cols = [frame[c].to_numpy(np.float32) for c in ("x0", "y0", "dx", "dy")]
    direct = ops.mi_search(ref, mon, *cols, radius=2)
    assert found["mi_peak"].to_numpy().tobytes() == direct.peak.tobytes() and np.array_equal(found["mi_status"].to_numpy(), direct.status)
