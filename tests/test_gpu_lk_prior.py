"""GPU suite: the tracker under a geometric prior - km_pyrlk_initial, km_prior_mask[_dev] and
km_klt_tile_frame_prior_dev against tests/lk_prior_restatement.py, bit for bit; inputs in tests/lk_prior_cases.py (192 x 160 at most).

The restatement is pinned to the CPU oracle by tests/test_lk_prior_host.py.  Here: explicit guesses through the seeded kernels (winSize 25:
the compile-time form; 21 and 31: the generic form with 2 and 4 runs per lane), the frame entry point (mask under the prior, guesses from
the prior in the kernel's prologue, forward / backward in one launch, frame block, ZNCC column), the identity prior against the unseeded
entry points GPU against GPU, the mask kernel, and the refusals.
"""
import ctypes as C_

import numpy as np
import pytest

import frame_restatement as FR
import lk_cases as LC
import lk_prior_cases as C
import lk_prior_restatement as PR

pytestmark = pytest.mark.gpu

KSIZE = 5
THRESHOLD = 0.4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    bad = (_bits(got) != _bits(want)).reshape(len(want), -1).any(1) if len(want) else np.zeros(0, bool)
    if bad.any():
        k = int(np.argmax(bad))
        pytest.fail(f"{what}: {int(bad.sum())} of {len(want)} rows differ from the restatement; first: row {k} got {got[k].ravel()!r} expected {want[k].ravel()!r}",
                    pytrace=False)


# ---- km_pyrlk_initial: explicit guesses -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", C.WINDOWS)
def test_explicit_guesses_against_the_restatement(ops, win):
    """Every guess case of a window size in ONE launch (the cases are rows of one list), in both directions of the pair: integer and
    fractional guesses, the odd shift, search windows across each border, level-1 origins at -win and -win - 1, guesses 3 and 4 px from
    the key point, a search that re-centres, templates at the rim."""
    ref, mon = C.pair(7, 3)
    cases = C.guess_cases(win)
    pts = np.concatenate([p for _, p, _ in cases])
    guesses = np.concatenate([g for _, _, g in cases])
    names = [n for n, p, _ in cases for _ in range(len(p))]
    for a, b, label in ((ref, mon, "ref -> mon"), (mon, ref, "mon -> ref")):
        want = PR.pyr_lk_initial(a, b, pts, guesses, win).reshape(-1, 2)
        got = ops.pyrlk_initial(a, b, pts, guesses, winSize=(win, win)).reshape(-1, 2)
        bad = np.flatnonzero((_bits(got) != _bits(want)).any(1))
        assert bad.size == 0, (f"winSize {win} {label}: {bad.size} of {len(pts)} rows differ; first: case '{names[bad[0]]}' point {pts[bad[0]]} guess "
                               f"{guesses[bad[0]]} got {got[bad[0]]!r} expected {want[bad[0]]!r}")
    # what the cases are there for (CPU facts about the last direction's expectation)
    moved = np.abs(want - guesses).max(1)
    assert (moved > 3).any() and (moved == 0).any()                    # a search that left its patch; a point left at its guess


# ---- km_klt_tile_frame_prior_dev ------------------------------------------------------------------------------------------------------------
def _content(name, shift):
    ref, mon = C.pair(*shift)
    if name == "holes":
        ref, mon = ref.copy(), mon.copy()
        mon[70:96, 108:140] = 0                                        # no data: corners whose guess lands here are not selected
        ref[40:52, 60:80] = 0
    return ref, mon


def _expected_frame(O, ref, mon, P, box, win, conf, base=None):
    """The frame block's content by the restatement (stages in front of the tracker by the CPU oracle)."""
    x, y, w, h = box if box else (0, 0, ref.shape[1], ref.shape[0])
    rb, mb = ref[y:y + h, x:x + w], mon[y:y + h, x:x + w]
    m = PR.mask(rb, mb, P, base=None if base is None else base[y:y + h, x:x + w], x_off=x, y_off=y)
    lr, lm = O.laplacian_u8(O.to_uint8(rb), KSIZE), O.laplacian_u8(O.to_uint8(mb), KSIZE)
    p0 = O.good_features(lr, m, conf.maxCorners, conf.qualityLevel, conf.minDistance, conf.blocksize)
    if p0 is None:
        return None, m
    g, ok = PR.guess(P, p0, x, y)
    assert ok.all()
    p1, p0r = PR.track_fb(lr, lm, p0, g, win)
    frame, rows, n_init = FR.frame_of_tracks(p0, p1, p0r, len(p0), x, y, conf.maxCorners, conf.maxCorners)
    z = np.full(rows, np.nan)
    keep = frame["score"].to_numpy() >= np.float32(THRESHOLD)
    if keep.any():
        z[keep] = O.zncc_batch(ref, mon, *(frame[c].to_numpy()[keep] for c in ("x0", "y0", "dx", "dy")))
    frame["zncc_score"] = z
    st = PR.fb_columns(p0, p1, p0r)[1] < 0.1                          # the rows the cut kept, in corner order: the frame's labels index them
    frame.attrs.update(Ninit=n_init, prior=((g[:, 0] - p0[:, 0, 0])[st], (g[:, 1] - p0[:, 0, 1])[st]))
    return frame, m


def _assert_frame(got, want, what, pair):
    """The float32 columns, the labels and Ninit against the restatement, bit for bit.  The ZNCC column is the library's existing score
    kernel, which this suite holds to the oracle within 1e-9 and not to the bit (tests/test_gpu_parity.py::test_zncc_matches_oracle): the
    column must be THAT kernel's value on the same rows of the raw rasters, bit for bit (`pair.zncc`: km_zncc_batch_dev, scored at
    round(x0 + dx)), NaN exactly where score < threshold, and within that 1e-9 of the oracle's value."""
    assert got is not None, f"{what}: no frame"
    FR.assert_same_frame(got[list(FR.COLUMNS)], want[list(FR.COLUMNS)], what)
    a, b = got["zncc_score"].to_numpy(), want["zncc_score"].to_numpy()
    keep = want["score"].to_numpy() >= np.float32(THRESHOLD)
    assert a.dtype == np.float64 and np.array_equal(np.isnan(a), np.isnan(b)) and np.isnan(a[~keep]).all(), f"{what}: zncc_score: rows scored"
    if keep.any():
        again = pair.zncc(*(want[c].to_numpy()[keep] for c in ("x0", "y0", "dx", "dy")))
        assert a[keep].tobytes() == np.asarray(again, np.float64).tobytes(), f"{what}: zncc_score differs from the score kernel's on the same rows"
        assert np.nanmax(np.abs(a[keep] - b[keep])) <= 1e-9, f"{what}: zncc_score against the oracle"
    assert got.attrs["Ninit"] == want.attrs["Ninit"], what


@pytest.mark.parametrize("win", C.WINDOWS)
def test_frame_under_a_prior_against_the_restatement(ops, O, win):
    from karios_amd.core import KLTConfiguration
    from karios_amd.matcher import prior as prior_mod
    from karios_amd.resident import ResidentPair
    conf = KLTConfiguration(maxCorners=C.MAX_CORNERS, matching_winsize=win, laplacian_kernel_size=KSIZE)
    facts = []
    for name, shift, P, box in C.frame_priors() + [("holes", (7, 3), PR.shift_prior(7, 3), None)]:
        ref, mon = _content(name, shift)
        want, _ = _expected_frame(O, ref, mon, P, box, win, conf)
        pair = ResidentPair.upload(mon, ref, ctx=ops._lib.default_context())
        got = pair.match_tile(conf, box=box, zncc_threshold=THRESHOLD, prior=P)
        _assert_frame(got, want, f"{name}, winSize {win}", pair)
        # the two columns behind the reference's: the float32 g - p0 of every row
        order = np.asarray(want.index)
        _assert_same(got["dx_prior"].to_numpy(), want.attrs["prior"][0][order], f"{name}: dx_prior")
        _assert_same(got["dy_prior"].to_numpy(), want.attrs["prior"][1][order], f"{name}: dy_prior")
        facts.append((name, want.attrs["Ninit"], len(want), int(np.isfinite(want["zncc_score"]).sum())))
    print(facts)
    assert all(n_init >= 20 and rows >= 5 and scored >= 5 for _, n_init, rows, scored in facts)
    assert any(rows < n_init for _, n_init, rows, _ in facts)          # (a case where the forward-backward cut drops rows)


def test_user_mask_under_a_prior(ops, O):
    """base = the user mask (a window of a wider buffer on the device side is the pair's own business: here dense)."""
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair
    ref, mon = C.pair(7, 3)
    base = np.zeros(ref.shape, np.uint8)
    base[20:140, 30:170] = 3
    base[60:80, 80:120] = 0
    conf = KLTConfiguration(maxCorners=C.MAX_CORNERS, matching_winsize=25, laplacian_kernel_size=KSIZE)
    P = PR.shift_prior(7, 3)
    want, m = _expected_frame(O, ref, mon, P, None, 25, conf, base=base)
    pair = ResidentPair.upload(mon, ref, base, ctx=ops._lib.default_context())
    got = pair.match_tile(conf, zncc_threshold=THRESHOLD, prior=P)
    _assert_frame(got, want, "user mask", pair)
    x, y = got["x0"].to_numpy().astype(int), got["y0"].to_numpy().astype(int)
    assert (base[y, x] != 0).all()


# ---- the identity prior, GPU against GPU ----------------------------------------------------------------------------------------------------
def test_identity_guesses_equal_the_unseeded_tracker_on_the_lk_fixtures(ops):
    """`pyrlk_initial(pts, pts)` against `calc_optical_flow_pyr_lk(pts)` on the existing LK cases the seeded form serves (two-level
    pyramids): saturated contrast, the eigenvalue cut, degenerate and negative weights - every window size from 25 to 40."""
    n = 0
    for case_id in LC.case_ids():
        case = LC.case(case_id)
        h, w = case.prev.shape
        if (w + 1) // 2 <= case.win or (h + 1) // 2 <= case.win:
            continue
        want = ops.calc_optical_flow_pyr_lk(case.prev, case.next, case.pts, winSize=(case.win, case.win))
        got = ops.pyrlk_initial(case.prev, case.next, case.pts, case.pts, winSize=(case.win, case.win))
        _assert_same(got.reshape(-1, 2), want.reshape(-1, 2), f"{case} identity guesses")
        n += 1
    assert n >= 30


@pytest.mark.parametrize("win", [25, 31])
def test_identity_prior_equals_the_unseeded_frame(ops, win):
    from karios_amd.core import KLTConfiguration
    from karios_amd.matcher import prior as prior_mod
    from karios_amd.resident import ResidentPair
    conf = KLTConfiguration(maxCorners=60, matching_winsize=win, laplacian_kernel_size=KSIZE)
    for name, (ref, mon), box in (("texture", C.pair(2, -1), None), ("texture box", C.pair(2, -1), (16, 8, 168, 148)), ("holes", _content("holes", (0, 0)), None)):
        pair = ResidentPair.upload(mon, ref, ctx=ops._lib.default_context())
        want = pair.match_tile(conf, box=box, zncc_threshold=THRESHOLD)
        got = pair.match_tile(conf, box=box, zncc_threshold=THRESHOLD, prior=prior_mod.IDENTITY)
        assert want is not None and len(want) >= 10
        FR.assert_same_frame(got[list(FR.COLUMNS)], want[list(FR.COLUMNS)], f"{name} winSize {win}")
        assert got["zncc_score"].to_numpy().tobytes() == want["zncc_score"].to_numpy().tobytes()
        assert not got["dx_prior"].to_numpy().any() and not got["dy_prior"].to_numpy().any()


# ---- the mask kernel ------------------------------------------------------------------------------------------------------------------------
def test_mask_kernel_against_the_restatement(ops):
    for case in C.mask_cases():
        want = PR.mask(case["ref"], case["mon"], case["prior"], case["base"], case["nodata_ref"], case["nodata_mon"], case["x_off"], case["y_off"])
        got = ops.prior_mask(case["ref"], case["mon"], case["prior"], mask=case["base"], nodata_ref=case["nodata_ref"], nodata_mon=case["nodata_mon"],
                             x_off=case["x_off"], y_off=case["y_off"])
        assert got.dtype == np.uint8 and np.array_equal(got, want), f"{case['name']}: {int((got != want).sum())} bytes differ"


def test_mask_kernel_on_device_tensors_and_a_larger_raster(ops):
    """Device tensors in, a device tensor out (windows of wider tensors: row strides), and the 192 x 160 content under a 3 degree rotation."""
    import torch
    dev = torch.device("cuda", 0)
    ref, mon = C.pair(7, 3)
    P = C.rotation_prior(3.0, sx=7, sy=3)
    want = PR.mask(ref, mon, P, x_off=5, y_off=9)
    assert 0 < want.sum() < want.size
    wide = lambda a: torch.as_tensor(np.pad(a, ((0, 0), (0, 13))), device=dev)[:, :a.shape[1]]
    got = ops.prior_mask(wide(ref), wide(mon), P, x_off=5, y_off=9)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    case = next(c for c in C.mask_cases() if c["name"] == "uint16 rotation 3 deg")
    want = PR.mask(case["ref"], case["mon"], case["prior"], case["base"], case["nodata_ref"], case["nodata_mon"], case["x_off"], case["y_off"])
    t = lambda a: torch.as_tensor(a.view(np.int16) if a.dtype == np.uint16 else a, device=dev)
    got = ops.prior_mask(t(case["ref"]), t(case["mon"]), case["prior"], mask=wide(case["base"]), nodata_ref=case["nodata_ref"], nodata_mon=case["nodata_mon"],
                         x_off=case["x_off"], y_off=case["y_off"], dtype=np.uint16)
    assert np.array_equal(got.cpu().numpy(), want)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing(ops):
    """Every refusal returns its code, leaves the context clean (km_ctx_sync) and the next unseeded call returns its usual bits."""
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair
    lib_mod = ops._lib
    c = lib_mod.default_context()
    ref, mon = C.pair(7, 3)
    pts = C.guess_cases(25)[0][1]
    usual = ops.calc_optical_flow_pyr_lk(ref, mon, pts, winSize=(25, 25))
    conf = KLTConfiguration(maxCorners=C.MAX_CORNERS, matching_winsize=25, laplacian_kernel_size=KSIZE)
    pair = ResidentPair.upload(mon, ref, ctx=c)
    usual_frame = pair.match_tile(conf, zncc_threshold=THRESHOLD)
    P = PR.shift_prior(7, 3)

    def after(what):
        assert c.lib.km_ctx_sync(c.handle) == 0, what
        assert np.array_equal(_bits(ops.calc_optical_flow_pyr_lk(ref, mon, pts, winSize=(25, 25))), _bits(usual)), what
        again = pair.match_tile(conf, zncc_threshold=THRESHOLD)
        FR.assert_same_frame(again[list(FR.COLUMNS)], usual_frame[list(FR.COLUMNS)], what)

    p = lambda a: a.ctypes.data_as(C_.c_void_p)
    out = np.empty_like(pts)

    def initial(a, b, guesses, win, max_level, points=pts):
        return c.lib.km_pyrlk_initial(c.handle, p(a), p(b), a.shape[0], a.shape[1], p(points), p(guesses), len(points), win, max_level, 30, 0.03, p(out))
    small = np.ascontiguousarray(ref[:60, :60])
    bad = pts.copy()
    bad[1, 0] = np.nan
    for what, rc, want in (("maxLevel 2", initial(ref, mon, pts, 25, 2), lib_mod.E_UNSUPPORTED), ("maxLevel 0", initial(ref, mon, pts, 25, 0), lib_mod.E_UNSUPPORTED),
                           ("winSize 41", initial(ref, mon, pts, 41, 1), lib_mod.E_UNSUPPORTED), ("no level 1", initial(small, small, pts, 31, 1), lib_mod.E_UNSUPPORTED),
                           ("winSize 2", initial(ref, mon, pts, 2, 1), lib_mod.E_ARG), ("maxLevel -1", initial(ref, mon, pts, 25, -1), lib_mod.E_ARG),
                           ("a guess that is not finite", initial(ref, mon, bad, 25, 1), lib_mod.E_ARG),
                           ("a point that is not finite", initial(ref, mon, pts, 25, 1, points=bad), lib_mod.E_ARG)):
        assert rc == want, f"{what}: {rc}"
        after(what)
    # "lk2" 0: the first form stays unseeded
    c.set_option("lk2", 0)
    try:
        assert initial(ref, mon, pts, 25, 1) == lib_mod.E_UNSUPPORTED
    finally:
        c.set_option("lk2", 1)
    after("lk2 0")
    # the frame entry point
    with pytest.raises(lib_mod.KariosHipError, match="frame_clip"):
        c.set_option("frame_clip", 1)
        try:
            pair.match_tile(conf, zncc_threshold=THRESHOLD, prior=P)
        finally:
            c.set_option("frame_clip", 0)
    after("frame_clip 1")
    with pytest.raises(lib_mod.KariosHipError, match="window"):
        c.check(c.lib.km_set_image_window(c.handle, 0, 0, 400, 400), "km_set_image_window")
        try:
            pair.match_tile(conf, zncc_threshold=THRESHOLD, prior=P)
        finally:
            c.lib.km_set_image_window(c.handle, 0, 0, 0, 0)
    after("image window")
    with pytest.raises(lib_mod.KariosHipError, match="two-level"):
        pair.match_tile(conf, box=(0, 0, 50, 160), zncc_threshold=THRESHOLD, prior=P)           # (50 + 1) / 2 <= 25: no level 1
    after("box without level 1")
    with pytest.raises(ValueError):
        pair.match_tile(conf, zncc_threshold=THRESHOLD, prior=np.r_[P[:8], np.nan])
    nan_prior = np.r_[P[:8], np.nan]
    rc = c.lib.km_prior_mask(c.handle, p(ref), p(mon), 0, ref.shape[0], ref.shape[1], ref.shape[1], ref.shape[1], None, 0, None, None,
                             nan_prior.ctypes.data_as(C_.POINTER(C_.c_double)), 0.0, 0.0, p(np.empty(ref.shape, np.uint8)))
    assert rc == lib_mod.E_ARG
    after("a prior that is not finite")
    # the outlier clip under a prior runs on the residuals, behind the frame, with "frame_clip" off
    clipped = pair.match_tile(KLTConfiguration(maxCorners=C.MAX_CORNERS, matching_winsize=25, laplacian_kernel_size=KSIZE, outliers_filtering=True),
                              zncc_threshold=THRESHOLD, prior=P)
    assert clipped is not None and c.get_option("frame_clip", 0) == 0 and len(clipped) >= 5
    after("residual clip")


# ---- the layers above the frame -------------------------------------------------------------------------------------------------------------
def test_klt_match_tracker_and_results_under_a_prior(ops, O, tmp_path):
    """`KLT.match(..., prior=)` is the frame entry point's frame; `klt_tracker(..., prior=)` is the restatement's forward / backward on
    the corners it selects; `handle_klt_results(..., prior=)` scores although a large shift is in play and writes the two prior columns
    behind the reference's.  With the default None nothing changes (GPU against GPU)."""
    import pandas as pd
    from karios_amd import results
    from karios_amd.core import KLTConfiguration, NumpyRasterImage
    from karios_amd.matcher import KLT, klt_tracker, prior as prior_mod
    from karios_amd.resident import ResidentPair
    sx, sy = 14, -6
    ref, mon = C.pair(sx, sy)
    P = prior_mod.from_shift(sy, sx)                                   # as LargeOffsetMatcher.match() returns the pair: (row, column)
    conf = KLTConfiguration(maxCorners=C.MAX_CORNERS, matching_winsize=25, laplacian_kernel_size=KSIZE)
    pair = ResidentPair.upload(mon, ref, ctx=ops._lib.default_context())
    want = pair.match_tile(conf, prior=P)
    frames_ = list(KLT(conf).match(NumpyRasterImage(mon), NumpyRasterImage(ref), None, prior=P))
    assert len(frames_) == 1 and list(frames_[0].columns) == ["x0", "y0", "dx", "dy", "score", "dx_prior", "dy_prior"]
    pd.testing.assert_frame_equal(frames_[0], want, check_exact=True)
    assert np.abs(want["dx"].to_numpy() - sx).max() < 0.01 and np.abs(want["dy"].to_numpy() - sy).max() < 0.01        # the sign: totals
    assert (want["dx_prior"] == sx).all() and (want["dy_prior"] == sy).all()
    unseeded = list(KLT(conf).match(NumpyRasterImage(mon), NumpyRasterImage(ref), None))
    assert list(unseeded[0].columns) == ["x0", "y0", "dx", "dy", "score"]
    pd.testing.assert_frame_equal(unseeded[0], list(KLT(conf).match(NumpyRasterImage(mon), NumpyRasterImage(ref), None, prior=None))[0], check_exact=True)
    # klt_tracker on the Laplacians
    lr, lm = O.laplacian_u8(ref, KSIZE), O.laplacian_u8(mon, KSIZE)
    got, n_init = klt_tracker(lr, lm, None, conf, prior=P)
    inside = PR.mask(np.ones_like(ref), np.ones_like(mon), P)
    p0 = O.good_features(lr, inside, conf.maxCorners, conf.qualityLevel, conf.minDistance, conf.blocksize)
    g, _ = PR.guess(P, p0)
    p1, p0r = PR.track_fb(lr, lm, p0, g, 25)
    cols, _ = PR.fb_columns(p0, p1, p0r)
    assert n_init == len(p0) and len(got) == len(cols["x0"]) >= 20
    for c in FR.COLUMNS:
        _assert_same(got[c].to_numpy(), cols[c], f"klt_tracker {c}")
    # handle_klt_results
    csv = tmp_path / "points.csv"
    out = results.handle_klt_results([want.copy()], csv, pair, 0.4, large_shift_applied=True, prior=P)
    assert list(out.columns) == results.CSV_COLUMNS + ["dx_prior", "dy_prior"] and np.isfinite(out["zncc_score"]).sum() >= 20
    assert np.isfinite(out["mutual_info_score"]).sum() >= 20
    assert open(csv).readline().strip().split(";") == results.CSV_COLUMNS + ["dx_prior", "dy_prior"]
    z = O.zncc_batch(ref, mon, *(out[c].to_numpy() for c in ("x0", "y0", "dx", "dy")))
    assert np.nanmax(np.abs(out["zncc_score"].to_numpy() - z)) <= 1e-9          # on the raw rasters, at round(x0 + dx)
    # the reference's path for comparison: its scores are skipped once the raster was shifted
    skipped = results.handle_klt_results([unseeded[0].copy()], tmp_path / "shifted.csv", pair, 0.4, large_shift_applied=True)
    assert "zncc_score" not in skipped.columns
