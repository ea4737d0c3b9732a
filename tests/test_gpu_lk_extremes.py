"""The LK kernels (csrc/k_lk.hip, k_lk2.hip) on the fixtures of tests/lk_cases.py: saturated contrast (mismatch sums that reach 2^31 over four
neighbouring lanes), windows at the eigenvalue cut, start positions with degenerate and negative bilinear weights.  Every comparison
is `array_equal` against `oracle.pyr_lk` - forward only (`km_pyrlk`) and forward + backward in one launch (`km_klt_track` with given
corners, against the oracle's two calls) - in both forms of the kernel ("lk2" 1 / 0) and, in the resident-patch form, with the byte
pairs kept or cut again every iteration ("lk_reuse" 1 / 0).  tests/test_lk_cases_host.py proves what each fixture exercises.

Non-finite key-point coordinates are out of scope: C leaves their conversion to int undefined and the oracle has no answer."""
import numpy as np
import pytest

import lk_cases as LC

pytestmark = pytest.mark.gpu

FORMS = ({"lk2": 1, "lk_reuse": 1}, {"lk2": 1, "lk_reuse": 0}, {"lk2": 0, "lk_reuse": 1})
_expected = {}


@pytest.fixture
def lk_options(ops):
    """Sets the tracker's context options and puts the defaults back afterwards."""
    ctx = ops._lib.default_context()

    def set_form(form):
        for k, v in form.items():
            ctx.set_option(k, v)

    yield set_form
    ctx.set_option("lk2", 1)
    ctx.set_option("lk_reuse", 1)


def _oracle_tracks(O, case):
    """(p1, p0r, forward iterations per level, backward iterations per level) of the oracle, once per fixture."""
    key = str(case)
    if key not in _expected:
        p1, f0, f1 = O.pyr_lk(case.prev, case.next, case.pts, case.win, return_iters="levels")
        p0r, b0, b1 = O.pyr_lk(case.next, case.prev, p1, case.win, return_iters="levels")
        for a in (p1, p0r):
            a.setflags(write=False)
        _expected[key] = (p1, p0r, (f0.copy(), f1.copy()), (b0.copy(), b1.copy()))
    return _expected[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, f"{what}: shape {got.shape}, expected {exp.shape}"
    bad = (_bits(got) != _bits(exp)).reshape(len(exp), -1).any(1)
    if bad.any():
        k = int(np.argmax(bad))
        pytest.fail(f"{what}: {int(bad.sum())} of {len(exp)} differ from the oracle, largest difference {np.nanmax(np.abs(got - exp)):.6g}; "
                    f"first: index {k} got {got[k].ravel()} expected {exp[k].ravel()}", pytrace=False)


@pytest.mark.parametrize("case_id", LC.case_ids())
def test_fixture_matches_the_oracle_in_every_form(ops, O, lk_options, case_id):
    case = LC.case(case_id)
    p1, p0r, fwd, bwd = _oracle_tracks(O, case)
    conf = O.default_conf(maxCorners=len(case.pts), matching_winsize=case.win)
    failures = []
    for form in FORMS:
        lk_options(form)
        got = ops.calc_optical_flow_pyr_lk(case.prev, case.next, case.pts, winSize=(case.win, case.win))
        tracks = ops.klt_track(case.prev, case.next, None, conf, p0=case.pts)
        for name, g, e in (("forward", got, p1), ("one launch: p0", tracks[0], case.pts), ("one launch: p1", tracks[1], p1),
                           ("one launch: p0r", tracks[2], p0r)):
            try:
                _assert_same(g, e, f"{case} {form} {name}")
            except (AssertionError, pytest.fail.Exception) as err:
                failures.append(str(err))
        if case.cls == "cut":
            # skipped at both levels, there and back: what the skipped levels leave in nextPt is the key point itself, bit for bit
            still = (fwd[0] == 0) & (fwd[1] == 0) & (bwd[0] == 0) & (bwd[1] == 0)
            assert (_bits(tracks[1])[still] == _bits(case.pts)[still]).all() and (_bits(tracks[2])[still] == _bits(case.pts)[still]).all()
            assert (_bits(got)[still] == _bits(case.pts)[still]).all()
    assert not failures, "\n".join(failures)


def test_cut_fixtures_hold_points_that_never_move(O):
    """(what the bit-for-bit assertion above stands on: enough key points that both passes skip at both levels)"""
    n = 0
    for case in LC.cut_cases():
        _, _, fwd, bwd = _oracle_tracks(O, case)
        n += int(((fwd[0] == 0) & (fwd[1] == 0) & (bwd[0] == 0) & (bwd[1] == 0)).sum())
    assert n >= 8


def _tile_against_oracle(ops, O, ref, mon, win, max_corners):
    conf = O.default_conf(maxCorners=max_corners, matching_winsize=win, laplacian_kernel_size=LC.FRAME_KSIZE)
    exp = O.klt_tile(mon, ref, conf)
    p0 = O.good_features(exp["lap_ref"], exp["mask"], max_corners, conf.qualityLevel, conf.minDistance, conf.blocksize)
    p1 = O.pyr_lk(exp["lap_ref"], exp["lap_mon"], p0, win)
    p0r = O.pyr_lk(exp["lap_mon"], exp["lap_ref"], p1, win)
    status, tracks = ops.klt_tile(ref, mon, conf, mon_ksize=LC.FRAME_KSIZE, ref_ksize=LC.FRAME_KSIZE)
    assert status == "ok" and len(p0) >= 20
    _assert_same(tracks[0], p0, f"klt_tile winSize {win}: corners")
    _assert_same(tracks[1], p1, f"klt_tile winSize {win}: p1")
    _assert_same(tracks[2], p0r, f"klt_tile winSize {win}: p0r")


def test_fused_tile_on_raw_blocks_whose_laplacian_saturates(ops, O):
    """A raw uint8 pair of 1 / 255 blocks through the fused tile pipeline (stretch -> Laplacian -> mask -> corners -> tracker) with
    matching_winsize 38: the pipeline's own tracker launch on saturated Laplacians (integer corners under an even window: weights
    4096 x 4)."""
    ref, mon = LC.raw_blocks_pair()
    _tile_against_oracle(ops, O, ref, mon, 38, 300)


def test_fused_tile_on_raw_stripes_with_wrapping_windows(ops, O):
    """The raw striped pair, 120 x 200, winSize 37: the corners' windows reach 2^31 over four lanes
    (tests/test_lk_cases_host.py::test_raw_striped_pair_hands_the_tracker_wrapping_windows)."""
    ref, mon = LC.raw_stripes_pair()
    _tile_against_oracle(ops, O, np.ascontiguousarray(ref[:, :200]), np.ascontiguousarray(mon[:, :200]), LC.RAW_WIN, 400)


def test_batched_units_on_raw_stripes_with_wrapping_windows(ops, O):
    """Two units (512 x 96 and 520 x 97) of the raw striped pair submitted as a batch, winSize 37, frames against the oracle's tile.
    The corners' windows do wrap (the host test named above counts them per unit) - but the batched tracker launch itself cannot be
    held to the oracle on them: saturated stripes are a plateau image for the corner stage (the box sums of the eigenvalue map are
    equal over whole runs of pixels), the speculative corner path of the batched form flags such a unit (stage / kept-list
    overflow; flags 6 and 71 when this was written) and the unit is repeated alone, through the single-tile kernel.  What this
    case holds is that repeat on wrapping windows; the batched tracker kernel meets them in the kernel-size search below."""
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair, submit_units
    ref, mon = LC.raw_stripes_pair()
    pair = ResidentPair.upload(mon, ref, ctx=ops._lib.default_context())
    conf = KLTConfiguration(maxCorners=LC.UNIT_MAX_CORNERS, matching_winsize=LC.RAW_WIN, laplacian_kernel_size=LC.FRAME_KSIZE)
    batch = submit_units([(pair, b, None) for b in LC.UNIT_BOXES], conf)
    assert batch is not None                                     # (the batch form covers these units)
    raws = batch.wait()
    print("flags of the speculative corner path per unit:", [int(r.flags) for r in raws])
    oc = O.default_conf(maxCorners=LC.UNIT_MAX_CORNERS, matching_winsize=LC.RAW_WIN, laplacian_kernel_size=LC.FRAME_KSIZE)
    for k, (x, y, w, h) in enumerate(LC.UNIT_BOXES):
        f = (batch.redo(k) if raws[k].flags else raws[k]).to_frame()
        exp = O.klt_tile(mon[y:y + h, x:x + w], ref[y:y + h, x:x + w], oc)
        assert len(exp["x0"]) >= 8
        _assert_same(f["x0"].to_numpy(), exp["x0"] + x, f"unit {k} x0")
        _assert_same(f["y0"].to_numpy(), exp["y0"] + y, f"unit {k} y0")
        for col in ("dx", "dy", "score"):
            _assert_same(f[col].to_numpy(), exp[col], f"unit {k} {col}")


def test_kernel_size_search_tracks_wrapping_windows_in_one_launch(ops, O):
    """The batched tracker kernel (`lk2_units_kernel<5, ..>`) on wrapping windows: the kernel-size search runs the trackers of all
    (mon kernel, ref kernel) pairs as ONE launch of it, whatever became of the corner units (flagged ones are repaired through the exact
    corner path first).  Unit 0 of the raw striped pair (512 x 96), candidates 3 and 5, winSize 37: every inlier ratio, the winner,
    Ninit and the winner's columns against the reference's loop carried out with the oracle."""
    import itertools
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair
    x, y, w, h = LC.UNIT_BOXES[0]
    ref, mon = (np.ascontiguousarray(a[y:y + h, x:x + w]) for a in LC.raw_stripes_pair())
    cands = [3, 5]
    conf = KLTConfiguration(maxCorners=LC.UNIT_MAX_CORNERS, matching_winsize=LC.RAW_WIN, laplacian_kernel_size="auto")
    mask, _ = O.auto_mask(mon, ref)
    laps_m = {k: O.laplacian_u8(O.to_uint8(mon), k) for k in cands}
    laps_r = {k: O.laplacian_u8(O.to_uint8(ref), k) for k in cands}
    p0s = {k: O.good_features(laps_r[k], mask, conf.maxCorners, conf.qualityLevel, conf.minDistance, conf.blocksize) for k in cands}
    want, best, best_ratio, best_res = {}, None, -1.0, None
    for mk, rk in itertools.product(cands, repeat=2):
        pts, ninit = O.klt_tracker(laps_r[rk], laps_m[mk], mask, conf, p0=p0s[rk])
        want[(mk, rk)] = len(pts["x0"]) / ninit
        if want[(mk, rk)] > best_ratio:
            best_ratio, best, best_res = want[(mk, rk)], (mk, rk), (pts, ninit)
    assert best_ratio > 0.1
    frame, scores, got_best, ninit = ResidentPair.upload(mon, ref, ctx=ops._lib.default_context()).match_tile_auto_ksize(conf, candidates=cands)
    print("inlier ratios", scores, "expected", want)
    assert scores == pytest.approx(want, abs=0) and got_best == best and ninit == best_res[1]
    order = np.lexsort((best_res[0]["y0"], best_res[0]["x0"]))
    for col in ("x0", "y0", "dx", "dy", "score"):
        _assert_same(frame[col].to_numpy(), np.asarray(best_res[0][col], np.float32)[order], f"kernel-size search {col}")
