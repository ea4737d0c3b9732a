"""The fixtures of tests/lk_cases.py do what they are there for (CPU only; run with -s to see the counts).

`saturated`: the first level-0 iteration's mismatch sums, dealt to the lanes as the kernels (`lk_run_desc`, lk_device.hpp) deal the window's runs, reach 2^31 over
four neighbouring lanes where the fixture says so and nowhere else.  `cut`: windows on both sides of `minEig < 1e-4f`, within 1 % of
it, and the oracle skips exactly the levels the restatement says it skips.  `weights`: every start position has the bilinear
weights the fixture claims, the negative fourth weight among them.
"""
import numpy as np
import pytest

import lk_cases as LC
import lk_restatement as R


def _origin(case, k, level=0):
    x, y = case.pts[k, 0]
    (ipx, a), (ipy, b) = R.template_fraction(x, case.win, level), R.template_fraction(y, case.win, level)
    return ipx, ipy, a, b


def _first_iteration_sums(O, case, strict=True):
    """Per key point: (largest |per-lane sum|, largest |four-lane sum|) over both components of the first level-0 iteration.
    `strict` off: (0, 0) for a key point that the cut skips or that level 1 sends where the search window overhangs the image."""
    start = LC.level0_start(O, case)
    half = np.float32(case.win - 1) * np.float32(0.5)
    deriv = R.scharr(case.prev)
    out = []
    for k in range(len(case.pts)):
        ipx, ipy, a, b = _origin(case, k)
        assert a == 0 and b == 0, "template origin is not an integer pixel"
        tI, tIx, tIy = R.template(case.prev, ipx, ipy, case.win, deriv)
        sx, sy = start[k, 0] - half, start[k, 1] - half
        if not strict and not (R.normal_matrix(tIx, tIy, case.win)["tracked"] and 0 <= sx < case.prev.shape[1] - case.win - 1
                               and 0 <= sy < case.prev.shape[0] - case.win - 1):
            out.append((0, 0))
            continue
        assert R.normal_matrix(tIx, tIy, case.win)["tracked"]
        sums = [R.lane_sums(t, case.win) for t in R.mismatch_terms(tI, tIx, tIy, case.next, start[k, 0] - half, start[k, 1] - half)]
        out.append((max(s[0] for s in sums), max(s[1] for s in sums)))
    return np.array(out, np.int64)


def test_restatement_deals_runs_as_the_kernel_does():
    """Runs per lane of every window the kernels serve (the `nr` of kl_track), every pixel dealt once, a lane's runs 64 apart."""
    for win in range(3, 41):
        lane, nr = R.lane_of(win)
        rpr = (win + 4) // 5
        assert nr == (win * rpr + 63) // 64 and lane.shape == (win, win) and lane.min() == 0 and lane.max() <= 63
        assert np.bincount(lane.ravel()).max() <= 5 * nr
    assert [R.runs_per_lane(w) for w in LC.SATURATED_WINDOWS] == [2, 3, 4, 4, 5, 5, 5, 5]
    assert all(R.runs_per_lane(w) == 4 for w in LC.TAILORED_WINDOWS)


def test_saturated_fixtures_reach_the_int32_range_where_they_say(O):
    for nr in range(1, 6):
        b = R.theoretical_four_lane_bound(nr)
        print(f"NR {nr}: four lanes hold at most 4 * {5 * nr} * 8160 * 4080 = {b:.4g} ({'<' if b < R.WRAP else '>='} 2^31)")
    wrapping = {}
    for case in LC.saturated_cases():
        s = _first_iteration_sums(O, case)
        _, it0, _ = O.pyr_lk(case.prev, case.next, case.pts, case.win, return_iters="levels")
        n = int((s[:, 1] >= R.WRAP).sum())
        print(f"{case}: NR {R.runs_per_lane(case.win)}, largest per-lane sum {s[:, 0].max():.3g}, largest four-lane sum {s[:, 1].max():.3g}, "
              f"{n} of {len(s)} key points reach 2^31, level-0 iterations {it0.min()}..{it0.max()}")
        assert it0.min() >= 1                      # the oracle iterates at level 0: the cut does not hide these points
        assert s[:, 0].max() < R.WRAP              # a lane's own int32 always holds its sum
        assert s[:, 1].max() <= R.theoretical_four_lane_bound(R.runs_per_lane(case.win))
        wrapping[(case.name, case.win)] = n
    for win in LC.SATURATED_WINDOWS:
        total = sum(n for (name, w), n in wrapping.items() if w == win and name != "stripes9")
        if win >= 36:
            assert total >= 8 and wrapping[("stripes", win)] >= 8
        elif win <= 30:
            assert total == 0
    # the scene tailored to NR = 4: above 2^31 at every window it is used with
    assert all(wrapping[("stripes9", w)] >= 1 for w in LC.TAILORED_WINDOWS)
    assert sum(wrapping[("stripes9", w)] for w in LC.TAILORED_WINDOWS) >= 8
    assert all(n == 0 for (name, w), n in wrapping.items() if w <= 30)


def _raw_corner_case(O, ref, mon, win, max_corners):
    """What the entry points that start from pixels hand to the tracker: the Laplacian pair, and those corners whose windows lie
    inside the image with room to move (the others are tracked too, but the restatement has no border)."""
    conf = O.default_conf(maxCorners=max_corners, matching_winsize=win, laplacian_kernel_size=LC.FRAME_KSIZE)
    exp = O.klt_tile(mon, ref, conf)
    p0 = O.good_features(exp["lap_ref"], exp["mask"], max_corners, conf.qualityLevel, conf.minDistance, conf.blocksize)
    H, W = ref.shape
    half = (win - 1) // 2
    xy = p0.reshape(-1, 2)
    inside = (xy[:, 0] - half >= 4) & (xy[:, 0] + half + 5 <= W) & (xy[:, 1] - half >= 4) & (xy[:, 1] + half + 5 <= H)
    return LC.Case("raw", "saturated", win, exp["lap_ref"], exp["lap_mon"], np.ascontiguousarray(p0[inside])), len(p0), exp


def test_raw_striped_pair_hands_the_tracker_wrapping_windows(O):
    """The frame-level and the batched-units case of tests/test_gpu_lk_extremes.py start from pixels: their Laplacians are the striped
    scene, their corners sit at the phase breaks, and with winSize 37 the corners' windows reach 2^31 over four lanes."""
    ref, mon = LC.raw_stripes_pair()
    boxes = {"tile": (0, 0, 200, 120)}
    boxes.update({f"unit {k}": b for k, b in enumerate(LC.UNIT_BOXES)})
    for name, (x, y, w, h) in boxes.items():
        r, m = np.ascontiguousarray(ref[y:y + h, x:x + w]), np.ascontiguousarray(mon[y:y + h, x:x + w])
        case, n_all, exp = _raw_corner_case(O, r, m, LC.RAW_WIN, 400 if name == "tile" else LC.UNIT_MAX_CORNERS)
        if name != "tile":
            assert n_all == LC.UNIT_MAX_CORNERS
        assert set(np.unique(exp["lap_ref"])) <= {0, 254, 255} and (exp["mask"] > 0).all()
        s = _first_iteration_sums(O, case, strict=False)
        n = int((s[:, 1] >= R.WRAP).sum())
        print(f"raw stripes, {name}: {n_all} corners, {len(case.pts)} with the window inside, {n} of them reach 2^31 over four lanes; "
              f"{len(exp['x0'])} rows in the oracle's frame")
        assert n >= 8 and len(exp["x0"]) >= 8


def _restated_tracked(case, level=0):
    img = case.prev
    deriv = R.scharr(img)
    out = []
    for k in range(len(case.pts)):
        ipx, ipy, a, b = _origin(case, k)
        assert a == 0 and b == 0
        _, tIx, tIy = R.template(img, ipx, ipy, case.win, deriv)
        out.append(R.normal_matrix(tIx, tIy, case.win))
    return out


def _assert_windows_inside(case):
    """Template window + derivative ring inside the image at both levels: an iteration count of 0 can only mean the cut."""
    H, W = case.prev.shape
    for k in range(len(case.pts)):
        for level, (h, w) in enumerate(((H, W), ((H + 1) // 2, (W + 1) // 2))):
            ipx, ipy, _, _ = _origin(case, k, level)
            assert 1 <= ipx and ipx + case.win + 2 <= w and 1 <= ipy and ipy + case.win + 2 <= h, (str(case), k, level)


def test_cut_fixtures_lie_on_both_sides_and_the_oracle_skips_what_the_restatement_skips(O):
    combos, both_skipped = set(), 0
    for case in LC.cut_cases():
        _assert_windows_inside(case)
        nm = _restated_tracked(case)
        tracked = np.array([m["tracked"] for m in nm])
        p1, it0, it1 = O.pyr_lk(case.prev, case.next, case.pts, case.win, return_iters="levels")
        np.testing.assert_array_equal(it0 >= 1, tracked, err_msg=str(case))
        combos |= set(zip((it0 >= 1).tolist(), (it1 >= 1).tolist()))
        none = (it0 == 0) & (it1 == 0)
        both_skipped += int(none.sum())
        np.testing.assert_array_equal(p1[none], np.asarray(case.pts)[none])
        e = np.array([float(m["minEig"]) for m in nm])
        near = np.abs(e / 1e-4 - 1) <= LC.NEAR
        d_small = np.array([m["D"] < R.FLT_EPSILON for m in nm])
        print(f"{case}: {len(nm)} key points, tracked {int(tracked.sum())}, skipped {int((~tracked).sum())}; within 1 % of the cut: "
              f"{int((near & tracked).sum())} above, {int((near & ~tracked).sum())} below; D < FLT_EPSILON: {int(d_small.sum())}, "
              f"of them D != 0: {int(sum(d_small[i] and m['D'] != 0 for i, m in enumerate(nm)))}; level 1 tracked {int((it1 >= 1).sum())}")
        if case.info.get("near"):
            assert (near & tracked).sum() >= 8 and (near & ~tracked).sum() >= 8
            assert (~near & tracked).any() and (~near & ~tracked).any()
        if case.info.get("singular"):
            assert not tracked.any() and d_small.all()
        if case.info.get("rounding"):
            assert not tracked.any() and d_small.any() and (~d_small).any()
        if case.info.get("only level 0"):
            assert tracked.all() and (it1 == 0).all()
        if case.info.get("flat_return"):
            _, b0, b1 = O.pyr_lk(case.next, case.prev, p1, case.win, return_iters="levels")
            assert tracked.all() and (b0 == 0).all() and (b1 == 0).all()
            assert (p1 != np.asarray(case.pts)).any()
        if case.name == "levels":
            n = {k: len(v) for k, v in LC.LEVELS_POINTS.items()}
            lo = 0
            for kind, want in (("only level 1", (False, True)), ("both", (True, True)), ("none", (False, False))):
                got = set(zip((it0[lo:lo + n[kind]] >= 1).tolist(), (it1[lo:lo + n[kind]] >= 1).tolist()))
                assert got == {want}, (kind, got)
                lo += n[kind]
    assert combos == {(True, True), (True, False), (False, True), (False, False)}
    assert both_skipped >= 8
    print(f"cut: {both_skipped} key points are skipped at both levels")


def test_rounding_sized_determinant_exists():
    """`stripes_d_dots`: the exact determinant of the integer normal matrix is positive, the float32 one is what rounding leaves of it."""
    case = next(c for c in LC.cut_cases() if c.name == "stripes_d_dots")
    nm = _restated_tracked(case)
    exact = [m["iA11"] * m["iA22"] - m["iA12"] ** 2 for m in nm]
    assert all(d >= 0 for d in exact) and any(d > 0 for d in exact)
    assert any(m["D"] < 0 for m in nm) and any(m["D"] == 0 for m in nm) and any(m["D"] > 0 for m in nm)
    assert all(abs(float(m["D"])) <= 8 * np.spacing(m["A11"] * m["A22"]) for m in nm)
    print("stripes_d_dots: float32 D", sorted({float(m["D"]) for m in nm}), "exact determinant / 2^40 up to", max(exact) / 2.0 ** 40)


def _mode(w):
    return 2 if w[1] == w[2] == w[3] == 0 else 1 if w[2] == w[3] == 0 else 0


def test_weight_fixtures_have_the_weights_they_claim():
    assert R.lk_weights(*LC.EXAMPLE[0]) == LC.EXAMPLE[1]
    for (a, b), w in LC.FRACTIONS:
        assert R.lk_weights(a, b) == w and sum(w) == 16384
    assert sum(w[3] == -1 for _, w in LC.FRACTIONS) >= 4
    for case in LC.weights_cases():
        modes = [set(), set()]
        negative = 0
        H, W = case.prev.shape
        for k, claim in enumerate(case.info["claims"]):
            ipx, ipy, a, b = _origin(case, k)
            assert R.lk_weights(a, b) == claim, (str(case), k)
            assert 1 <= ipx and ipx + case.win + 2 <= W and 1 <= ipy and ipy + case.win + 2 <= H
            negative += claim[3] == -1
            modes[0].add(_mode(claim))
            modes[1].add(_mode(R.lk_weights(*_origin(case, k, 1)[2:])))
        print(f"{case}: {len(case.pts)} start positions, {negative} with w11 == -1, template modes at level 0 {sorted(modes[0])}, at level 1 {sorted(modes[1])}")
        assert negative >= 4 and len(case.info["claims"]) == len(case.pts)
        assert modes[0] == {0, 1, 2} and modes[1] == {0, 1, 2}


def test_fixtures_are_small_and_deterministic():
    a, b = LC.all_cases(), LC.all_cases()
    assert [str(c) for c in a] == LC.case_ids() and len(set(LC.case_ids())) == len(a)
    for x, y in zip(a, b):
        assert x.prev.dtype == np.uint8 and x.prev.shape == x.next.shape and x.prev.shape[0] <= 160 and x.prev.shape[1] <= 200
        assert x.pts.dtype == np.float32 and x.pts.shape[1:] == (1, 2) and 1 <= len(x.pts) <= 400 and np.isfinite(x.pts).all()
        np.testing.assert_array_equal(x.prev, y.prev)
        np.testing.assert_array_equal(x.pts, y.pts)


def test_literal_float_accumulation_on_the_cut_fixtures_is_recorded(O):
    """How many `cut` key points OpenCV's four-lane float32 accumulation (`oracle.pyr_lk_cv`) decides differently from the integer
    oracle: recorded, not asserted - the kernels follow the integer oracle, as every LK test here does."""
    total = differ = moved = 0
    for case in LC.cut_cases():
        a = O.pyr_lk(case.prev, case.next, case.pts, case.win).reshape(-1, 2)
        b = O.pyr_lk_cv(case.prev, case.next, case.pts, case.win).reshape(-1, 2)
        p = np.asarray(case.pts).reshape(-1, 2)
        m = (a != p).any(1) != (b != p).any(1)
        print(f"{case}: {int(m.sum())} of {len(p)} key points move under one accumulation and stay under the other; "
              f"{int((a != b).any(1).sum())} differ in some bit")
        total += len(p); moved += int(m.sum()); differ += int((a != b).any(1).sum())
    print(f"cut: the literal float accumulation decides {moved} of {total} key points differently ({differ} differ in some bit)")
