"""CPU suite: the three per-key-point scores (zncc_score, mutual_info_score, mi_score) as the library computes them.

1. tests/score_restatement.py - the definition, in exact arithmetic - against the installed numpy on every fixture: the joint histogram
   equals `np.histogram2d(float64, float64, bins=32)` cell for cell (and numpy raises where the restatement gives no table), both
   entropy ratios and the correlation agree with the literal float64 numpy expressions and with the reference's recorded results
   (tests/golden/mutual_info.npz, zncc.npz) within the project's 1e-9 gate.  The observed maxima are printed (pytest -s).
2. The fixtures have teeth: three deliberately wrong bin rules move some sweep chip's score by more than 1e-6; the conditions the fixtures
   rest on (samples exactly on bin edges, both a NaN and a finite class per group) are asserted.
3. csrc/mi_math.hpp - the text the kernel compiles - as a stand-alone program (tests/hoststub/mi_magic_main.cpp) built by g++ under the
   address and undefined-behaviour sanitizers: EVERY range R = 1 .. 65535 and EVERY sample d = 0 .. R against floor(32 d / R), about
   2^31 pairs (the sanitized build walks them all in seconds: no second, unsanitized build is needed).
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import sanitizer_harness as san
import score_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-9
TYPES = [np.dtype(t).name for t in R.TYPES]
INT_TYPES = [np.dtype(t).name for t in R.INT_TYPES]
nan = float("nan")


# ---- the literal numpy expressions ------------------------------------------------------------------------------------------------------
def literal_table(c1, c2):
    try:
        return np.histogram2d(c1.astype(np.float64).ravel(), c2.astype(np.float64).ravel(), bins=32)[0]
    except ValueError:            # "autodetected range of [nan, nan] is not finite"
        return None


def literal_mi(H):
    if H is None:
        return nan, nan
    p = H / H.sum()
    px, py = p.sum(axis=1), p.sum(axis=0)

    def ent(q, log):
        q = q[q > 0]
        return -np.sum(q * log(q))
    hx, hy, hxy = ent(px, np.log), ent(py, np.log), ent(p.ravel(), np.log)
    bx, by, bxy = ent(px, np.log2), ent(py, np.log2), ent(p.ravel(), np.log2)
    return (nan if hxy == 0 else (hx + hy) / hxy), (nan if bx + by == 0 else 2.0 * (bx + by - bxy) / (bx + by))


def literal_zncc(p1, p2):
    p1, p2 = p1.astype(np.float64), p2.astype(np.float64)
    with np.errstate(all="ignore"):
        m1, m2, s1, s2 = p1.mean(), p2.mean(), p1.std(), p2.std()
        if s1 == 0 or s2 == 0:
            return nan
        return float(np.mean(((p1 - m1) / s1) * ((p2 - m2) / s2)))


@functools.lru_cache(maxsize=None)
def literal(dtype):
    """{(group, name): (3 x n literal scores, number of chips whose table differs from numpy's)}"""
    out = {}
    for c in R.fixtures(dtype):
        lit = np.full((3, len(c.x0)), np.nan)
        differ = 0
        for k in range(len(c.x0)):
            got = R.chips(c.ref, c.mon, c.x0[k], c.y0[k], c.dx[k], c.dy[k])
            if got is None:
                continue
            H, mine = literal_table(*got), R.mi_counts(*got)
            differ += (H is None) != (mine is None) or (H is not None and not np.array_equal(H, mine))
            lit[0, k] = literal_zncc(R.window(got[0]), R.window(got[1]))
            lit[1, k], lit[2, k] = literal_mi(H)
        out[(c.group, c.name)] = (lit, differ)
    return out


def worst(got, want):
    """Largest |got - want| over the finite entries (0 when there is none), after the NaN patterns were found equal."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    d = np.abs(got - want)[~np.isnan(want)]
    return float(d.max()) if d.size else 0.0


# ---- 1. the definition --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
def test_tables_equal_numpy_cell_for_cell(dtype):
    cases = literal(dtype)
    assert len(cases) >= 6
    for (group, name), (_lit, differ) in cases.items():
        assert differ == 0, (group, name)


@pytest.mark.parametrize("dtype", TYPES)
def test_scores_equal_the_literal_numpy_expressions(dtype):
    lit = literal(dtype)
    for group in R.groups(dtype):
        top = [0.0, 0.0, 0.0]
        for c, want in R.expected(dtype, group):
            got = lit[(c.group, c.name)][0]
            for i in range(3):
                top[i] = max(top[i], worst(got[i], want[i]))
        print(f"restatement vs numpy [{dtype} {group}]: zncc {top[0]:.3g} studholme {top[1]:.3g} nmi {top[2]:.3g}")
        assert max(top) <= GATE, (group, top)


def test_restatement_equals_the_recorded_reference_results():
    g = np.load(os.path.join(ROOT, "tests", "golden", "mutual_info.npz"))
    kp = (g["x0"], g["y0"], g["dx"], g["dy"])
    top = 0.0
    for ref_key, mon_key, sfx in (("ref", "mon", ""), ("ref_flat", "mon", "_flat"), ("ref_flat", "mon_flat", "_flat2")):
        got = R.scores(g[ref_key], g[mon_key], *kp)
        top = max(top, worst(got[1], g["studholme" + sfx]), worst(got[2], g["nmi" + sfx]))
    z = np.load(os.path.join(ROOT, "tests", "golden", "zncc.npz"))
    for ref_key, exp_key in (("ref", "zncc"), ("ref_flat", "zncc_flat")):
        got = R.scores(z[ref_key], z["mon"], z["x0"], z["y0"], z["dx"], z["dy"])
        top = max(top, worst(got[0], z[exp_key]))
    print(f"restatement vs recorded reference results: {top:.3g}")
    assert top <= GATE


@pytest.mark.parametrize("half", [0, 21])
def test_window_fixtures_equal_the_literal_numpy_expressions(half):
    top = 0.0
    for w in R.window_fixtures():
        want = R.windows_exact(w, half)
        got = np.array([literal_zncc(w.img1[a - half:a + half + 1, b - half:b + half + 1], w.img2[c - half:c + half + 1, d - half:d + half + 1])
                        for a, b, c, d in zip(w.u1, w.v1, w.u2, w.v2)])
        top = max(top, worst(got, want))
        assert np.isnan(want).all() == (half == 0), w.name          # one pixel has no variance
    print(f"window restatement vs numpy [half {half}]: {top:.3g}")
    assert top <= GATE


# ---- 2. teeth and conditions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["magic_floor", "round", "no_fold"])
@pytest.mark.parametrize("dtype", INT_TYPES)
def test_a_wrong_bin_rule_moves_a_sweep_score(dtype, rule):
    """M = floor(2^s / R) instead of ceil, rounding instead of floor, the maximum not folded into bin 31: plain Python, no kernel code."""
    (c, want), = R.expected(dtype, "sweep")
    moved = 0.0
    for k in range(len(c.x0)):
        c1, c2 = R.chips(c.ref, c.mon, c.x0[k], c.y0[k], c.dx[k], c.dy[k])
        st, nmi = R.mi_scores(R.mi_counts(c1, c2, rule))
        moved = max(moved, abs(st - want[1, k]), abs(nmi - want[2, k]))
        if moved > 1e-6:
            break
    assert moved > 1e-6


@pytest.mark.parametrize("dtype", INT_TYPES)
def test_sweep_chips_hold_what_they_were_built_for(dtype):
    case, ranges = R.sweep(np.dtype(dtype).type)
    tmin, tmax = R.limits(dtype)
    K = len(ranges)
    assert case.ref.shape == (R.CHIP, R.CHIP * K) and K == len(case.x0) and (K >= 900 or np.dtype(dtype).itemsize == 1)
    seen_lo, seen_hi, straddle = 0, 0, 0
    for k, rng in enumerate(ranges):
        c1, c2 = R.chips(case.ref, case.mon, case.x0[k], case.y0[k], 0, 0)
        assert int(c1.max()) - int(c1.min()) == rng and int(c2.max()) - int(c2.min()) == ranges[K - 1 - k]
        for c, r in ((c1, rng), (c2, ranges[K - 1 - k])):
            d = c.astype(np.int64).ravel() - int(c.min())
            if r >= 32:
                assert int((32 * d % r == 0).sum()) >= 20
            for i in range(1, 33):       # the integers on both sides of every edge
                up = -((-i * r) // 32)
                assert (d == up).any() and (d == max(up - 1, 0)).any() and (d == min(i * r // 32 + 1, r)).any()
        seen_lo += int(c1.min()) == tmin
        seen_hi += int(c1.max()) == tmax
        straddle += int(c1.min()) < 0 < int(c1.max())
    assert seen_lo >= K // 3 and seen_hi >= K // 3 and (straddle > 0) == (tmin < 0)
    assert {1, 2, 255}.issubset(ranges) and (np.dtype(dtype).itemsize == 1 or {511, 512, 513, 32767, 32768, 32769, 65534, 65535}.issubset(ranges))


# what every group must contain: (a NaN ZNCC, a finite ZNCC, a NaN MI, a finite MI); the sweep and the float edges are all finite by design
CLASSES = {"sweep": (0, 1, 0, 1), "float_edges": (0, 1, 0, 1), "degenerate": (1, 1, 1, 1), "zncc": (1, 1, 0, 1), "placement": (1, 1, 1, 1),
           "nonfinite_rim": (0, 1, 1, 0), "nonfinite_window": (1, 0, 1, 0)}


@pytest.mark.parametrize("dtype", TYPES)
def test_every_group_holds_its_nan_and_its_finite_class(dtype):
    assert set(R.groups(dtype)) == set(CLASSES) - ({"nonfinite_rim", "nonfinite_window", "float_edges"} if dtype != "float32" else {"sweep"})
    for group in R.groups(dtype):
        want = np.hstack([w for _c, w in R.expected(dtype, group)])
        zn, mi = np.isnan(want[0]), np.isnan(want[1])
        assert np.array_equal(mi, np.isnan(want[2]))
        have = (zn.any(), (~zn).any(), mi.any(), (~mi).any())
        assert have == tuple(bool(v) for v in CLASSES[group]), (group, have)
    if dtype == "float32":
        # the rim cases are the ones the float kernel used to score: a finite ZNCC beside a NaN MI
        (_c, want), = R.expected(dtype, "nonfinite_rim")
        assert np.isfinite(want[0]).all() and np.isnan(want[1]).all()


def test_placement_rounds_half_to_even_and_truncates():
    (c, want), = R.expected("uint16", "placement")
    at = {(float(a), float(b), float(d), float(e)): k for k, (a, b, d, e) in enumerate(zip(c.x0, c.y0, c.dx, c.dy))}
    fin = lambda *p: bool(np.isfinite(want[1, at[p]]))          # noqa: E731
    W, H = c.ref.shape[1], c.ref.shape[0]
    assert (W, H) == (70, 64)
    assert fin(28.0, 28.0, 0.0, 0.0) and fin(41.0, 35.0, 0.0, 0.0) and not fin(27.0, 28.0, 0.0, 0.0) and not fin(41.0, 36.0, 0.0, 0.0)
    assert not fin(41.0, 30.0, 0.5, 0.0) and fin(40.0, 30.0, 0.5, 0.0)        # 41.5 -> 42 (outside), 40.5 -> 40
    assert fin(28.0, 30.0, -0.5, 0.0) and fin(29.0, 30.0, -1.5, 0.0)          # 27.5 -> 28
    assert not fin(28.0, 30.0, -1.5, 0.0) and not fin(29.0, 30.0, -2.5, 0.0)  # 26.5 -> 26 (outside)
    assert not fin(40.0, 30.0, 1.5, 0.0) and fin(41.0, 30.0, -0.5, 0.0)
    assert R.round_half_even_f32(27.5) == 28 and R.round_half_even_f32(28.5) == 28 and R.round_half_even_f32(-0.5) == 0
    assert fin(np.float32(28.9), np.float32(28.9), 0.0, 0.0) and not fin(np.float32(27.99), 30.0, 0.0, 0.0)


# ---- 3. mi_math.hpp, every (R, d) -----------------------------------------------------------------------------------------------------------
def test_magic_division_equals_floor_for_every_range_and_sample(tmp_path):
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")
    exe = tmp_path / "mi_magic_main"
    san.build(os.path.join(ROOT, "tests", "hoststub", "mi_magic_main.cpp"), exe, shared=False)
    out = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
    words = out.stdout.split()
    got = dict(zip(words[::2], (int(v) for v in words[1::2])))
    assert got["pairs"] == 65535 * 65536 // 2 + 2 * 65535 and got["bad"] == 0 and got["max_M"] <= 1 << 22
    # the kernel compiles the same text
    text = open(os.path.join(ROOT, "karios_amd", "csrc", "k_mi.hip")).read()
    assert '#include "mi_math.hpp"' in text and "mi::magic(" in text and "mi::bin_of(mi::quotient(" in text and "ldexp" not in text
