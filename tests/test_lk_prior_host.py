"""CPU suite: the tracker under a geometric prior (tests/lk_prior_restatement.py is the definition,
tests/lk_prior_cases.py holds the inputs).

1. The restatement is pinned to the oracle: with guess == pts it is `oracle.pyr_lk` bit for bit (winSize 21, 25, 31, the existing LK
   fixtures and key points whose windows cross the borders).
2. The prior's arithmetic: exact sums for an integer shift, no guess where w <= 0; csrc/prior_math.hpp and the host launcher of
   csrc/k_prior.hpp as a stand-alone program under the address and undefined-behaviour sanitizers, byte for byte against the mask rule.
3. Sign and meaning: the seeded frame against the reference's path - `shift_image`, the unseeded oracle, offsets added back.
4. No perfect track of nothing: what the mask rule prevents, shown by running without it.
5. The surface: ABI, signatures, `matcher.prior`, the residual clip, `handle_klt_results`' columns.
"""
import inspect
import os
import struct
import subprocess

import numpy as np
import pandas as pd
import pytest

import lk_cases as LC
import lk_prior_cases as C
import lk_prior_restatement as PR
import sanitizer_harness as san

from karios_amd import _lib  # noqa: E402
from karios_amd.matcher import prior as prior_mod  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the restatement is pinned to the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [21, 25, 31])
def test_restatement_with_guess_equal_to_points_is_the_oracle(O, win):
    scenes = dict(LC._saturated_scenes())
    pairs = [(name, scenes[name][0], scenes[name][1], LC._grid(win, range(52, 61), range(52, 69, 4))) for name in ("stripes", "checker", "blocks")]
    ref, mon = LC._textured_pair()
    pairs.append(("textured", ref, mon, LC.weight_points(win)[0]))
    h, w = ref.shape
    rim = np.array([[3, 4], [w - 2, h - 3], [1, 80], [100, 1], [w - 1, h - 1], [-5, 20], [50.5, -8.25], [w + 40, 60]], np.float32).reshape(-1, 1, 2)
    pairs.append(("textured, windows across the borders", ref, mon, rim))
    cut = next(c for c in LC.cut_cases())
    pairs.append(("cut fixture", cut.prev, cut.next, cut.pts))
    for name, a, b, pts in pairs:
        got = PR.pyr_lk_initial(a, b, pts, pts, win)
        assert _same_bits(got, O.pyr_lk(a, b, pts, win)), f"{name}, winSize {win}"


def test_restated_pyramid_level_is_the_oracles(O):
    for img in (C.pair()[0], C.pair()[0][:-1, :-3]):
        assert np.array_equal(PR.pyrdown(img), O.pyrdown_u8(img))


# ---- 2. the prior's arithmetic --------------------------------------------------------------------------------------------------------------
def test_integer_shift_gives_exact_sums():
    pts = np.array([[x, y] for y in (0, 7, 159, 4000) for x in (0, 33, 191, 10979)], np.float32)
    for sx, sy in ((14, -6), (7, 3), (-5000, 2049), (0, 0)):
        for off in ((0, 0), (4096, 512)):
            g, ok = PR.guess(PR.shift_prior(sx, sy), pts, *off)
            assert ok.all() and _same_bits(g, pts + np.float32([sx, sy]))
            gx, gy, ok2 = prior_mod.guesses(prior_mod.from_shift(sy, sx), pts[:, 0], pts[:, 1], *off)       # (row, column): LargeOffsetMatcher's order
            assert ok2.all() and _same_bits(np.stack([gx, gy], 1), g)


def test_no_guess_where_w_is_not_positive():
    P = C.horizon_prior()                                              # w = 1 - x / 120
    pts = np.array([[x, 40] for x in (0, 60, 119, 120, 121, 191)], np.float32)
    g, ok = PR.guess(P, pts)
    assert ok.tolist() == [True, True, True, False, False, False]
    assert _same_bits(g[~ok], pts[~ok])                                # a row without a guess keeps the key point
    assert np.all(np.isfinite(g[ok]))
    rx, ry, has = PR.targets(P, C.H, C.W)
    assert not has[:, 120:].any() and has[:, :100].any()
    ref, mon = C.pair()
    assert not PR.mask(ref, mon, P)[:, 120:].any()
    # w == 0 exactly, w = +inf, w = NaN
    for P9 in ([1, 0, 0, 0, 1, 0, 0, 0, 0.0], [1, 0, 0, 0, 1, 0, 0, 0, np.inf], [1, 0, 0, 0, 1, 0, np.nan, 0, 1.0]):
        assert not PR.guess(np.array(P9, np.float64), pts)[1].any()


def test_host_transcription_of_the_guess_equals_the_restatement():
    pts = np.array([[x, y] for y in (0, 9, 77, 159) for x in (0, 11, 96, 191)], np.float32)
    for P in (C.rotation_prior(3.0), C.horizon_prior(), PR.shift_prior(6.6, 3.3), C.rotation_prior(1.0, sx=7, sy=3)):
        for off in ((0.0, 0.0), (16.0, 8.0)):
            g, ok = PR.guess(P, pts, *off)
            gx, gy, ok2 = prior_mod.guesses(P, pts[:, 0], pts[:, 1], *off)
            assert np.array_equal(ok, ok2) and _same_bits(np.stack([gx, gy], 1), g)


MAIN = r"""
#include "k_prior.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
// {int dtype, H, W, has_base, has_nd_ref, has_nd_mon; long long sref, smon, sbase (pixels); double nd_ref, nd_mon, P[9], x_off, y_off}
// ref (H * sref pixels, malloc'd to the byte) mon base -> mask (H * W), poisoned first.  Guesses: int n; n x 2 float32 -> n x 2 float32, n bytes.
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    struct { int dtype, H, W, has_base, has_nd_ref, has_nd_mon; long long sref, smon, sbase; double nd_ref, nd_mon, P[9], x_off, y_off; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    const size_t es = h.dtype == KM_U8 ? 1 : h.dtype == KM_F32 ? 4 : 2;
    // (the last row of a strided raster ends at its last pixel: the sanitizer sees a read past it)
    std::vector<char> ref(((size_t)(h.H - 1) * h.sref + h.W) * es), mon(((size_t)(h.H - 1) * h.smon + h.W) * es);
    std::vector<uint8_t> base(h.has_base ? (size_t)(h.H - 1) * h.sbase + h.W : 1), mask((size_t)h.H * h.W + 1, 0x5a);
    if (!rd(in, ref.data(), ref.size()) || !rd(in, mon.data(), mon.size()) || (h.has_base && !rd(in, base.data(), base.size()))) return 2;
    kp_mask_args a;
    a.ref = ref.data(); a.mon = mon.data(); a.dtype = h.dtype; a.H = h.H; a.W = h.W; a.sref = (ptrdiff_t)h.sref; a.smon = (ptrdiff_t)h.smon;
    a.base = h.has_base ? base.data() : nullptr; a.sbase = (ptrdiff_t)h.sbase;
    a.has_nd_ref = h.has_nd_ref; a.has_nd_mon = h.has_nd_mon; a.nd_ref = h.nd_ref; a.nd_mon = h.nd_mon;
    memcpy(a.P, h.P, sizeof a.P); a.x_off = h.x_off; a.y_off = h.y_off; a.mask = mask.data();
    if (kp_prior_mask(nullptr, a) != KM_OK) return 3;
    if (mask.back() != 0x5a) return 4;
    for (size_t i = 0; i + 1 < mask.size(); i++) if (mask[i] > 1) return 5;          // every byte written, 1 / 0
    a.dtype = 9;
    if (kp_prior_mask(nullptr, a) != KM_E_ARG) return 6;
    int n = 0;
    if (!rd(in, &n, sizeof n)) return 2;
    std::vector<float> pts(2 * (size_t)n + 1), g(2 * (size_t)n + 1);
    std::vector<uint8_t> ok((size_t)n + 1);
    if (!rd(in, pts.data(), 8 * (size_t)n)) return 2;
    for (int k = 0; k < n; k++) {
        g[2 * k] = pts[2 * k]; g[2 * k + 1] = pts[2 * k + 1];
        ok[k] = pm::guess(h.P, h.x_off, h.y_off, pts[2 * k], pts[2 * k + 1], g[2 * k], g[2 * k + 1]) ? 1 : 0;
    }
    const bool w = fwrite(mask.data(), 1, (size_t)h.H * h.W, out) == (size_t)h.H * h.W && (n == 0 || (fwrite(g.data(), 4, 2 * (size_t)n, out) == 2 * (size_t)n &&
                   fwrite(ok.data(), 1, (size_t)n, out) == (size_t)n));
    return fclose(out) || !w ? 2 : 0;
}
"""


def _strided(a, extra, fill):
    """`a` as a window of a wider buffer (row stride = width + extra)."""
    wide = np.full((a.shape[0], a.shape[1] + extra), fill, a.dtype)
    wide[:, :a.shape[1]] = a
    return wide[:, :a.shape[1]]


def _payload(case, pts):
    ref, mon = _strided(case["ref"], 5, 3), _strided(case["mon"], 2, 3)
    base = None if case["base"] is None else _strided(case["base"], 7, 1)
    H, W = ref.shape
    stride = lambda a: a.strides[0] // a.itemsize
    raw = lambda a: a.base.tobytes()[:((H - 1) * stride(a) + W) * a.itemsize]
    head = struct.pack("<6i3q13d", _lib._DTYPES[ref.dtype], H, W, int(base is not None), int(case["nodata_ref"] is not None), int(case["nodata_mon"] is not None),
                       stride(ref), stride(mon), stride(base) if base is not None else 0, float(case["nodata_ref"] or 0), float(case["nodata_mon"] or 0),
                       *[float(v) for v in case["prior"]], case["x_off"], case["y_off"])
    pts = np.ascontiguousarray(pts, np.float32)
    return head + raw(ref) + raw(mon) + (raw(base) if base is not None else b"") + struct.pack("<i", len(pts)) + pts.tobytes()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")
    d = tmp_path_factory.mktemp("prior_main")
    src, exe = d / "prior_main.cpp", d / "prior_main"
    src.write_text(MAIN)
    san.build(src, exe, shared=False)

    def run(data):
        fin, fout = d / "in.bin", d / "out.bin"
        fin.write_bytes(data)
        out = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr[-4000:])
        return fout.read_bytes()
    return run


def test_shared_header_and_host_launcher_equal_the_restatement(program):
    """csrc/prior_math.hpp + the plain-loop launcher of csrc/k_prior.hpp, compiled by g++ with -ffp-contract=off under ASan / UBSan, on
    strided rasters that end at their last pixel: the mask byte for byte, the guesses bit for bit."""
    rng = np.random.default_rng(5)
    some = 0
    for case in C.mask_cases():
        H, W = case["ref"].shape
        pts = np.concatenate([rng.integers(-20, 120, (40, 2)).astype(np.float32), rng.random((24, 2)).astype(np.float32) * np.float32(90)])
        raw = program(_payload(case, pts))
        n = len(pts)
        assert len(raw) == H * W + 9 * n
        got = np.frombuffer(raw[:H * W], np.uint8).reshape(H, W)
        want = PR.mask(case["ref"], case["mon"], case["prior"], case["base"], case["nodata_ref"], case["nodata_mon"], case["x_off"], case["y_off"])
        assert np.array_equal(got, want), f"{case['name']}: {int((got != want).sum())} mask bytes differ"
        g, ok = PR.guess(case["prior"], pts, case["x_off"], case["y_off"])
        got_g = np.frombuffer(raw[H * W:H * W + 8 * n], np.float32).reshape(n, 2)
        got_ok = np.frombuffer(raw[H * W + 8 * n:], np.uint8).astype(bool)
        assert np.array_equal(got_ok, ok) and _same_bits(got_g, g), case["name"]
        some += int(0 < want.sum() < H * W)
    assert some >= 12                                                  # (most cases hold both values)


def test_mask_cases_reach_every_clause():
    """The fixture does what it is there for: each clause of the rule decides some pixel of some case."""
    hit = dict(base=0, no_guess=0, outside=0, mon_invalid=0, nan=0, nodata_mon=0, tie=0)
    for case in C.mask_cases():
        ref, mon, P = case["ref"], case["mon"], case["prior"]
        H, W = ref.shape
        base_ok = (case["base"] != 0) if case["base"] is not None else PR._valid(ref, case["nodata_ref"])
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        qx, qy, has = PR._map(P, xx, yy, case["x_off"], case["y_off"])
        rx, ry, inside = PR.targets(P, H, W, case["x_off"], case["y_off"])
        mon_ok = PR._valid(mon, case["nodata_mon"])[ry, rx]
        hit["base"] += int((~base_ok).sum())
        hit["no_guess"] += int((base_ok & ~has).sum())
        hit["outside"] += int((base_ok & has & ~inside).sum())
        hit["mon_invalid"] += int((base_ok & inside & ~mon_ok).sum())
        if mon.dtype == np.float32:
            hit["nan"] += int((base_ok & inside & ~np.isfinite(mon[ry, rx])).sum())
        if case["nodata_mon"] is not None:
            hit["nodata_mon"] += int((base_ok & inside & (mon[ry, rx] == case["nodata_mon"])).sum())
        with np.errstate(all="ignore"):
            hit["tie"] += int((has & (np.abs(qx - np.floor(qx) - 0.5) == 0)).sum())           # exact halves: the rounding rule decides
    assert all(v > 0 for v in hit.values()), hit


# ---- 3. sign and meaning --------------------------------------------------------------------------------------------------------------------
# max and median |delta| of (dx, dy) between the seeded frame and shift-then-track, measured on the CPU with the restatement and the oracle
# alone over the rows both keep.  The even shift is an integer at both levels: the two computations then meet the
# same integers and converge on the same float32 positions.  The odd shift is half a pixel at level 1.  The test asserts twice the maximum.
MEASURED = {
    ((14, -6), 25): (0.0, 0.0), ((14, -6), 21): (0.0, 0.0), ((14, -6), 31): (0.0, 0.0),
    ((7, 3), 25): (0.001495361328125, 0.000152587890625), ((7, 3), 21): (0.00103759765625, 0.000152587890625),
    ((7, 3), 31): (0.00093841552734375, 0.0001678466796875),
}


@pytest.fixture(scope="module")
def seeded_and_shifted(O):
    """(shift, win) -> the two computations' columns, computed once."""
    out = {}
    for (sx, sy) in C.SHIFTS:
        ref, mon = C.pair(sx, sy)
        P = prior_mod.from_shift(sy, sx)
        p0 = O.good_features(ref, PR.mask(ref, mon, P), C.MAX_CORNERS, C.QUALITY, C.MIN_DISTANCE, C.BLOCK)
        g, ok = PR.guess(P, p0)
        assert ok.all()
        mon_s = O.shift_image(mon, y_off=sy, x_off=sx)                 # the reference's way: a second monitored raster
        for win in C.WINDOWS:
            p1, p0r = PR.track_fb(ref, mon, p0, g, win)
            q1 = O.pyr_lk(ref, mon_s, p0, win)
            q0r = O.pyr_lk(mon_s, ref, q1, win)
            out[((sx, sy), win)] = (p0.reshape(-1, 2), p1.reshape(-1, 2), PR.fb_columns(p0, p1, p0r)[1], q1.reshape(-1, 2), PR.fb_columns(p0, q1, q0r)[1])
    return out


@pytest.mark.parametrize("win", C.WINDOWS)
@pytest.mark.parametrize("shift", C.SHIFTS)
def test_seeded_frame_means_what_shift_then_track_means(seeded_and_shifted, shift, win):
    sx, sy = shift
    p0, p1, d, q1, d2 = seeded_and_shifted[(shift, win)]
    assert 35 <= len(p0) <= 45                                         # about 40 corners
    margin = win + 8                                                   # of a border, or of the zero fill of the shifted raster
    x, y = p0[:, 0], p0[:, 1]
    inner = (x >= margin + max(-sx, 0)) & (x < C.W - margin - max(sx, 0)) & (y >= margin + max(-sy, 0)) & (y < C.H - margin - max(sy, 0))
    assert (~inner).sum() <= 0.25 * len(p0)
    rows = inner & (d < 0.1) & (d2 < 0.1)
    assert rows.sum() >= 0.7 * len(p0)
    seeded = p1 - p0                                                   # total displacements, as they come out
    added_back = (q1 - p0) + np.float32([sx, sy])                      # core.py:248-249
    delta = np.abs(seeded - added_back)[rows]
    print(f"shift {shift} winSize {win}: {int(rows.sum())} rows, max |delta| {delta.max()!r}, median {np.median(delta)!r}")
    assert np.abs(seeded[rows] - np.float32([sx, sy])).max() < 0.01    # the sign: the content moved by (+sx, +sy)
    assert delta.max() <= 2 * MEASURED[(shift, win)][0]


# ---- 4. no perfect track of nothing ---------------------------------------------------------------------------------------------------------
def test_mask_rule_is_what_prevents_perfect_tracks_of_nothing(O):
    ref, mon = C.pair()
    P = prior_mod.from_shift(0, C.W // 2)
    outcome = {}
    for rule in (True, False):
        p0 = O.good_features(ref, PR.mask(ref, mon, P, rule=rule), C.MAX_CORNERS, C.QUALITY, C.MIN_DISTANCE, C.BLOCK)
        g, _ = PR.guess(P, p0)
        p1, p0r = PR.track_fb(ref, mon, p0, g, 25)
        cols, d = PR.fb_columns(p0, p1, p0r)
        outside = ~((g[:, 0] >= 0) & (g[:, 0] < C.W) & (g[:, 1] >= 0) & (g[:, 1] < C.H))
        outcome[rule] = (len(p0), int(outside.sum()), int(((d == 0) & outside).sum()), cols["score"][(d[d < 0.1] == 0)])
    n, n_outside, n_perfect, _ = outcome[True]
    assert n >= 20 and n_outside == 0 and n_perfect == 0               # under the rule every selected corner has its guess inside
    n, n_outside, n_perfect, scores = outcome[False]
    assert n_outside >= 1 and n_perfect >= 1 and (scores == 1.0).all()  # without it: d == 0, score 1.0, of nothing


# ---- 5. the surface -------------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = {"km_pyrlk_initial": 13, "km_prior_mask": 16, "km_prior_mask_dev": 16, "km_klt_tile_frame_prior_dev": 25}


def test_abi_carries_the_entry_points():
    import ctypes
    header = open(os.path.join(ROOT, "include", "karios_hip.h")).read()
    api = open(os.path.join(ROOT, "karios_amd", "csrc", "api_tile.hip")).read()          # an existing API file: the host build's list stands
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        assert name in _lib.SIGNATURES and f"int {name}(" in header and hasattr(lib, name) and f"int {name}(" in api, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "k_prior.hip" in open(os.path.join(ROOT, "karios_amd", "csrc", "Makefile")).read()
    from karios_amd import matcher, ops, resident, results
    assert callable(ops.pyrlk_initial) and callable(ops.prior_mask)
    for fn in (resident.ResidentPair.match_tile, matcher.KLT.match, matcher.klt_tracker, results.handle_klt_results):
        assert inspect.signature(fn).parameters["prior"].default is None


def test_priors_from_the_pre_aligner_and_the_align_step():
    assert prior_mod.from_shift(-6, 14).tolist() == [1, 0, 14, 0, 1, -6, 0, 0, 1]          # (row, column) in, x then y inside
    m = np.array([[0.99, -0.02, 3.5], [0.02, 1.01, -7.25], [1e-6, -2e-6, 1.0]])            # mon -> ref (global_align.py:427)

    class Alignment:
        matrix = m
    P = prior_mod.from_alignment(Alignment())
    assert P.dtype == np.float64 and np.array_equal(P.reshape(3, 3), np.linalg.inv(m)) and np.array_equal(prior_mod.from_alignment(m), P)
    # ref -> mon -> ref
    g, ok = PR.guess(P, np.float32([[40, 50]]))
    back = m @ np.array([g[0, 0], g[0, 1], 1.0])
    assert ok.all() and np.allclose(back[:2] / back[2], [40, 50], atol=1e-4)
    for bad in ([1, 2, 3], np.full(9, np.nan), np.r_[np.ones(8), np.inf]):
        with pytest.raises(ValueError):
            prior_mod.as_prior(bad)


def test_residual_clip_runs_in_corner_order_on_the_residuals(monkeypatch):
    """A rotation spreads dx, dy by design: the clip must see dx - dx_prior.  `ops.sigma_clip` is replaced by numpy's (`frames.sigma_clip`,
    which it equals bit for bit on the device) so that this runs without one."""
    from karios_amd import frames, ops
    seen = {}

    def fake(dx, dy, ctx=None):
        seen["dx"], seen["dy"] = dx.copy(), dy.copy()
        return frames.sigma_clip(dx, dy)
    monkeypatch.setattr(ops, "sigma_clip", fake)
    rng = np.random.default_rng(3)
    n = 50
    labels = rng.permutation(n)
    dxp, dyp = np.linspace(-30, 30, n).astype(np.float32), np.linspace(25, -25, n).astype(np.float32)       # far wider than the clip's 20 px
    res = (rng.standard_normal((n, 2)) * 0.05).astype(np.float32)
    res[labels == 7] = (4.0, 0.0)                                      # one row whose residual is an outlier
    frame = pd.DataFrame({"x0": np.arange(n, dtype=np.float32), "y0": np.zeros(n, np.float32), "dx": dxp + res[:, 0], "dy": dyp + res[:, 1],
                          "score": np.ones(n, np.float32), "dx_prior": dxp, "dy_prior": dyp}, index=labels)
    out = prior_mod.clip_residuals(frame)
    order = np.argsort(labels)
    assert np.array_equal(seen["dx"], (frame["dx"].to_numpy() - dxp)[order]) and seen["dx"].dtype == np.float32      # corner order, residuals
    assert len(out) == n - 1 and 7.0 not in labels[np.isin(frame["x0"], out["x0"])].tolist()
    assert np.array_equal(out["x0"].to_numpy(), np.sort(out["x0"].to_numpy()))                                       # the frame's row order stands
    kept_labels = labels[np.isin(frame["x0"].to_numpy(), out["x0"].to_numpy())]
    assert np.array_equal(np.asarray(out.index), np.argsort(np.argsort(kept_labels)))                                # position among the survivors


def test_prior_columns_are_the_float32_guess_minus_the_key_point():
    P = C.rotation_prior(1.0, sx=7, sy=3)
    x0 = np.float32([16 + 40, 16 + 90, 16 + 133])
    y0 = np.float32([8 + 30, 8 + 77, 8 + 120])
    frame = pd.DataFrame({"x0": x0, "y0": y0})
    dxp, dyp = prior_mod.prior_columns(frame, P, 16, 8)
    g, _ = PR.guess(P, np.stack([x0 - 16, y0 - 8], 1), 16, 8)
    assert dxp.dtype == np.float32 and _same_bits(dxp, g[:, 0] - (x0 - 16)) and _same_bits(dyp, g[:, 1] - (y0 - 8))
