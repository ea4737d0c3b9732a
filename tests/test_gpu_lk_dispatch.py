"""The tracker's window table (csrc/lk_launch.hpp: `lk_shape_of`) through every door that launches by it: the single launch in both
forms (`lk2_kernel*`, `lk_kernel<NR>`), the seeded launch (`lk2_seeded_kernel*`), the batched units (`lk2_units_kernel*`), and what each
door answers to a window outside 3..40.

Windows: 16 | 17, 30 | 31, 35 | 36 - the last and first window of the classes of 1 | 2, 3 | 4, 4 | 5 runs per lane -, 26 (2 | 3 lies
at 25 | 26, and 25 has kernels of its own, which the other suites hold), and 40, the upper bound.  The expected values are the CPU
oracle's, computed once per window; the seeded launch is held to the unseeded one (GPU against GPU, the pattern of
tests/test_gpu_lk_prior.py), which the same test holds to the oracle.

Shapes: one 120 x 200 Laplacian pair - level 1 is 60 x 100, wider than every window, so the second form serves it - with 40 key
points, twenty of them 2 .. 6 px from a border (their patches cross it at every window: the byte staging path, the derivative mask);
two units of 512 x 96 and 520 x 97 (tests/lk_cases.py: UNIT_BOXES) of a 120 x 540 textured pair."""
import functools

import numpy as np
import pytest

import lk_cases as LC

pytestmark = pytest.mark.gpu

WINDOWS = (16, 17, 26, 30, 31, 35, 36, 40)
KSIZE = 5
UNIT_MAX_CORNERS = 40


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, exp, what):
    got, exp = np.asarray(got, np.float32).reshape(-1, 2), np.asarray(exp, np.float32).reshape(-1, 2)
    assert got.shape == exp.shape, f"{what}: shape {got.shape}, expected {exp.shape}"
    bad = (_bits(got) != _bits(exp)).any(1)
    if bad.any():
        k = int(np.argmax(bad))
        pytest.fail(f"{what}: {int(bad.sum())} of {len(exp)} differ; first: index {k} got {got[k]!r} expected {exp[k]!r}", pytrace=False)


@functools.lru_cache(maxsize=None)
def _pair():
    """(prev, next): uint8 Laplacians of a 120 x 200 textured pair, read-only."""
    from karios_amd import synth
    from oracle import oracle as O
    mon, ref = synth.make_pair(120, 200, 0.4, -0.3, seed=20261021)
    out = O.laplacian_u8(O.to_uint8(ref), KSIZE), O.laplacian_u8(O.to_uint8(mon), KSIZE)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _points():
    """(40, 1, 2) float32: a 5 x 4 grid inside, four points along each border, one in each corner; integer and fractional positions."""
    h, w = 120, 200
    inside = [(x, y) for y in (30, 50.5, 70.25, 90) for x in (30, 65.5, 100.25, 135, 170.75)]
    top = [(40, 2), (90.5, 3.5), (140, 5), (180.25, 6.25)]
    left = [(2, 35), (3.5, 55.5), (5, 75), (6.25, 95.25)]
    border = top + [(x, h - 1 - y) for x, y in top] + left + [(w - 1 - x, y) for x, y in left]
    corners = [(3, 3), (w - 4.5, 2.5), (2.25, h - 4), (w - 3, h - 3.75)]
    pts = np.array(inside + border + corners, np.float64).astype(np.float32).reshape(-1, 1, 2)
    pts.setflags(write=False)
    return pts


def test_the_key_points_meet_every_border():
    pts = _points().reshape(-1, 2)
    assert len(pts) == 40
    for near in (pts[:, 0] < 16, pts[:, 0] > 199 - 16, pts[:, 1] < 16, pts[:, 1] > 119 - 16):
        assert near.sum() >= 4
    # the patch of a window starts (win - 1) / 2 + 3 px left of / above its key point: across the border for the smallest window
    assert (np.minimum.reduce([pts[:, 0], pts[:, 1], 199 - pts[:, 0], 119 - pts[:, 1]]) < 7.5 + 3).sum() >= 20


@functools.lru_cache(maxsize=None)
def _oracle_tracks(win):
    from oracle import oracle as O
    O.build()
    prev, nxt = _pair()
    p1 = O.pyr_lk(prev, nxt, _points(), win)
    p0r = O.pyr_lk(nxt, prev, p1, win)
    for a in (p1, p0r):
        a.setflags(write=False)
    return p1, p0r


@pytest.fixture
def lk2_option(ops):
    ctx = ops._lib.default_context()
    yield lambda v: ctx.set_option("lk2", v)
    ctx.set_option("lk2", 1)


# ---- (i) the single launch, both forms; (ii) the seeded launch ---------------------------------------------------------------------
@pytest.mark.parametrize("win", WINDOWS)
def test_single_launch_in_both_forms_against_the_oracle(ops, O, lk2_option, win):
    prev, nxt = _pair()
    pts = _points()
    p1, p0r = _oracle_tracks(win)
    assert np.abs(p1 - pts).max() > 0.1                                  # (the tracker has something to do)
    conf = O.default_conf(maxCorners=len(pts), matching_winsize=win)
    for lk2 in (1, 0):
        lk2_option(lk2)
        got = ops.calc_optical_flow_pyr_lk(prev, nxt, pts, winSize=(win, win))
        _assert_same(got, p1, f"winSize {win} lk2 {lk2}: forward")
        tracks = ops.klt_track(prev, nxt, None, conf, p0=pts)           # forward + backward in one launch
        _assert_same(tracks[0], pts, f"winSize {win} lk2 {lk2}: one launch, p0")
        _assert_same(tracks[1], p1, f"winSize {win} lk2 {lk2}: one launch, p1")
        _assert_same(tracks[2], p0r, f"winSize {win} lk2 {lk2}: one launch, p0r")


@pytest.mark.parametrize("win", WINDOWS)
def test_seeded_launch_from_the_key_points_equals_the_unseeded_launch(ops, O, win):
    prev, nxt = _pair()
    pts = _points()
    p1, p0r = _oracle_tracks(win)
    for a, b, start, exp, label in ((prev, nxt, pts, p1, "forward"), (nxt, prev, p1, p0r, "backward")):
        want = ops.calc_optical_flow_pyr_lk(a, b, start, winSize=(win, win))
        _assert_same(want, exp, f"winSize {win} {label}: unseeded against the oracle")
        got = ops.pyrlk_initial(a, b, start, start, winSize=(win, win))
        _assert_same(got, want, f"winSize {win} {label}: guesses = points")


# ---- (iii) batched units ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _raw_pair():
    from karios_amd import synth
    mon, ref = synth.make_pair(120, 540, 0.4, -0.3, seed=20261022)
    for a in (mon, ref):
        a.setflags(write=False)
    return mon, ref


@pytest.mark.parametrize("win", WINDOWS)
def test_a_batch_of_two_units_equals_the_units_alone_and_the_oracle(ops, O, win):
    from test_gpu_units import same_rows
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair, submit_units
    mon, ref = _raw_pair()
    pair = ResidentPair.upload(mon, ref, ctx=ops._lib.default_context())
    conf = KLTConfiguration(maxCorners=UNIT_MAX_CORNERS, matching_winsize=win, laplacian_kernel_size=KSIZE)
    alone = [pair.submit_tile(conf, box=b).result() for b in LC.UNIT_BOXES]
    batch = submit_units([(pair, b, None) for b in LC.UNIT_BOXES], conf)
    assert batch is not None                                             # (the batch form covers these units)
    got = list(batch.wait())
    for k, (g, w) in enumerate(zip(got, alone)):
        assert g.flags == 0 and w.flags == 0, (k, g.flags, w.flags)      # (the batched tracker's own rows, not a repeat)
        assert w.n_rows >= 8 and same_rows(g, w), f"winSize {win} unit {k}"
    x, y, w, h = LC.UNIT_BOXES[1]
    exp = O.klt_tile(mon[y:y + h, x:x + w], ref[y:y + h, x:x + w],
                     O.default_conf(maxCorners=UNIT_MAX_CORNERS, matching_winsize=win, laplacian_kernel_size=KSIZE))
    f = got[1].to_frame()
    assert len(exp["x0"]) >= 8
    for col, off in (("x0", x), ("y0", y), ("dx", 0), ("dy", 0), ("score", 0)):
        a, b = f[col].to_numpy(), np.asarray(exp[col] + off, np.float32)
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"winSize {win} unit 1 {col} against the oracle"


# ---- (iv) windows outside 3 .. 40 -----------------------------------------------------------------------------------------------------
def test_windows_outside_the_table_are_refused_as_before(ops, lk2_option):
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair, submit_units
    lib_mod = ops._lib
    prev, nxt = _pair()
    pts = _points()

    def refusal(call):
        with pytest.raises(lib_mod.KariosHipError) as e:
            call()
        return e.value.code, str(e.value)

    for lk2 in (1, 0):
        lk2_option(lk2)
        code, text = refusal(lambda: ops.calc_optical_flow_pyr_lk(prev, nxt, pts, winSize=(2, 2)))
        assert code == lib_mod.E_ARG and "pyrlk: winSize 2 / maxLevel 1" in text, (code, text)
        code, text = refusal(lambda: ops.calc_optical_flow_pyr_lk(prev, nxt, pts, winSize=(41, 41)))
        assert code == lib_mod.E_UNSUPPORTED and "winSize 41 (supported 3..40)" in text, (code, text)
    lk2_option(1)
    code, text = refusal(lambda: ops.pyrlk_initial(prev, nxt, pts, pts, winSize=(2, 2)))
    assert code == lib_mod.E_ARG and "pyrlk_initial: winSize 2 / maxLevel 1" in text, (code, text)
    code, text = refusal(lambda: ops.pyrlk_initial(prev, nxt, pts, pts, winSize=(41, 41)))
    assert code == lib_mod.E_UNSUPPORTED and "pyrlk_initial: winSize 41 / maxLevel 1 (the seeded tracker: maxLevel 1, winSize <= 40)" in text, (code, text)
    mon, ref = _raw_pair()
    pair = ResidentPair.upload(mon, ref, ctx=lib_mod.default_context())
    units = [(pair, b, None) for b in LC.UNIT_BOXES]
    code, text = refusal(lambda: submit_units(units, KLTConfiguration(maxCorners=UNIT_MAX_CORNERS, matching_winsize=2, laplacian_kernel_size=KSIZE)))
    assert code == lib_mod.E_ARG and "winSize 2 must be > 2" in text, (code, text)
    # (the batch form does not cover the window: no error, the caller goes unit by unit)
    assert submit_units(units, KLTConfiguration(maxCorners=UNIT_MAX_CORNERS, matching_winsize=41, laplacian_kernel_size=KSIZE)) is None
    # and the next calls return their usual bits
    _assert_same(ops.calc_optical_flow_pyr_lk(prev, nxt, pts, winSize=(17, 17)), _oracle_tracks(17)[0], "after the refusals")
