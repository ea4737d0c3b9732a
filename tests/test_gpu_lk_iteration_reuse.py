"""LK iteration loop of the resident-patch form (csrc/k_lk2.hip, `lk2_track_point`): an iteration reads the search patch from LDS and
cuts the runs' vertical byte pairs again only when the window's integer position moved since the previous iteration of the pass
(km_set_option "lk_reuse", default 1); with 0 every iteration does.  The integers are the same either way, so every comparison here
is `array_equal` - against the oracle, and between the two settings - on p1, p0r and the frame columns.

Single-tile entry points (`km_pyrlk`, `km_klt_track` -> `lk2_kernel*`) on 160 x 640 Laplacian pairs with about 300 key points; the
batched form (`lk2_units_kernel*`) on two units of 96 x 512 and 61 x 515 of a uint8 pair."""
import numpy as np
import pytest

from karios_amd import synth

pytestmark = pytest.mark.gpu

H, W = 160, 640
_scenes = {}


def _scene(O, sx, sy, warp=0.0, seed=20260311):
    """(lap_ref, lap_mon, p0): uint8 Laplacians of a textured pair whose monitored image is the reference moved by (sx, sy) plus a smooth
    warp of amplitude `warp` px and noise, and about 300 integer corners of the reference (goodFeaturesToTrack).  Built once per key."""
    key = (sx, sy, warp, seed)
    if key not in _scenes:
        from scipy import ndimage as ndi
        base = synth.make_base(H, W, seed)
        P = synth.PAD
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        wx = warp * np.sin(2 * np.pi * xx / 97.0 + yy / 31.0)
        wy = warp * np.cos(2 * np.pi * yy / 61.0 + xx / 43.0)
        mon_f = ndi.map_coordinates(base, [P + yy - sy - wy, P + xx - sx - wx], order=1).astype(np.float32)
        mon_f += np.random.default_rng(seed + 1).normal(0, 15.0, (H, W)).astype(np.float32)
        ref = np.clip(np.rint(base[P:P + H, P:P + W]), 1, 16000).astype(np.uint16)
        mon = np.clip(np.rint(mon_f), 1, 16000).astype(np.uint16)
        lap_ref, lap_mon = O.laplacian_u8(O.to_uint8(ref), 7), O.laplacian_u8(O.to_uint8(mon), 7)
        p0 = O.good_features(lap_ref, None, 300, 0.02, 12, 9)
        assert p0 is not None and len(p0) >= 200
        for a in (lap_ref, lap_mon, p0):
            a.setflags(write=False)
        _scenes[key] = (lap_ref, lap_mon, p0)
    return _scenes[key]


def _on_and_off(ops, run):
    """`run()` with "lk_reuse" 1 and 0 -> (result with reuse, result without)."""
    ctx = ops._lib.default_context()
    out = []
    try:
        for v in (1, 0):
            ctx.set_option("lk_reuse", v)
            out.append(run())
    finally:
        ctx.set_option("lk_reuse", 1)
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def _check_track(ops, O, lap_ref, lap_mon, p0, win=25):
    """Forward + backward in one launch (`km_klt_track` with given corners): reuse on == reuse off == the oracle's two calls."""
    conf = O.default_conf(maxCorners=len(p0), matching_winsize=win)
    on, off = _on_and_off(ops, lambda: ops.klt_track(lap_ref, lap_mon, None, conf, p0=p0))
    p1 = O.pyr_lk(lap_ref, lap_mon, p0, win)
    p0r = O.pyr_lk(lap_mon, lap_ref, p1, win)
    _same(on, (np.asarray(p0, np.float32).reshape(-1, 1, 2), p1, p0r))
    _same(off, on)
    return p1, p0r


def test_floor_never_moves_after_the_first_iteration(ops, O):
    """Shift (0.3, 0.3) px, integer corners: the forward pass starts at an integer position (at level 1 at a multiple of 0.5), the first
    step lands about 0.3 (0.15) px further and every later step is a correction of hundredths of a pixel, so floor(nextPt) is the start's in
    every iteration: the first iteration of each level cuts the byte pairs, every later one reuses them.  The oracle's iteration counts
    show that there ARE later iterations."""
    lap_ref, lap_mon, p0 = _scene(O, 0.3, 0.3)
    p1, _ = _check_track(ops, O, lap_ref, lap_mon, p0)
    _, it0, it1 = O.pyr_lk(lap_ref, lap_mon, p0, 25, return_iters="levels")
    assert np.median(it0) >= 2 and np.median(it1) >= 2
    d = (p1 - p0).reshape(-1, 2)
    assert np.median(np.abs(d - 0.3)) < 0.1 and (np.floor(p0.reshape(-1, 2) + d) == p0.reshape(-1, 2)).mean() > 0.9


def test_floor_flips_between_consecutive_iterations(ops, O):
    """Shift (1.0, 1.0) px plus a smooth warp of +-0.02 px and noise: level 1 converges to start + 0.5 and level 0 to start + 1.0 - an
    integer coordinate for the integer corners, approached from either side by steps of hundredths of a pixel.  floor(nextPt) is then
    start or start + 1 from one iteration to the next: iterations that cut the pairs and iterations that reuse them alternate within a
    pass.  The results lie on both sides of the integer, which is what makes the floor flip."""
    lap_ref, lap_mon, p0 = _scene(O, 1.0, 1.0, warp=0.02)
    p1, p0r = _check_track(ops, O, lap_ref, lap_mon, p0)
    d = (p1 - p0).reshape(-1, 2)
    near = np.abs(d - 1.0).max(1) < 0.08
    assert near.mean() > 0.5
    assert (d[near] < 1.0).any() and (d[near] > 1.0).any()
    _, it0, _ = O.pyr_lk(lap_ref, lap_mon, p0, 25, return_iters="levels")
    assert np.median(it0) >= 2


@pytest.mark.parametrize("shift", [(5.6, -5.3), (-5.9, 5.4)])
def test_restage_inside_the_loop_with_reused_iterations_behind_it(ops, O, shift):
    """A shift of 5 - 6 px is more than the patches' margin (LK2_M = 3): level 0 starts 2 x 2.7 px away from where its patch was centred,
    so the search patch is re-centred (`lk2_restage`) inside the iteration loop - which invalidates the kept pairs -, and the iterations
    behind it converge by sub-pixel steps and reuse them.  The backward pass does the same from sub-pixel starts."""
    lap_ref, lap_mon, p0 = _scene(O, shift[0], shift[1], seed=20260312)
    p1, _ = _check_track(ops, O, lap_ref, lap_mon, p0)
    assert (np.abs(p1 - p0).reshape(-1, 2).max(1) > 3).mean() > 0.5      # (more than LK2_M: these points' level-0 patch was re-centred)


def test_borders_and_points_that_leave_the_image(ops, O):
    """Key points closer than winSize to each of the four borders (border staging with REFLECT_101 instead of dword loads, `need_mask` for
    the derivatives), points whose window is carried out of the image by the shift or starts outside it (the `break` exits of the loop,
    levels skipped altogether): a pass that ends early must not leave pairs behind that a later pass or level takes for its own."""
    lap_ref, lap_mon, p0 = _scene(O, 2.4, -1.6, seed=20260313)
    xs = np.arange(3, W - 2, 29, dtype=np.float32)
    ys = np.arange(2, H - 1, 13, dtype=np.float32)
    edge = [(x, y) for x in xs for y in (0.0, 5.0, 20.0, H - 21.0, H - 4.0, H - 1.0)] + \
           [(x, y) for y in ys for x in (0.0, 3.0, 19.0, W - 22.0, W - 3.0, W - 1.0)]
    gone = [(-30.0, 5.0), (W + 40.0, 100.0), (100.0, H + 90.0), (-1e6, 1e6), (-13.0, 40.0), (W + 11.5, 80.25), (300.5, -12.25), (200.0, H + 12.0),
            (-24.0, -24.0), (W - 0.5, H - 0.5)]
    pts = np.concatenate([p0.reshape(-1, 2)[:120], np.array(edge + gone, np.float32)]).reshape(-1, 1, 2)
    _check_track(ops, O, lap_ref, lap_mon, pts)
    # the other direction: the shift now carries windows out over the opposite borders
    _check_track(ops, O, lap_mon, lap_ref, pts)


@pytest.mark.parametrize("max_count", [1, 2, 30])
def test_iteration_caps(ops, O, max_count):
    """maxCount 1: only the cutting iteration runs; 2: exactly one iteration may reuse; 30: the cap is never the reason to stop.  Forward
    (`km_pyrlk`), then a backward launch from the forward pass's sub-pixel results."""
    lap_ref, lap_mon, p0 = _scene(O, 0.3, 0.3)

    def run():
        f = ops.calc_optical_flow_pyr_lk(lap_ref, lap_mon, p0, maxCount=max_count)
        return f, ops.calc_optical_flow_pyr_lk(lap_mon, lap_ref, f, maxCount=max_count)

    on, off = _on_and_off(ops, run)
    p1 = O.pyr_lk(lap_ref, lap_mon, p0, 25, max_count=max_count)
    _same(on, (p1, O.pyr_lk(lap_mon, lap_ref, p1, 25, max_count=max_count)))
    _same(off, on)


def test_epsilon_that_stops_after_the_first_iteration(ops, O):
    """epsilon 5 px: the first step (0.3 - 1 px) is already below it, so every level and pass ends behind its first - cutting - iteration
    and the kept pairs are never used; the next level / pass has to cut its own."""
    lap_ref, lap_mon, p0 = _scene(O, 1.0, 1.0, warp=0.02)

    def run():
        f = ops.calc_optical_flow_pyr_lk(lap_ref, lap_mon, p0, epsilon=5.0)
        return f, ops.calc_optical_flow_pyr_lk(lap_mon, lap_ref, f, epsilon=5.0)

    on, off = _on_and_off(ops, run)
    p1, it = O.pyr_lk(lap_ref, lap_mon, p0, 25, eps=5.0, return_iters=True)
    assert it.max() <= 1
    _same(on, (p1, O.pyr_lk(lap_mon, lap_ref, p1, 25, eps=5.0)))
    _same(off, on)


def test_oscillation_stop(ops, O):
    """The construction of test_gpu_parity.py::test_lk_oscillation_literal (|delta + prevDelta| driven to float32(0.01) and one ulp either
    side) under both settings: the predicate decides on the steps alone, never on whether an iteration cut or reused its pairs.  The
    flip-flop scene above is where the stop fires inside the kernel (steps of alternating sign around an integer coordinate)."""
    from test_oracle_golden import _oscillation_quads
    q, want = _oscillation_quads()
    on, off = _on_and_off(ops, lambda: ops.lk_oscillation_probe(q))
    np.testing.assert_array_equal(on, want)
    np.testing.assert_array_equal(off, want)


@pytest.mark.parametrize("win", [9, 25, 38])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "forward_backward"])
def test_window_sizes(ops, O, win, backward):
    """winSize 9 / 25 / 38 = 1 / 2 / 5 runs per lane (NR): the generic kernels `lk2_kernel<NR, 0, ..>` and the win-25 kernel with its
    compile-time sizes; forward only (`km_pyrlk`) and forward + backward in one launch (`km_klt_track`)."""
    lap_ref, lap_mon, p0 = _scene(O, 0.3, 0.3)
    if backward:
        _check_track(ops, O, lap_ref, lap_mon, p0, win)
    else:
        on, off = _on_and_off(ops, lambda: ops.calc_optical_flow_pyr_lk(lap_ref, lap_mon, p0, winSize=(win, win)))
        np.testing.assert_array_equal(on, O.pyr_lk(lap_ref, lap_mon, p0, win))
        np.testing.assert_array_equal(off, on)


def test_batched_units_in_a_pipelined_stream(ops, O):
    """Two units (96 x 512 and 61 x 515: one block row short of a second band, an odd width) of a uint8 pair through `submit_many`, three
    submissions in a pipelined FrameStream: the tail of a submission - `lk2_units_kernel_win25` among it - is launched by the NEXT
    submission (or the drain), with the option as it stood when the submission was prepared.  Frames with reuse == frames without ==
    the oracle's tile."""
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair, submit_units
    from karios_amd.stream import FrameStream
    mon16, ref16 = synth.make_pair(200, 660, 0.3, 0.3, seed=20260314)
    mon, ref = (mon16 >> 5).astype(np.uint8), (ref16 >> 5).astype(np.uint8)
    ctx = ops._lib.default_context()
    pair = ResidentPair.upload(mon, ref, ctx=ctx)
    conf = KLTConfiguration(maxCorners=400)
    boxes = [(0, 0, 512, 96), (101, 90, 515, 61)]
    units = [(pair, b, None) for b in boxes]
    probe = submit_units(units, conf)
    assert probe is not None and len(probe.wait()) == 2          # (the batch form covers these units: the stream below uses it)

    def run():
        done = []
        with FrameStream(None, depth=2) as s:
            for _ in range(3):
                done += s.submit_many(units, conf)
                assert ctx.get_option("units_pipeline", 0) == 1
            done += s.drain()
        assert not all(d.redone for d in done)                   # (a unit repeated alone would go through the single-tile kernel)
        return [d.frame for d in done]

    on, off = _on_and_off(ops, run)
    assert len(on) == len(off) == 6
    for a, b in zip(on, off):
        assert list(a.columns) == list(b.columns) and len(a) == len(b) > 20
        for col in a.columns:
            np.testing.assert_array_equal(a[col].to_numpy(), b[col].to_numpy())
    for k, (x, y, w, h) in enumerate(boxes):
        exp = O.klt_tile(mon[y:y + h, x:x + w], ref[y:y + h, x:x + w], O.default_conf(maxCorners=400))
        for f in on[k::2]:
            np.testing.assert_array_equal(f["x0"].to_numpy(), exp["x0"] + x)
            np.testing.assert_array_equal(f["y0"].to_numpy(), exp["y0"] + y)
            np.testing.assert_array_equal(f["dx"].to_numpy(), exp["dx"])
            np.testing.assert_array_equal(f["dy"].to_numpy(), exp["dy"])
