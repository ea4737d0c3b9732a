"""The corner detector's retry paths - key-buffer regrow, stage-overflow fallback to the two-kernel path, second selection
pass on all candidates, growth of the ranked prefix - and the wrap of the 3-slot frame ring fire only on unusual images or
by timing in normal operation.  The `km_set_option` test knobs shrink the capacities behind them so that each path runs
here on ordinary images; the result must not change (oracle parity, reference selection semantics klt.py:120)."""
import importlib.util
import os

import numpy as np
import pytest

from karios_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
fuzz = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fuzz)


def _lap(O, H, W, seed=0):
    mon, ref = synth.make_pair(H, W, 0.4, -0.3, seed=seed)
    return O.laplacian_u8(O.to_uint8(ref), 7)


@pytest.mark.parametrize("knobs,flag", [
    (dict(key_cap=48), 1), (dict(stage_cap=3), 2), (dict(topk_factor=1), 4), (dict(select_first=8), 8),
    (dict(key_cap=48, stage_cap=3, topk_factor=1, select_first=8, defer=0), 1 | 2 | 4 | 8),
    (dict(key_cap=48, topk_factor=1, select_first=8, fused_eig=0), 1 | 4 | 8),
])
def test_each_retry_path_runs_and_keeps_the_corners(ops, O, knobs, flag):
    img = _lap(O, 420, 610, seed=5)
    exp = O.good_features(img, None, 600, 0.01, 6.0, 15)
    with fuzz.forced_paths(knobs) as fp:
        got = ops.good_features_to_track(img, 600, 0.01, 6.0, blockSize=15)
        flags = int(fp.ctx.stats().path_flags)
    np.testing.assert_array_equal(got, exp)
    assert flags & flag == flag, f"path flags {flags:#x}: knobs {knobs} did not reach path(s) {flag:#x}"
    # and the knobs are gone again
    ops.good_features_to_track(img, 600, 0.01, 6.0, blockSize=15)
    assert int(fp.ctx.stats().path_flags) == 0


@pytest.mark.parametrize("seed", range(3000, 3040))
def test_speculative_path_tile_case_matches_oracle(ops, O, seed):
    """Random tile cases with the synchronisation-free corner path switched on (flagged tiles are repeated exactly)."""
    from karios_amd.resident import ResidentPair
    case = fuzz.draw_case(seed, max_size=380)
    case["knobs"] = dict(speculative=1)
    case["async_ring"] = 3 if seed % 3 == 0 else 0
    fails = fuzz.run_case(case, ops, O, ResidentPair)
    assert not fails, f"{fails} for {case}"


@pytest.mark.parametrize("seed", range(2000, 2060))
def test_forced_path_tile_case_matches_oracle(ops, O, seed):
    from karios_amd.resident import ResidentPair
    case = fuzz.draw_case(seed, max_size=380)
    case["knobs"] = fuzz.draw_knobs(seed)
    case["async_ring"] = (seed % 4) + 3 if seed % 2 else 0
    fails = fuzz.run_case(case, ops, O, ResidentPair)
    assert not fails, f"{fails} for {case}"


def test_frame_ring_wrap_keeps_every_waited_frame(ops, O):
    """Five submissions without a wait (3 slots): the library must finish an overwritten slot's frame before reusing it,
    and the three newest frames must be the synchronous ones."""
    from karios_amd.resident import ResidentPair
    mon, ref = synth.make_pair(300, 340, 0.3, 0.2, seed=11)
    conf = O.default_conf(maxCorners=300)
    pair = ResidentPair.upload(mon, ref)
    boxes = [(0, 0, 340, 300), (10, 20, 300, 250), (40, 0, 280, 300), (0, 30, 340, 260), (5, 5, 330, 290)]
    want = [pair.match_tile(conf, box=b, zncc_threshold=0.4) for b in boxes]
    pend = [pair.submit_tile(conf, box=b, zncc_threshold=0.4) for b in boxes]
    for p, w in list(zip(pend, want))[-3:]:
        f = p.result().to_frame()          # (a tile flagged by the synchronisation-free corner path is repeated exactly)
        assert list(f.columns) == list(w.columns) and len(f) == len(w)
        for col in f.columns:
            np.testing.assert_array_equal(f[col].to_numpy(), w[col].to_numpy())


def test_speculative_corner_path_flags_and_repeats(ops, O):
    """The synchronisation-free corner path (k_select2.hip) works with fixed capacities; a tile that does not fit raises a flag
    and is repeated through the exact path.  The test knob "spec_flag" raises a flag artificially: the tile is repeated and
    the result does not change; without it the same image is not flagged."""
    from karios_amd._lib import default_context
    from karios_amd.resident import ResidentPair
    mon, ref = synth.make_pair(420, 500, 0.4, 0.2, seed=3)
    ctx = default_context()
    for max_corners, expect_retry in ((700, True), (700, False), (3, False)):
        ctx.set_option("speculative", 1)
        ctx.set_option("spec_flag", 32 if expect_retry else 0)
        conf = O.default_conf(maxCorners=max_corners, laplacian_kernel_size=5)
        exp = O.klt_tile(mon, ref, conf)
        status, tracks = ops.klt_tile(ref, mon, conf, mon_ksize=5, ref_ksize=5)
        assert bool(ctx.stats().path_flags & 16) == expect_retry, ctx.stats().path_flags
        assert status == "ok" and len(tracks[0]) == exp["Ninit"] == max_corners
        pair = ResidentPair.upload(mon, ref)
        frame = pair.match_tile(conf, zncc_threshold=0.4)
        assert bool(ctx.stats().path_flags & 16) == expect_retry
        for col in ("x0", "y0", "dx", "dy", "score"):
            np.testing.assert_array_equal(frame[col].to_numpy(), exp[col])
        pend = pair.submit_tile(conf, zncc_threshold=0.4)
        raw = pend.wait()
        assert bool(raw.flags) == expect_retry
        f2 = pend.result().to_frame()
        for col in ("x0", "y0", "dx", "dy", "score", "zncc_score"):
            np.testing.assert_array_equal(f2[col].to_numpy(), frame[col].to_numpy())
        ctx.set_option("speculative", 0)
        f3 = pair.match_tile(conf, zncc_threshold=0.4)
        assert ctx.stats().path_flags & 16 == 0
        for col in ("x0", "y0", "dx", "dy", "score", "zncc_score"):
            np.testing.assert_array_equal(f3[col].to_numpy(), frame[col].to_numpy())
        ctx.set_option("spec_flag", 0)


def test_scatter_launch_second_read_when_the_stash_is_too_small(ops, O):
    """Launch 2 of the synchronisation-free ranking stashes a workgroup's kept keys in LDS (3072 slots) and reads the key buffer a
    second time when they do not fit.  "stash_cap" shrinks the stash so that every workgroup with kept keys takes the second read:
    same corners, same tracks, no flag."""
    from karios_amd._lib import default_context
    mon, ref = synth.make_pair(420, 500, 0.4, 0.2, seed=3)
    ctx = default_context()
    conf = O.default_conf(maxCorners=700, laplacian_kernel_size=5)
    exp = O.klt_tile(mon, ref, conf)
    try:
        for stash in (1, 7, 0):
            ctx.set_option("speculative", 1)
            ctx.set_option("stash_cap", stash)
            status, tracks = ops.klt_tile(ref, mon, conf, mon_ksize=5, ref_ksize=5)
            assert status == "ok" and not ctx.stats().path_flags & 16          # went through the speculative path, not repeated
            p0 = O.good_features(exp["lap_ref"], exp["mask"], 700, 0.1, 10, 15)
            np.testing.assert_array_equal(tracks[0], p0)
            np.testing.assert_array_equal(tracks[1], O.pyr_lk(exp["lap_ref"], exp["lap_mon"], p0, 25))
    finally:
        ctx.set_option("stash_cap", 0)


def test_page_locked_array_may_outlive_its_context(ops):
    """A `pinned_empty` array released after its context is gone (advisor, round 2): the finalizer then frees the block without
    touching the destroyed context (km_host_free(NULL, p)); the staging area a context owns is dropped before the context."""
    import gc
    from karios_amd._lib import Context, pinned_empty
    from karios_amd.resident import ResidentPair
    ctx = Context(0)
    keep = pinned_empty((300, 400), np.uint16, ctx)
    keep[:] = 7
    mon, ref = synth.make_pair(300, 400, 0.5, 0.25)
    pair = ResidentPair.upload(mon, ref, ctx=ctx)
    z = pair.zncc(np.array([100.0], np.float32), np.array([100.0], np.float32), np.array([0.5], np.float32), np.array([0.25], np.float32))
    assert z.shape == (1,) and "_kp_staging" in ctx.__dict__          # the context now owns page-locked staging
    del pair
    ctx.close()
    assert "_kp_staging" not in ctx.__dict__ and ctx.handle is None
    assert int(keep.sum()) == 7 * 300 * 400                            # still readable
    del keep
    gc.collect()                                                       # finalizer runs with the context closed: must not crash
    ctx2 = Context(0)                                                  # the device is still usable
    ctx2.sync()
    ctx2.close()


def test_frame_origin_must_be_a_tile_offset(ops, O):
    """The (x0, y0) ordering key of the device frame is built from corner + tile origin as non-negative integers (advisor, round 2):
    a negative or non-finite origin is refused, a large one is ordered exactly (bucket index clamped, order decided by the keys)."""
    from karios_amd._lib import KariosHipError
    from karios_amd.resident import ResidentPair
    mon, ref = synth.make_pair(300, 420, 0.4, 0.2, seed=11)
    conf = O.default_conf(maxCorners=500)
    pair = ResidentPair.upload(mon, ref)
    base = pair.match_tile(conf)
    for bad in ((-1.0, 0.0), (0.0, float("nan")), (float("inf"), 0.0), (3e9, 0.0)):
        with pytest.raises(KariosHipError, match="tile origin"):
            pair.match_tile(conf, origin=bad)
    far = pair.match_tile(conf, origin=(1 << 20, 1 << 21))             # beyond the bucket range of the placement kernel
    np.testing.assert_array_equal(far["x0"].to_numpy(), base["x0"].to_numpy() + np.float32(1 << 20))
    np.testing.assert_array_equal(far["y0"].to_numpy(), base["y0"].to_numpy() + np.float32(1 << 21))
    for col in ("dx", "dy", "score"):
        np.testing.assert_array_equal(far[col].to_numpy(), base[col].to_numpy())
    assert (np.diff(far["x0"].to_numpy()) >= 0).all()


def test_band_tracker_with_a_three_level_pyramid_equals_the_full_image(ops, O):
    """km_band_track_dev on a row band with maxLevel 2 (the matcher itself uses 1): the rows of level l that the 5-tap pyrDown
    computed from a mirrored band edge are declared absent with the recurrence trim_l = ceil((trim_{l-1} + 2) / 2) = 1, 2, 2
    (advisor, round 2: one row per level was too few from level 2 on) - tracks inside the band equal the full image's, a window that
    reaches the trimmed rows raises the flag instead of reading them."""
    import ctypes as C
    from karios_amd._lib import default_context
    from karios_amd.ops import make_params
    from karios_amd.resident import DeviceBuffer
    H, W, ys, hs = 600, 500, 104, 392
    mon, ref = synth.make_pair(H, W, 0.7, -0.4, seed=21)
    lap_ref, lap_mon = O.laplacian_u8(O.to_uint8(ref), 7), O.laplacian_u8(O.to_uint8(mon), 7)
    ctx = default_context()
    d_ref, d_mon = DeviceBuffer(ctx, hs * W), DeviceBuffer(ctx, hs * W)
    d_ref.upload(lap_ref[ys:ys + hs])
    d_mon.upload(lap_mon[ys:ys + hs])
    prm = make_params(O.default_conf(maxCorners=100))
    prm.max_level = 2
    p0 = O.good_features(lap_ref, None, 4000, 0.02, 6, 9).reshape(-1, 2)
    inside = p0[(p0[:, 1] >= 230) & (p0[:, 1] <= 370)][:300].copy()
    assert len(inside) > 50

    def band_track(pts):
        p1, p0r, left = np.empty_like(pts), np.empty_like(pts), C.c_int()
        ctx.check(ctx.lib.km_band_track_dev(ctx.handle, C.c_void_p(d_ref.ptr), C.c_void_p(d_mon.ptr), hs, W, ys, H, C.byref(prm),
                                            pts.ctypes.data_as(C.c_void_p), len(pts), p1.ctypes.data_as(C.c_void_p), p0r.ctypes.data_as(C.c_void_p),
                                            C.byref(left)), "km_band_track_dev")
        return p1, p0r, left.value

    p1, p0r, left = band_track(inside)
    e1 = O.pyr_lk(lap_ref, lap_mon, inside, 25, max_level=2)
    e0r = O.pyr_lk(lap_mon, lap_ref, e1, 25, max_level=2)
    assert left == 0
    np.testing.assert_array_equal(p1, e1.reshape(-1, 2))
    np.testing.assert_array_equal(p0r, e0r.reshape(-1, 2))
    # a point whose level-2 window needs the rows next to the band edge
    edge = np.array([[250.0, ys + 44.0]], np.float32)
    assert band_track(edge)[2] == 1


def test_early_minmax_of_back_to_back_units_belongs_to_the_right_unit():
    """A unit submitted directly behind another one computes its min / max on the second stream beside the previous unit's LK
    (`mm_early`, KM_PATH_MM_EARLY).  Units of different content, size and pixel type, through one context, must each get the
    stretch of THEIR OWN rasters (`_to_uint8`, klt.py:42-49): frames equal to the blocking call with the feature switched off."""
    import pandas as pd
    from karios_amd._lib import Context
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair
    from karios_amd.stream import FrameStream
    conf = KLTConfiguration(maxCorners=500)
    specs = [(520, 640, 1.0, 0, np.uint16), (700, 530, 0.31, 900, np.uint16), (512, 512, 2.5, 40, np.float32), (610, 700, 0.05, 3000, np.uint16),
             (520, 640, 1.7, -200, np.int16), (530, 520, 1.0, 0, np.uint8), (640, 600, 0.6, 12000, np.uint16)]
    ctx, plain = Context(0), Context(0)
    plain.set_option("mm_early", 0)
    pairs, want, raw = [], [], []
    for i, (H, W, gain, bias, dt) in enumerate(specs):
        mon, ref = synth.make_pair(H, W, 0.3 + 0.1 * i, -0.2, seed=40 + i)
        conv = lambda a: (np.clip(a.astype(np.float64) * gain + bias, 0, 255) if dt == np.uint8 else a.astype(np.float64) * gain + bias).astype(dt)
        mon, ref = conv(mon // (64 if dt == np.uint8 else 1)), conv(ref // (64 if dt == np.uint8 else 1))
        raw.append((mon, ref))
        pairs.append(ResidentPair.upload(mon, ref, ctx=ctx))
        want.append(ResidentPair.upload(mon, ref, ctx=plain).match_tile(conf, zncc_threshold=0.4))
    got, early = [], 0
    with FrameStream(0.4, depth=1, score_columns=False) as s:
        for p in pairs:
            got += [r.frame for r in s.submit(p, conf)]
            early += bool(int(ctx.stats().path_flags) & 32)
        got += [r.frame for r in s.drain()]
    assert early >= len(specs) - 2, f"the early min / max path ran for {early} of {len(specs)} units"   # (not the first; not the uint8 unit)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(want, got)):
        assert (a is None) == (b is None), i
        if a is not None:
            pd.testing.assert_frame_equal(a.reset_index(drop=True), b.reset_index(drop=True), check_exact=True, obj=f"unit {i}")
    # a call in between takes the feature off for the unit that follows it: here the call PRODUCES that unit's raster on the main
    # stream (km_shift_image_dev), which a kernel on the second stream would not be ordered behind
    p0 = pairs[0].submit_tile(conf, zncc_threshold=0.4)
    shifted = pairs[1].shifted_monitored(3, -2)
    p1 = shifted.submit_tile(conf, zncc_threshold=0.4)
    assert not int(ctx.stats().path_flags) & 32
    p3 = pairs[3].submit_tile(conf, zncc_threshold=0.4)
    assert int(ctx.stats().path_flags) & 32
    want_shifted = ResidentPair.upload(raw[1][0], raw[1][1], ctx=plain).shifted_monitored(3, -2).match_tile(conf, zncc_threshold=0.4)
    pd.testing.assert_frame_equal(want_shifted.reset_index(drop=True), p1.result().to_frame().reset_index(drop=True), check_exact=True)
    pd.testing.assert_frame_equal(want[3].reset_index(drop=True), p3.result().to_frame().reset_index(drop=True), check_exact=True)
    pd.testing.assert_frame_equal(want[0].reset_index(drop=True), p0.result().to_frame().reset_index(drop=True), check_exact=True)
    ctx.close(); plain.close()


def test_contexts_can_be_created_used_and_closed_repeatedly(ops):
    """Every stream, event and buffer of a context has an owner that releases it with the context (csrc/common.hpp).  Three fresh
    contexts in turn go through the lazy creation sites a frame stream reaches - stage timers, the copy stream with a ticket, a
    submitted tile, two pipelined batched submissions with their flush - and are closed; a fourth one, created after all that, still
    works.  Frames must not depend on which context made them: header and every row of every column equal bit for bit (`same_rows`
    of tests/test_gpu_units.py: the words as integers - a score below the threshold is a NaN, which no float comparison finds equal
    to itself - and no further than the last row, behind which a column is device memory no kernel wrote).  (Nothing is
    measured here: that no handle or allocation is left behind is proven on the CPU against the stand-in HIP layer,
    tests/test_ctx_lifetime_host.py.)"""
    from karios_amd._lib import Context, pinned_empty
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair, submit_units
    from test_gpu_units import same_rows
    conf = KLTConfiguration(maxCorners=64, blocksize=3, matching_winsize=25)
    mon, ref = synth.make_pair(128, 512, 0.5, 0.25, seed=5)
    assert mon.dtype == np.uint16

    def life_of_a_context():
        ctx = Context(0)
        ctx.set_profiling(True)
        mon_p, ref_p = pinned_empty(mon.shape, mon.dtype, ctx), pinned_empty(ref.shape, ref.dtype, ctx)
        mon_p[:], ref_p[:] = mon, ref
        pair = ResidentPair.upload(mon_p, ref_p, ctx=ctx)
        tile = pair.submit_tile(conf, zncc_threshold=0.4)
        ctx.set_option("units_pipeline", 1)
        units = [(pair, (0, 0, 512, 64), None), (pair, (0, 64, 512, 64), None)]      # two units of 64 x 512
        batches = [submit_units(units, conf, 0.4), submit_units(units, conf, 0.4)]
        assert None not in batches
        raws = [tile.wait()] + [r for b in batches for r in b.wait()]               # (the last wait flushes the deferred tail)
        assert all(r.flags == 0 and r.n_rows > 0 for r in raws), [(r.flags, r.n_rows) for r in raws]
        del pair, tile, batches                  # (the frames' blocks are copies: they outlive the context)
        ctx.close()
        assert ctx.handle is None
        return raws

    first = life_of_a_context()
    assert len(first) == 5
    for cycle in (2, 3, 4):                  # (4: the context created after three went through create, use, close)
        for k, (got, want) in enumerate(zip(life_of_a_context(), first)):
            assert same_rows(got, want), (cycle, k)
