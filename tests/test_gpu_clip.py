"""The tracker's outlier filter (`outliers_filtering`, reference karios/matcher/klt.py:52-71) on the device: `ops.sigma_clip`
(km_sigma_clip_dev, csrc/k_clip.hip) against numpy and the restatement, and the clip as a stage of every frame path
(km_set_option "frame_clip"): one tile against the kept host path and the oracle, batched units against unit-by-unit submissions, the
software pipeline with the filter alternating, a flagged unit's exact repeat, the frame sink of `parallel.match_distributed`."""
import functools

import numpy as np
import pytest

import clip_restatement as R

from karios_amd import frames, synth

pytestmark = pytest.mark.gpu
f32 = np.float32


@functools.lru_cache(maxsize=None)
def fixtures():
    return {name: (dx, dy) for name, dx, dy in R.fixtures()}


@functools.lru_cache(maxsize=None)
def restated(name):
    return R.sigma_clip(*fixtures()[name])


def numpy_clip(dx, dy):
    with np.errstate(all="ignore"):
        return frames.sigma_clip(dx, dy)


# ---- ops.sigma_clip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS + ("order", "special"))
def test_sigma_clip_equals_numpy_and_the_restatement(ops, kind):
    names = list(R.special_cases()) if kind == "special" else [n for n in fixtures() if n.startswith(kind + "_")]
    assert names
    for start in range(0, len(names), 16):
        part = names[start:start + 16]
        got = ops.sigma_clip_batch([fixtures()[n] for n in part])
        for name, (keep, rounds) in zip(part, got):
            dx, dy = fixtures()[name]
            assert keep.dtype == np.int64 and np.array_equal(keep, numpy_clip(dx, dy)), name
            assert rounds == restated(name)[1] and np.array_equal(keep, restated(name)[0]), name


def test_one_batched_call_with_units_of_every_kind(ops):
    """Units of different length in ONE launch (unit = blockIdx.y): an empty one, one that ends empty, one of the full 32768 rows."""
    names = ["empty", "tails_1000", "nan_dx", "offset_8193", "far_32768", "single", "order_12000_5", "exactly_20", "tails_2", "constant_dy"]
    got = ops.sigma_clip_batch([fixtures()[n] for n in names])
    for name, (keep, rounds) in zip(names, got):
        assert np.array_equal(keep, numpy_clip(*fixtures()[name])) and rounds == restated(name)[1], name
    assert [len(got[names.index(n)][0]) for n in ("empty", "nan_dx", "single", "constant_dy")] == [0, 0, 0, 0]
    assert got[0][1] == 0 and got[2][1] == 1 and len(got[4][0]) > 20000
    # the single-pair form, and the same call a second time (the workspace is reused)
    dx, dy = fixtures()["order_8969_2"]
    keep, rounds = ops.sigma_clip(dx, dy, return_rounds=True)
    assert np.array_equal(keep, numpy_clip(dx, dy)) and rounds == restated("order_8969_2")[1]
    assert np.array_equal(ops.sigma_clip(dx, dy), keep)


def test_sigma_clip_on_device_tensors(ops):
    import torch
    names = ["tails_257", "order_12000_2", "empty", "far_20000"]
    dev = torch.device("cuda", ops._lib.default_context().device)
    units = [tuple(torch.from_numpy(a).to(dev) for a in fixtures()[n]) for n in names]
    got = ops.sigma_clip_batch(units)
    for name, (keep, rounds) in zip(names, got):
        assert keep.device.type == "cuda" and keep.dtype == torch.int64
        assert np.array_equal(keep.cpu().numpy(), numpy_clip(*fixtures()[name])) and rounds == restated(name)[1], name
    with pytest.raises(ops.KariosHipError):
        ops.sigma_clip(torch.zeros(R.MAX_ROWS + 1, device=dev), torch.zeros(R.MAX_ROWS + 1, device=dev))
    # a numpy pair the device form does not hold goes to numpy on the host
    big = (0.3 * np.random.default_rng(3).standard_t(3, R.MAX_ROWS + 5)).astype(f32)
    assert np.array_equal(ops.sigma_clip(big, big[::-1].copy()), numpy_clip(big, big[::-1].copy()))


# ---- the clip as a stage of the frame paths ------------------------------------------------------------------------------------------------
def displaced_scene(H, W, seed, blocks):
    """`synth.make_pair` whose monitored image is displaced by a further sub-pixel amount inside `blocks` = [((ex, ey), (y0, y1, x0,
    x1)), ...]: the tracks there pass the forward-backward test and fail the 3-sigma rule."""
    mon, ref = synth.make_pair(H, W, 0.5, 0.25, seed=seed)
    mon = mon.copy()
    for (ex, ey), (y0, y1, x0, x1) in blocks:
        other, _ = synth.make_pair(H, W, 0.5 + ex, 0.25 + ey, seed=seed)
        mon[y0:y1, x0:x1] = other[y0:y1, x0:x1]
    return mon, ref


TILE_BLOCKS = [((0.9, -0.8), (40, 120, 400, 500)), ((0.45, 0.4), (150, 230, 100, 260))]      # chosen on the CPU with the oracle


def test_one_tile_equals_the_host_path_and_the_oracle(ops, O):
    from karios_amd.resident import ResidentPair
    mon, ref = displaced_scene(256, 640, 21, TILE_BLOCKS)
    on, off = O.default_conf(maxCorners=400, outliers_filtering=True), O.default_conf(maxCorners=400)
    exp, exp_off = O.klt_tile(mon, ref, on), O.klt_tile(mon, ref, off)
    pair = ResidentPair.upload(mon, ref)
    plain = pair.match_tile(off)
    # the scene does what it was chosen for: the clip drops at least 5 % of the rows that passed the FB test, in at least two rounds
    order = np.argsort(plain.index.to_numpy())
    keep, rounds = R.sigma_clip(plain["dx"].to_numpy()[order], plain["dy"].to_numpy()[order])
    assert rounds >= 2 and len(keep) <= 0.95 * len(plain) and len(exp["x0"]) <= 0.95 * len(exp_off["x0"])
    host = pair._match_tile_host_clip(on, None, 0, 0, 0.4)
    host = pair.score_frame(host, 0.4, mutual_info=True)
    got = pair.match_tile(on, zncc_threshold=0.4, mutual_info=True)
    assert len(got) == len(keep) == len(exp["x0"]) and got.attrs["Ninit"] == host.attrs["Ninit"] == exp["Ninit"]
    assert got.index.equals(host.index)
    for col in ("x0", "y0", "dx", "dy", "score", "zncc_score", "mutual_info_score", "mi_score"):
        np.testing.assert_array_equal(got[col].to_numpy(), host[col].to_numpy(), err_msg=col)
    for col in ("x0", "y0", "dx", "dy", "score"):
        np.testing.assert_array_equal(got[col].to_numpy(), exp[col], err_msg=col)
    assert np.isfinite(got["zncc_score"].to_numpy()).sum() > 100
    # the bare frame, the raw form and the submitted form deliver the same rows
    bare = pair.match_tile(on)
    raw = pair.match_tile_raw(on, zncc_threshold=0.4, mutual_info=True).to_frame()
    sub = pair.submit_tile(on, zncc_threshold=0.4, mutual_info=True).result().to_frame()
    for f, cols in ((bare, ("x0", "y0", "dx", "dy", "score")), (raw, tuple(got.columns)), (sub, tuple(got.columns))):
        assert f.index.equals(got.index)
        for col in cols:
            np.testing.assert_array_equal(f[col].to_numpy(), got[col].to_numpy(), err_msg=col)
    # the filter off: nothing moved
    assert pair.match_tile(off).equals(plain) and len(plain) == len(exp_off["x0"])


UNIT_BLOCKS = [((0.9, -0.8), (100, 260, 300, 520)), ((0.45, 0.4), (500, 700, 900, 1200)), ((1.1, 0.9), (650, 800, 150, 400))]
UNIT_BOXES = [(0, 0, 700, 450), (700, 0, 700, 900), (100, 380, 1024, 520)]      # three shapes, each >= 512 columns


@functools.lru_cache(maxsize=None)
def unit_scene():
    return displaced_scene(900, 1400, 33, UNIT_BLOCKS)


def same_rows(a, b, header_words=4) -> bool:
    """Two frame blocks hold the same frame: header and, column by column, the first n_rows entries.  (header_words 2: an exact repeat
    does not carry the candidate count of the synchronisation-free corner path in word 3.)"""
    ia, ib = a.block.view(np.int32), b.block.view(np.int32)
    if not np.array_equal(ia[:header_words], ib[:header_words]) or a.cap != b.cap or a.with_zncc != b.with_zncc:
        return False
    n, cap = int(ia[0]), a.cap
    base = 4 + 6 * cap
    return (all(np.array_equal(ia[4 + k * cap:4 + k * cap + n], ib[4 + k * cap:4 + k * cap + n]) for k in range(6)) and
            all(np.array_equal(ia[base + 2 * k * cap:base + 2 * k * cap + 2 * n], ib[base + 2 * k * cap:base + 2 * k * cap + 2 * n])
                for k in range(int(a.with_zncc))))


@pytest.fixture(scope="module")
def unit_frames(ops):
    """The three units one by one (blocking tile calls), filter on and off: what every batched / pipelined form must deliver."""
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import RawFrame, ResidentPair
    ctx = ops._lib.default_context()
    pair = ResidentPair.upload(*unit_scene(), ctx=ctx)
    on, off = KLTConfiguration(maxCorners=900, outliers_filtering=True), KLTConfiguration(maxCorners=900)

    def one(conf, box):
        raw = pair.match_tile_raw(conf, box, 0.4)
        return RawFrame(raw.block.copy(), raw.cap, raw.with_zncc)
    want = {True: [one(on, b) for b in UNIT_BOXES], False: [one(off, b) for b in UNIT_BOXES]}
    # the filter has work to do in every unit, and the unit-by-unit frame IS the host path's
    for k, box in enumerate(UNIT_BOXES):
        assert want[True][k].flags == 0 and want[True][k].n_rows <= 0.97 * want[False][k].n_rows, k
        host = pair._match_tile_host_clip(on, box, box[0], box[1], 0.4)
        f = want[True][k].to_frame()
        assert f.index.equals(host.index)
        for col in ("x0", "y0", "dx", "dy", "score", "zncc_score"):
            np.testing.assert_array_equal(f[col].to_numpy(), host[col].to_numpy(), err_msg=f"{k} {col}")
    return ctx, pair, on, off, want


def test_units_submitted_together_are_clipped_like_units_one_by_one(unit_frames):
    from karios_amd.resident import submit_units
    ctx, pair, on, off, want = unit_frames
    units = [(pair, b, None) for b in UNIT_BOXES]
    for rep in range(2):
        for flag in (True, False):
            batch = submit_units(units, on if flag else off, 0.4)
            assert batch is not None and len(batch) == 3
            for k, (g, w) in enumerate(zip(batch.wait(), want[flag])):
                assert g.flags == 0 and same_rows(g, w), (rep, flag, k)
    # a submitted tile and its pending form
    for k, box in enumerate(UNIT_BOXES):
        assert same_rows(pair.submit_tile(on, box, 0.4).result(), want[True][k]), k


def test_the_pipeline_keeps_every_submissions_own_setting_and_repeats_flagged_units_clipped(unit_frames):
    from karios_amd.stream import FrameStream
    ctx, pair, on, off, want = unit_frames
    units = [(pair, b, None) for b in UNIT_BOXES]
    flags = [True, False, True, True, False, True]
    with FrameStream(0.4, depth=1, score_columns=False) as s:        # (pipeline on: a submission's tail is enqueued by the next one)
        done = []
        for flag in flags:
            done += s.submit_many(units, on if flag else off, tags=[flag] * 3)
        done += s.drain()
        assert ctx.get_option("units_pipeline", 0) == 1
        assert [d.tag for d in done] == [f for f in flags for _ in range(3)] and not any(d.redone for d in done)
        for i, d in enumerate(done):
            assert same_rows(d.raw, want[d.tag][i % 3]), i
        # a forced flag on every unit: the exact repeat runs with the submission's own setting
        ctx.set_option("spec_flag", 32)
        try:
            again = s.submit_many(units, on, tags=[True] * 3) + s.submit_many(units, off, tags=[False] * 3) + s.drain()
        finally:
            ctx.set_option("spec_flag", 0)
    assert len(again) == 6 and all(d.redone and d.flags & 32 for d in again)
    for i, d in enumerate(again):
        assert d.raw.flags == 0 and same_rows(d.raw, want[d.tag][i % 3], header_words=2), i
    assert ctx.get_option("frame_clip", 0) == 0


def test_klt_match_on_resident_rasters_keeps_the_frame_stream_with_the_filter_on(unit_frames, monkeypatch):
    """`KLT.match` on `DeviceRasterImage`s: a configuration with the filter on no longer changes which path runs - the tile grid goes
    through `FrameStream` as batched submissions, and every frame is the host path's."""
    import torch
    from karios_amd import stream as stream_module
    from karios_amd.core import KLTConfiguration
    from karios_amd.core.image import DeviceRasterImage
    from karios_amd.matcher import KLT
    ctx, pair, _on, _off, _want = unit_frames
    mon, ref = unit_scene()
    dev = torch.device("cuda", ctx.device)
    mon_t, ref_t = (torch.from_numpy(a.view(np.int16)).to(dev) for a in (mon, ref))
    torch.cuda.synchronize()
    conf = KLTConfiguration(maxCorners=900, tile_size=700, outliers_filtering=True)
    batches = []
    real = stream_module.submit_units
    monkeypatch.setattr(stream_module, "submit_units", lambda *a, **k: (batches.append(len(a[0])), real(*a, **k))[1])
    klt = KLT(conf, ctx=ctx)
    got = list(klt.match(DeviceRasterImage(mon_t, np.uint16), DeviceRasterImage(ref_t, np.uint16), None))
    boxes = [tuple(t) for t in klt.tile_boxes(1400, 900)]
    assert sum(batches) == len(got) == len(boxes) == 4
    for box, f in zip(boxes, got):
        host = pair._match_tile_host_clip(conf, box, box[0], box[1])
        assert f.index.equals(host.index) and len(f) > 100
        for col in ("x0", "y0", "dx", "dy", "score"):
            np.testing.assert_array_equal(f[col].to_numpy(), host[col].to_numpy(), err_msg=col)


def test_the_frame_sink_of_match_distributed_receives_clipped_blocks(unit_frames, monkeypatch):
    from karios_amd.core import KLTConfiguration, NumpyRasterImage
    from karios_amd.parallel import ResidentUnit, enumerate_units, match_distributed
    ctx, _pair, _on, _off, _want = unit_frames
    mon, ref = unit_scene()
    conf = KLTConfiguration(maxCorners=900, tile_size=700, outliers_filtering=True)
    bands = {0: (NumpyRasterImage(mon), NumpyRasterImage(ref))}
    sinks = []
    real = ctx.set_frame_sink
    monkeypatch.setattr(ctx, "set_frame_sink", lambda *a, **k: (sinks.append(a[0]), real(*a, **k))[1])
    got = match_distributed(bands, 1, 1400, 900, conf, score=True, halo=64, ctx=ctx)
    units = enumerate_units(1, 1400, 900, conf)
    assert len(got) == len(units) == 4 and sum(p is not None for p in sinks) == 4         # every unit went through the sink
    for u, f in zip(units, got):
        ru = ResidentUnit.load(u, bands[0][0], bands[0][1], None, halo=64, ctx=ctx)
        host = ru.pair._match_tile_host_clip(conf, ru.local_box, u.x_off, u.y_off, 0.4)
        assert f.index.equals(host.index) and len(f) > 100
        for col in ("x0", "y0", "dx", "dy", "score", "zncc_score"):
            np.testing.assert_array_equal(f[col].to_numpy(), host[col].to_numpy(), err_msg=col)


def test_a_frame_beyond_the_clips_capacity_stays_on_the_host_path(ops):
    """maxCorners 0 sizes the block for a quarter of the tile's pixels: beyond 32768 rows the library refuses the clipped call before it
    queues anything and `match_tile` takes the host path; the raw and submitted forms say so."""
    import ctypes as C
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import KariosHipError, ResidentPair
    ctx = ops._lib.default_context()
    mon, ref = displaced_scene(256, 640, 21, TILE_BLOCKS)
    pair = ResidentPair.upload(mon, ref, ctx=ctx)
    conf = KLTConfiguration(maxCorners=0, minDistance=4, outliers_filtering=True)
    assert pair._frame_capacity(conf, None) == 40960
    f = pair.match_tile(conf)
    host = pair._match_tile_host_clip(conf, None, 0, 0)
    assert f.equals(host) and len(f) > 200
    with pytest.raises(KariosHipError):
        pair.match_tile_raw(conf)
    with pytest.raises(KariosHipError):
        pair.submit_tile(conf)
    with pair._frame_clip(True):
        with pytest.raises(KariosHipError, match="32768"):
            pair._match_tile_device_frame(KLTConfiguration(maxCorners=0, minDistance=4), None, 0, 0)
    assert ctx.get_option("frame_clip", 0) == 0
    assert pair.match_tile(KLTConfiguration(maxCorners=0, minDistance=4)) is not None          # (the context still works)
