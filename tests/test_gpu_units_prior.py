"""Batched units under a geometric prior each (km_klt_units_frame_prior_submit, csrc/api_units.hip).  The contract
is bit-identity with km_klt_tile_frame_prior_dev unit by unit - the prior's corner mask of every unit in one launch, the seeded tracker
family on the seeds that travel with the lane's table - and through it the restatement (tests/lk_prior_restatement.py).  Also: identity
priors against the unseeded batch, prior / non-prior submissions alternating in the software pipeline, user masks, flagged units, the
frame sink, the refusals, and the Python layers above (`submit_units`, `FrameStream`, `ResidentPair.match_pipelined`)."""
import ctypes as C_

import numpy as np
import pytest

import units_prior_cases as UC

pytestmark = pytest.mark.gpu

THRESHOLD = 0.4


def same_rows(a, b, columns=None) -> bool:
    """Two frame blocks hold the same frame (`same_rows` of tests/test_gpu_units.py): header and, column by column, the first n_rows
    entries.  `columns` = 0: the float32 columns alone (a bare block of a batch against the tile call's, which always has score columns)."""
    ia, ib = a.block.view(np.int32), b.block.view(np.int32)
    if not np.array_equal(ia[:4], ib[:4]) or a.cap != b.cap or (columns is None and a.with_zncc != b.with_zncc):
        return False
    n, cap = int(ia[0]), a.cap
    cols32 = all(np.array_equal(ia[4 + k * cap:4 + k * cap + n], ib[4 + k * cap:4 + k * cap + n]) for k in range(6))
    base = 4 + 6 * cap
    n64 = int(a.with_zncc) if columns is None else columns
    cols64 = all(np.array_equal(ia[base + 2 * k * cap:base + 2 * k * cap + 2 * n], ib[base + 2 * k * cap:base + 2 * k * cap + 2 * n]) for k in range(n64))
    return cols32 and cols64


def _conf(max_corners=UC.MAX_CORNERS, **kw):
    from karios_amd.core import KLTConfiguration
    return KLTConfiguration(maxCorners=max_corners, matching_winsize=UC.WIN, laplacian_kernel_size=UC.KSIZE, **kw)


_uploaded = {}


def _units(ops, dtype="uint16", masks=False):
    """-> (ctx, [(pair, box, origin)], [prior]) of `UC.units()`; one upload per content (and test session)."""
    from karios_amd.resident import ResidentPair
    ctx = ops._lib.default_context()
    out = []
    for u in UC.units():
        key = (u["which"], u["shift"], dtype, masks)
        if key not in _uploaded:
            ref, mon = UC.pair(u["which"], *u["shift"], dtype=dtype)
            mask = None
            if masks:
                mask = (np.random.default_rng(5).random(ref.shape) < 0.8).astype(np.uint8) * 3
                mask[:, 200:230] = 0
            _uploaded[key] = ResidentPair.upload(mon, ref, mask, ctx=ctx)
        out.append((_uploaded[key], u["box"], u["origin"]))
    return ctx, out, [u["prior"] for u in UC.units()]


def _tile(pair, conf, box, origin, P, thr, mi=False):
    """km_klt_tile_frame_prior_dev on one unit: the raw block."""
    from karios_amd.resident.tiles import _origin
    return pair._prior_tile_raw(conf, box, *_origin(origin, box), np.asarray(P, np.float64), thr, None, None, mi)


def _tiles(units, priors, conf, thr, mi=False):
    return [_tile(p, conf, b, o, P, thr, mi) for (p, b, o), P in zip(units, priors)]


@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
@pytest.mark.parametrize("scores", [None, "zncc", "full"])
def test_a_batch_under_priors_equals_the_tile_calls_unit_by_unit(ops, scores, dtype):
    from karios_amd.resident import submit_units
    ctx, units, priors = _units(ops, dtype)
    conf = _conf()
    thr, mi = (None if scores is None else THRESHOLD), scores == "full"
    want = _tiles(units, priors, conf, thr, mi)
    facts = [(w.n_rows, int(w.block[1:2].view(np.int32)[0]), w.flags) for w in want]
    print(facts)
    assert all(rows >= 5 and n_init >= 20 and flags == 0 for rows, n_init, flags in facts)
    assert any(rows < n_init for rows, n_init, _ in facts)             # (the forward-backward cut drops rows somewhere)
    for rep in range(3):                                               # (slot ring, workspace reuse)
        batch = submit_units(units, conf, thr, mi, priors=priors)
        assert batch is not None and len(batch) == len(units) and batch.prior_steps is not None
        for k, (g, w) in enumerate(zip(batch.wait(), want)):
            assert g.flags == 0 and same_rows(g, w, None if scores else 0), (rep, k, UC.units()[k]["name"])


def test_one_unit_of_a_batch_against_the_restatement(ops, O):
    """`dx_prior, dy_prior` too: the batch's frames carry them (`PendingBatch.frame`)."""
    import test_gpu_lk_prior as T
    from karios_amd.resident import submit_units
    assert (T.KSIZE, T.THRESHOLD) == (UC.KSIZE, THRESHOLD)
    ctx, units, priors = _units(ops, "uint8")
    conf = _conf(UC.MAX_CORNERS_RESTATED)
    k = UC.RESTATED_UNIT
    u = UC.units()[k]
    ref, mon = UC.pair(u["which"], *u["shift"])
    want, _ = T._expected_frame(O, ref, mon, u["prior"], u["box"], UC.WIN, conf)
    batch = submit_units(units, conf, THRESHOLD, priors=priors)
    got = batch.frame(k)
    got.attrs["Ninit"] = int(batch.wait()[k].block[1:2].view(np.int32)[0])
    T._assert_frame(got, want, u["name"], units[k][0])
    order = np.asarray(want.index)
    T._assert_same(got["dx_prior"].to_numpy(), want.attrs["prior"][0][order], "dx_prior")
    T._assert_same(got["dy_prior"].to_numpy(), want.attrs["prior"][1][order], "dy_prior")
    assert want.attrs["Ninit"] >= 20 and len(want) >= 5


def test_identity_priors_equal_the_unseeded_batch(ops):
    from karios_amd.matcher import prior as prior_mod
    from karios_amd.resident import submit_units
    ctx, units, _ = _units(ops, "uint16")
    units = [units[0], units[1], units[4]]                 # (content within 15 px of the identity's guess is still tracked or dropped alike)
    conf = _conf()
    want = submit_units(units, conf, THRESHOLD).wait()
    got = submit_units(units, conf, THRESHOLD, priors=prior_mod.IDENTITY).wait()
    assert all(w.flags == 0 for w in want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert same_rows(g, w), k


@pytest.mark.parametrize("flush_between", [False, True])
def test_prior_and_plain_submissions_alternate_in_the_pipeline(ops, flush_between):
    """prior(PA) -> prior(PB != PA) -> no prior -> prior(PA), pipelined against unpipelined: a tail launched with the other lane's seeds or
    with the other family shows here."""
    from karios_amd.resident import submit_units
    ctx, units, priors = _units(ops, "uint16")
    conf = _conf()
    ua, ub = units[:3], units[3:]
    pa, pb = priors[:3], priors[3:]
    pb_on_a = [priors[1], priors[2], priors[0]]            # other priors on the units of the first submission
    steps = [(ua, pa), (ua, pb_on_a), (ub, None), (ub, pb), (ua, pa)]

    def run(piped):
        ctx.set_option("units_pipeline", 1 if piped else 0)
        try:
            pend = []
            for i, (us, ps) in enumerate(steps):
                pend.append(submit_units(us, conf, THRESHOLD, priors=ps))
                assert pend[-1] is not None
                if flush_between and i == 1:
                    ctx.flush(-1)
                if len(pend) >= 3:                         # (a context holds three frames in flight)
                    pend[len(pend) - 3].wait()
            return [p.wait() for p in pend]
        finally:
            ctx.set_option("units_pipeline", 0)

    want, got = run(False), run(True)
    for s, (gs, ws) in enumerate(zip(got, want)):
        for k, (g, w) in enumerate(zip(gs, ws)):
            assert same_rows(g, w), (s, k)
    assert not same_rows(want[0][0], want[1][0])           # (the two prior submissions of the same units differ)


def test_units_with_a_user_mask_under_priors(ops):
    from karios_amd.resident import submit_units
    ctx, units, priors = _units(ops, "uint16", masks=True)
    _, plain, _ = _units(ops, "uint16")
    conf = _conf()
    want = _tiles(units, priors, conf, THRESHOLD)
    unmasked = _tiles(plain, priors, conf, THRESHOLD)
    got = submit_units(units, conf, THRESHOLD, priors=priors).wait()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.flags == 0 and w.n_rows >= 5 and same_rows(g, w), k
    assert any(not same_rows(w, p) for w, p in zip(want, unmasked))    # (the base mask took corners away)


def test_flagged_units_are_redone_under_their_priors_and_the_sink_receives_every_block(ops):
    from karios_amd import frames
    from karios_amd.resident import DeviceBuffer, RawFrame
    from karios_amd.stream import FrameStream
    ctx, units, priors = _units(ops, "uint16")
    conf = _conf()
    want = _tiles(units, priors, conf, THRESHOLD)
    words = frames.block_words(conf.maxCorners, 1)
    pitch = 4 * words + 64
    sink = DeviceBuffer(ctx, pitch * len(units))
    ctx.set_frame_sink(sink.ptr, pitch * len(units), pitch)
    try:
        with FrameStream(THRESHOLD, depth=1, score_columns=False) as s:
            got = s.submit_many(units, conf, priors=priors) + s.drain()
            ctx.sync()
            blocks = sink.download((len(units), pitch // 4), np.float32)
            ctx.set_option("spec_flag", 32)
            flagged = s.submit_many(units, conf, priors=priors) + s.drain()
            ctx.set_option("spec_flag", 0)
    finally:
        ctx.set_option("spec_flag", 0)
        ctx.set_frame_sink(None)
    assert not any(d.redone for d in got) and all(d.redone and d.flags & 32 for d in flagged)
    for k, (g, f, w) in enumerate(zip(got, flagged, want)):
        assert same_rows(g.raw, w) and same_rows(RawFrame(blocks[k, :words], conf.maxCorners, 1), w), k
        assert f.raw.flags == 0 and f.frame.equals(g.frame), k      # (the exact path's block: header words 2 / 3 are zero, the frame is the same)
        assert list(g.frame.columns[-2:]) == ["dx_prior", "dy_prior"]


def _raw_submit(ctx, units, conf, priors, window=False):
    """km_klt_units_frame_prior_submit as it is, with nothing of `submit_units` around it -> (status, ticket)."""
    from karios_amd import _lib
    from karios_amd.resident.tiles import TileCalls
    prm = TileCalls._params(conf)
    arr = (_lib.KmUnit * len(units))()
    for k, (pair, box, origin) in enumerate(units):
        x, y, bx, by, off = pair._box(box)
        u = arr[k]
        es = pair.dtype.itemsize
        u.d_ref, u.d_mon, u.sref, u.smon, u.H, u.W = pair.ref_ptr + off * es, pair.mon_ptr + off * es, pair.x_size, pair.x_size, by, bx
        u.x_off, u.y_off = float(x), float(y)
        u.d_ref_full, u.d_mon_full, u.sref_f, u.smon_f, u.Hf, u.Wf = pair.ref_ptr, pair.mon_ptr, pair.x_size, pair.x_size, pair.y_size, pair.x_size
        if window and k == 1:
            u.win_ox, u.win_oy, u.win_H, u.win_W = 0, 0, pair.y_size, pair.x_size
    ticket = C_.c_int(-7)
    table = None if priors is None else np.ascontiguousarray(np.stack(priors), np.float64)
    rc = ctx.lib.km_klt_units_frame_prior_submit(ctx.handle, arr, len(units), units[0][0].code, None, None, C_.byref(prm), THRESHOLD, prm.max_corners,
                                                 None if table is None else table.ctypes.data_as(C_.POINTER(C_.c_double)), C_.byref(ticket))
    return rc, ticket.value


def test_refusals_queue_nothing(ops):
    from karios_amd import _lib
    from karios_amd.resident import submit_units
    ctx, units, priors = _units(ops, "uint16")
    units, priors = units[:3], priors[:3]
    conf = _conf()
    want = submit_units(units, conf, THRESHOLD).wait()
    bad = [p.copy() for p in priors]
    bad[2][4] = np.inf
    ctx.set_option("frame_clip", 1)
    try:
        refused = [_raw_submit(ctx, units, conf, priors)]
    finally:
        ctx.set_option("frame_clip", 0)
    refused += [_raw_submit(ctx, units, conf, priors, window=True), _raw_submit(ctx, units, conf, bad)]
    text = ctx.lib.km_last_error(ctx.handle).decode()
    assert "unit 2" in text and "prior[4]" in text, text
    refused.append(_raw_submit(ctx, units, conf, None))
    assert [rc for rc, _ in refused] == [_lib.E_UNSUPPORTED, _lib.E_UNSUPPORTED, _lib.E_ARG, _lib.E_ARG] and all(t == -7 for _, t in refused)
    ctx.sync()
    for k, (g, w) in enumerate(zip(submit_units(units, conf, THRESHOLD).wait(), want)):
        assert same_rows(g, w), k


@pytest.mark.parametrize("clip", [False, True])
def test_the_stream_and_the_pair_yield_the_frames_of_the_tile_loop(ops, clip):
    from karios_amd.stream import FrameStream
    ctx, units, priors = _units(ops, "uint16")
    conf = _conf(outliers_filtering=clip)
    # a unit narrower than 512 columns inside the list: its chunk goes one by one, under the same priors
    narrow = (units[0][0], (40, 30, 400, 500), None)
    units, priors = units[:2] + [narrow] + units[2:], priors[:2] + [priors[0]] + priors[2:]
    want = [p.match_tile(conf, box=b, zncc_threshold=THRESHOLD, origin=o, prior=P) for (p, b, o), P in zip(units, priors)]
    print([None if w is None else len(w) for w in want])
    # (where prior and content agree to the pixel every residual is exactly zero, the deviation is zero and the reference's clip keeps
    # no row: such a unit's frame is empty, by either route)
    assert all(w is not None for w in want) and sum(len(w) >= 5 for w in want) >= (3 if clip else len(want))
    with FrameStream(THRESHOLD, depth=1, score_columns=False) as s:
        got = s.submit_many(units[:2] + units[3:], conf, priors=priors[:2] + priors[3:]) + s.drain()
        mixed = s.submit_many(units, conf, priors=priors) + s.drain()
    for g, w in zip(got, want[:2] + want[3:]):
        assert g.frame.equals(w)
    assert len(mixed) == len(want) and all(g.frame.equals(w) for g, w in zip(mixed, want))
    # the tiles of one pair under one prior
    pair, P = units[0][0], priors[0]
    boxes = [(0, 0, 560, 620), (560, 0, 560, 620)]
    loop = [pair.match_tile(conf, box=b, zncc_threshold=THRESHOLD, prior=P) for b in boxes]
    piped = list(pair.match_pipelined(conf, boxes=boxes, zncc_threshold=THRESHOLD, prior=P))
    assert len(piped) == 2 and all(g.equals(w) for g, w in zip(piped, loop))


@pytest.mark.parametrize("clip", [False, True])
def test_klt_match_under_a_prior_on_resident_rasters_goes_through_the_batches(ops, clip):
    """Fixed kernel size and polarity, rasters in HBM: the tile grid (620 and 500 columns: the second tile takes the one-by-one route) in
    tile order, each frame the frame of `match_tile(prior=)`."""
    import torch
    from karios_amd.core.image import DeviceRasterImage
    from karios_amd.matcher import KLT
    from karios_amd.resident import ResidentPair
    ref, mon = UC.pair("A", 7, 3, dtype="uint16")
    dev = torch.device("cuda", 0)
    mon_t, ref_t = (torch.from_numpy(a.view(np.int16).copy()).to(dev) for a in (mon, ref))
    torch.cuda.synchronize()
    conf = _conf(tile_size=620, outliers_filtering=clip)
    P = UC.shift_prior(6.6, 3.3)                           # (not the content's shift to the pixel: the residuals have a spread to clip on)
    klt = KLT(conf)
    got = list(klt.match(DeviceRasterImage(mon_t, np.uint16), DeviceRasterImage(ref_t, np.uint16), None, prior=P))
    grid = [tuple(t) for t in klt.tile_boxes(mon.shape[1], mon.shape[0])]
    assert grid == [(0, 0, 620, 620), (620, 0, 500, 620)]
    pair = ResidentPair.upload(mon, ref, ctx=ops._lib.default_context())
    want = [pair.match_tile(conf, box=b, prior=P) for b in grid]
    assert len(got) == 2 and all(len(w) >= 5 for w in want)
    for g, w in zip(got, want):
        assert g.equals(w) and list(g.columns[-2:]) == ["dx_prior", "dy_prior"]
