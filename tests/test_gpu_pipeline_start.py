"""The start of a software pipeline of batched submissions (csrc/api_units.hip) on the real runtime.

A pipelined submission that does not directly follow another one runs its min / max and its setup on the second stream at once, on lane 0 -
the workspace of every other entry point.  The second stream therefore has to be ordered behind the main stream there: behind the uploads
the main stream was made to wait for, behind tiles still in flight, behind a kernel that writes the rasters.  The proof that it is lies in
tests/test_stream_order_host.py (a happens-before checker under the host build); these two tests state the same properties end to end, once
each - a race lost on the GPU gives other numbers, not a fault, and nothing here repeats or waits for one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIT_EXACT = ("x0", "y0", "dx", "dy", "score")


def assert_same_frame(got, want, what):
    """Every column bit for bit, ZNCC within 1e-9 (NaN where the row was not scored) as elsewhere in the suite."""
    assert (got is None) == (want is None), what
    if got is None:
        return
    assert len(got) == len(want) and len(want) > 0, (what, len(got), len(want))
    for col in BIT_EXACT:
        assert np.array_equal(got[col].to_numpy(), want[col].to_numpy()), (what, col)
    np.testing.assert_allclose(got["zncc_score"].to_numpy(), want["zncc_score"].to_numpy(), rtol=0, atol=1e-9, equal_nan=True, err_msg=str(what))


def test_first_pipelined_submission_on_a_fresh_context_waits_for_its_uploads(ops):
    """Context(), ResidentPair.upload from page-locked arrays, FrameStream.submit_many of four units as the FIRST call: the second stream
    is created inside that submission, after the pair's upload ticket was joined - its min / max must still see the rasters complete.
    2048 x 2048 uint16, units of 512 x 2048.  The upload has to outlast the submission's host path for a missing wait to show, and nobody
    has measured at what size it does: this test may pass on a library without the wait - it is the guard on the real runtime, the host
    program is the proof."""
    from karios_amd import pinned_empty, synth
    from karios_amd._lib import Context
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair
    from karios_amd.stream import FrameStream
    mon, ref = synth.make_pair(2048, 2048, 0.5, 0.25, seed=41)
    conf = KLTConfiguration(maxCorners=1500)
    boxes = [(0, 512 * k, 2048, 512) for k in range(4)]
    # the reference first, on a context of its own whose uploads have landed before anything runs
    calm = Context()
    try:
        pair = ResidentPair.upload(mon, ref, ctx=calm)
        calm.check(calm.lib.km_upload_wait(calm.handle), "km_upload_wait")
        want = [pair.match_tile(conf, box=b, zncc_threshold=0.4) for b in boxes]
        del pair
    finally:
        calm.close()
    ctx = Context()
    try:
        pm, pr = pinned_empty(mon.shape, mon.dtype, ctx), pinned_empty(ref.shape, ref.dtype, ctx)
        np.copyto(pm, mon)
        np.copyto(pr, ref)
        pair = ResidentPair.upload(pm, pr, ctx=ctx)
        with FrameStream(0.4, depth=1) as s:
            got = s.submit_many([(pair, b, None) for b in boxes], conf) + s.drain()
        assert len(got) == 4
        for k, (g, w) in enumerate(zip(got, want)):
            assert_same_frame(g.frame, w, ("unit", k))
        del pair, pm, pr
    finally:
        ctx.close()


def test_pipelined_batches_between_asynchronous_tiles_equal_the_blocking_calls(ops):
    """One context, depth 3: a pipelined batch of four units directly behind two submit_tile frames that are still pending - they own lane
    0's scalar block, LK table and partials, which the batch's setup resets - then directly behind shifted_monitored(...), whose output
    the batch's min / max reads.  Every frame, the two tiles' included, equals its blocking counterpart.  Tiles 256 x 640, units 128 x 512."""
    from karios_amd import synth
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair
    from karios_amd.stream import FrameStream
    ctx = ops._lib.default_context()
    mon, ref = synth.make_pair(512, 640, 0.5, 0.25, seed=42)
    conf = KLTConfiguration(maxCorners=300)
    pair = ResidentPair.upload(mon, ref, ctx=ctx)
    tiles = [(0, 0, 640, 256), (0, 256, 640, 256)]
    units = [(64, 128 * k, 512, 128) for k in range(4)]
    want_tiles = [pair.match_tile(conf, box=b, zncc_threshold=0.4) for b in tiles]
    want_units = [pair.match_tile(conf, box=b, zncc_threshold=0.4) for b in units]
    with FrameStream(0.4, depth=3) as s:
        done = []
        for b in tiles:
            done += s.submit(pair, conf, b)
        assert not done                                    # (both tiles still pending when the batch is submitted)
        done += s.submit_many([(pair, b, None) for b in units], conf)
        done += s.drain()
        assert len(done) == 6
        for k, (g, w) in enumerate(zip(done[:2], want_tiles)):
            assert_same_frame(g.frame, w, ("tile", k))
        for k, (g, w) in enumerate(zip(done[2:], want_units)):
            assert_same_frame(g.frame, w, ("unit behind tiles", k))
        # ... and behind a kernel that writes the monitored raster on the main stream
        moved = pair.shifted_monitored(1, -2)
        got = s.submit_many([(moved, b, None) for b in units], conf) + s.drain()
    want_moved = [moved.match_tile(conf, box=b, zncc_threshold=0.4) for b in units]
    assert len(got) == 4
    for k, (g, w) in enumerate(zip(got, want_moved)):
        assert_same_frame(g.frame, w, ("unit behind shift", k))
    assert any(not np.array_equal(a["dx"].to_numpy(), b["dx"].to_numpy()) for a, b in zip(want_moved, want_units))      # (the shift is in the frames)
