"""GPU suite - the frame stage alone (csrc/k_frame.hip: fb_compact_kernel, fb_place_kernel, fb_gather_kernel, frame_launch) through the
test hook `km_frame_from_tracks` / `ops.frame_from_tracks`, against the restatement of the reference's tail (tests/frame_restatement.py,
klt.py:142-168, 341-348) on the cases of tests/frame_cases.py: the cut one ulp either side of float32(0.1), NaN / inf, denormal
displacements, the count word and the capacity, the bucket map of the LDS placement, ties in the ordering key (duplicates, and origins at
which float32 collapses neighbouring columns), the radix sort above 32768 rows, 16 units of very different length in one launch, a
workspace that held a larger call before.

One unit runs through `kf_frame`, several through `kf_frame_units`.  No tolerances anywhere: header words 0 (rows) and 1
(n_init) and the index labels exactly, the float columns as uint32 words (-0.0, denormals; NaN by position) - the stage is integer order
plus single correctly rounded float32 operations.  The same cases run on the host in tests/test_frame_host.py."""
import numpy as np
import pytest

import frame_cases as fc
import frame_restatement as R
from karios_amd import frames
from karios_amd._lib import E_UNSUPPORTED, KariosHipError

pytestmark = pytest.mark.gpu


def _check(ops, units, n_max, cap, want, what):
    blocks = ops.frame_from_tracks(units, n_max, cap, raw=True)
    assert len(blocks) == len(units)
    for j, (block, (frame, rows, n_init)) in enumerate(zip(blocks, want)):
        hdr = block[:4].view(np.int32)
        assert (int(hdr[0]), int(hdr[1])) == (rows, n_init), f"{what}, unit {j}: header {hdr[:2]}, expected {(rows, n_init)}"
        R.assert_same_frame(frames.block_to_frame(block, cap), frame, f"{what}, unit {j}")


@pytest.mark.parametrize("name", list(fc.CASES))
def test_frame_stage_equals_the_restatement(ops, name):
    for i, call in enumerate(fc.build(name)):
        what = f"{name}[{i}] {call.note}"
        if call.refused:
            with pytest.raises(KariosHipError) as refusal:
                ops.frame_from_tracks(call.units, call.n_max, call.cap)
            assert refusal.value.code == E_UNSUPPORTED, f"{what}: {refusal.value}"
            continue
        want = R.frames_of(call.units, call.n_max, call.cap)
        _check(ops, call.units, call.n_max, call.cap, want, what)
        if call.each_alone:
            for j, u in enumerate(call.units):
                _check(ops, [u], call.n_max, call.cap, [want[j]], f"{what}, unit {j} alone")


def test_frames_and_none_come_back_through_block_to_frame(ops):
    call = fc.build("count_word")[0]                     # n = 0: no live row, no frame
    assert ops.frame_from_tracks(call.units, call.n_max, call.cap) == [None]
    call = fc.build("deltas")[0]
    (got,) = ops.frame_from_tracks(call.units, call.n_max, call.cap)
    R.assert_same_frame(got, R.frames_of(call.units, call.n_max, call.cap)[0][0], "deltas")


@pytest.mark.parametrize("p0, origin", [([[0.5, 1]], 0), ([[-1, 1]], 0), ([[np.nan, 1]], 0), ([[1, np.inf]], 0), ([[1, 1]], 0.5), ([[2.0 ** 25, 1]], 0)])
def test_the_wrapper_refuses_what_the_ordering_key_does_not_hold(ops, p0, origin):
    u = fc.unit(p0, p0, p0, x_off=origin)
    with pytest.raises(KariosHipError):
        ops.frame_from_tracks([u], 1, 1)
    # ... but not behind the count word, where nothing is read
    if origin == 0:
        assert ops.frame_from_tracks([dict(u, n=0)], 1, 1) == [None]
