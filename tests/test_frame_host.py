"""CPU suite - the frame stage alone, on the host (csrc/k_frame.hip's steps as tests/frame_restatement.py restates them from the
reference's tail, klt.py:142-168, 341-348).

For every case of tests/frame_cases.py the restatement must equal
  * the Python fallback `frames.track_columns` + `frames.assemble` (with the library's rules - count word, capacity - applied around it),
  * `frames.block_to_frame` of the blocks that `km_frame_from_tracks` returns in the stand-alone host program tests/hoststub/frame_main.cpp
    (`frame --tracks IN OUT`: the host half of the library over the stand-in kernels, g++ -fsanitize=address,undefined; the sanitizer
    runtime is linked into the program, it runs as it is): header words 0 and 1, every column word for word, the index labels.
No tolerances: the stage is integer order plus single correctly rounded float32 operations.  The builders assert their own
preconditions (tests/frame_cases.py); the same cases run on the device in tests/test_gpu_frame.py."""
import os
import subprocess

import numpy as np
import pytest

import frame_cases as fc
import frame_restatement as R
from karios_amd import frames

STUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hoststub")
E_UNSUPPORTED = -4


def _record(units, n_max, cap):
    k = len(units)
    meta = np.zeros((k, 4), np.int32)
    for j, u in enumerate(units):
        meta[j, 0], meta[j, 1] = u["n"], u["width"]
        meta[j, 2:] = np.array([u["x_off"], u["y_off"]], np.float32).view(np.int32)
    lists = [np.stack([u[name] for u in units]).astype(np.float32) for name in ("p0", "p1", "p0r")]
    return b"".join([np.array([k, n_max, cap], np.int32).tobytes(), meta.tobytes()] + [a.tobytes() for a in lists])


@pytest.fixture(scope="module")
def host_blocks(tmp_path_factory):
    """Every call of every case (and every unit of an `each_alone` call on its own) through the host program, one context per case
    order: {(case, call index, unit index or None): (status, blocks or None)}."""
    subprocess.check_call(["make", "-s", "-C", STUB, "_build/frame"])
    work = tmp_path_factory.mktemp("frame_tracks")
    keys, shapes, chunks = [], [], []
    for name in fc.CASES:
        for i, call in enumerate(fc.build(name)):
            keys.append((name, i, None)); shapes.append((len(call.units), call.cap)); chunks.append(_record(call.units, call.n_max, call.cap))
            if call.each_alone:
                for j, u in enumerate(call.units):
                    keys.append((name, i, j)); shapes.append((1, call.cap)); chunks.append(_record([u], call.n_max, call.cap))
    src, dst = work / "in.bin", work / "out.bin"
    src.write_bytes(b"".join(chunks))
    out = subprocess.run([os.path.join(STUB, "_build", "frame"), "--tracks", str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("FRAME-TRACKS OK") and out.stderr == "", out.stdout[-2000:] + out.stderr[-6000:]
    raw, at, got = dst.read_bytes(), 0, {}
    for key, (k, cap) in zip(keys, shapes):
        status = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
        blocks = None
        if status == 0:
            words = frames.block_words(cap)
            blocks = np.frombuffer(raw, np.float32, k * words, at).reshape(k, words); at += 4 * k * words
        got[key] = (status, blocks)
    assert at == len(raw)
    return got


def _check_blocks(blocks, want, cap, what):
    for j, (block, (frame, rows, n_init)) in enumerate(zip(blocks, want)):
        hdr = block[:4].view(np.int32)
        assert (int(hdr[0]), int(hdr[1])) == (rows, n_init), f"{what}, unit {j}: header {hdr[:2]}, expected {(rows, n_init)}"
        R.assert_same_frame(frames.block_to_frame(block, cap), frame, f"{what}, unit {j}")


@pytest.mark.parametrize("name", list(fc.CASES))
def test_restatement_equals_the_host_program(name, host_blocks):
    for i, call in enumerate(fc.build(name)):
        status, blocks = host_blocks[(name, i, None)]
        what = f"{name}[{i}] {call.note}"
        if call.refused:
            assert status == E_UNSUPPORTED, f"{what}: status {status}"
            continue
        assert status == 0, f"{what}: status {status}"
        want = R.frames_of(call.units, call.n_max, call.cap)
        _check_blocks(blocks, want, call.cap, what)
        if call.each_alone:
            for j in range(len(call.units)):
                status, alone = host_blocks[(name, i, j)]
                assert status == 0
                _check_blocks(alone, [want[j]], call.cap, f"{what}, unit {j} alone")


@pytest.mark.parametrize("name", list(fc.CASES))
def test_restatement_equals_the_python_fallback(name):
    for i, call in enumerate(fc.build(name)):
        if call.refused:
            continue
        for j, (u, (frame, rows, n_init)) in enumerate(zip(call.units, R.frames_of(call.units, call.n_max, call.cap))):
            what = f"{name}[{i}] {call.note}, unit {j}"
            live = R.live_rows(u["n"], call.n_max)                 # the library's rules around the fallback: count word, capacity
            if live == 0:
                assert frame is None and n_init == 0, what
                continue
            with np.errstate(all="ignore"):
                cols, n = frames.track_columns(u["p0"][:live], u["p1"][:live], u["p0r"][:live])
                cols = {k: v[:call.cap] for k, v in cols.items()}
                got = frames.assemble(cols, np.float32(u["x_off"]), np.float32(u["y_off"]))
            assert n == n_init and len(got) == rows, what
            R.assert_same_frame(got, frame, what)


def test_every_case_of_the_issue_is_built():
    assert list(fc.CASES) == ["cut", "score_sweep", "deltas", "count_word", "capacity", "placement", "ties", "radix", "units", "stale_workspace"]
    placed = [c.facts for c in fc.build("ties")[1:]]
    assert [f["distinct"] for f in placed] == [21] * 3 + [6] * 3 + [1] * 3       # 40 columns at 2^24 (+ 1 rounds away), 2^26, 2^30
