"""Descriptor matching of the align step on the GPU (k_match.hip, api_match.hip) against its definition, tests/match_restatement.py:
indices as integers, distances by their float32 bits, nothing excluded."""
from __future__ import annotations

import ctypes as C
import logging
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_restatement as R  # noqa: E402

from karios_amd import _lib, synth  # noqa: E402
from karios_amd.matcher import global_align  # noqa: E402
from karios_amd.ops import knn_match, match_lowe_mutual  # noqa: E402  (the feature's names: the file fails without them)

pytestmark = pytest.mark.gpu


def assert_knn_equal(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def assert_matches_equal(got, want):
    for g, w in zip(got[:2], want[:2]):
        assert g.dtype == np.int32
        np.testing.assert_array_equal(g, w)
    np.testing.assert_array_equal(got[2].view(np.uint32), np.asarray(want[2], np.float32).view(np.uint32))
    assert tuple(got[3]) == tuple(want[3])


def scene(n_mon, n_ref, seed=1):
    """The synthetic scene scaled from the one whose counts are known (5 000 x 7 001: 2 000 common, 300 rivals)."""
    n_common = max(1, min(n_mon, n_ref) * 2 // 5) if min(n_mon, n_ref) >= 5 else 0
    n_rival = min(n_common * 3 // 20, n_mon - n_common)
    return synth.descriptor_scene(n_mon, n_ref, n_common, n_rival, 30, seed)


class DeviceRows:
    """Rows on the device with a row stride (elements) that may exceed 128."""

    def __init__(self, ctx, rows, stride=128):
        padded = np.zeros((max(len(rows), 1), stride), rows.dtype)
        padded[:len(rows), :128] = rows
        if stride > 128:
            padded[:, 128:] = 77                                 # must never be read as descriptor elements
        self.ctx, self.n, self.stride = ctx, len(rows), stride
        self.ptr, self.cap = ctx.dev_alloc(padded.nbytes)
        ctx.check(ctx.lib.km_h2d(ctx.handle, C.c_void_p(self.ptr), _lib.ptr(padded), padded.nbytes), "km_h2d")

    def release(self):
        self.ctx.dev_release(self.ptr, self.cap)


def dev_array(ctx, shape, dtype):
    n = max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 16)
    return ctx.dev_alloc(n)


def fetch(ctx, dptr, shape, dtype):
    out = np.empty(shape, dtype)
    if out.nbytes:
        ctx.check(ctx.lib.km_d2h(ctx.handle, _lib.ptr(out), C.c_void_p(dptr), out.nbytes), "km_d2h")
    return out


def knn_dev(ctx, q, t, k, stride=128):
    dq, dt = DeviceRows(ctx, q, stride), DeviceRows(ctx, t, stride)
    (pi, ci), (pd, cd) = dev_array(ctx, (len(q), k), np.int32), dev_array(ctx, (len(q), k), np.float32)
    try:
        ctx.check(ctx.lib.km_knn_match_u8_dev(ctx.handle, C.c_void_p(dq.ptr), len(q), stride, C.c_void_p(dt.ptr), len(t), stride, 128, k,
                                              C.c_void_p(pi), C.c_void_p(pd)), "km_knn_match_u8_dev")
        return fetch(ctx, pi, (len(q), k), np.int32), fetch(ctx, pd, (len(q), k), np.float32)
    finally:
        for p, cap in ((pi, ci), (pd, cd)):
            ctx.dev_release(p, cap)
        dq.release()
        dt.release()


def match_dev(ctx, mon, ref, ratio=0.75, cap=None, stride=128):
    cap = len(mon) if cap is None else cap
    dm, dr = DeviceRows(ctx, mon, stride), DeviceRows(ctx, ref, stride)
    bufs = [dev_array(ctx, (cap,), np.int32), dev_array(ctx, (cap,), np.int32), dev_array(ctx, (cap,), np.float32)]
    counts = (C.c_int * 3)(-1, -1, -1)
    try:
        rc = ctx.lib.km_match_lowe_mutual_dev(ctx.handle, C.c_void_p(dm.ptr), len(mon), stride, C.c_void_p(dr.ptr), len(ref), stride,
                                              _lib.dtype_code(mon), 128, ratio, cap, C.c_void_p(bufs[0][0]), C.c_void_p(bufs[1][0]),
                                              C.c_void_p(bufs[2][0]), counts)
        if rc != 0:
            return rc, ctx.lib.km_last_error(ctx.handle).decode(), tuple(counts)
        n = counts[2]
        return (fetch(ctx, bufs[0][0], (n,), np.int32), fetch(ctx, bufs[1][0], (n,), np.int32), fetch(ctx, bufs[2][0], (n,), np.float32),
                tuple(counts))
    finally:
        for p, c in bufs:
            ctx.dev_release(p, c)
        dm.release()
        dr.release()


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


SHAPES = [(1, 1), (1, 2), (5, 3), (64, 64), (129, 257), (1000, 4099), (20000, 30011)]


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("k", [1, 2])
def test_knn_equals_the_restatement(ctx, n, m, k):
    rng = np.random.default_rng(n * 7 + m)
    sets = [(rng.integers(0, 256, (n, 128), dtype=np.uint8), rng.integers(0, 256, (m, 128), dtype=np.uint8))]   # asymmetric: q != t
    if min(n, m) >= 5:
        sets.append(scene(n, m))
    for q, t in sets:
        want = R.knn(q, t, k)
        got = knn_match(q, t, k)
        assert_knn_equal(got, want)
        again = knn_match(q, t, k)
        assert_knn_equal(again, got)                                                   # two runs, bitwise
        if n <= 1000:
            assert_knn_equal(knn_dev(ctx, q, t, k, stride=160), want)                  # the device form, row stride > 128
            assert_knn_equal(knn_match(q.astype(np.float32), t.astype(np.float32), k), want)
    if (n, m) == (1000, 4099):
        big = np.zeros((n, 200), np.uint8)                                             # host rows with a stride, too
        big[:, 30:158] = sets[0][0]
        assert_knn_equal(knn_match(big[:, 30:158], sets[0][1], k), R.knn(sets[0][0], sets[0][1], k))


def test_knn_device_form_large(ctx):
    q, t = scene(20000, 30011, seed=4)
    assert_knn_equal(knn_dev(ctx, q, t, 2, stride=144), R.knn(q, t, 2))
    assert_knn_equal(knn_dev(ctx, t, q, 1, stride=144), R.knn(t, q, 1))


def test_ties_lowest_index_first(ctx):
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (700, 128), dtype=np.uint8)
    order = rng.permutation(2100)
    train = np.concatenate([base, base, base])[order]            # every row three times at scattered positions
    for k in (1, 2):
        want = R.knn(base, train, k)
        got = knn_match(base, train, k)
        assert_knn_equal(got, want)
        assert (got[1] == 0).all()
    idx = knn_match(base, train, 2)[0]
    pos = np.sort(np.argsort(order, kind="stable").reshape(3, 700), axis=0)   # positions of the three copies of every row
    np.testing.assert_array_equal(idx[:, 0], pos[0])
    np.testing.assert_array_equal(idx[:, 1], pos[1])
    assert_knn_equal(knn_match(train, train, 2), R.knn(train, train, 2))      # query == train


@pytest.mark.parametrize("n_query", [1, 300, 7000])
def test_float_distance_collision_across_tiles_and_chunks(ctx, n_query):
    """Two train rows whose d2 differ and whose float32 distances are equal: the lower index wins, wherever the two sit relative to
    the kernel's 128-row tiles and its chunks of the train rows (one tile per chunk for few queries, several for many)."""
    q, far, near = R.collision_rows()
    rng = np.random.default_rng(13)
    others = rng.integers(200, 256, (5000, 128), dtype=np.uint8)               # all farther from the zero row than the two
    queries = np.concatenate([q[None], rng.integers(0, 256, (n_query - 1, 128), dtype=np.uint8)])
    positions = [(127, 128), (128, 127), (0, 4999), (4999, 0), (1279, 1280), (1280, 1279), (255, 1407), (31, 32), (3, 7)]
    if n_query > 1000:
        positions = [(127, 128), (128, 127), (255, 256), (256, 255), (1279, 1280)]
    for p_far, p_near in positions:
        train = others.copy()
        train[p_far], train[p_near] = far, near
        d2 = R.squared_distances(q[None], train)[0]
        assert d2[p_far] == d2[p_near] + 1 and np.sort(d2)[2] > d2[p_far]       # the two are the nearest, one unit apart
        for k in (1, 2):
            want = R.knn(queries, train, k)
            assert want[0][0, 0] == min(p_far, p_near)                         # ... and the lower INDEX leads
            if p_far < p_near:
                assert int(np.lexsort((np.arange(len(d2)), d2))[0]) == p_near  # ranking by (d2, j) would say otherwise
            assert_knn_equal(knn_match(queries, train, k), want)


def test_range_of_the_int8_offset(ctx):
    z, f = np.zeros((3, 128), np.uint8), np.full((2, 128), 255, np.uint8)
    got = knn_match(z, f, 2)
    assert_knn_equal(got, R.knn(z, f, 2))
    assert (got[1] == np.sqrt(np.float32(R.D2_MAX))).all()
    rng = np.random.default_rng(17)
    edge = rng.integers(127, 129, (300, 128)).astype(np.uint8)                  # both sides of the offset
    mixed = np.concatenate([edge, z, f, rng.integers(0, 256, (50, 128), dtype=np.uint8)])
    for k in (1, 2):
        assert_knn_equal(knn_match(mixed, mixed[::-1].copy(), k), R.knn(mixed, mixed[::-1].copy(), k))
        assert_knn_equal(knn_match(edge, f, k), R.knn(edge, f, k))


@pytest.mark.parametrize("n,m", [(5000, 7001), (20000, 30011)])
def test_match_lowe_mutual_equals_the_restatement(ctx, n, m):
    mon, ref = scene(n, m)
    want = R.match_lowe_mutual(mon, ref)
    raw, lowe, mutual = want[3]
    assert raw > lowe > mutual > (n * 2 // 5) / 2, want[3]                      # both filters reject something, most pairs survive
    if (n, m) == (5000, 7001):
        assert want[3] == (5000, 2235, 1944)
    got = match_lowe_mutual(mon, ref)
    assert_matches_equal(got, want)
    assert_matches_equal(match_lowe_mutual(mon.astype(np.float32), ref.astype(np.float32)), want)
    assert_matches_equal(match_dev(ctx, mon, ref, stride=136), want)
    assert_matches_equal(match_dev(ctx, mon.astype(np.float32), ref.astype(np.float32), stride=132), want)
    assert_matches_equal(match_lowe_mutual(mon, ref, ratio=0.9), R.match_lowe_mutual(mon, ref, 0.9))


@pytest.mark.parametrize("s", [2, 5, 100])
def test_lowe_at_exact_equality(ctx, s):
    for below, counts in ((False, (1, 0, 0)), (True, (1, 1, 1))):
        q, a, b = R.lowe_rows(s, below)
        want = R.match_lowe_mutual(q[None], np.stack([a, b]))
        assert want[3] == counts
        assert_matches_equal(match_lowe_mutual(q[None], np.stack([a, b])), want)
        assert_matches_equal(match_lowe_mutual(q[None], np.stack([b, a])), R.match_lowe_mutual(q[None], np.stack([b, a])))
    dup = np.stack([a, a])
    assert_matches_equal(match_lowe_mutual(a[None], dup), R.match_lowe_mutual(a[None], dup))
    assert match_lowe_mutual(a[None], dup)[3] == (1, 0, 0)


def test_capacity_and_empty_sets(ctx):
    mon, ref = scene(5000, 7001)
    want = R.match_lowe_mutual(mon, ref)
    rc, msg, counts = match_dev(ctx, mon, ref, cap=100)
    assert rc == _lib.E_ARG and counts == want[3] and "1944" in msg
    assert_matches_equal(match_dev(ctx, mon, ref, cap=want[3][2]), want)         # exactly enough
    for a, b in ((mon[:0], ref), (mon, ref[:0]), (mon[:50], ref[:1])):
        got = match_lowe_mutual(a, b)
        assert got[0].size == got[1].size == got[2].size == 0 and got[3] == (len(a), 0, 0)
        assert_matches_equal(got, R.match_lowe_mutual(a, b))
        got = match_dev(ctx, a, b)
        assert got[0].size == 0 and got[3] == (len(a), 0, 0)
    idx, dist = knn_match(mon[:7], ref[:0], 2)
    assert (idx == -1).all() and np.isinf(dist).all()
    idx, dist = knn_match(mon[:7], ref[:1], 2)
    assert_knn_equal((idx, dist), R.knn(mon[:7], ref[:1], 2))
    assert knn_match(mon[:0], ref, 1)[0].shape == (0, 1)


@pytest.mark.parametrize("bad", [17.5, -1.0, 256.0, float("nan"), float("inf")])
def test_non_integer_float_descriptors_are_refused(ctx, bad):
    mon, ref = scene(600, 900)
    mon, ref = mon.astype(np.float32), ref.astype(np.float32)
    for which in (0, 1):
        a, b = mon.copy(), ref.copy()
        (a, b)[which][411, 93] = bad
        (a, b)[which][500, 2] = bad                                             # the FIRST offending element is named
        with pytest.raises(_lib.KariosHipError, match=r"\(row 411, column 93\)") as e:
            match_lowe_mutual(a, b)
        assert e.value.code == _lib.E_ARG and ("ref" if which else "mon") in str(e.value)
        with pytest.raises(ValueError, match=r"row 411, column 93"):
            knn_match(a, b, 2)
    assert_matches_equal(match_lowe_mutual(mon, ref), R.match_lowe_mutual(mon, ref))   # the context is usable afterwards


def test_argument_errors(ctx):
    mon, ref = scene(20, 30)
    with pytest.raises(ValueError):
        knn_match(mon, ref, 3)
    with pytest.raises(ValueError):
        knn_match(mon[:, :64], ref, 1)
    with pytest.raises(ValueError):
        knn_match(mon.astype(np.float64), ref, 1)
    with pytest.raises(ValueError):
        match_lowe_mutual(mon, ref.astype(np.float32))
    idx, dist = np.zeros((20, 2), np.int32), np.zeros((20, 2), np.float32)
    rc = ctx.lib.km_knn_match_u8(ctx.handle, _lib.ptr(mon), 20, 128, _lib.ptr(ref), 30, 128, 64, 2, _lib.ptr(idx), _lib.ptr(dist))
    assert rc == _lib.E_UNSUPPORTED
    rc = ctx.lib.km_knn_match_u8(ctx.handle, _lib.ptr(mon), 20, 128, _lib.ptr(ref), 30, 128, 128, 3, _lib.ptr(idx), _lib.ptr(dist))
    assert rc == _lib.E_ARG


class _KeyPoint:
    def __init__(self, x, y):
        self.pt = (x, y)


def test_match_descriptors(ctx, caplog):
    mon, ref = scene(5000, 7001)
    rng = np.random.default_rng(19)
    xy_mon = rng.uniform(0, 10980, (5000, 2)).astype(np.float32)
    xy_ref = rng.uniform(0, 10980, (7001, 2)).astype(np.float32)
    qi, ti, _d, counts = R.match_lowe_mutual(mon, ref)
    with caplog.at_level(logging.INFO, logger=global_align.logger.name):
        src, dst = global_align.match_descriptors(xy_mon, mon, xy_ref, ref)
    assert src.dtype == dst.dtype == np.float32 and src.shape == dst.shape == (counts[2], 2)
    np.testing.assert_array_equal(src, xy_mon[qi])
    np.testing.assert_array_equal(dst, xy_ref[ti])
    assert "Matches: raw=5000  Lowe<0.75=2235  mutual=1944" in caplog.text
    kp_mon = [_KeyPoint(float(x), float(y)) for x, y in xy_mon]
    kp_ref = [_KeyPoint(float(x), float(y)) for x, y in xy_ref]
    src2, dst2 = global_align.match_descriptors(kp_mon, mon.astype(np.float32), kp_ref, ref.astype(np.float32))
    np.testing.assert_array_equal(src2, src)
    np.testing.assert_array_equal(dst2, dst)
    assert global_align.LOWE_RATIO == 0.75 and global_align.MIN_MATCHES == 4
    with pytest.raises(RuntimeError, match="^SIFT found no descriptors in one or both images$"):
        global_align.match_descriptors(xy_mon, None, xy_ref, ref)
    with pytest.raises(RuntimeError, match=r"^Too few SIFT keypoints: mon=3 ref=7001 \(need ≥4\)$"):
        global_align.match_descriptors(xy_mon[:3], mon[:3], xy_ref, ref)
    unrelated = synth.descriptor_scene(40, 50, 0, 0, 30, 5)
    n_good = R.match_lowe_mutual(*unrelated)[3][2]
    assert n_good < 4
    with pytest.raises(RuntimeError, match=rf"^Too few good matches after Lowe \+ cross-check: {n_good} \(need ≥4\)$"):
        global_align.match_descriptors(xy_mon[:40], unrelated[0], xy_ref[:50], unrelated[1])


def test_large_case_through_the_chunked_and_multi_block_paths(ctx):
    """60 000 x 80 000: 235 query blocks, chunks of several tiles; the restatement takes about two minutes on 16 host cores, the GPU
    a fraction of a second."""
    mon, ref = scene(60000, 80000, seed=7)
    t0 = time.perf_counter()
    want_fwd = R.knn(mon, ref, 2)
    t1 = time.perf_counter()
    got_fwd = knn_match(mon, ref, 2)
    t2 = time.perf_counter()
    print(f"large case: restatement knn(60000, 80000, 2) {t1 - t0:.1f} s, GPU host form {t2 - t1:.3f} s")
    assert_knn_equal(got_fwd, want_fwd)
