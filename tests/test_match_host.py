"""CPU suite of the descriptor matching: tests/match_restatement.py (the definition of k_match.hip) against a literal plain-Python
transcription of OpenCV's k-best insertion, the float32 collision of neighbouring squared distances, Lowe's test at exact equality,
and against cv2 where cv2 imports."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_restatement as R  # noqa: E402

from karios_amd import synth  # noqa: E402  (numpy only: nothing here touches the GPU library)


def opencv_knn(Q, T, k):
    """OpenCV 4.8's BatchDistInvoker for NORM_L2 on float32 rows, transcribed: per query row the distances to all train rows
    (float32 sum of squared float32 differences - exact for these integers -, then std::sqrt), inserted into a k-long list kept in
    ascending order: a new distance goes in front of the entries it is STRICTLY smaller than, the train rows come in index order."""
    Q, T = np.asarray(Q, np.float32), np.asarray(T, np.float32)
    out_i = np.full((len(Q), k), -1, np.int32)
    out_d = np.full((len(Q), k), np.inf, np.float32)
    for i in range(len(Q)):
        bd, bi = [np.float32(np.inf)] * k, [-1] * k
        for j in range(len(T)):
            s = np.float32(0)
            for c in range(128):
                t = np.float32(Q[i, c] - T[j, c])
                s = np.float32(s + np.float32(t * t))
            d = np.float32(np.sqrt(s))
            if d < bd[k - 1]:
                p = k - 2
                while p >= 0 and bd[p] > d:
                    bd[p + 1], bi[p + 1] = bd[p], bi[p]
                    p -= 1
                bd[p + 1], bi[p + 1] = d, j
        out_i[i], out_d[i] = bi, bd
    return out_i, out_d


def assert_same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(np.asarray(a[1], np.float32).view(np.uint32), np.asarray(b[1], np.float32).view(np.uint32))


@pytest.mark.parametrize("k", [1, 2])
def test_restatement_equals_the_insertion_loop(k):
    rng = np.random.default_rng(5)
    for n, m in ((3, 1), (4, 2), (6, 9)):
        Q, T = rng.integers(0, 256, (n, 128), dtype=np.uint8), rng.integers(0, 256, (m, 128), dtype=np.uint8)
        assert_same(R.knn(Q, T, k), opencv_knn(Q, T, k))
    # ties and duplicates: every train row three times, the queries among them (distance 0 twice)
    base = rng.integers(0, 256, (4, 128), dtype=np.uint8)
    T = np.concatenate([base, base[::-1], base])[rng.permutation(12)]
    assert_same(R.knn(base, T, k), opencv_knn(base, T, k))
    got_i, got_d = R.knn(base, T, 2)
    assert (got_d == 0).all() and (got_i[:, 0] < got_i[:, 1]).all()
    # float32 rows holding the same integers are the same descriptors
    assert_same(R.knn(base.astype(np.float32), T.astype(np.float32), k), R.knn(base, T, k))


def test_missing_columns_and_empty_sets():
    rng = np.random.default_rng(6)
    Q, T = rng.integers(0, 256, (3, 128), dtype=np.uint8), rng.integers(0, 256, (1, 128), dtype=np.uint8)
    idx, dist = R.knn(Q, T, 2)
    assert (idx[:, 0] == 0).all() and (idx[:, 1] == -1).all() and np.isinf(dist[:, 1]).all() and np.isfinite(dist[:, 0]).all()
    idx, dist = R.knn(Q, T[:0], 2)
    assert (idx == -1).all() and np.isinf(dist).all()
    assert R.knn(Q[:0], T, 1)[0].shape == (0, 1)
    for mon, ref in ((Q, T), (Q, T[:0]), (Q[:0], T)):           # M = 1: no pair has two entries
        qi, ti, d, counts = R.match_lowe_mutual(mon, ref)
        assert qi.size == ti.size == d.size == 0 and counts == (len(mon), 0, 0)


def test_equal_float_distance_prefers_the_lower_index_not_the_smaller_d2():
    q, far, near = R.collision_rows()
    d2 = R.squared_distances(q[None], np.stack([far, near]))[0]
    assert tuple(d2) == (4197201, 4197200)
    dist = R.distances(d2)
    assert dist[0] == dist[1]
    T = np.stack([far, near])                                   # the larger d2 at the lower index
    idx, _ = R.knn(q[None], T, 1)
    assert idx[0, 0] == 0
    assert int(np.lexsort((np.arange(2), d2))[0]) == 1          # ranking by (d2, j) would have returned the other row
    assert_same(R.knn(q[None], T, 2), opencv_knn(q[None], T, 2))
    assert_same(R.knn(q[None], T[::-1], 2), opencv_knn(q[None], T[::-1], 2))


def test_float32_square_roots_collide_from_4197200_on():
    d2 = np.arange(0, R.D2_MAX + 1, dtype=np.int64)
    s = R.distances(d2)
    same = np.nonzero(s[1:] == s[:-1])[0]
    assert same[0] == 4197200 and same.size == 700562


@pytest.mark.parametrize("s", [2, 5, 100])
def test_lowe_at_exact_equality_and_one_unit_below(s):
    q, a, b = R.lowe_rows(s, False)
    d2 = R.squared_distances(q[None], np.stack([a, b]))[0]
    assert tuple(d2) == (9 * s * s, 16 * s * s)
    qi, ti, d, counts = R.match_lowe_mutual(q[None], np.stack([a, b]))
    assert counts == (1, 0, 0) and qi.size == 0                 # 3 s < 0.75 * 4 s is false
    q, a, b = R.lowe_rows(s, True)
    d2 = R.squared_distances(q[None], np.stack([a, b]))[0]
    assert tuple(d2) == (9 * s * s - 1, 16 * s * s)
    qi, ti, d, counts = R.match_lowe_mutual(q[None], np.stack([a, b]))
    assert counts == (1, 1, 1) and tuple(qi) == (0,) and tuple(ti) == (0,) and d[0] == np.sqrt(np.float32(9 * s * s - 1))
    dup = np.stack([a, a])                                      # exact duplicates: 0 < 0.75 * 0 is false for the duplicate query
    assert R.match_lowe_mutual(a[None], dup)[3] == (1, 0, 0)


def test_non_integer_descriptors_are_refused():
    a = np.zeros((2, 128), np.float32)
    for bad in (17.5, -1.0, 256.0, np.nan, np.inf):
        b = a.copy()
        b[1, 77] = bad
        with pytest.raises(ValueError, match=r"row 1, column 77"):
            R.knn(b, a, 1)


def test_scene_exercises_both_filters():
    mon, ref = synth.descriptor_scene(5000, 7001, 2000, 300, 30, 1)
    assert mon.shape == (5000, 128) and ref.shape == (7001, 128) and mon.dtype == ref.dtype == np.uint8
    qi, ti, d, (raw, lowe, mutual) = R.match_lowe_mutual(mon, ref)
    assert (raw, lowe, mutual) == (5000, 2235, 1944)
    assert raw > lowe > mutual > 1000 and qi.size == mutual and (np.diff(qi) > 0).all()
    # the vectorised filter against the reference's loop, written out
    fi, fd = R.knn(mon, ref, 2)
    bi, _ = R.knn(ref, mon, 1)
    good = [i for i in range(raw) if float(fd[i, 0]) < 0.75 * float(fd[i, 1]) and bi[fi[i, 0], 0] == i]
    assert good == list(qi)


def test_knn_equals_cv2_when_present():
    cv2 = pytest.importorskip("cv2")   # absent here: parity with cv2 stays unpinned in DESIGN section 2's sense
    mon, ref = synth.descriptor_scene(300, 400, 100, 20, 30, 2)
    q, far, near = R.collision_rows()
    mon, ref = np.concatenate([mon, q[None]]), np.concatenate([ref, far[None], near[None]])
    matcher = cv2.BFMatcher(cv2.NORM_L2, crossCheck=False)
    for k in (1, 2):
        pairs = matcher.knnMatch(mon.astype(np.float32), ref.astype(np.float32), k=k)
        idx, dist = R.knn(mon, ref, k)
        np.testing.assert_array_equal(np.array([[m.trainIdx for m in p] for p in pairs], np.int32), idx)
        np.testing.assert_array_equal(np.array([[m.distance for m in p] for p in pairs], np.float32).view(np.uint32), dist.view(np.uint32))
