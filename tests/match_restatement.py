"""numpy restatement of the descriptor matching of the align step (karios/matcher/global_align.py:178-202:
cv2.BFMatcher(NORM_L2).knnMatch in both directions, Lowe's ratio test, the mutual check), as libkarios_hip.so computes it
(k_match.hip).

This is the DEFINITION the GPU kernels are held to, bit for bit (tests/test_gpu_match.py).  OpenCV is absent, so parity of `knn`
with cv2 itself is unpinned; tests/test_match_host.py compares the two when cv2 imports and anchors this file on a
literal transcription of OpenCV's insertion loop.  Points marked [cv4.8] come from knowledge of OpenCV 4.8's sources (batch_distance.cpp,
stat.simd / norm, sift.simd.hpp), [ref] from the reference's Python, [def] are choices of this project.

Descriptors are rows of 128 integers 0 .. 255 [cv4.8: SIFT stores saturate_cast<uchar>(...) and hands the rows out as float32], given
as uint8 or as float32 holding such integers.

Test infrastructure only: karios_amd never imports this module.
"""
from __future__ import annotations

import numpy as np

D2_MAX = 128 * 255 * 255   # 8 323 200 < 2**24: every squared distance, and every partial sum of a product, is exact in float32


def as_integers(desc) -> np.ndarray:
    """The rows as int64; ValueError for a float32 element that is no integer in 0 .. 255 [def: refused, never rounded]."""
    a = np.asarray(desc)
    if a.ndim != 2 or a.shape[1] != 128:
        raise ValueError(f"descriptors of shape {a.shape}")
    if a.dtype != np.uint8:
        with np.errstate(invalid="ignore"):
            bad = ~((a >= 0) & (a <= 255) & (a == np.trunc(a)))
        if bad.any():
            r, c = np.argwhere(bad)[0]
            raise ValueError(f"element (row {r}, column {c}) is not an integer in 0 .. 255")
    return a.astype(np.int64)


def squared_distances(Q, T) -> np.ndarray:
    """d2[i, j] = sum_c (Q[i, c] - T[j, c])**2 as int64, through a float32 BLAS product: every partial sum of q . t is an integer
    <= 128 * 255**2 < 2**24, so float32 holds it exactly in any order of summation."""
    Q, T = as_integers(Q), as_integers(T)
    dot = (Q.astype(np.float32) @ T.astype(np.float32).T).astype(np.int64)
    return (Q ** 2).sum(1)[:, None] + (T ** 2).sum(1)[None, :] - 2 * dot


def distances(d2) -> np.ndarray:
    """The float32 nearest to sqrt(d2) [cv4.8: batchDistL2_32f takes std::sqrt of the float32 sum per element, BEFORE the k-best
    insertion]; float32(d2) is exact and numpy's float32 sqrt is correctly rounded."""
    return np.sqrt(np.asarray(d2).astype(np.float32))


def keys(d2) -> np.ndarray:
    """Order-preserving 64-bit key (float32 bits of the distance << 32 | train index): ascending keys = ascending (distance as float32,
    train index) [cv4.8: the insertion of BatchDistInvoker compares the float distances strictly and visits the train rows in index
    order, so among EQUAL FLOAT distances the lower index stays in front - also where its d2 is the larger one: from d2 = 4 197 200
    upwards neighbouring integers can share one float32 square root]."""
    d = distances(d2)
    return (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(d.shape[1], dtype=np.uint64)[None, :]


def knn(Q, T, k, blk=512):
    """BFMatcher(NORM_L2).knnMatch(Q, T, k) -> (idx int32 [N, k], dist float32 [N, k]): the first min(k, M) ranks; unused columns
    -1 / +inf [def]."""
    Q, T = np.asarray(Q), np.asarray(T)
    n, m = Q.shape[0], T.shape[0]
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, np.float32)
    kk = min(k, m)
    if n == 0 or kk == 0:
        return idx, dist
    for s in range(0, n, blk):
        key = keys(squared_distances(Q[s:s + blk], T))
        part = np.partition(key, kk - 1, axis=1)[:, :kk] if m > kk else key
        part = np.sort(part, axis=1)
        idx[s:s + blk, :kk] = (part & np.uint64(0xFFFFFFFF)).astype(np.int32)
        dist[s:s + blk, :kk] = (part >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, dist


def match_lowe_mutual(mon, ref, ratio=0.75):
    """[ref: global_align.py:178-202] -> (query_idx int32, train_idx int32, distance float32, (raw, lowe, mutual)).
    Lowe: a pair with fewer than two entries is skipped (M < 2); `m.distance < LOWE_RATIO * n.distance` is Python arithmetic on the two
    float32 attributes: float64(dist1) < ratio * float64(dist2), the product rounded once in float64 (0 < 0.75 * 0 is false: exact
    duplicates drop out).  Mutual: the nearest mon row of the match's ref row must be the match's mon row.  Rows in ascending mon
    index (the order of the reference's list comprehension)."""
    mon, ref = np.asarray(mon), np.asarray(ref)
    n, m = mon.shape[0], ref.shape[0]
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    if n == 0 or m < 2:
        return (*empty, (n, 0, 0))
    fi, fd = knn(mon, ref, 2)
    lowe = np.nonzero(fd[:, 0].astype(np.float64) < np.float64(ratio) * fd[:, 1].astype(np.float64))[0]
    if lowe.size == 0:
        return (*empty, (n, 0, 0))
    bi, _ = knn(ref, mon, 1)
    good = lowe[bi[fi[lowe, 0], 0] == lowe]
    return good.astype(np.int32), fi[good, 0], fd[good, 0], (n, int(lowe.size), int(good.size))


# ---- rows with chosen squared distances (shared by tests/test_match_host.py and tests/test_gpu_match.py) ----------------------------
def row_at(d2):
    """A row at squared distance d2 from the zero row: squares of values <= 255 that sum to d2, taken greedily."""
    r, left = np.zeros(128, np.int64), d2
    for c in range(128):
        v = min(255, int(np.sqrt(left)))
        r[c], left = v, left - v * v
    assert left == 0
    return r.astype(np.uint8)


def collision_rows():
    """A query row and two train rows with d2 = 4 197 201 and 4 197 200, which share one float32 distance."""
    lo, hi = 4197200, 4197201
    assert np.sqrt(np.float32(lo)) == np.sqrt(np.float32(hi))
    q = np.zeros(128, np.uint8)
    return q, row_at(hi), row_at(lo)


def lowe_rows(s, below):
    """Query 0 and two train rows at d2 = 9 s^2 (- 1 with `below`) and 16 s^2."""
    q = np.zeros(128, np.uint8)
    a, b = np.zeros(128, np.uint8), np.zeros(128, np.uint8)
    a[:9] = s
    b[:16] = s
    if below:
        a = row_at(9 * s * s - 1)
    return q, a, b
