"""Descriptor matching (csrc/api_match.hip) and the RANSAC homography (csrc/api_ransac.hip) of the align step."""
import ctypes as C

import numpy as np

from .._lib import Context, dtype_code, ptr, row_stride
from ._place import Place, _ctx

DESCRIPTOR_DIM = 128


def _as_descriptors(arr, what):
    """uint8 or float32 [n, 128] with contiguous rows, as sift.detectAndCompute returns them; ValueError for anything else."""
    a = np.asarray(arr)
    if a.ndim != 2 or a.shape[1] != DESCRIPTOR_DIM:
        raise ValueError(f"{what}: expected descriptors of shape [n, {DESCRIPTOR_DIM}], got {a.shape}")
    if a.dtype != np.uint8 and a.dtype != np.float32:
        raise ValueError(f"{what}: expected uint8 or float32 descriptors, got {a.dtype}")
    if a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or (a.shape[0] > 1 and a.strides[0] < DESCRIPTOR_DIM * a.itemsize):
        raise ValueError(f"{what}: rows must be contiguous")
    return a


def _u8_descriptors(a, what):
    """float32 descriptors as uint8; ValueError (naming the element) when one is not an integer in 0 .. 255."""
    if a.dtype == np.uint8:
        return a
    with np.errstate(invalid="ignore"):
        bad = ~((a >= 0) & (a <= 255) & (a == np.trunc(a)))
    if bad.any():
        r, col = np.argwhere(bad)[0]
        raise ValueError(f"{what}: element (row {r}, column {col}) = {a[r, col]!r} is not an integer in 0 .. 255")
    return a.astype(np.uint8)


def knn_match(query, train, k: int = 2, ctx: Context | None = None):
    """cv2.BFMatcher(NORM_L2).knnMatch(query, train, k) (global_align.py:178-179, 193) for k = 1 or 2 -> (idx int32 [n, k],
    dist float32 [n, k]): the train rows ranked by (float32 distance, train index); columns beyond len(train) hold -1 / +inf."""
    q, t = _as_descriptors(query, "knn_match query"), _as_descriptors(train, "knn_match train")
    if k not in (1, 2):
        raise ValueError(f"knn_match: k = {k} (1 or 2)")
    q, t = _u8_descriptors(q, "knn_match query"), _u8_descriptors(t, "knn_match train")
    idx = np.full((q.shape[0], k), -1, np.int32)
    dist = np.full((q.shape[0], k), np.inf, np.float32)
    if q.shape[0] and t.shape[0]:
        c = _ctx(ctx)
        c.check(c.lib.km_knn_match_u8(c.handle, ptr(q), q.shape[0], row_stride(q), ptr(t), t.shape[0], row_stride(t), DESCRIPTOR_DIM, int(k),
                                      ptr(idx), ptr(dist)), "km_knn_match_u8")
    return idx, dist


def match_lowe_mutual(desc_mon, desc_ref, ratio: float = 0.75, ctx: Context | None = None):
    """knnMatch(mon, ref, 2), Lowe's ratio test, knnMatch(ref, mon, 1) and the mutual check (global_align.py:178-202) in one call
    -> (query_idx int32, train_idx int32, distance float32, (raw, lowe, mutual)): the mutual rows in ascending mon index.  float32
    descriptors must hold integers 0 .. 255 (KariosHipError with code E_ARG otherwise)."""
    m, r = _as_descriptors(desc_mon, "match_lowe_mutual mon"), _as_descriptors(desc_ref, "match_lowe_mutual ref")
    if m.dtype != r.dtype:
        raise ValueError(f"match_lowe_mutual: descriptor dtypes differ ({m.dtype}, {r.dtype})")
    n = m.shape[0]
    qi, ti, dist = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
    counts = (C.c_int * 3)(n, 0, 0)
    if n and r.shape[0]:
        c = _ctx(ctx)
        c.check(c.lib.km_match_lowe_mutual(c.handle, ptr(m), n, row_stride(m), ptr(r), r.shape[0], row_stride(r), dtype_code(m), DESCRIPTOR_DIM,
                                           float(ratio), n, ptr(qi), ptr(ti), ptr(dist), counts), "km_match_lowe_mutual")
    k = counts[2]
    return qi[:k], ti[:k], dist[:k], (counts[0], counts[1], counts[2])


# ---- RANSAC homography of the align step (csrc/api_ransac.hip) --------------------------------------------------------------------
RANSAC_STATS = ("ran", "evaluated", "best_iter", "best_count", "lm_iters", "first_batch", "batches")


def _as_points(arr, what):
    """float32 [n, 2] whose rows hold x, y next to each other (a row stride is fine); cv2's [n, 1, 2] is accepted."""
    a = np.asarray(arr)
    if a.ndim == 3 and a.shape[1] == 1:
        a = a[:, 0, :]
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{what}: expected points of shape [n, 2], got {a.shape}")
    if a.dtype != np.float32:
        a = a.astype(np.float32)
    if a.strides[1] != 4 or a.strides[0] % 4 or (a.shape[0] > 1 and a.strides[0] < 8):
        a = np.ascontiguousarray(a)
    return a


def find_homography(src_pts, dst_pts, ransac_reproj_threshold: float = 3.0, max_iters: int = 10000, confidence: float = 0.999,
                    ctx: Context | None = None, return_stats: bool = False, return_iterations: bool = False):
    """cv2.findHomography(src_pts, dst_pts, cv2.RANSAC, ransac_reproj_threshold, maxIters=max_iters, confidence=confidence)
    (global_align.py:223-230) -> (matrix float64 [3, 3] or None, mask uint8 [n, 1]), cv2's return shape.  Points: float32 [n, 2]
    numpy arrays, or torch tensors on the context's device (the device form; the mask still comes back as a numpy array).
    return_stats adds a dict of RANSAC_STATS; return_iterations adds (inlier counts, valid flags) of every evaluated iteration."""
    place = Place((src_pts,))
    if place.dev:
        s, d = src_pts, dst_pts
        if not place.holds(d) or any(place.dtype(a) != np.float32 or a.dim() != 2 or a.shape[1] != 2 for a in (s, d)):
            raise ValueError("find_homography: device points must be float32 tensors of shape [n, 2]")
        if s.stride(1) != 1 or d.stride(1) != 1:
            raise ValueError("find_homography: x and y of a device point must be adjacent")
    else:
        s, d = _as_points(src_pts, "find_homography src_pts"), _as_points(dst_pts, "find_homography dst_pts")
    n = s.shape[0]
    args = (place.pointer(s), place.strides(s)[0] if n > 1 else 2, place.pointer(d), place.strides(d)[0] if d.shape[0] > 1 else 2)
    mask = place.empty((max(n, 1), 1), np.uint8)
    mask[...] = 0
    if d.shape[0] != n:
        raise ValueError(f"find_homography: {n} source points, {d.shape[0]} destination points")
    H = np.zeros(9, np.float64)
    found = C.c_int(0)
    stats = (C.c_int64 * 8)()
    room = max(int(max_iters), 1)
    it_counts = np.zeros(room if return_iterations else 0, np.int32)
    it_valid = np.zeros(room if return_iterations else 0, np.int32)
    place.call(_ctx(ctx), "km_find_homography_ransac", *args, n, float(ransac_reproj_threshold), int(max_iters), float(confidence),
               H.ctypes.data_as(C.POINTER(C.c_double)), place.pointer(mask), C.byref(found), stats,
               *((ptr(it_counts), ptr(it_valid)) if return_iterations else (None, None)))
    out = (H.reshape(3, 3) if found.value else None, place.to_host(mask[:n]))
    if return_stats:
        out += (dict(zip(RANSAC_STATS, (int(v) for v in stats))),)
    if return_iterations:
        k = int(stats[1])
        out += ((it_counts[:k], it_valid[:k]),)
    return out
