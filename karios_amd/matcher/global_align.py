"""Global align step -- mirror of `karios.matcher.global_align` (reference global_align.py) on the GPU.

`_to_uint8` and `_preprocess` (percentile stretch + CLAHE, the dense front half) run on the GPU; so does SIFT
(`karios_amd.matcher.Sift`, passed as `sift=`); the descriptor matching behind it (both BFMatcher.knnMatch calls, Lowe's test, the mutual check: `match_descriptors`) runs on the GPU;
so do `cv2.findHomography` with RANSAC (`estimate_homography`), the ECC refinement of every candidate (`refine_global_alignment`) and
the renders of `apply_global_alignment` without its GeoTIFF writes (`render_global_alignment`).  `detect_global_alignment` chains
them as the reference does: with `sift=Sift()` the whole step runs on the GPU, with `sift=None` SIFT is cv2's, as before.
Every GPU call goes through `karios_amd.ops`.  The reference's arithmetic is kept as it is, casts included; INTEGRATION.md
section 6 notes the direction in which it composes the ECC residual.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from .. import ops

logger = logging.getLogger(__name__)

ECC_MAX_ITERS = 200
ECC_EPS = 1e-6
ECC_MIN_VALID = 1000   # _refine_with_ecc: "need >1000" (it skips below 1000)
LOWE_RATIO = 0.75      # global_align.py:51
MIN_MATCHES = 4        # global_align.py:53: cv2.findHomography needs at least 4 point pairs
RANSAC_THRESHOLD_PX = 3.0   # global_align.py:52
RANSAC_MAX_ITERS = 10000    # global_align.py:228
RANSAC_CONFIDENCE = 0.999   # global_align.py:229
SIFT_NFEATURES = 0          # global_align.py:48-50: cv2.SIFT_create(nfeatures=, contrastThreshold=, edgeThreshold=); 0 = unlimited
SIFT_CONTRAST_THRESHOLD = 0.02
SIFT_EDGE_THRESHOLD = 10


@dataclass
class GlobalAlignment:
    """Outcome of the global alignment: homography mon -> ref (global_align.py:68-85)."""

    matrix: np.ndarray  # 3x3 homography, mon pixel coords -> ref pixel coords
    n_inliers: int
    n_matches: int
    # (name, 3x3 matrix, ECC score) for every refinement candidate that converged, the chosen one included
    candidates: list = field(default_factory=list)

    @property
    def score(self) -> float:
        """RANSAC inlier ratio in [0, 1]."""
        return self.n_inliers / self.n_matches if self.n_matches else 0.0


def _to_uint8(arr: np.ndarray) -> np.ndarray:
    """Stretch between the 2nd and 98th percentile of the finite values (global_align.py:87-101): uint8 input passes through
    untouched, nothing finite gives zeros; other dtypes than uint16 / int16 / float32 go through astype(float32) on the host first.
    One host synchronisation between the order statistics and the stretch, for numpy's interpolation."""
    return ops.to_uint8_percentile(arr, (2.0, 98.0))


def _preprocess(arr: np.ndarray) -> np.ndarray:
    """uint8 stretch + CLAHE(clipLimit=2.0, tileGridSize=(8, 8)) to equalize radiometry across the two images
    (global_align.py:104-108); the raster is uploaded once."""
    return ops.preprocess(arr, (2.0, 98.0), 2.0, (8, 8))


def _points(kp) -> np.ndarray:
    """Key points as a float32 [n, 2] array: an array of coordinates (or an object that converts to one: `Sift`'s KeyPoints), or a
    sequence of objects with `.pt` (cv2.KeyPoint)."""
    if isinstance(kp, np.ndarray):
        pts = kp
    elif hasattr(kp, "__array__"):
        pts = np.asarray(kp)
    else:
        pts = np.array([k.pt for k in kp], dtype=np.float32).reshape(-1, 2)
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError(f"key points: expected an [n, 2] array or objects with .pt, got shape {pts.shape}")
    return pts.astype(np.float32)


def match_descriptors(kp_mon, desc_mon, kp_ref, desc_ref):
    """The matching of detect_global_alignment between SIFT and RANSAC (global_align.py:168-210) on the GPU: the checks on the
    descriptors, knnMatch(mon, ref, 2) + Lowe's ratio test + knnMatch(ref, mon, 1) + mutual check in one call, the log line, and the
    point arrays -> (src_pts, dst_pts), float32 [n_good, 2] in the reference's order, ready for cv2.findHomography.
    kp_*: [n, 2] arrays of (x, y) or sequences of objects with `.pt`; desc_*: uint8 or float32 [n, 128]."""
    if desc_mon is None or desc_ref is None:
        raise RuntimeError("SIFT found no descriptors in one or both images")
    if len(kp_mon) < MIN_MATCHES or len(kp_ref) < MIN_MATCHES:
        raise RuntimeError(
            f"Too few SIFT keypoints: mon={len(kp_mon)} ref={len(kp_ref)} "
            f"(need ≥{MIN_MATCHES})"
        )
    logger.info("Keypoints detected: mon=%d  ref=%d", len(kp_mon), len(kp_ref))
    query_idx, train_idx, _dist, (raw, lowe, mutual) = ops.match_lowe_mutual(desc_mon, desc_ref, LOWE_RATIO)
    logger.info("Matches: raw=%d  Lowe<%.2f=%d  mutual=%d", raw, LOWE_RATIO, lowe, mutual)
    if mutual < MIN_MATCHES:
        raise RuntimeError(
            f"Too few good matches after Lowe + cross-check: {mutual} (need ≥{MIN_MATCHES})"
        )
    return _points(kp_mon)[query_idx], _points(kp_ref)[train_idx]


def estimate_homography(src_pts, dst_pts):
    """cv2.findHomography(src_pts, dst_pts, cv2.RANSAC, RANSAC_THRESHOLD_PX, maxIters=10000, confidence=0.999) and what the reference
    does with its result (global_align.py:223-231) on the GPU -> (3x3 float64 matrix, n_inliers)."""
    matrix, inlier_mask = ops.find_homography(src_pts, dst_pts, RANSAC_THRESHOLD_PX, RANSAC_MAX_ITERS, RANSAC_CONFIDENCE)
    if matrix is None:
        raise RuntimeError("RANSAC failed to estimate a homography")
    n_inliers = int(inlier_mask.sum())
    logger.info("RANSAC initial fit: %s  inliers=%d/%d (%.1f%%)", _decompose(matrix), n_inliers, len(src_pts),
                100.0 * n_inliers / len(src_pts))
    return matrix, n_inliers


def _default_sift():
    try:
        import cv2
    except ImportError as exc:
        raise ImportError(
            "detect_global_alignment: SIFT is the one part of the align step karios_amd does not provide; "
            "install OpenCV (cv2) or pass sift=<object with detectAndCompute(image, None)>") from exc
    return cv2.SIFT_create(nfeatures=SIFT_NFEATURES, contrastThreshold=SIFT_CONTRAST_THRESHOLD, edgeThreshold=SIFT_EDGE_THRESHOLD)


def detect_global_alignment(mon_arr, ref_arr, prior=None, sift=None) -> GlobalAlignment:
    """detect_global_alignment of the reference (global_align.py:143-270): preprocess both images, SIFT (`sift.detectAndCompute`,
    cv2's SIFT when `sift` is None, the GPU's with `sift=karios_amd.matcher.Sift()`), descriptor matching, the prior's log line, RANSAC, ECC refinement of the candidates."""
    if sift is None:
        sift = _default_sift()
    mon_u8 = _preprocess(mon_arr)
    ref_u8 = _preprocess(ref_arr)
    mh, mw = mon_u8.shape
    rh, rw = ref_u8.shape
    logger.info("SIFT feature matching: mon=%dx%d  ref=%dx%d  contrast=%.3f  Lowe=%.2f  RANSAC=%.1fpx",
                mw, mh, rw, rh, SIFT_CONTRAST_THRESHOLD, LOWE_RATIO, RANSAC_THRESHOLD_PX)
    kp_mon, desc_mon = sift.detectAndCompute(mon_u8, None)
    kp_ref, desc_ref = sift.detectAndCompute(ref_u8, None)
    src_pts, dst_pts = match_descriptors(kp_mon, desc_mon, kp_ref, desc_ref)
    n_matches = len(src_pts)
    if prior is not None:
        # global_align.py:212-221, informational: the matches against the prior's upper-left 2 x 3 (translation + scale)
        prior = np.asarray(prior)
        predicted = (prior[:2, :2] @ src_pts.T).T + prior[:2, 2]
        errors = np.linalg.norm(dst_pts - predicted, axis=1)
        logger.info("Match error vs geotransform prior: median=%.1fpx  min=%.1fpx  max=%.1fpx",
                    float(np.median(errors)), float(errors.min()), float(errors.max()))
    matrix, n_inliers = estimate_homography(src_pts, dst_pts)
    return refine_global_alignment(mon_u8, ref_u8, matrix, n_inliers, n_matches, prior=prior)


def _prior_from_georefs(monitored, reference) -> Optional[np.ndarray]:
    """3x3 homography mon pixel -> ref pixel implied by the two geotransforms (global_align.py:112-140); duck-typed: the images
    need `projection`, `spatial_ref.IsSame`, `x_res`, `y_res`, `x_min`, `y_max`.  None without a usable prior."""
    if not monitored.projection or not reference.projection:
        return None
    try:
        if not monitored.spatial_ref.IsSame(reference.spatial_ref):
            return None
    except Exception:
        return None
    sx = monitored.x_res / reference.x_res
    sy = monitored.y_res / reference.y_res
    tx = (monitored.x_min - reference.x_min) / reference.x_res
    ty = (monitored.y_max - reference.y_max) / reference.y_res
    return np.array([[sx, 0.0, tx], [0.0, sy, ty], [0.0, 0.0, 1.0]], dtype=np.float64)


def _decompose(matrix: np.ndarray) -> str:
    """Compact diagnostic string of a 3x3 homography (global_align.py:273-292)."""
    sx = float(np.hypot(matrix[0, 0], matrix[0, 1]))
    sy = float(np.hypot(matrix[1, 0], matrix[1, 1]))
    rot = float(np.degrees(np.arctan2(matrix[1, 0], matrix[0, 0])))
    persp = float(np.hypot(matrix[2, 0], matrix[2, 1]))
    return (
        f"rot={rot:+.3f}°  sx={sx:.4f} sy={sy:.4f}  "
        f"tx={float(matrix[0,2]):+.2f} ty={float(matrix[1,2]):+.2f}  "
        f"persp={persp:.6f}"
    )


def _sobel_magnitude(img: np.ndarray) -> np.ndarray:
    """Sobel gradient magnitude normalised to [0, 1], float32 (global_align.py:295-306)."""
    return ops.sobel_magnitude(img)


def _refine_candidates(mon_u8, ref_u8, inits):
    """_refine_with_ecc for several starting matrices in one call (the template's Sobel magnitude is computed once)
    -> [(matrix or None, cc or nan)]."""
    out = []
    for init, (_final, cc, _it, valid, status, residual) in zip(
            inits, ops.refine_ecc_candidates(mon_u8, ref_u8, [np.asarray(m) for m in inits], ECC_MAX_ITERS, ECC_EPS)):
        if status == ops._lib.ECC_SKIPPED:
            logger.warning("ECC skipped: pre-warped mon has only %d valid pixels (need >1000)", valid)
            out.append((None, float("nan")))
        elif status != ops._lib.ECC_CONVERGED:
            logger.warning("findTransformECC raised: the algorithm stopped before its convergence")
            out.append((None, float("nan")))
        else:
            # the reference's composition, kept as it is
            out.append((residual.astype(np.float64) @ np.asarray(init).astype(np.float64), float(cc)))
    return out


def _refine_with_ecc(mon_u8: np.ndarray, ref_u8: np.ndarray, init: np.ndarray):
    """Refine the mon -> ref homography with ECC on Sobel magnitudes (global_align.py:309-359)
    -> (refined 3x3, ecc score), or (None, nan) on failure."""
    return _refine_candidates(mon_u8, ref_u8, [init])[0]


def refine_global_alignment(mon_u8, ref_u8, ransac_matrix, n_inliers, n_matches, prior=None) -> GlobalAlignment:
    """The candidate loop of detect_global_alignment after RANSAC (global_align.py:233-270): ECC from the RANSAC matrix and
    from the geotransform prior, the highest score wins (strict >), the RANSAC matrix stays when none converges."""
    candidates = [("RANSAC", ransac_matrix)]
    if prior is not None:
        candidates.append(("prior", prior))
    converged = []
    best_matrix, best_ecc, best_source = None, -np.inf, ""
    results = _refine_candidates(mon_u8, ref_u8, [m for _, m in candidates])
    for (name, _init), (refined, ecc_score) in zip(candidates, results):
        if refined is None:
            logger.warning("ECC from %s: failed", name)
            continue
        logger.info("ECC from %s: %s  ECC=%.4f", name, _decompose(refined), ecc_score)
        converged.append((name, refined, ecc_score))
        if ecc_score > best_ecc:
            best_ecc, best_matrix, best_source = ecc_score, refined, name
    matrix = ransac_matrix
    if best_matrix is not None:
        logger.info("Selected alignment: ECC-refined from %s (ECC=%.4f)", best_source, best_ecc)
        matrix = best_matrix
    else:
        logger.warning("All ECC refinements failed; keeping RANSAC estimate")
    return GlobalAlignment(matrix=matrix, n_inliers=n_inliers, n_matches=n_matches, candidates=converged)


def _array(img):
    return img.array if hasattr(img, "array") else np.asarray(img)


def render_global_alignment(monitored, reference, mask, alignment: GlobalAlignment):
    """The numeric part of apply_global_alignment (global_align.py:415-506), without the GeoTIFF writes
    -> (aligned mon, aligned mask or None, {candidate name: aligned mon of that candidate}).
    monitored / reference / mask: arrays or images with `.array` (and `.no_data_value` for monitored)."""
    mon_arr = _array(monitored)
    rh, rw = _array(reference).shape
    warp_m = alignment.matrix
    nodata = getattr(monitored, "no_data_value", None)
    border_mon = float(nodata) if nodata is not None else 0.0
    mon_f32 = mon_arr.astype(np.float32)
    aligned_mon = ops.warp_perspective(mon_f32, warp_m, (rw, rh), flags=ops.INTER_LINEAR,
                                       border_value=border_mon).astype(mon_arr.dtype)
    alternatives = {}
    for cand_name, cand_matrix, _cand_ecc in alignment.candidates:
        if cand_matrix is alignment.matrix or np.allclose(cand_matrix, alignment.matrix):
            continue
        alternatives[cand_name] = ops.warp_perspective(mon_f32, cand_matrix.astype(np.float32), (rw, rh), flags=ops.INTER_LINEAR,
                                                       border_value=border_mon).astype(mon_arr.dtype)
    aligned_mask = None
    if mask is not None:
        aligned_mask = ops.warp_perspective(_array(mask).astype(np.uint8), warp_m, (rw, rh), flags=ops.INTER_NEAREST, border_value=0)
    return aligned_mon, aligned_mask, alternatives
