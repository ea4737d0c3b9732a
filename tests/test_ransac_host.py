"""CPU suite: the RANSAC homography of the align step (cv2.findHomography with cv2.RANSAC, karios/matcher/global_align.py:223-230).

1. Anchors of tests/ransac_restatement.py, the definition the library is held to.
2. csrc/ransac_math.hpp - the text the kernels and the library's host side compile - built by g++ with -ffp-contract=off under the
   address and undefined-behaviour sanitizers and compared with the restatement bit for bit (tests/ransac_host_driver.py, in a
   subprocess with libasan preloaded).
3. The host glue of karios_amd.matcher.global_align with ops.find_homography replaced.
4. The ABI carries the two entry points.
"""
import logging
import os
import re
import sys

import numpy as np
import pytest

import ransac_restatement as R
import sanitizer_harness as san

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. anchors ---------------------------------------------------------------------------------------------------------------------------
def test_rng_stream_and_uniform():
    rng = R.RNG()
    assert [rng.next() for _ in range(4)] == [130063605, 3133359004, 2578348940, 925327173]
    rng = R.RNG()
    assert [rng.uniform(1000), rng.uniform(7)] == [130063605 % 1000, 3133359004 % 7]


def test_update_num_iters_table():
    """log(1 - 0.999) / log(1 - w^4), rounded: the table of the design note; the cap of 10 000 holds the shares the note files under
    "<= 0.17" from 0.16 down (at 0.17 itself the formula gives 8 267)."""
    assert [R.update_num_iters(0.999, 1 - w, 4, 10000) for w in (0.5, 0.3, 0.2)] == [107, 849, 4314]
    assert R.update_num_iters(0.999, 1 - 0.1, 4, 10000) == 10000 and R.update_num_iters(0.999, 1 - 0.16, 4, 10000) == 10000
    assert R.update_num_iters(0.999, 1 - 0.17, 4, 10000) == 8267
    assert R.update_num_iters(0.999, 0.0, 4, 10000) == 0        # every pair an inlier: denom underflows, the loop stops
    assert R.update_num_iters(0.999, 1.0, 4, 10000) == 10000    # no inlier at all
    assert R.update_num_iters(0.999, 0.5, 4, 50) == 50          # never above the current niters


def test_check_subset():
    good = np.array([[0, 0], [100, 0], [100, 100], [0, 100]], np.float32)
    assert R.check_subset(good, good + 5)
    collinear = good.copy()
    collinear[3] = [50, 0]                                       # on the line through points 0 and 1
    assert not R.check_subset(collinear, good) and not R.check_subset(good, collinear)
    reflected = good[[1, 0, 2, 3]]                               # two triples change orientation, two do not
    assert not R.check_subset(good, reflected)
    mirrored = good * np.float32([-1, 1])                        # all four change: a reflection is consistent
    assert R.check_subset(good, mirrored)


def _project(H, pts):
    p = np.concatenate([pts.astype(np.float64), np.ones((len(pts), 1))], 1) @ H.T
    return (p[:, :2] / p[:, 2:]).astype(np.float32)


def test_four_pairs_return_the_homography():
    H = np.array([[1.01, -0.02, 12.5], [0.015, 0.99, -7.25], [1e-6, -2e-6, 1.0]])
    src = np.array([[100, 200], [9000, 300], [8800, 9500], [400, 9100]], np.float64)
    p = np.concatenate([src, np.ones((4, 1))], 1) @ H.T
    dst = p[:, :2] / p[:, 2:]
    # float32 inputs are what findHomography reads: make them exact first, then fit the homography they define
    src32, dst32 = src.astype(np.float32), dst.astype(np.float32)
    got, mask = R.find_homography(src32, dst32)
    assert mask.dtype == np.uint8 and mask.shape == (4, 1) and (mask == 1).all()
    q = np.concatenate([src32.astype(np.float64), np.ones((4, 1))], 1) @ got.T
    assert np.abs(q[:, :2] / q[:, 2:] - dst32.astype(np.float64)).max() < 1e-6
    # the matrix itself, against the exact float64 solve of the same four float32 pairs
    A, b = [], []
    for (x, y), (u, v) in zip(src32.astype(np.float64), dst32.astype(np.float64)):
        A += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        b += [u, v]
    want = np.append(np.linalg.solve(np.array(A), np.array(b)), 1.0).reshape(3, 3)
    assert np.abs(got / want - 1).max() < 1e-9
    with pytest.raises(ValueError):
        R.find_homography(src32[:3], dst32[:3])


def test_planted_scene_returns_the_planted_flags():
    from karios_amd import synth
    src, dst, planted, H = synth.homography_scene(1500, 0.4, 0.0, seed=11)
    info = {}
    got, mask = R.find_homography(src, dst, info=info)
    assert np.array_equal(mask[:, 0] != 0, planted)
    assert info["best_count"] == planted.sum() and 0 < info["ran"] < 10000 and 1 <= info["lm_iters"] <= 10
    assert np.abs(_project(got, src[planted]).astype(np.float64) - dst[planted]).max() < 0.05
    # failure: nothing but noise, fewer than 4 inliers for every model
    rng = np.random.default_rng(5)
    a, b = rng.uniform(0, 10980, (60, 2)).astype(np.float32), rng.uniform(0, 10980, (60, 2)).astype(np.float32)
    got, mask = R.find_homography(a, b, 1e-6, 300)      # the threshold is below float32 rounding at these coordinates
    assert got is None and mask.shape == (60, 1) and not mask.any()


def test_jacobi_against_eigh():
    rng = np.random.default_rng(1)
    for _ in range(20):
        A = rng.normal(size=(9, 9))
        A = A + A.T
        W, V, rot = R.jacobi(A)
        want = np.linalg.eigh(A)[0][::-1]
        assert rot < 30 * 81 and np.abs(W - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(V @ A @ V.T - np.diag(W)).max() < 1e-12 * np.abs(want).max() * 10


def test_against_cv2_when_it_imports():
    cv2 = pytest.importorskip("cv2")
    from karios_amd import synth
    src, dst, _planted, _H = synth.homography_scene(3000, 0.3, 0.4, seed=7)
    want, wmask = cv2.findHomography(src, dst, cv2.RANSAC, 3.0, maxIters=10000, confidence=0.999)
    got, mask = R.find_homography(src, dst, 3.0, 10000, 0.999)
    assert np.array_equal(mask, wmask)
    assert np.abs(got / want - 1).max() <= 1e-6


# ---- 2. the shared header -------------------------------------------------------------------------------------------------------------------
SHIM = r"""
#include "ransac_math.hpp"
#include <vector>
extern "C" {
void rs_rng(int k, uint32_t *out) { uint64_t s = ~(uint64_t)0; for (int i = 0; i < k; i++) out[i] = rs::rng_next(s); }
int rs_subsets(const float *pairs, int n, int k, int *idx)
{
    uint64_t s = ~(uint64_t)0;
    int i = 0;
    for (; i < k; i++) if (!rs::get_subset(pairs, n, s, idx + 4 * i)) break;
    return i;
}
int rs_check_subset(const float *a, const float *b) { return rs::check_subset(a, b); }
int rs_update(double p, double ep, int mp, int cap) { return rs::update_num_iters(p, ep, mp, cap); }
int rs_dlt(const float *M, const float *m, int count, double *H) { return rs::dlt(M, m, count, H); }
void rs_dlt4_many(const float *pairs, const int *idx, int k, double *H, int *ok)
{
    for (int i = 0; i < k; i++) {
        float M[8], m[8];
        for (int j = 0; j < 4; j++) {
            const float *q = pairs + 4 * (size_t)idx[4 * i + j];
            M[2 * j] = q[0]; M[2 * j + 1] = q[1]; m[2 * j] = q[2]; m[2 * j + 1] = q[3];
        }
        for (int j = 0; j < 9; j++) H[9 * i + j] = 0;
        ok[i] = rs::dlt(M, m, 4, H + 9 * i);
    }
}
int rs_jacobi(const double *A, int n, double *W, double *V)
{
    rs::PlainStore st;
    for (int i = 0; i < n * n; i++) st.A[i] = A[i];
    const int rotations = rs::jacobi(st, n);
    for (int i = 0; i < n; i++) W[i] = st.W[i];
    for (int i = 0; i < n * n; i++) V[i] = st.V[i];
    return rotations;
}
void rs_err(const float *Hf, const float *quad, int n, float *err)
{
    for (int i = 0; i < n; i++) err[i] = rs::reproj_err(Hf + 9 * (size_t)i, quad[4 * i], quad[4 * i + 1], quad[4 * i + 2], quad[4 * i + 3]);
}
int rs_count(const float *pairs, const double *H, int n, double threshold)
{
    float Hf[9];
    for (int j = 0; j < 9; j++) Hf[j] = (float)H[j];
    const float thr = rs::threshold_sq(threshold);
    int c = 0;
    for (int i = 0; i < n; i++) c += rs::reproj_err(Hf, pairs[4 * i], pairs[4 * i + 1], pairs[4 * i + 2], pairs[4 * i + 3]) <= thr;
    return c;
}
void rs_replay(const int *counts, const int *valid, int k, int n, double confidence, int max_iters, int *out)
{
    rs::Replay r;
    rs::replay_init(r, max_iters);
    // in pieces, as the library's batches arrive
    for (int lo = 0, step = 1; lo < k && r.iter < r.niters && r.iter == lo; lo += step, step *= 2) {
        const int hi = lo + step < k ? lo + step : k;
        rs::replay(r, hi, counts + lo, valid + lo, n, confidence);
    }
    out[0] = r.niters; out[1] = r.max_good; out[2] = r.best_iter; out[3] = r.iter;
}
int rs_refine(const float *M, const float *m, int count, double *H) { return rs::refine_on_inliers(M, m, count, H); }
}
"""


def test_shared_header_matches_the_restatement_under_sanitizers(tmp_path):
    env = san.san_env()
    src, so = tmp_path / "ransac_shim.cpp", tmp_path / "libransac_shim.so"
    src.write_text(SHIM)
    san.build(src, so)
    san.run([sys.executable, os.path.join(ROOT, "tests", "ransac_host_driver.py"), str(so)], "RANSAC-HOST OK", 1500, env)


# ---- 3. host glue -----------------------------------------------------------------------------------------------------------------------
def test_estimate_homography_error_and_log_line(monkeypatch, caplog):
    from karios_amd import ops
    from karios_amd.matcher import global_align as GA
    src = np.zeros((10, 2), np.float32)
    seen = {}

    def fake(s, d, thr, max_iters, confidence):
        seen.update(thr=thr, max_iters=max_iters, confidence=confidence)
        return seen["matrix"], np.array([[1]] * 7 + [[0]] * 3, np.uint8)

    monkeypatch.setattr(ops, "find_homography", fake)
    seen["matrix"] = None
    with pytest.raises(RuntimeError, match="RANSAC failed to estimate a homography"):
        GA.estimate_homography(src, src)
    assert (seen["thr"], seen["max_iters"], seen["confidence"]) == (3.0, 10000, 0.999) == (GA.RANSAC_THRESHOLD_PX, 10000, 0.999)
    seen["matrix"] = np.array([[1.0, 0.0, 2.5], [0.0, 1.0, -1.0], [0.0, 0.0, 1.0]])
    with caplog.at_level(logging.INFO, logger=GA.logger.name):
        matrix, n_inliers = GA.estimate_homography(src, src)
    assert matrix is seen["matrix"] and n_inliers == 7
    line = [r.getMessage() for r in caplog.records if "RANSAC initial fit" in r.getMessage()]
    assert len(line) == 1 and "tx=+2.50 ty=-1.00" in line[0] and line[0].endswith("inliers=7/10 (70.0%)")


def test_detect_global_alignment_call_order_and_import_error(monkeypatch):
    from karios_amd.matcher import global_align as GA
    calls = []

    class FakeSift:
        def detectAndCompute(self, image, mask):
            calls.append(("sift", image, mask))
            return f"kp{image}", f"desc{image}"

    monkeypatch.setattr(GA, "_preprocess", lambda arr: calls.append(("preprocess", arr)) or _Img(arr))
    monkeypatch.setattr(GA, "match_descriptors", lambda *a: calls.append(("match",) + a) or (np.ones((6, 2), np.float32), np.ones((6, 2), np.float32)))
    monkeypatch.setattr(GA, "estimate_homography", lambda s, d: calls.append(("ransac", len(s))) or ("M", 5))
    monkeypatch.setattr(GA, "refine_global_alignment", lambda *a, **k: calls.append(("refine", a, k)) or "alignment")
    prior = np.eye(3)
    assert GA.detect_global_alignment("mon", "ref", prior=prior, sift=FakeSift()) == "alignment"
    assert [c[0] for c in calls] == ["preprocess", "preprocess", "sift", "sift", "match", "ransac", "refine"]
    assert calls[0][1] == "mon" and calls[1][1] == "ref" and calls[2][1].name == "mon" and calls[2][2] is None and calls[3][1].name == "ref"
    assert calls[4][1:] == ("kpmon", "descmon", "kpref", "descref")
    (mon_u8, ref_u8, matrix, n_inliers, n_matches), kw = calls[6][1], calls[6][2]
    assert (mon_u8.name, ref_u8.name, matrix, n_inliers, n_matches) == ("mon", "ref", "M", 5, 6) and kw["prior"] is prior
    # without cv2 and without a sift object: a clear ImportError
    monkeypatch.setitem(sys.modules, "cv2", None)
    with pytest.raises(ImportError, match="SIFT is the one part of the align step karios_amd does not provide"):
        GA.detect_global_alignment("mon", "ref")


class _Img:
    shape = (8, 9)

    def __init__(self, name):
        self.name = name

    def __format__(self, spec):
        return self.name


# ---- 4. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_signature_table_carry_the_entry_points():
    from karios_amd import _lib
    header = open(os.path.join(ROOT, "include", "karios_hip.h")).read()
    for name in ("km_find_homography_ransac", "km_find_homography_ransac_dev"):
        assert re.search(rf"\bint {name}\s*\(", header) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == 15
    assert "global_align.py:223-230" in header and ' *   "ransac_first_batch"' in header
    assert hasattr(_lib.load(), "km_find_homography_ransac_dev")
    # nothing of the product imports the restatement
    for dirpath, _, files in os.walk(os.path.join(ROOT, "karios_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "ransac_restatement" not in open(os.path.join(dirpath, f)).read(), f
