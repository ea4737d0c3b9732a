"""numpy / plain-Python restatement of cv2.findHomography(src, dst, cv2.RANSAC, threshold, maxIters=, confidence=) as the global align
step calls it (karios/matcher/global_align.py:223-230), as libkarios_hip.so computes it (ransac_math.hpp, k_ransac.hip, api_ransac.hip).

This is the DEFINITION the library is held to, bit for bit (tests/test_ransac_host.py for the shared header, tests/test_gpu_ransac.py
for the kernels).  OpenCV's sources are not at hand and cv2 is absent, so parity with cv2 itself is unpinned;
tests/test_ransac_host.py compares the two when cv2 imports.  Points marked [cv4.8] come from knowledge of OpenCV 4.8's sources
(fundam.cpp, ptsetreg.cpp, levmarq.cpp, rand.cpp, lapack.cpp, matmul), [ref] from the reference's Python, [def] are choices of this
project.  An OpenCV built with the Eigen library (HAVE_EIGEN) does not run the Jacobi routine restated here at all: cv::eigen then
goes through Eigen::SelfAdjointEigenSolver, another algorithm with other roundings.  What is restated is the build without it.

Python floats are IEEE float64 and every operation below is rounded on its own (no fused multiply-add), which is what the library's
-ffp-contract=off gives.  Sums over points run in index order (`seq_sum`).

Test infrastructure only: karios_amd never imports this module.
"""
from __future__ import annotations

import math

import numpy as np

DBL_EPSILON = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
FLT_EPSILON = 1.1920928955078125e-07
MODEL_POINTS = 4
SUBSET_ATTEMPTS = 1000   # [cv4.8] getSubset's maxAttempts (its default); only a scene that fails this many draws in a row can tell
LM_MAX_ITERS = 10        # [cv4.8] createLMSolver(HomographyRefineCallback, 10)


# ---- rand.cpp ----------------------------------------------------------------------------------------------------------------------------
class RNG:
    """[cv4.8] cv::RNG: 64-bit state, multiply-with-carry step with multiplier 4164903690, the output is the low 32 bits.
    RANSACPointSetRegistrator::run seeds it with (uint64)-1."""

    def __init__(self, state=0xFFFFFFFFFFFFFFFF):
        self.state = state if state else 0xFFFFFFFF

    def next(self) -> int:
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform(self, n: int) -> int:
        """[cv4.8] uniform(0, n) = next() % n."""
        return self.next() % n


# ---- checkSubset / getSubset ----------------------------------------------------------------------------------------------------------------
def have_collinear(p, count) -> bool:
    """[cv4.8] haveCollinearPoints: only the LAST point is tested against the lines through two earlier ones.  The coordinate
    differences are float32 subtractions widened to float64; the test itself is float64 against FLT_EPSILON."""
    p = np.asarray(p, np.float32)
    i = count - 1
    for j in range(i):
        dx1, dy1 = float(p[j, 0] - p[i, 0]), float(p[j, 1] - p[i, 1])
        for k in range(j):
            dx2, dy2 = float(p[k, 0] - p[i, 0]), float(p[k, 1] - p[i, 1])
            if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def _det3_ones(p, a, b, c) -> float:
    """[cv4.8] determinant(Matx33d) of the rows (x, y, 1) of three points, cofactors along the first row."""
    a00, a01, a10, a11, a20, a21 = float(p[a, 0]), float(p[a, 1]), float(p[b, 0]), float(p[b, 1]), float(p[c, 0]), float(p[c, 1])
    return a00 * (a11 * 1.0 - a21 * 1.0) - a01 * (a10 * 1.0 - a20 * 1.0) + 1.0 * (a10 * a21 - a20 * a11)


def check_subset(src4, dst4) -> bool:
    """[cv4.8] HomographyEstimatorCallback::checkSubset for count == 4: no collinear triple on either side (as far as
    haveCollinearPoints looks), and the orientation of the four point triples is kept by all of them or reversed by all of them."""
    src4, dst4 = np.asarray(src4, np.float32), np.asarray(dst4, np.float32)
    if have_collinear(src4, 4) or have_collinear(dst4, 4):
        return False
    negative = 0
    for a, b, c in ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3)):
        negative += _det3_ones(src4, a, b, c) * _det3_ones(dst4, a, b, c) < 0
    return negative in (0, 4)


def get_subset(src, dst, rng, max_attempts=SUBSET_ATTEMPTS):
    """[cv4.8] getSubset: 4 indices, each redrawn while it repeats an earlier one; checkSubset at the end; None after max_attempts
    subsets failed."""
    n = len(src)
    for _ in range(max_attempts):
        idx = []
        for _i in range(MODEL_POINTS):
            v = rng.uniform(n)
            while v in idx:
                v = rng.uniform(n)
            idx.append(v)
        if check_subset(src[idx], dst[idx]):
            return idx
    return None


def update_num_iters(p, ep, model_points, max_iters) -> int:
    """[cv4.8] RANSACUpdateNumIters; cvRound rounds half to even, as Python's round does."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - math.pow(1.0 - ep, model_points)
    if denom < DBL_MIN:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else int(round(num / denom))


# ---- lapack.cpp: Jacobi -----------------------------------------------------------------------------------------------------------------
def hypot_plain(a, b) -> float:
    """[def] hypot as three individually rounded float64 operations.  libm's hypot and the device library's differ in the last bit;
    the inputs are entries of a Hartley-normalised system, so a * a + b * b cannot overflow."""
    return math.sqrt(a * a + b * b)


def _jacobi_ind(A, n, idx, indR, indC):
    if idx < n - 1:
        m, mv = idx + 1, abs(A[idx][idx + 1])
        for i in range(idx + 2, n):
            val = abs(A[idx][i])
            if mv < val:
                mv, m = val, i
        indR[idx] = m
    if idx > 0:
        m, mv = 0, abs(A[0][idx])
        for i in range(1, idx):
            val = abs(A[i][idx])
            if mv < val:
                mv, m = val, i
        indC[idx] = m


def jacobi(A):
    """[cv4.8] JacobiImpl_<double>: the form that keeps, per row, the column of its largest off-diagonal entry right of the diagonal
    (indR) and, per column, the row of its largest entry above it (indC), annihilates the largest of those pivots, and refreshes the
    two indices of rows / columns k and l only.  At most 30 n^2 rotations; stops when |pivot| <= DBL_EPSILON.  Only the upper
    triangle is read.  -> (W descending, V with eigenvector i in row i, rotations)."""
    A = [[float(v) for v in row] for row in np.asarray(A, np.float64)]
    n = len(A)
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    W = [A[k][k] for k in range(n)]
    indR, indC = [0] * n, [0] * n
    for k in range(n):
        _jacobi_ind(A, n, k, indR, indC)
    iters = 0
    if n > 1:
        while iters < n * n * 30:
            k, mv = 0, abs(A[0][indR[0]])
            for i in range(1, n - 1):
                val = abs(A[i][indR[i]])
                if mv < val:
                    mv, k = val, i
            l = indR[k]
            for i in range(1, n):
                val = abs(A[indC[i]][i])
                if mv < val:
                    mv, k, l = val, indC[i], i
            p = A[k][l]
            if abs(p) <= DBL_EPSILON:
                break
            y = (W[l] - W[k]) * 0.5
            t = abs(y) + hypot_plain(p, y)
            s = hypot_plain(p, t)
            c = t / s
            s = p / s
            t = (p / t) * p
            if y < 0:
                s, t = -s, -t
            A[k][l] = 0.0
            W[k] -= t
            W[l] += t
            for i in range(k):
                a0, b0 = A[i][k], A[i][l]
                A[i][k], A[i][l] = a0 * c - b0 * s, a0 * s + b0 * c
            for i in range(k + 1, l):
                a0, b0 = A[k][i], A[i][l]
                A[k][i], A[i][l] = a0 * c - b0 * s, a0 * s + b0 * c
            for i in range(l + 1, n):
                a0, b0 = A[k][i], A[l][i]
                A[k][i], A[l][i] = a0 * c - b0 * s, a0 * s + b0 * c
            for i in range(n):
                a0, b0 = V[k][i], V[l][i]
                V[k][i], V[l][i] = a0 * c - b0 * s, a0 * s + b0 * c
            _jacobi_ind(A, n, k, indR, indC)
            _jacobi_ind(A, n, l, indR, indC)
            iters += 1
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            V[m], V[k] = V[k], V[m]
    return np.array(W), np.array(V), iters


def jacobi_batch(A):
    """`jacobi` on a stack of matrices [B, n, n] at once (every matrix goes through exactly the scalar routine's steps; matrices that
    have converged rest).  tests/test_ransac_host.py holds the two forms together."""
    A = np.array(A, np.float64)
    B, n, _ = A.shape
    cols = np.arange(n)
    V = np.broadcast_to(np.eye(n), (B, n, n)).copy()
    W = A[:, cols, cols].copy()
    indR, indC = np.zeros((B, n), np.int64), np.zeros((B, n), np.int64)
    rot = np.zeros(B, np.int64)

    def refresh(sel, idx):
        row = np.abs(A[sel, idx, :])
        new = np.where(cols[None, :] > idx[:, None], row, -1.0).argmax(1)
        ok = idx < n - 1
        indR[sel[ok], idx[ok]] = new[ok]
        col = np.abs(A[sel, :, idx])
        new = np.where(cols[None, :] < idx[:, None], col, -1.0).argmax(1)
        ok = idx > 0
        indC[sel[ok], idx[ok]] = new[ok]

    everyone = np.arange(B)
    for k in range(n):
        refresh(everyone, np.full(B, k))
    active = np.ones(B, bool)
    for _ in range(n * n * 30 if n > 1 else 0):
        sel = np.nonzero(active)[0]
        if sel.size == 0:
            break
        rv = np.abs(A[sel[:, None], cols[None, :n - 1], indR[sel][:, :n - 1]])
        cv = np.abs(A[sel[:, None], indC[sel][:, 1:], cols[None, 1:]])
        j = np.concatenate([rv, cv], 1).argmax(1)          # the first of the largest, in the order the scalar search visits them
        isrow = j < n - 1
        jr, jc = np.clip(j, 0, n - 2), np.clip(j - (n - 2), 1, n - 1)
        k = np.where(isrow, jr, indC[sel, jc])
        l = np.where(isrow, indR[sel, jr], jc)
        p = A[sel, k, l]
        go = ~(np.abs(p) <= DBL_EPSILON)
        active[sel[~go]] = False
        sel, k, l, p = sel[go], k[go], l[go], p[go]
        if sel.size == 0:
            continue
        y = (W[sel, l] - W[sel, k]) * 0.5
        t = np.abs(y) + np.sqrt(p * p + y * y)
        s = np.sqrt(p * p + t * t)
        c = t / s
        s = p / s
        t = (p / t) * p
        s, t = np.where(y < 0, -s, s), np.where(y < 0, -t, t)
        A[sel, k, l] = 0.0
        W[sel, k] -= t
        W[sel, l] += t
        for i in range(n):
            r0, c0 = np.where(i < k, i, k), np.where(i < k, k, i)
            r1, c1 = np.where(i < l, i, l), np.where(i < l, l, i)
            do = (i != k) & (i != l)
            a0, b0 = A[sel, r0, c0], A[sel, r1, c1]
            A[sel, r0, c0] = np.where(do, a0 * c - b0 * s, a0)
            A[sel, r1, c1] = np.where(do, a0 * s + b0 * c, b0)
        a0, b0 = V[sel, k, :], V[sel, l, :]
        V[sel, k, :] = a0 * c[:, None] - b0 * s[:, None]
        V[sel, l, :] = a0 * s[:, None] + b0 * c[:, None]
        refresh(sel, k)
        refresh(sel, l)
        rot[sel] += 1
    for k in range(n - 1):
        m = k + W[:, k:].argmax(1)
        wk, wm = W[everyone, k].copy(), W[everyone, m].copy()
        W[everyone, k], W[everyone, m] = wm, wk
        vk, vm = V[everyone, k].copy(), V[everyone, m].copy()
        V[everyone, k], V[everyone, m] = vm, vk
    return W, V, rot


# ---- fundam.cpp: HomographyEstimatorCallback::runKernel -----------------------------------------------------------------------------------
def seq_sum(t):
    """0 + t[0] + t[1] + ... in index order along the LAST axis, every addition rounded (np.add.accumulate is sequential)."""
    t = np.asarray(t, np.float64)
    return np.add.accumulate(np.concatenate([np.zeros(t.shape[:-1] + (1,)), t], -1), -1)[..., -1]


def _dlt_system(M, m):
    """Points [..., count, 2] -> (LtL [..., 9, 9], invHnorm, Hnorm2 [..., 3, 3], ok [...]).
    [cv4.8] centroids as float64 sums of the float32 coordinates divided by count; scales count / sum |coordinate - centroid|, the
    solve refused when one of the four sums is below DBL_EPSILON; LtL accumulated point by point, upper triangle, then mirrored."""
    M, m = np.asarray(M, np.float32).astype(np.float64), np.asarray(m, np.float32).astype(np.float64)
    count = M.shape[-2]
    cm = np.stack([seq_sum(m[..., 0]), seq_sum(m[..., 1])], -1) / count
    cM = np.stack([seq_sum(M[..., 0]), seq_sum(M[..., 1])], -1) / count
    sm = np.stack([seq_sum(np.abs(m[..., 0] - cm[..., None, 0])), seq_sum(np.abs(m[..., 1] - cm[..., None, 1]))], -1)
    sM = np.stack([seq_sum(np.abs(M[..., 0] - cM[..., None, 0])), seq_sum(np.abs(M[..., 1] - cM[..., None, 1]))], -1)
    ok = ~((np.abs(sm) < DBL_EPSILON).any(-1) | (np.abs(sM) < DBL_EPSILON).any(-1))
    with np.errstate(all="ignore"):
        sm, sM = count / sm, count / sM
        x, y = (m[..., 0] - cm[..., None, 0]) * sm[..., None, 0], (m[..., 1] - cm[..., None, 1]) * sm[..., None, 1]
        X, Y = (M[..., 0] - cM[..., None, 0]) * sM[..., None, 0], (M[..., 1] - cM[..., None, 1]) * sM[..., None, 1]
        one, zero = np.ones_like(x), np.zeros_like(x)
        Lx = [X, Y, one, zero, zero, zero, -x * X, -x * Y, -x]
        Ly = [zero, zero, zero, X, Y, one, -y * X, -y * Y, -y]
        LtL = np.zeros(M.shape[:-2] + (9, 9))
        for j in range(9):
            for k in range(j, 9):
                LtL[..., j, k] = LtL[..., k, j] = seq_sum(Lx[j] * Lx[k] + Ly[j] * Ly[k])
        z, o = np.zeros_like(sm[..., 0]), np.ones_like(sm[..., 0])
        inv_hnorm = np.stack([1.0 / sm[..., 0], z, cm[..., 0], z, 1.0 / sm[..., 1], cm[..., 1], z, z, o], -1).reshape(M.shape[:-2] + (3, 3))
        hnorm2 = np.stack([sM[..., 0], z, -cM[..., 0] * sM[..., 0], z, sM[..., 1], -cM[..., 1] * sM[..., 1], z, z, o], -1).reshape(M.shape[:-2] + (3, 3))
    return LtL, inv_hnorm, hnorm2, ok


def _mul3(a, b):
    """[cv4.8] gemm's 3 x 3 special case: a[r][0] * b[0][c] + a[r][1] * b[1][c] + a[r][2] * b[2][c], left to right."""
    return np.stack([np.stack([a[..., r, 0] * b[..., 0, c] + a[..., r, 1] * b[..., 1, c] + a[..., r, 2] * b[..., 2, c] for c in range(3)], -1)
                     for r in range(3)], -2)


def _denormalise(h0, inv_hnorm, hnorm2):
    """[cv4.8] H = (invHnorm * H0) * Hnorm2, then convertTo with scale 1 / H[2][2] (x * scale + 0)."""
    with np.errstate(all="ignore"):
        u = _mul3(_mul3(inv_hnorm, h0), hnorm2)
        return u * (1.0 / u[..., 2, 2])[..., None, None] + 0.0


def run_kernel(M, m):
    """[cv4.8] runKernel on count >= 4 pairs M -> m (float32 [count, 2]) -> 3 x 3 float64, or None where OpenCV returns 0.  The
    eigenvector of the smallest eigenvalue of LtL is the last row Jacobi hands back."""
    LtL, inv_hnorm, hnorm2, ok = _dlt_system(M, m)
    if not ok:
        return None
    _w, V, _ = jacobi(LtL)
    return _denormalise(V[8].reshape(3, 3), inv_hnorm, hnorm2)


def run_kernel4_batch(M4, m4):
    """`run_kernel` on a stack of 4-point subsets [B, 4, 2] -> (H [B, 3, 3], valid [B]); H is zero where not valid."""
    LtL, inv_hnorm, hnorm2, ok = _dlt_system(M4, m4)
    H = np.zeros((len(LtL), 3, 3))
    if ok.any():
        _w, V, _ = jacobi_batch(LtL[ok])
        H[ok] = _denormalise(V[:, 8].reshape(-1, 3, 3), inv_hnorm[ok], hnorm2[ok])
    return H, ok


# ---- computeError / findInliers ---------------------------------------------------------------------------------------------------------------
def reproj_err(H, src, dst):
    """[cv4.8] computeError: the model cast to float32, everything float32, left to right, no contraction.  H [..., 3, 3] broadcasts
    against the points [n, 2] -> err [..., n]."""
    h = np.asarray(H, np.float64).astype(np.float32).reshape(np.shape(H)[:-2] + (9, 1))
    src, dst = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    x, y, mx, my = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    with np.errstate(all="ignore"):
        ww = np.float32(1) / (h[..., 6, :] * x + h[..., 7, :] * y + np.float32(1))
        dx = (h[..., 0, :] * x + h[..., 1, :] * y + h[..., 2, :]) * ww - mx
        dy = (h[..., 3, :] * x + h[..., 4, :] * y + h[..., 5, :]) * ww - my
        return dx * dx + dy * dy


def threshold_sq(threshold) -> np.float32:
    """[cv4.8] findInliers: float t = (float)(thresh * thresh); a pair is an inlier iff err <= t."""
    return np.float32(float(threshold) * float(threshold))


def find_inliers(H, src, dst, threshold):
    with np.errstate(invalid="ignore"):
        return reproj_err(H, src, dst) <= threshold_sq(threshold)


# ---- ptsetreg.cpp: RANSACPointSetRegistrator::run -------------------------------------------------------------------------------------------
class Iterations:
    """The per-iteration facts of the loop, which depend on the points alone: subset, 4-point model, its valid flag and inlier count.
    `upto(k)` evaluates iterations until k are known (or getSubset has failed: `failed_at`)."""

    def __init__(self, src, dst, threshold, chunk=512):
        self.src, self.dst, self.threshold, self.chunk = np.asarray(src, np.float32), np.asarray(dst, np.float32), threshold, chunk
        self.rng = RNG()
        self.idx, self.H, self.valid, self.count = np.zeros((0, 4), np.int64), np.zeros((0, 3, 3)), np.zeros(0, bool), np.zeros(0, np.int64)
        self.failed_at = None

    def upto(self, k):
        while len(self.idx) < k and self.failed_at is None:
            new = []
            while len(new) < min(self.chunk, k - len(self.idx)):
                s = get_subset(self.src, self.dst, self.rng)
                if s is None:
                    self.failed_at = len(self.idx) + len(new)
                    break
                new.append(s)
            if not new:
                break
            new = np.array(new, np.int64)
            H, valid = run_kernel4_batch(self.src[new], self.dst[new])
            count = np.zeros(len(new), np.int64)
            step = max(1, (1 << 22) // len(self.src))
            for a in range(0, len(new), step):
                count[a:a + step] = find_inliers(H[a:a + step], self.src, self.dst, self.threshold).sum(-1)
            count[~valid] = 0
            self.idx, self.H = np.concatenate([self.idx, new]), np.concatenate([self.H, H])
            self.valid, self.count = np.concatenate([self.valid, valid]), np.concatenate([self.count, count])
        return min(k, len(self.idx))


def ransac(src, dst, threshold, max_iters, confidence, its=None):
    """[cv4.8] the loop for count > 4 -> dict(found, H, mask, ran, best_iter, best_count, its).  An iteration whose runKernel gives no
    model scores nothing; a model is taken when goodCount > max(maxGoodCount, 3); niters is then updated from its outlier share."""
    src, dst = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    n = len(src)
    its = its if its is not None else Iterations(src, dst, threshold)
    niters = max(max_iters, 1)
    best, best_iter, it = 0, -1, 0
    while it < niters:
        have = its.upto(min(niters, it + its.chunk))
        if have <= it:          # getSubset failed at this iteration: the loop ends here (at iteration 0: no model)
            break
        while it < have and it < niters:
            if its.valid[it] and its.count[it] > max(best, MODEL_POINTS - 1):
                best, best_iter = int(its.count[it]), it
                niters = update_num_iters(confidence, (n - best) / n, MODEL_POINTS, niters)
            it += 1
    out = dict(found=best > 0, H=None, mask=np.zeros((n, 1), np.uint8), ran=it, best_iter=best_iter, best_count=best, its=its)
    if best > 0:
        out["H"] = its.H[best_iter].copy()
        out["mask"] = find_inliers(out["H"], src, dst, threshold).astype(np.uint8).reshape(n, 1)
    return out


# ---- levmarq.cpp: LMSolverImpl::run on HomographyRefineCallback ---------------------------------------------------------------------------
def _lm_eval(M, m, h, want_jac):
    """[cv4.8] HomographyRefineCallback::compute at the 8 parameters h -> (S = |r|^2, max |r|, J^T J, J^T r).  [def] the three sums
    run over the rows 2 i, 2 i + 1 in index order (OpenCV's norm / mulTransposed / gemm block theirs)."""
    Mx, My = M[:, 0].astype(np.float64), M[:, 1].astype(np.float64)
    ww = h[6] * Mx + h[7] * My + 1.0
    with np.errstate(all="ignore"):
        ww = np.where(np.abs(ww) > DBL_EPSILON, 1.0 / ww, 0.0)
    xi = (h[0] * Mx + h[1] * My + h[2]) * ww
    yi = (h[3] * Mx + h[4] * My + h[5]) * ww
    r = np.stack([xi - m[:, 0].astype(np.float64), yi - m[:, 1].astype(np.float64)], 1).reshape(-1)
    S, rinf = float(seq_sum(r * r)), float(np.abs(r).max()) if len(r) else 0.0
    if not want_jac:
        return S, rinf, None, None
    z = np.zeros_like(ww)
    J0 = [Mx * ww, My * ww, ww, z, z, z, -Mx * ww * xi, -My * ww * xi]
    J1 = [z, z, z, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi]
    A, v = np.zeros((8, 8)), np.zeros(8)
    for a in range(8):
        for b in range(a, 8):
            A[a, b] = A[b, a] = seq_sum(np.stack([J0[a] * J0[b], J1[a] * J1[b]], 1).reshape(-1))
        v[a] = seq_sum(np.stack([J0[a] * r[0::2], J1[a] * r[1::2]], 1).reshape(-1))
    return S, rinf, A, v


def _eig_solve8(Ap, b):
    """[cv4.8] cv::solve / cv::invert with DECOMP_EIG: Jacobi, then SVBkSb - eigenvalues at or below 2 DBL_EPSILON times their sum are
    skipped.  b given: the solution x; b None: the diagonal of the inverse."""
    W, V, _ = jacobi(Ap)
    threshold = 0.0
    for w in W:
        threshold += float(w)
    threshold *= DBL_EPSILON * 2
    x = [0.0] * 8
    for i in range(8):
        wi = float(W[i])
        if abs(wi) <= threshold:
            continue
        wi = 1 / wi
        if b is not None:
            s = 0.0
            for j in range(8):
                s += float(V[i, j]) * float(b[j])
            s *= wi
            for j in range(8):
                x[j] = x[j] + s * float(V[i, j])
        else:
            for j in range(8):
                x[j] = x[j] + float(V[i, j]) * (float(V[i, j]) * wi)
    return np.array(x)


def lm_refine(M, m, h):
    """[cv4.8] LMSolverImpl::run (maxIters 10, epsx = epsf = FLT_EPSILON) on the 8 free parameters -> (h, iterations)."""
    M, m = np.asarray(M, np.float32), np.asarray(m, np.float32)
    x = np.array(h, np.float64)
    S, rinf, A, v = _lm_eval(M, m, x, True)
    D = A.diagonal().copy()
    Rlo, Rhi = 0.25, 0.75
    lam, lc = 1.0, 0.75
    it = 0
    while True:
        Ap = A.copy()
        for j in range(8):
            Ap[j, j] += lam * D[j]
        d = _eig_solve8(Ap, v)
        xd = x - d
        Sd, rdinf, _, _ = _lm_eval(M, m, xd, False)
        dS = 0.0
        for i in range(8):
            s = 0.0
            for k in range(8):
                s += float(A[i, k]) * float(d[k])
            dS += float(d[i]) * (-s + 2 * float(v[i]))
        R = (S - Sd) / (dS if abs(dS) > DBL_EPSILON else 1)
        if R > Rhi:
            lam *= 0.5
            if lam < lc:
                lam = 0.0
        elif R < Rlo:
            t = 0.0
            for i in range(8):
                t += float(d[i]) * float(v[i])
            nu = (Sd - S) / (t if abs(t) > DBL_EPSILON else 1) + 2
            nu = min(max(nu, 2.0), 10.0)
            if lam == 0:
                diag = _eig_solve8(A, None)
                maxval = DBL_EPSILON
                for i in range(8):
                    maxval = max(maxval, abs(float(diag[i])))
                lam = lc = 1.0 / maxval
                nu *= 0.5
            lam *= nu
        if Sd < S:
            S, x = Sd, xd
            S, rinf, A, v = _lm_eval(M, m, x, True)
        it += 1
        dinf = float(np.abs(d).max())
        if not (it < LM_MAX_ITERS and dinf >= FLT_EPSILON and rinf >= FLT_EPSILON):
            break
    return x, it


# ---- fundam.cpp: findHomography -------------------------------------------------------------------------------------------------------------
def find_homography(src, dst, threshold=3.0, max_iters=10000, confidence=0.999, method="ransac", info=None):
    """[cv4.8] cv::findHomography(src, dst, RANSAC (or 0), threshold, mask, max_iters, confidence) -> (H float64 3 x 3 or None,
    mask uint8 [n, 1]).  `info`, a dict, receives ran / best_iter / best_count / lm_iters / its."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 2), np.asarray(dst, np.float32).reshape(-1, 2)
    n = len(src)
    info = info if info is not None else {}
    info.update(ran=0, best_iter=-1, best_count=0, lm_iters=0)
    if n < 4 or len(dst) != n:
        raise ValueError(f"findHomography needs at least 4 point pairs, got {n}")
    if threshold <= 0:
        threshold = 3.0
    if method == 0 or n == 4:
        H = run_kernel(src, dst)
        mask = np.ones((n, 1), np.uint8)
    else:
        r = ransac(src, dst, threshold, max_iters, confidence, info.get("its"))
        info.update({k: r[k] for k in ("ran", "best_iter", "best_count", "its")})
        H, mask = r["H"], r["mask"]
    if H is None:
        return None, np.zeros((n, 1), np.uint8)
    if n > 4:
        keep = mask[:, 0] != 0
        M, m = src[keep], dst[keep]
        if len(M) > 0:
            again = run_kernel(M, m) if method != 0 else None     # [cv4.8] its result is kept when it gives one
            if again is not None:
                H = again
            h8, info["lm_iters"] = lm_refine(M, m, H.reshape(-1)[:8])
            H = np.concatenate([h8, H.reshape(-1)[8:]]).reshape(3, 3)
    return H, mask
