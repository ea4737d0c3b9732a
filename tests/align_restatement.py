"""numpy restatement of the arithmetic behind the global align step (karios/matcher/global_align.py): cv2.warpPerspective,
the Sobel gradient magnitude and cv2.findTransformECC(MOTION_HOMOGRAPHY), as libkarios_hip.so computes them (k_align.hip).

This is the DEFINITION the GPU kernels are held to (tests/test_gpu_align.py).  OpenCV is absent, so parity with cv2 itself is
unpinned (as for the Laplacian and LK).  Points marked [cv4.8] come from knowledge of OpenCV 4.8's sources
(imgwarp.cpp, ecc.cpp, lapack.cpp), not from the reference tree; points marked [def] are choices of this project where OpenCV's
result depends on the CPU's vector width or on a library (IPP) and is therefore not one fixed number.

Test infrastructure only: karios_amd never imports this module.
"""
from __future__ import annotations

import numpy as np

INTER_NEAREST, INTER_LINEAR, WARP_INVERSE_MAP = 0, 1, 16
INT_MIN, INT_MAX = -2147483648.0, 2147483647.0


class EccNoConvergence(RuntimeError):
    """cv2.error with StsNoConv: NaN rho, or lambda_d <= 0 ("the correlation is going to be minimized")."""


def _reflect101(p, n):
    p = np.asarray(p)
    if n == 1:
        return np.zeros_like(p)
    p = np.abs(p)
    period = 2 * n - 2
    p = p % period
    return np.where(p >= n, period - p, p)


def invert3x3(M):
    """cv::invert(DECOMP_LU) of a 3 x 3 double matrix: cofactors over det3, times 1/det; a singular matrix gives zeros [cv4.8]."""
    m = np.asarray(M, np.float64).reshape(3, 3)
    d = (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
         + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))
    if d == 0.0:
        return np.zeros((3, 3))
    d = 1.0 / d
    t = np.empty(9)
    t[0] = (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) * d
    t[1] = (m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]) * d
    t[2] = (m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]) * d
    t[3] = (m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]) * d
    t[4] = (m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]) * d
    t[5] = (m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]) * d
    t[6] = (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]) * d
    t[7] = (m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]) * d
    t[8] = (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]) * d
    return t.reshape(3, 3)


def _clamp_int(v):
    # std::max(INT_MIN, std::min(INT_MAX, v)) with std::min(a, b) = b < a ? b : a  (NaN -> INT_MAX) [cv4.8]
    v = np.where(v < INT_MAX, v, INT_MAX)
    return np.where(INT_MIN < v, v, INT_MIN)


def _sat_short(v):
    return np.clip(v, -32768, 32767)


def warp_taps(M, dH, dW, linear, rows=None):
    """Source positions of the destination pixels of rows `rows` (default all) for the INVERSE map M (fp64 3 x 3).
    Linear: (sx, sy, fx, fy), 1/32-px fractions; nearest: (sx, sy).  WarpPerspectiveInvoker [cv4.8]: blocks of bw0 columns,
    X0 / Y0 / W0 at the block's first column, then + M * x1 within the block."""
    m = np.asarray(M, np.float64).reshape(9)
    bh0 = min(16, dH)
    bw0 = min(1024 // bh0, dW)
    y = (np.arange(dH) if rows is None else np.asarray(rows)).astype(np.float64)[:, None]
    xs = np.arange(dW)
    xb = (xs - xs % bw0).astype(np.float64)[None, :]
    x1 = (xs % bw0).astype(np.float64)[None, :]
    X0 = m[0] * xb + m[1] * y + m[2]
    Y0 = m[3] * xb + m[4] * y + m[5]
    W0 = m[6] * xb + m[7] * y + m[8]
    W = W0 + m[6] * x1
    num = 32.0 if linear else 1.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        W = np.where(W != 0, num / np.where(W != 0, W, 1.0), 0.0)
        fX = _clamp_int((X0 + m[0] * x1) * W)
        fY = _clamp_int((Y0 + m[3] * x1) * W)
    X = np.rint(fX).astype(np.int64)   # saturate_cast<int>(double) = cvRound: half to even
    Y = np.rint(fY).astype(np.int64)
    if not linear:
        return _sat_short(X), _sat_short(Y)
    return _sat_short(X >> 5), _sat_short(Y >> 5), X & 31, Y & 31


def _tap(src, sx, sy, cval):
    H, W = src.shape
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    v = src[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)]
    return np.where(inside, v, cval)


def u8_border(border_value):
    """saturate_cast<uchar>(double): round half to even, saturate, NaN -> 0."""
    b = float(border_value)
    if b != b:
        return 0
    return int(min(255, max(0, np.rint(b))))


def warp_perspective(src, M, dsize, flags=INTER_LINEAR, border_value=0.0, rows=None):
    """cv2.warpPerspective(src, M, dsize, flags, BORDER_CONSTANT, borderValue) for uint8 / float32 single-channel images.
    `rows`: compute only these destination rows (the render checks at full size)."""
    src = np.asarray(src)
    dW, dH = int(dsize[0]), int(dsize[1])
    M = np.asarray(M, np.float64).reshape(3, 3)   # Mat::convertTo(CV_64F): float32 matrices widen exactly
    if not (flags & WARP_INVERSE_MAP):
        M = invert3x3(M)
    linear = (flags & 15) == INTER_LINEAR
    if src.dtype == np.uint8:
        cval = u8_border(border_value)
    elif src.dtype == np.float32:
        cval = np.float32(border_value)
    else:
        raise TypeError(src.dtype)
    if not linear:
        sx, sy = warp_taps(M, dH, dW, False, rows)
        return _tap(src, sx, sy, cval).astype(src.dtype)
    sx, sy, fx, fy = warp_taps(M, dH, dW, True, rows)
    H, W = src.shape
    allout = (sx >= W) | (sx + 1 < 0) | (sy >= H) | (sy + 1 < 0)
    v0, v1 = _tap(src, sx, sy, cval), _tap(src, sx + 1, sy, cval)
    v2, v3 = _tap(src, sx, sy + 1, cval), _tap(src, sx + 1, sy + 1, cval)
    if src.dtype == np.uint8:
        # BilinearTab_i: (32 - fy)(32 - fx) * 32 ...; OpenCV saturates the (0, 0) entry to 32767 and gives the lost unit to
        # another tap, which leaves (sum + 2^14) >> 15 unchanged for 8-bit values [cv4.8]
        wx1, wy1 = fx, fy
        wx0, wy0 = 32 - fx, 32 - fy
        s = (v0.astype(np.int64) * (wy0 * wx0 * 32) + v1.astype(np.int64) * (wy0 * wx1 * 32)
             + v2.astype(np.int64) * (wy1 * wx0 * 32) + v3.astype(np.int64) * (wy1 * wx1 * 32))
        out = np.clip((s + (1 << 14)) >> 15, 0, 255)
        return np.where(allout, cval, out).astype(np.uint8)
    f32 = np.float32
    tx = fx.astype(f32) * f32(1.0 / 32)
    ty = fy.astype(f32) * f32(1.0 / 32)
    ax, ay = f32(1) - tx, f32(1) - ty
    with np.errstate(invalid="ignore", over="ignore"):
        s = v0 * (ay * ax)
        s = s + v1 * (ay * tx)
        s = s + v2 * (ty * ax)
        s = s + v3 * (ty * tx)
    return np.where(allout, cval, s).astype(np.float32)


def sobel_magnitude(img):
    """_sobel_magnitude (global_align.py): cv2.Sobel 3 x 3 (REFLECT_101, exact integers), cv2.magnitude (gx^2 + gy^2 exact in
    float32, correctly rounded sqrt), divided by the maximum in float32."""
    a = np.asarray(img, np.uint8).astype(np.int32)
    H, W = a.shape
    ry = _reflect101(np.arange(-1, H + 1), H)
    rx = _reflect101(np.arange(-1, W + 1), W)
    p = a[ry][:, rx]
    gx = (p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
    gy = (p[2:, :-2] - p[:-2, :-2]) + 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])
    mag = np.sqrt((gx * gx + gy * gy).astype(np.float32))
    m = float(mag.max())
    return mag / np.float32(m) if m > 0 else mag


# ---- findTransformECC (ecc.cpp) ----------------------------------------------------------------------------------------
G0, G1, G2 = np.float32(0.375), np.float32(0.25), np.float32(0.0625)


def gauss5(a):
    """GaussianBlur(5 x 5, sigma 0) on float32: separable {1, 4, 6, 4, 1} / 16, REFLECT_101, rows first; every pass
    k0 * c + k1 * (l1 + r1) + k2 * (l2 + r2) in float32, no fused multiply-add [def: OpenCV's symmetric small filter form]."""
    a = np.asarray(a, np.float32)
    H, W = a.shape
    rx = _reflect101(np.arange(-2, W + 2), W)
    p = a[:, rx]
    t = G0 * p[:, 2:-2]
    t = t + G1 * (p[:, 1:-3] + p[:, 3:-1])
    t = t + G2 * (p[:, :-4] + p[:, 4:])
    ry = _reflect101(np.arange(-2, H + 2), H)
    p = t[ry]
    o = G0 * p[2:-2]
    o = o + G1 * (p[1:-3] + p[3:-1])
    o = o + G2 * (p[:-4] + p[4:])
    return o.astype(np.float32)


def ecc_premask(mask, shape):
    """threshold(inputMask, 0, 1) (ones without a mask), blur as float32, * (float)(0.5 / 0.95), round half to even to
    uint8 [cv4.8]."""
    pm = np.ones(shape, np.float32) if mask is None else (np.asarray(mask) > 0).astype(np.float32)
    b = gauss5(pm) * np.float32(0.5 / 0.95)
    return np.rint(b).astype(np.uint8)


def ecc_gradients(blurred, premask):
    """filter2D with [-0.5, 0, 0.5] (REFLECT_101) along x / y: s = 0 + (-0.5) l, s += 0.5 r; times the pre-mask [cv4.8]."""
    a = np.asarray(blurred, np.float32)
    H, W = a.shape
    rx = _reflect101(np.arange(-1, W + 1), W)
    ry = _reflect101(np.arange(-1, H + 1), H)
    h, q = np.float32(-0.5), np.float32(0.5)
    gx = (np.float32(0) + h * a[:, rx[:-2]]) + q * a[:, rx[2:]]
    gy = (np.float32(0) + h * a[ry[:-2]]) + q * a[ry[2:]]
    pmf = premask.astype(np.float32)
    return (gx * pmf).astype(np.float32), (gy * pmf).astype(np.float32)


def ecc_prepare(template, image, input_mask=None):
    """-> (blurred template, blurred image, gx, gy, premask) of findTransformECC's set-up."""
    t = gauss5(np.asarray(template, np.float32))
    i = gauss5(np.asarray(image, np.float32))
    pm = ecc_premask(input_mask, i.shape)
    gx, gy = ecc_gradients(i, pm)
    return t, i, gx, gy, pm


def ecc_jacobian(gxw, gyw, hs, ws, mp):
    """image_jacobian_homo_ECC in float32, step by step [cv4.8 structure; def: no fused multiply-add]."""
    f = np.float32
    X = np.broadcast_to(np.arange(ws, dtype=f)[None, :], (hs, ws))
    Y = np.broadcast_to(np.arange(hs, dtype=f)[:, None], (hs, ws))
    h = mp.reshape(9).astype(f)
    h0, h1, h2, h3, h4, h5, h6, h7 = h[0], h[3], h[6], h[1], h[4], h[7], h[2], h[5]
    den = (X * h2 + Y * h5) + f(1)
    hatX = ((-(X * h0)) - Y * h3 - h6) / den
    hatY = ((-(X * h1)) - Y * h4 - h7) / den
    g1 = gxw / den
    g2 = gyw / den
    temp = hatX * g1 + hatY * g2
    return [g1 * X, g2 * X, temp * X, g1 * Y, g2 * Y, temp * Y, g1, g2]


def ecc_terms(t, img, gx, gy, pm, mp):
    """The per-pixel terms (66 fp64 hs x ws arrays) of the sums of one iteration: m, mI, mI^2, mT, mT^2, mTI, the 36 Hessian
    terms J_k J_l (upper triangle, row by row), J_k I, J_k m, J_k m T.  Every product is exact in fp64: m is 0 or 1, the rest
    are products of two float32 values."""
    hs, ws = t.shape
    M = np.asarray(mp, np.float32).astype(np.float64)
    dsz = (ws, hs)
    Iw = warp_perspective(img, M, dsz, INTER_LINEAR | WARP_INVERSE_MAP, 0.0).astype(np.float64)
    gxw = warp_perspective(gx, M, dsz, INTER_LINEAR | WARP_INVERSE_MAP, 0.0)
    gyw = warp_perspective(gy, M, dsz, INTER_LINEAR | WARP_INVERSE_MAP, 0.0)
    m = warp_perspective(pm, M, dsz, INTER_NEAREST | WARP_INVERSE_MAP, 0.0).astype(np.float64)
    J = [j.astype(np.float64) for j in ecc_jacobian(gxw, gyw, hs, ws, np.asarray(mp, np.float32))]
    T = t.astype(np.float64)
    s = [m, m * Iw, m * Iw * Iw, m * T, m * T * T, m * T * Iw]
    for k in range(8):
        for l in range(k, 8):
            s.append(J[k] * J[l])
    s += [J[k] * Iw for k in range(8)]
    s += [J[k] * m for k in range(8)]
    s += [J[k] * m * T for k in range(8)]
    return s


def ecc_sums(t, img, gx, gy, pm, mp):
    """The 66 fp64 sums of one iteration (numpy's summation order), in ecc_terms' order."""
    return np.array([term.sum() for term in ecc_terms(t, img, gx, gy, pm, mp)], np.float64)


def lu_inv_f32(A):
    """Mat::inv() of a float32 matrix: hal::LU32f (Gaussian elimination, partial pivoting, eps = 10 FLT_EPSILON) on [A | I];
    a singular matrix gives zeros [cv4.8]."""
    f = np.float32
    a = np.array(A, f)
    n = a.shape[0]
    b = np.eye(n, dtype=f)
    eps = f(np.finfo(np.float32).eps * 10)
    for i in range(n):
        k = i
        for j in range(i + 1, n):
            if abs(a[j, i]) > abs(a[k, i]):
                k = j
        if abs(a[k, i]) < eps:
            return np.zeros((n, n), f)
        if k != i:
            a[[i, k], i:] = a[[k, i], i:]
            b[[i, k]] = b[[k, i]]
        d = f(-1) / a[i, i]
        for j in range(i + 1, n):
            alpha = f(a[j, i] * d)
            for c in range(i + 1, n):
                a[j, c] = f(a[j, c] + f(alpha * a[i, c]))
            for c in range(n):
                b[j, c] = f(b[j, c] + f(alpha * b[i, c]))
    for i in range(n - 1, -1, -1):
        for j in range(n):
            s = b[i, j]
            for c in range(i + 1, n):
                s = f(s - f(a[i, c] * b[c, j]))
            b[i, j] = f(s / a[i, i])
    return b


def _matvec_f32(A, v):
    """float32 gemm of a small matrix and a vector: products and sum in double, stored as float32 [cv4.8 GEMMSingleMul]."""
    out = np.empty(A.shape[0], np.float32)
    for i in range(A.shape[0]):
        acc = 0.0
        for j in range(A.shape[1]):
            acc += float(A[i, j]) * float(v[j])
        out[i] = np.float32(acc)
    return out


def ecc_step(s, mp):
    """The host algebra of one iteration from the 66 sums: -> (rho, updated float32 map).  Raises EccNoConvergence."""
    N, SmI, SmI2, SmT, SmT2, SmTI = (float(x) for x in s[:6])
    H = np.empty((8, 8))
    idx = 6
    for k in range(8):
        for l in range(k, 8):
            H[k, l] = H[l, k] = s[idx]
            idx += 1
    SJI, SJm, SJmT = s[idx:idx + 8], s[idx + 8:idx + 16], s[idx + 16:idx + 24]
    inv_n = 1.0 / N if N else 0.0   # meanStdDev: scale = nz ? 1 / nz : 0
    mi, mt = SmI * inv_n, SmT * inv_n
    si = np.sqrt(max(SmI2 * inv_n - mi * mi, 0.0))
    st = np.sqrt(max(SmT2 * inv_n - mt * mt, 0.0))
    tmp_norm = np.sqrt(N * st * st)
    img_norm = np.sqrt(N * si * si)
    corr = SmTI - mi * SmT - mt * SmI + N * mt * mi
    hinv = lu_inv_f32(H.astype(np.float32))
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = corr / (img_norm * tmp_norm)
    if rho != rho:
        raise EccNoConvergence("NaN encountered.")
    IP = SJI - mi * SJm          # image projection (the raw value outside the mask, ecc.cpp's in-place subtract)
    TP = SJmT - mt * SJm         # template projection
    ip32, tp32 = IP.astype(np.float32), TP.astype(np.float32)
    iph = _matvec_f32(hinv, ip32)
    dot = lambda a, b: sum(float(x) * float(y) for x, y in zip(a, b))   # noqa: E731
    lam_n = img_norm * img_norm - dot(ip32, iph)
    lam_d = corr - dot(tp32, iph)
    if lam_d <= 0.0:
        raise EccNoConvergence("The algorithm stopped before its convergence. The correlation is going to be minimized.")
    lam = lam_n / lam_d
    ep = (lam * TP - IP).astype(np.float32)   # projection of error = lambda templateZM - imageWarped (linear)
    dp = _matvec_f32(hinv, ep)
    m = np.asarray(mp, np.float32).reshape(9).copy()
    for slot, k in zip((0, 3, 6, 1, 4, 7, 2, 5), range(8)):   # update_warping_matrix_ECC, MOTION_HOMOGRAPHY
        m[slot] = np.float32(m[slot] + dp[k])
    return float(rho), m.reshape(3, 3)


def find_transform_ecc(template, image, warp, criteria, input_mask=None, gauss_filt_size=5, return_iters=False):
    """cv2.findTransformECC(template, image, warp, MOTION_HOMOGRAPHY, criteria, inputMask, gaussFiltSize) -> (cc, warp)."""
    if gauss_filt_size != 5:
        raise NotImplementedError("gaussFiltSize 5 only")
    ctype, max_iter, eps = criteria
    n_it = int(max_iter) if ctype & 1 else 200        # TERM_CRITERIA_COUNT = 1, TERM_CRITERIA_EPS = 2
    eps = float(eps) if ctype & 2 else -1.0
    t, i, gx, gy, pm = ecc_prepare(template, image, input_mask)
    mp = np.asarray(warp, np.float32).reshape(3, 3).copy()
    rho, last = -1.0, -eps
    it = 0
    while it + 1 <= n_it and abs(rho - last) >= eps:
        it += 1
        s = ecc_sums(t, i, gx, gy, pm, mp)
        last = rho
        rho, mp = ecc_step(s, mp)
    return (rho, mp, it) if return_iters else (rho, mp)


# ---- _refine_with_ecc, per candidate (km_refine_ecc_candidates) --------------------------------------------------------
ST_CONVERGED, ST_SKIPPED, ST_NO_CONVERGENCE = 0, 1, 2


def refine_ecc_candidates(mon_u8, ref_u8, inits, max_iters=200, eps=1e-6, min_valid=1000):
    """-> list of (final fp64 3 x 3 or None, cc or nan, iterations, valid pixels, status, float32 residual or None) per initial
    matrix (karios_amd.ops.refine_ecc_candidates)."""
    rh, rw = ref_u8.shape
    template = None
    out = []
    for init in inits:
        init = np.asarray(init)
        warped = warp_perspective(mon_u8, init.astype(np.float32), (rw, rh), INTER_LINEAR, 0)
        valid = (warped > 0).astype(np.uint8)
        nv = int(valid.sum())
        if nv < min_valid:
            out.append((None, float("nan"), 0, nv, ST_SKIPPED, None))
            continue
        if template is None:
            template = sobel_magnitude(ref_u8)
        try:
            cc, res, it = find_transform_ecc(template, sobel_magnitude(warped), np.eye(3, dtype=np.float32), (3, max_iters, eps),
                                             valid * 255, 5, return_iters=True)
        except EccNoConvergence:
            out.append((None, float("nan"), 0, nv, ST_NO_CONVERGENCE, None))
            continue
        out.append((res.astype(np.float64) @ init.astype(np.float64), float(cc), it, nv, ST_CONVERGED, res))
    return out
