"""TEST INFRASTRUCTURE - the definition of the tracker under a geometric prior (include/karios_hip.h:
km_pyrlk_initial, km_prior_mask, km_klt_tile_frame_prior_dev), in plain numpy.

1. The prior: 9 float64 values, row-major, reference pixel -> monitored pixel; every float64 operation rounded on its own (numpy never
   fuses), in the order of csrc/prior_math.hpp, of which `guess` and `mask` are the transcription.
2. The seeded tracker: `ko_pyrlk` (oracle/karios_oracle.c:511-637) with ONE change - on the top level the search starts at
   guess * scale where the oracle starts at the key point (cv2's rule for OPTFLOW_USE_INITIAL_FLOW).  The template bounds test on
   `prev` only, the per-iteration bounds `break`, the cut, the oscillation stop and the hand-down `* 2.f` are the oracle's.  It is
   PINNED to the oracle: with guess == pts it returns `oracle.pyr_lk` bit for bit (tests/test_lk_prior_host.py).
3. Forward / backward: p1 from the guess g; the backward pass from p1 - (g - p0), float32, in that order - it never reads p0.
4. The mask rule that keeps a guess outside the monitored box from scoring a perfect track of nothing.
"""
from __future__ import annotations

import numpy as np

from lk_restatement import FLT_EPSILON, FLT_SCALE, MIN_EIG, lk_weights

F32 = np.float32


# ------------------------------------------------------------------ 1. the prior
def shift_prior(sx, sy):
    return np.array([1.0, 0.0, float(sx), 0.0, 1.0, float(sy), 0.0, 0.0, 1.0])


def _map(P, x, y, x_off, y_off):
    """float64 arrays x, y (tile coordinates) -> (qx, qy, has_guess), tile coordinates."""
    P = np.asarray(P, np.float64).reshape(9)
    gx, gy = x + np.float64(x_off), y + np.float64(y_off)
    with np.errstate(all="ignore"):
        w = (P[6] * gx + P[7] * gy) + P[8]
        ok = (w > 0.0) & (w < np.inf)
        ws = np.where(ok, w, 1.0)
        qx = ((P[0] * gx + P[1] * gy) + P[2]) / ws
        qy = ((P[3] * gx + P[4] * gy) + P[5]) / ws
        qx = qx - np.float64(x_off)
        qy = qy - np.float64(y_off)
    return qx, qy, ok


def guess(P, pts, x_off=0.0, y_off=0.0):
    """(N, 2) float32 key points -> ((N, 2) float32 guesses, has_guess); a row without a guess keeps the key point."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    qx, qy, ok = _map(P, pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64), x_off, y_off)
    with np.errstate(all="ignore"):
        g = np.stack([qx.astype(np.float32), qy.astype(np.float32)], axis=1)
    return np.where(ok[:, None], g, pts).astype(np.float32), ok


def _valid(img, nodata):
    v = img != 0
    if img.dtype.kind == "f":
        v &= np.isfinite(img)
    if nodata is not None:
        v &= img.astype(np.float64) != np.float64(nodata)
    return v


def targets(P, H, W, x_off=0.0, y_off=0.0):
    """-> (rx, ry int64 H x W with 0 where there is no target, has_target): the monitored pixel each reference pixel is held against."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    qx, qy, ok = _map(P, xx, yy, x_off, y_off)
    with np.errstate(all="ignore"):
        fx, fy = np.rint(qx), np.rint(qy)                    # half to even
        ok = ok & (fx >= 0.0) & (fx < W) & (fy >= 0.0) & (fy < H)
    rx, ry = np.where(ok, fx, 0.0).astype(np.int64), np.where(ok, fy, 0.0).astype(np.int64)
    return rx, ry, ok


def mask(ref, mon, P, base=None, nodata_ref=None, nodata_mon=None, x_off=0.0, y_off=0.0, rule=True):
    """Rule 4 -> uint8 H x W.  `rule` False: `base` alone (the control of the test that shows what the rule prevents)."""
    ref, mon = np.asarray(ref), np.asarray(mon)
    H, W = ref.shape
    m = (np.asarray(base) != 0) if base is not None else _valid(ref, nodata_ref)
    if rule:
        rx, ry, ok = targets(P, H, W, x_off, y_off)
        m = m & ok & _valid(mon, nodata_mon)[ry, rx]
    return m.astype(np.uint8)


# ------------------------------------------------------------------ 2. the seeded tracker
def _reflect101(p, n):
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def pyrdown(img):
    """cv::pyrDown of a uint8 image (ko_pyrdown_u8): [1 4 6 4 1]^2, REFLECT_101, (s + 128) >> 8."""
    img = np.asarray(img, np.int64)
    H, W = img.shape
    k = (1, 4, 6, 4, 1)
    rows = sum(k[j] * img[_reflect101(2 * np.arange((H + 1) // 2) + j - 2, H)] for j in range(5))
    out = sum(k[i] * rows[:, _reflect101(2 * np.arange((W + 1) // 2) + i - 2, W)] for i in range(5))
    return ((out + 128) >> 8).astype(np.uint8)


def pyramid(img, win, max_level=1):
    levels = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(max_level):
        h, w = levels[-1].shape
        if (w + 1) // 2 <= win or (h + 1) // 2 <= win:
            break
        levels.append(pyrdown(levels[-1]))
    return levels


def _scharr_padded(img, pad):
    """Scharr derivatives (intensities REFLECT_101) of an image, zero outside it -> (Ix, Iy) int64 with `pad` zeros around."""
    p = np.pad(np.asarray(img, np.int64), 1, mode="reflect")
    a00, a01, a02 = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    a10, a12 = p[1:-1, :-2], p[1:-1, 2:]
    a20, a21, a22 = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    ix = ((a02 + a22) * 3 + a12 * 10) - ((a00 + a20) * 3 + a10 * 10)
    iy = ((a20 + a22) * 3 + a21 * 10) - ((a00 + a02) * 3 + a01 * 10)
    return np.pad(ix, pad), np.pad(iy, pad)


class _Level:
    def __init__(self, img, win):
        self.img = np.asarray(img, np.int64)
        self.H, self.W = self.img.shape
        self.win = win
        self._deriv = None

    def patch(self, y0, x0):
        """(win + 1)^2 intensities with top-left (x0, y0), REFLECT_101."""
        n = self.win + 1
        return self.img[np.ix_(_reflect101(y0 + np.arange(n), self.H), _reflect101(x0 + np.arange(n), self.W))]

    def deriv(self, y0, x0):
        if self._deriv is None:
            self.pad = self.win + 2
            self._deriv = _scharr_padded(self.img, self.pad)
        n, p = self.win + 1, self.pad
        s = np.s_[y0 + p:y0 + p + n, x0 + p:x0 + p + n]
        return self._deriv[0][s], self._deriv[1][s]


def _bilinear(p, w, shift):
    w00, w01, w10, w11 = w
    v = p[:-1, :-1] * w00 + p[:-1, 1:] * w01 + p[1:, :-1] * w10 + p[1:, 1:] * w11
    return (v + (1 << (shift - 1))) >> shift


def _oscillates(ddx, pdx, ddy, pdy):
    return float(np.abs(F32(ddx + pdx))) < 0.01 and float(np.abs(F32(ddy + pdy))) < 0.01


@np.errstate(all="ignore")
def track_point(I, J, pt, start, win, max_count=30, eps=0.03):
    """One point through the levels I (template) / J (search), lists of _Level, level 0 first -> (x, y) float32."""
    max_count = min(max(int(max_count), 0), 100)
    eps = min(max(float(eps), 0.0), 10.0)
    epsilon = eps * eps
    half = F32(win - 1) * F32(0.5)
    top = len(I) - 1
    resx, resy = F32(pt[0]), F32(pt[1])
    for level in range(top, -1, -1):
        sc = F32(1.0 / (1 << level))
        prx, pry = F32(pt[0]) * sc, F32(pt[1]) * sc
        if level == top:
            nx, ny = F32(start[0]) * sc, F32(start[1]) * sc          # the ONE change: the oracle has nx = prx, ny = pry
        else:
            nx, ny = resx * F32(2), resy * F32(2)
        resx, resy = nx, ny
        prx, pry = prx - half, pry - half
        ipx, ipy = int(np.floor(prx)), int(np.floor(pry))
        L, M = I[level], J[level]
        if ipx < -win or ipx >= L.W or ipy < -win or ipy >= L.H:
            continue
        w = lk_weights(prx - F32(ipx), pry - F32(ipy))
        tI = _bilinear(L.patch(ipy, ipx), w, 14 - 5)
        gx, gy = L.deriv(ipy, ipx)
        tIx, tIy = _bilinear(gx, w, 14), _bilinear(gy, w, 14)
        A11 = F32(int((tIx * tIx).sum())) * FLT_SCALE
        A12 = F32(int((tIx * tIy).sum())) * FLT_SCALE
        A22 = F32(int((tIy * tIy).sum())) * FLT_SCALE
        D = A11 * A22 - A12 * A12
        dA = A11 - A22
        q = dA * dA + F32(4) * A12 * A12
        min_eig = (A22 + A11 - np.sqrt(q)) / F32(2 * win * win)
        if min_eig < MIN_EIG or D < FLT_EPSILON:
            continue
        D = F32(1) / D
        nx, ny = nx - half, ny - half
        pdx = pdy = F32(0)
        for j in range(max_count):
            inx, iny = int(np.floor(nx)), int(np.floor(ny))
            if inx < -win or inx >= M.W or iny < -win or iny >= M.H:
                break
            w = lk_weights(nx - F32(inx), ny - F32(iny))
            diff = _bilinear(M.patch(iny, inx), w, 14 - 5) - tI
            b1 = F32(int((diff * tIx).sum())) * FLT_SCALE
            b2 = F32(int((diff * tIy).sum())) * FLT_SCALE
            ddx = (A12 * b2 - A22 * b1) * D
            ddy = (A12 * b1 - A11 * b2) * D
            nx, ny = nx + ddx, ny + ddy
            resx, resy = nx + half, ny + half
            if float(ddx) * float(ddx) + float(ddy) * float(ddy) <= epsilon:
                break
            if j > 0 and _oscillates(ddx, pdx, ddy, pdy):
                resx, resy = resx - ddx * F32(0.5), resy - ddy * F32(0.5)
                break
            pdx, pdy = ddx, ddy
        assert all(isinstance(v, np.float32) for v in (nx, ny, resx, resy, D))
    return resx, resy


def levels_of(img, win, max_level=1):
    return [_Level(a, win) for a in pyramid(img, win, max_level)]


def pyr_lk_initial(prev, nxt, pts, guesses, win=25, max_level=1, max_count=30, eps=0.03):
    """cv2.calcOpticalFlowPyrLK with OPTFLOW_USE_INITIAL_FLOW -> (N, 1, 2) float32.  `prev` / `nxt`: images, or `levels_of` of them."""
    I = prev if isinstance(prev, list) else levels_of(prev, win, max_level)
    J = nxt if isinstance(nxt, list) else levels_of(nxt, win, max_level)
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    guesses = np.asarray(guesses, np.float32).reshape(-1, 2)
    out = np.empty_like(pts)
    for k in range(len(pts)):
        out[k] = track_point(I, J, pts[k], guesses[k], win, max_count, eps)
    return out.reshape(-1, 1, 2)


# ------------------------------------------------------------------ 3. forward / backward
def backward_guess(p0, p1, g):
    p0, p1, g = (np.asarray(a, np.float32).reshape(-1, 2) for a in (p0, p1, g))
    out = p1 - (g - p0)
    assert out.dtype == np.float32
    return out


def track_fb(ref, mon, p0, g, win=25, max_level=1, max_count=30, eps=0.03):
    """-> (p1, p0r), each (N, 1, 2) float32."""
    A, B = levels_of(ref, win, max_level), levels_of(mon, win, max_level)
    p1 = pyr_lk_initial(A, B, p0, g, win, max_level, max_count, eps)
    p0r = pyr_lk_initial(B, A, p1, backward_guess(p0, p1, g), win, max_level, max_count, eps)
    return p1, p0r


def fb_columns(p0, p1, p0r):
    """klt.py:142-155 -> dict of float32 columns x0, y0, dx, dy, score of the kept rows (corner order), d of ALL rows."""
    p0, p1, p0r = (np.asarray(a, np.float32).reshape(-1, 1, 2) for a in (p0, p1, p0r))
    d = abs(p0 - p0r).reshape(-1, 2).max(-1)
    st = d < 0.1
    k0, k1 = p0[st], p1[st]
    return {"x0": k0[:, 0, 0], "y0": k0[:, 0, 1], "dx": k1[:, 0, 0] - k0[:, 0, 0], "dy": k1[:, 0, 1] - k0[:, 0, 1],
            "score": 1 - d[st] / 0.1}, d
