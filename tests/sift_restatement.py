"""numpy restatement of cv2.SIFT_create(nfeatures=0, contrastThreshold=, edgeThreshold=).detectAndCompute(img_u8, None) (OpenCV 4.8,
the float pyramid): the definition csrc/sift_math.hpp, k_sift.hip and api_sift.hip are held to, bit for bit.

Written from knowledge of OpenCV's algorithm, not from its text; parity with a cv2 binary is not pinned.  Every
point is marked [cv] (OpenCV knowledge) or [project] (a choice of this project that makes both sides reproducible).

[project] Transcendentals are explicit arithmetic, never libm / numpy / device intrinsics:
  exp64      float64: n = trunc(x log2e +- 0.5), r = (x - n ln2_hi) - n ln2_lo, Taylor polynomial of degree 13 by Horner, times 2^n
             built from its bits.  Every float32 weight is float32(exp64(float64(argument))).
  sincos_deg float64: quadrant q = trunc(a / 90 + 0.5), r = a - 90 q, x = r pi/180, Taylor polynomials (sin to x^15, cos to x^16)
             by Horner in x^2, quadrant swap; cast to float32.
  atan2_deg  float32: OpenCV's fastAtan2 polynomial [cv], step by step.
  sqrt, division: correctly rounded on both sides.  Rounding to an integer is round-half-even (cvRound) [cv].
[project] Every floating sum has one order:
  blur taps        centre first, then outwards: s = k0 x0; s += kj (x[-j] + x[+j]) for j = 1 .. radius; rows, then columns, the
                   row pass stored as float32.
  Gaussian kernel  taps exp64(-0.5/sigma^2 * (x*x)) in float64, summed in index order, tap = float32(t * (1 / sum)).
  orientation and descriptor histograms: one sample at a time, rows top to bottom, columns left to right within a row (the scalar
                   loop's order); the eight trilinear shares of a sample in the order 000, 001, 010, 011, 100, 101, 110, 111 of
                   (row, column, orientation).  Norms: index order.
[project] pow: k^j of the pyramid is exp64(j ln2 / nOctaveLayers), 2^((layer + xi) / n) of the size is float32(exp64(float64(e) ln2)).
[project] nOctaves = round(log2(m) - 2) + 1 is evaluated on integers: round(log2 m - 2) = (floor(log2(m^2)) - 3) >> 1 (a tie would
          need m = 2^(k + 2.5), never an integer).
Two points where a common description of the algorithm says otherwise, on purpose:
  [cv] the 3 x 3 system of the refinement is solved by Cramer's rule (Matx<float, 3, 3>::solve takes its closed form for 3 x 3 with
       DECOMP_LU; a zero determinant gives the zero vector), not by pivoted LU.
  [cv] the order of key points is x, y ascending, size DESCENDING, angle ascending, response DESCENDING, octave DESCENDING
       (KeyPoint_LessThan), and removeDuplicatedSorted drops a key point that equals its predecessor in (x, y, size, angle) alone.
       Key points equal in all six fields are the same record, so their mutual order cannot show; one survives.
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
N_LAYERS, SIGMA, INIT_SIGMA, BORDER, MAX_STEPS = 3, 1.6, 0.5, 5, 5
ORI_BINS, ORI_SIG_FCTR, ORI_RADIUS, ORI_PEAK_RATIO = 36, f32(1.5), f32(4.5), f32(0.8)
D_WIDTH, D_BINS, D_SCL_FCTR, D_MAG_THR, D_INT_FCTR = 4, 8, f32(3.0), f32(0.2), f32(512.0)
FLT_EPSILON = f32(1.1920929e-07)
MAX_OCTAVES = 16
KP_DTYPE = np.dtype([("x", f32), ("y", f32), ("size", f32), ("angle", f32), ("response", f32), ("octave", np.int32)])

LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
DEG2RAD = float.fromhex("0x1.1df46a2529d39p-6")
EXP_C = [1.0 / math.factorial(k) for k in range(14)]
SIN_C = [(-1.0) ** k / math.factorial(2 * k + 1) for k in range(8)]
COS_C = [(-1.0) ** k / math.factorial(2 * k) for k in range(9)]


# ---- transcendentals [project] ----------------------------------------------------------------------------------------------------
def exp64(x):
    """exp of float64 arguments in [-700, 700]; below -700 the result is 0."""
    x = np.asarray(x, f64)
    tiny = x < -700.0
    xc = np.where(tiny, 0.0, x)
    t = xc * LOG2E
    n = np.where(t >= 0, t + 0.5, t - 0.5).astype(np.int64)     # truncation
    nf = n.astype(f64)
    r = (xc - nf * LN2_HI) - nf * LN2_LO
    p = np.full(x.shape, EXP_C[13])
    for k in range(12, -1, -1):
        p = p * r + EXP_C[k]
    scale = ((n + 1023) << 52).view(f64)
    return np.where(tiny, 0.0, p * scale)


def exp32(x):
    return exp64(np.asarray(x, f32).astype(f64)).astype(f32)


def sincos_deg(a):
    """(cos, sin) as float32 of a float32 angle in degrees, 0 <= a <= 360."""
    a = np.asarray(a, f32).astype(f64)
    q = (a / 90.0 + 0.5).astype(np.int64)
    x = (a - 90.0 * q.astype(f64)) * DEG2RAD
    x2 = x * x
    s = np.full(x.shape, SIN_C[7])
    for k in range(6, -1, -1):
        s = s * x2 + SIN_C[k]
    s = s * x
    c = np.full(x.shape, COS_C[8])
    for k in range(7, -1, -1):
        c = c * x2 + COS_C[k]
    q = q & 3
    cos = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
    sin = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
    return cos.astype(f32), sin.astype(f32)


_R2D = f32(57.29577951308232)
AT_P1, AT_P3 = f32(0.9997878412794807) * _R2D, f32(-0.3258083974640975) * _R2D
AT_P5, AT_P7 = f32(0.1555786518463281) * _R2D, f32(-0.04432655554792128) * _R2D
AT_EPS = f32(2.220446049250313e-16)


def atan2_deg(y, x):
    """[cv] fastAtan2: degrees in [0, 360], float32."""
    y, x = np.asarray(y, f32), np.asarray(x, f32)
    ax, ay = np.abs(x), np.abs(y)
    big = ax >= ay
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(big, ay / (ax + AT_EPS), ax / (ay + AT_EPS)).astype(f32)
    c2 = c * c
    a = (((AT_P7 * c2 + AT_P5) * c2 + AT_P3) * c2 + AT_P1) * c
    a = np.where(big, a, f32(90) - a)
    a = np.where(x < 0, f32(180) - a, a)
    a = np.where(y < 0, f32(360) - a, a)
    return a.astype(f32)


def cv_round(x):
    return np.rint(x).astype(np.int64)


# ---- the dense part ------------------------------------------------------------------------------------------------------------------
def gaussian_kernel(sigma):
    """[cv] size round(8 sigma + 1) | 1, float64 taps normalised to sum 1, stored as float32; [project] the order of the sum."""
    sigma = float(sigma)
    n = int(np.rint(sigma * 8 + 1)) | 1
    scale2 = -0.5 / (sigma * sigma)
    x = np.arange(n, dtype=f64) - (n - 1) * 0.5
    t = exp64(scale2 * (x * x))
    s = 0.0
    for v in t:
        s += float(v)
    return (t * (1.0 / s)).astype(f32)


def _filter_axis(img, k, axis):
    r = len(k) // 2
    n = img.shape[axis]
    idx = np.arange(-r, n + r)
    if n == 1:
        idx[:] = 0
    else:                                                          # [cv] BORDER_REFLECT_101, reflected until it lands inside
        period = 2 * (n - 1)
        idx = np.abs(idx) % period
        idx = np.where(idx >= n, period - idx, idx)
    p = np.take(img, idx, axis=axis)
    sl = lambda o: np.take(p, np.arange(r + o, r + o + n), axis=axis)   # noqa: E731
    s = k[r] * sl(0)
    for j in range(1, r + 1):
        s = s + k[r + j] * (sl(-j) + sl(j))
    return s.astype(f32)


def gaussian_blur(img, sigma):
    k = gaussian_kernel(sigma)
    return _filter_axis(_filter_axis(img, k, 1), k, 0)


def base_image(img_u8, sigma):
    """[cv] float32, doubled by the linear warp with a replicated last sample, blurred up to `sigma`."""
    g = img_u8.astype(f32)
    h, w = g.shape
    gx = np.concatenate([g, g[:, -1:]], 1)
    d = np.empty((h, 2 * w), f32)
    d[:, 0::2] = g
    d[:, 1::2] = (gx[:, :-1] + gx[:, 1:]) * f32(0.5)
    dy = np.concatenate([d, d[-1:]], 0)
    out = np.empty((2 * h, 2 * w), f32)
    out[0::2] = d
    out[1::2] = (dy[:-1] + dy[1:]) * f32(0.5)
    sig_diff = np.sqrt(np.maximum(f32(sigma) * f32(sigma) - f32(INIT_SIGMA) * f32(INIT_SIGMA) * f32(4), f32(0.01)))
    return gaussian_blur(out, f32(sig_diff))


def n_octaves(h2, w2):
    m = min(h2, w2)
    return max(min((((m * m).bit_length() - 1 - 3) >> 1) + 1, MAX_OCTAVES), 0)


def level_sigmas(sigma, n_layers):
    sig = [float(sigma)]
    for i in range(1, n_layers + 3):
        prev = float(exp64((i - 1) * LN2 / n_layers)) * sigma
        total = float(exp64(i * LN2 / n_layers)) * sigma
        sig.append(math.sqrt(total * total - prev * prev))
    return sig


def build_pyramids(base, n_oct, sigma, n_layers):
    sig = level_sigmas(sigma, n_layers)
    gauss, dog = [], []
    for o in range(n_oct):
        g = [base if o == 0 else np.ascontiguousarray(gauss[o - 1][n_layers][0:2 * (gauss[o - 1][0].shape[0] // 2):2,
                                                                               0:2 * (gauss[o - 1][0].shape[1] // 2):2])]
        for i in range(1, n_layers + 3):
            g.append(gaussian_blur(g[i - 1], sig[i]))
        gauss.append(g)
        dog.append([g[i + 1] - g[i] for i in range(n_layers + 2)])
    return gauss, dog


def scan_extrema(dog_o, n_layers, threshold):
    """[cv] (layer, r, c) of every sample with |v| > threshold that is >= (v > 0) or <= (v < 0) all 26 neighbours."""
    out = []
    h, w = dog_o[0].shape
    if h <= 2 * BORDER or w <= 2 * BORDER:
        return np.zeros((0, 3), np.int64)
    for layer in range(1, n_layers + 1):
        v = dog_o[layer][BORDER:h - BORDER, BORDER:w - BORDER]
        ge = np.ones(v.shape, bool)
        le = np.ones(v.shape, bool)
        for pl in (dog_o[layer - 1], dog_o[layer], dog_o[layer + 1]):
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    nb = pl[BORDER + dr:h - BORDER + dr, BORDER + dc:w - BORDER + dc]
                    ge &= v >= nb
                    le &= v <= nb
        hit = (np.abs(v) > f32(threshold)) & (((v > 0) & ge) | ((v < 0) & le))
        r, c = np.nonzero(hit)
        out.append(np.stack([np.full(r.shape, layer), r + BORDER, c + BORDER], 1))
    return np.concatenate(out).astype(np.int64)


# ---- per candidate: the refinement [cv], vectorised over the candidates ----------------------------------------------------------------
IMG_SCALE = f32(1.0) / f32(255)
DERIV_SCALE, SECOND_SCALE, CROSS_SCALE = IMG_SCALE * f32(0.5), IMG_SCALE, IMG_SCALE * f32(0.25)


def _derivs(D, layer, r, c):
    """D: [n_layers + 2, h, w] float32 -> gradient and Hessian entries at the samples, float32, left to right."""
    img = lambda dl, dr, dc: D[layer + dl, r + dr, c + dc]   # noqa: E731
    dx = (img(0, 0, 1) - img(0, 0, -1)) * DERIV_SCALE
    dy = (img(0, 1, 0) - img(0, -1, 0)) * DERIV_SCALE
    ds = (img(1, 0, 0) - img(-1, 0, 0)) * DERIV_SCALE
    v2 = img(0, 0, 0) * f32(2)
    dxx = (img(0, 0, 1) + img(0, 0, -1) - v2) * SECOND_SCALE
    dyy = (img(0, 1, 0) + img(0, -1, 0) - v2) * SECOND_SCALE
    dss = (img(1, 0, 0) + img(-1, 0, 0) - v2) * SECOND_SCALE
    dxy = (img(0, 1, 1) - img(0, 1, -1) - img(0, -1, 1) + img(0, -1, -1)) * CROSS_SCALE
    dxs = (img(1, 0, 1) - img(1, 0, -1) - img(-1, 0, 1) + img(-1, 0, -1)) * CROSS_SCALE
    dys = (img(1, 1, 0) - img(1, -1, 0) - img(-1, 1, 0) + img(-1, -1, 0)) * CROSS_SCALE
    return dx, dy, ds, dxx, dyy, dss, dxy, dxs, dys


def _solve3(a00, a01, a02, a11, a12, a22, b0, b1, b2):
    """[cv] Cramer's rule of the symmetric 3 x 3 system in float32, the products in the closed form's order; det == 0 -> 0."""
    a10, a20, a21 = a01, a02, a12
    det = a00 * (a11 * a22 - a21 * a12) - a01 * (a10 * a22 - a20 * a12) + a02 * (a10 * a21 - a20 * a11)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = f32(1) / det
        x0 = d * (b0 * (a11 * a22 - a12 * a21) - a01 * (b1 * a22 - a12 * b2) + a02 * (b1 * a21 - a11 * b2))
        x1 = d * (a00 * (b1 * a22 - a12 * b2) - b0 * (a10 * a22 - a12 * a20) + a02 * (a10 * b2 - b1 * a20))
        x2 = d * (a00 * (a11 * b2 - b1 * a21) - a01 * (a10 * b2 - b1 * a20) + b0 * (a10 * a21 - a11 * a20))
    z = det == 0
    return np.where(z, f32(0), x0).astype(f32), np.where(z, f32(0), x1).astype(f32), np.where(z, f32(0), x2).astype(f32)


def refine(dog_o, cand, octv, n_layers, contrast_threshold, edge_threshold, sigma):
    """-> (ok [n] bool, fields): fields of the accepted candidates (KP_DTYPE without angle) + their final integer (layer, r, c)."""
    D = np.stack(dog_o)
    h, w = D.shape[1:]
    n = len(cand)
    layer, r, c = cand[:, 0].copy(), cand[:, 1].copy(), cand[:, 2].copy()
    alive = np.ones(n, bool)       # not rejected
    done = np.zeros(n, bool)       # converged
    xc, xr, xi = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(MAX_STEPS):
            act = np.nonzero(alive & ~done)[0]
            if not len(act):
                break
            dx, dy, ds, dxx, dyy, dss, dxy, dxs, dys = _derivs(D, layer[act], r[act], c[act])
            X0, X1, X2 = _solve3(dxx, dxy, dxs, dyy, dys, dss, dx, dy, ds)
            xc[act], xr[act], xi[act] = -X0, -X1, -X2
            a_c, a_r, a_i = np.abs(xc[act]), np.abs(xr[act]), np.abs(xi[act])
            conv = (a_i < f32(0.5)) & (a_r < f32(0.5)) & (a_c < f32(0.5))
            done[act[conv]] = True
            big = f32(2147483647 // 3)
            huge = ~conv & ~((a_i <= big) & (a_r <= big) & (a_c <= big))       # a NaN offset counts as huge [project]
            alive[act[huge]] = False
            mv = act[~conv & ~huge]
            c[mv] += cv_round(xc[mv])
            r[mv] += cv_round(xr[mv])
            layer[mv] += cv_round(xi[mv])
            out = (layer[mv] < 1) | (layer[mv] > n_layers) | (c[mv] < BORDER) | (c[mv] >= w - BORDER) | (r[mv] < BORDER) | (r[mv] >= h - BORDER)
            alive[mv[out]] = False
            layer[mv[out]], r[mv[out]], c[mv[out]] = 1, BORDER, BORDER
        ok = alive & done
        k = np.nonzero(ok)[0]
        dx, dy, ds, dxx, dyy, dss, dxy, dxs, dys = _derivs(D, layer[k], r[k], c[k])
        t = dx * xc[k] + dy * xr[k] + ds * xi[k]
        contr = D[layer[k], r[k], c[k]] * IMG_SCALE + t * f32(0.5)
        keep = ~((np.abs(contr) * f32(n_layers)).astype(f64) < float(contrast_threshold))
        tr, det = dxx + dyy, dxx * dyy - dxy * dxy
        e = float(edge_threshold)
        keep &= ~((det <= 0) | ((tr * tr).astype(f64) * e >= (e + 1.0) * (e + 1.0) * det.astype(f64)))
        k = k[keep]
        ok[:] = False
        ok[k] = True
        sc = f32(1 << octv)
        out = np.zeros(len(k), KP_DTYPE)
        out["x"] = (c[k].astype(f32) + xc[k]) * sc
        out["y"] = (r[k].astype(f32) + xr[k]) * sc
        out["octave"] = octv + (layer[k] << 8) + (cv_round((xi[k] + f32(0.5)) * f32(255)) << 16)
        p = exp64(((layer[k].astype(f32) + xi[k]) / f32(n_layers)).astype(f64) * LN2).astype(f32)
        out["size"] = (float(sigma) * p.astype(f64) * float(1 << octv) * 2.0).astype(f32)
        out["response"] = np.abs(contr[keep])
    return ok, out, layer[k], r[k], c[k]


# ---- per key point: orientation and descriptor --------------------------------------------------------------------------------------
def orientation_hist(img, r0, c0, radius, sigma):
    """[cv] calcOrientationHist -> (smoothed histogram float32 [36], its maximum)."""
    h, w = img.shape
    n = ORI_BINS
    expf_scale = f32(-1) / (f32(2) * sigma * sigma)
    i, j = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
    y, x = r0 + i, c0 + j
    m = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    i, j, y, x = i[m], j[m], y[m], x[m]                            # row-major: the scalar loop's order
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    wgt = exp32((i * i + j * j).astype(f32) * expf_scale)
    ori = atan2_deg(dy, dx)
    mag = np.sqrt(dx * dx + dy * dy)
    b = cv_round(f32(n) / f32(360) * ori)
    b = np.where(b >= n, b - n, b)
    b = np.where(b < 0, b + n, b)
    tmp = np.zeros(n, f32)
    np.add.at(tmp, b, wgt * mag)
    t = np.concatenate([tmp[-2:], tmp, tmp[:2]])
    hist = (t[0:n] + t[4:n + 4]) * f32(1.0 / 16) + (t[1:n + 1] + t[3:n + 3]) * f32(4.0 / 16) + t[2:n + 2] * f32(6.0 / 16)
    return hist.astype(f32), hist.max()


def orientation_angles(hist, omax):
    """[cv] every local peak >= 0.8 max, parabola through the three bins -> angles (float32), in bin order."""
    n = ORI_BINS
    thr = omax * ORI_PEAK_RATIO
    out = []
    for j in range(n):
        l, r2 = (j - 1) % n, (j + 1) % n
        if hist[j] > hist[l] and hist[j] > hist[r2] and hist[j] >= thr:
            b = f32(j) + f32(0.5) * (hist[l] - hist[r2]) / (hist[l] - f32(2) * hist[j] + hist[r2])
            b = f32(n) + b if b < 0 else (b - f32(n) if b >= n else b)
            a = f32(360) - f32(360) / f32(n) * b
            if abs(a - f32(360)) < FLT_EPSILON:
                a = f32(0)
            out.append(f32(a))
    return out


def descriptor(img, px, py, angle, scl):
    """[cv] calcSIFTDescriptor -> uint8 [128].  px, py: the point on this level (float32); angle: the key point's; scl = size/2 on
    this level."""
    d, n = D_WIDTH, D_BINS
    h, w = img.shape
    ori = f32(360) - f32(angle)
    if abs(ori - f32(360)) < FLT_EPSILON:
        ori = f32(0)
    ptx, pty = int(cv_round(f32(px))), int(cv_round(f32(py)))
    cos_t, sin_t = sincos_deg(ori)
    bins_per_deg = f32(n) / f32(360)
    exp_scale = f32(-1) / f32(d * d * 0.5)
    hist_width = D_SCL_FCTR * f32(scl)
    radius = int(cv_round(hist_width * f32(1.4142135623730951) * f32(d + 1) * f32(0.5)))
    radius = min(radius, int(math.sqrt(float(w) * w + float(h) * h)))
    cos_t, sin_t = f32(cos_t / hist_width), f32(sin_t / hist_width)
    i, j = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
    fi, fj = i.astype(f32), j.astype(f32)
    c_rot = fj * cos_t - fi * sin_t
    r_rot = fj * sin_t + fi * cos_t
    rbin = r_rot + f32(d // 2) - f32(0.5)
    cbin = c_rot + f32(d // 2) - f32(0.5)
    r, c = pty + i, ptx + j
    m = (rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d) & (r > 0) & (r < h - 1) & (c > 0) & (c < w - 1)
    rbin, cbin, r, c, c_rot, r_rot = rbin[m], cbin[m], r[m], c[m], c_rot[m], r_rot[m]
    dx = img[r, c + 1] - img[r, c - 1]
    dy = img[r - 1, c] - img[r + 1, c]
    wgt = exp32((c_rot * c_rot + r_rot * r_rot) * exp_scale)
    o = atan2_deg(dy, dx)
    mag = np.sqrt(dx * dx + dy * dy) * wgt
    obin = (o - ori) * bins_per_deg
    r0, c0, o0 = np.floor(rbin).astype(np.int64), np.floor(cbin).astype(np.int64), np.floor(obin).astype(np.int64)
    rbin, cbin, obin = rbin - r0.astype(f32), cbin - c0.astype(f32), obin - o0.astype(f32)
    o0 = np.where(o0 < 0, o0 + n, o0)
    o0 = np.where(o0 >= n, o0 - n, o0)
    v_r1 = mag * rbin
    v_r0 = mag - v_r1
    v_rc11 = v_r1 * cbin
    v_rc10 = v_r1 - v_rc11
    v_rc01 = v_r0 * cbin
    v_rc00 = v_r0 - v_rc01
    v111 = v_rc11 * obin
    v110 = v_rc11 - v111
    v101 = v_rc10 * obin
    v100 = v_rc10 - v101
    v011 = v_rc01 * obin
    v010 = v_rc01 - v011
    v001 = v_rc00 * obin
    v000 = v_rc00 - v001
    idx = ((r0 + 1) * (d + 2) + c0 + 1) * (n + 2) + o0
    s_c, s_r = n + 2, (d + 2) * (n + 2)
    where = np.stack([idx, idx + 1, idx + s_c, idx + s_c + 1, idx + s_r, idx + s_r + 1, idx + s_r + s_c, idx + s_r + s_c + 1], 1)
    what = np.stack([v000, v001, v010, v011, v100, v101, v110, v111], 1).astype(f32)
    hist = np.zeros((d + 2) * (d + 2) * (n + 2), f32)
    np.add.at(hist, where.ravel(), what.ravel())
    hist = hist.reshape(d + 2, d + 2, n + 2)
    hist[:, :, 0] += hist[:, :, n]
    hist[:, :, 1] += hist[:, :, n + 1]
    dst = hist[1:d + 1, 1:d + 1, :n].reshape(-1).copy()
    nrm2 = np.cumsum(dst * dst, dtype=f32)[-1]                     # cumsum adds in index order
    thr = np.sqrt(nrm2) * D_MAG_THR
    dst = np.minimum(dst, thr)
    nrm2 = np.cumsum(dst * dst, dtype=f32)[-1]
    scale = D_INT_FCTR / max(np.sqrt(nrm2), FLT_EPSILON)
    return np.clip(cv_round(dst * f32(scale)), 0, 255).astype(np.uint8)


# ---- the whole call -------------------------------------------------------------------------------------------------------------------
def sort_order(kp):
    """[cv] KeyPoint_LessThan: x, y ascending; size descending; angle ascending; response, octave descending."""
    return np.lexsort((-kp["octave"].astype(np.int64), -kp["response"], kp["angle"], -kp["size"], kp["y"], kp["x"]))


def detect_and_compute(img_u8, contrast_threshold=0.02, edge_threshold=10.0, n_layers=N_LAYERS, sigma=SIGMA, info=None):
    """-> (key points KP_DTYPE [n], descriptors uint8 [n, 128] or None).  info: dict filled with the stats the library reports and
    the intermediate lists (for the driver of sift_math.hpp)."""
    img_u8 = np.asarray(img_u8)
    assert img_u8.dtype == np.uint8 and img_u8.ndim == 2
    h, w = img_u8.shape
    n_oct = n_octaves(2 * h, 2 * w)
    stats = {"octaves": n_oct, "candidates": [], "refined": [], "keypoints": [], "before_dedup": 0, "after_dedup": 0}
    trace = {"cand": [], "refined": [], "kp": [], "gauss": None, "dog": None}
    kps, descs = [], []
    if n_oct > 0:
        base = base_image(img_u8, sigma)
        gauss, dog = build_pyramids(base, n_oct, sigma, n_layers)
        trace["gauss"], trace["dog"] = gauss, dog
        threshold = math.floor(0.5 * contrast_threshold / n_layers * 255)
        for o in range(n_oct):
            cand = scan_extrema(dog[o], n_layers, threshold)
            ok, fields, layer, r, c = refine(dog[o], cand, o, n_layers, contrast_threshold, edge_threshold, sigma) if len(cand) else \
                (np.zeros(0, bool), np.zeros(0, KP_DTYPE), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
            trace["cand"].append((cand, ok))
            trace["refined"].append((fields, layer, r, c))
            out_o = []
            for k in range(len(fields)):
                scl_octv = fields["size"][k] * f32(0.5) / f32(1 << o)
                img = gauss[o][layer[k]]
                hist, omax = orientation_hist(img, int(r[k]), int(c[k]), int(cv_round(ORI_RADIUS * scl_octv)), ORI_SIG_FCTR * scl_octv)
                for a in orientation_angles(hist, omax):
                    rec = fields[k].copy()
                    rec["angle"] = a
                    out_o.append(rec)
            out_o = np.array(out_o, KP_DTYPE) if out_o else np.zeros(0, KP_DTYPE)
            desc_o = np.zeros((len(out_o), 128), np.uint8)
            inv = f32(1) / f32(1 << o)
            for k in range(len(out_o)):
                kp = out_o[k]
                lay = (int(kp["octave"]) >> 8) & 255
                desc_o[k] = descriptor(gauss[o][lay], kp["x"] * inv, kp["y"] * inv, kp["angle"], kp["size"] * inv * f32(0.5))
            trace["kp"].append((out_o, desc_o))
            stats["candidates"].append(len(cand))
            stats["refined"].append(len(fields))
            stats["keypoints"].append(len(out_o))
            kps.append(out_o)
            descs.append(desc_o)
    kp = np.concatenate(kps) if kps else np.zeros(0, KP_DTYPE)
    desc = np.concatenate(descs) if descs else np.zeros((0, 128), np.uint8)
    stats["before_dedup"] = len(kp)
    order = sort_order(kp)
    kp, desc = kp[order], desc[order]
    if len(kp):
        same = np.zeros(len(kp), bool)
        same[1:] = (kp["x"][1:] == kp["x"][:-1]) & (kp["y"][1:] == kp["y"][:-1]) & (kp["size"][1:] == kp["size"][:-1]) & \
            (kp["angle"][1:] == kp["angle"][:-1])
        kp, desc = kp[~same], desc[~same]
    stats["after_dedup"] = len(kp)
    # [cv] firstOctave = -1: back to the coordinates of the image that came in
    kp["x"] *= f32(0.5)
    kp["y"] *= f32(0.5)
    kp["size"] *= f32(0.5)
    kp["octave"] = (kp["octave"] & ~255) | ((kp["octave"] - 1) & 255)
    if info is not None:
        info.update(stats=stats, trace=trace)
    return kp, (desc if len(kp) else None)
