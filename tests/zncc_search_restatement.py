"""The definition of the ZNCC search around each key point (km_zncc_search, csrc/zncc_math.hpp), in numpy.

The reference has no such search; what it does define is every number the search is made of:
`_zncc2(img1, img2, u1, v1, u2, v2, n)` (karios/matcher/zncc_service.py:45-126) is the value at an offset, and
`ZNCCService._compute_zncc` (:186-238) the window centres and the rule by which a row is skipped.  This file restates both and adds
the peak rule and the per-axis parabola, in the order of operations the library uses (float64, no fused multiply-add).

Two forms of the value: `two_pass` is the reference's own arithmetic (mean, population std, mean of products, numpy's float64); `moments`
is the exact-integer form the library uses for integer pixels, `cv / (sqrt(v1) * sqrt(v2))` with int64 moments - a function of the
pixels alone, so the device, the host launcher and this file agree on it bit for bit.
"""
import math
from collections import namedtuple

import numpy as np

HW, SIDE, NPX, MARGIN = 21, 43, 1849, 28
MAX_RADIUS, MAX_ROWS = 8, 1 << 20
SKIPPED, NO_VALUE, RIM_X, RIM_Y = 1, 2, 4, 8
Result = namedtuple("Result", "offset peak shift status surface")


def centres(x0, y0, dx, dy, ref_shape, mon_shape):
    """One row -> (X0, Y0, X1, Y1), or None where compute_zncc skips it.  float32 arithmetic, round half to even."""
    x0, y0, dx, dy = (np.float32(v) for v in (x0, y0, dx, dy))
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = np.float32(x0 + dx), np.float32(y0 + dy)
    if not all(abs(float(v)) < 1e9 for v in (x0, y0, sx, sy)):        # (NaN fails the comparison; beyond 1e9 lies outside every raster)
        return None
    X0, Y0, X1, Y1 = int(x0), int(y0), int(np.rint(sx)), int(np.rint(sy))
    if X0 - MARGIN < 0 or Y0 - MARGIN < 0 or X1 - MARGIN < 0 or Y1 - MARGIN < 0:
        return None
    if X0 >= ref_shape[1] - MARGIN or Y0 >= ref_shape[0] - MARGIN or X1 >= mon_shape[1] - MARGIN or Y1 >= mon_shape[0] - MARGIN:
        return None
    return X0, Y0, X1, Y1


def _windows(mon, X1, Y1, R):
    """-> (S x S x 43 x 43 view of the windows of a zero-padded copy of the region, S x S bool: the window lies in `mon`)."""
    S, RW = 2 * R + 1, SIDE + 2 * R
    bx, by = X1 - R - HW, Y1 - R - HW
    region = np.zeros((RW, RW), mon.dtype)
    ys, xs = max(by, 0), max(bx, 0)
    ye, xe = min(by + RW, mon.shape[0]), min(bx + RW, mon.shape[1])
    if ye > ys and xe > xs:
        region[ys - by:ye - by, xs - bx:xe - bx] = mon[ys:ye, xs:xe]
    o = np.arange(-R, R + 1)
    in_x = (X1 + o - HW >= 0) & (X1 + o + HW < mon.shape[1])
    in_y = (Y1 + o - HW >= 0) & (Y1 + o + HW < mon.shape[0])
    return np.lib.stride_tricks.sliding_window_view(region, (SIDE, SIDE)), in_y[:, None] & in_x[None, :]


def surface_two_pass(ref, mon, X0, Y0, X1, Y1, R):
    """_zncc2 at every offset, the reference's arithmetic: NaN where the window leaves `mon` (its IndexError) or has no variance."""
    a = ref[Y0 - HW:Y0 + HW + 1, X0 - HW:X0 + HW + 1].astype(np.float64)
    win, inside = _windows(mon, X1, Y1, R)
    b = win.astype(np.float64)
    sd1 = a.std()
    sd2 = b.std(axis=(2, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        an = (a - a.mean()) / sd1
        bn = (b - b.mean(axis=(2, 3), keepdims=True)) / sd2[:, :, None, None]
        z = (an[None, None] * bn).mean(axis=(2, 3))
    z[~inside | (sd2 == 0) | (sd1 == 0)] = np.nan
    return z


def surface_moments(ref, mon, X0, Y0, X1, Y1, R):
    """The same surface from exact int64 moments (integer pixel types; int16 biased by 2^15, which no value sees)."""
    bias = 32768 if ref.dtype == np.int16 else 0
    a = ref[Y0 - HW:Y0 + HW + 1, X0 - HW:X0 + HW + 1].astype(np.int64) + bias
    win, inside = _windows(mon, X1, Y1, R)
    b = win.astype(np.int64) + bias
    sa, saa = int(a.sum()), int((a * a).sum())
    sb, sbb, sab = b.sum(axis=(2, 3)), (b * b).sum(axis=(2, 3)), np.einsum("ijkl,kl->ij", b, a)
    v1 = NPX * saa - sa * sa
    S = 2 * R + 1
    z = np.full((S, S), np.nan)
    for i in range(S):
        for j in range(S):
            if not inside[i, j]:
                continue
            v2 = NPX * int(sbb[i, j]) - int(sb[i, j]) ** 2
            cv = NPX * int(sab[i, j]) - sa * int(sb[i, j])
            if v1 != 0 and v2 != 0:
                z[i, j] = float(cv) / (math.sqrt(float(v1)) * math.sqrt(float(v2)))
    return z


def _axis_step(zl, zc, zr, pos, S):
    """-> (step, the rim or a missing neighbour refused it)"""
    if pos == 0 or pos == S - 1 or math.isnan(zl) or math.isnan(zr):
        return 0.0, True
    den = (zl - 2.0 * zc) + zr
    if not den < 0.0:
        return 0.0, False
    return 0.5 * (zl - zr) / den, False


def finish(z, R, X0, Y0, X1, Y1):
    """Surface -> (offset (bx, by), peak, shift (x, y), status)."""
    S = 2 * R + 1
    if np.isnan(z).all():
        return (0, 0), np.nan, (np.nan, np.nan), NO_VALUE
    best = int(np.nanargmax(z.ravel()))                 # the first of equal values
    iy, ix = divmod(best, S)
    zz = [[float(v) for v in row] for row in z]
    sx, rim_x = _axis_step(zz[iy][ix - 1] if ix > 0 else np.nan, zz[iy][ix], zz[iy][ix + 1] if ix < S - 1 else np.nan, ix, S)
    sy, rim_y = _axis_step(zz[iy - 1][ix] if iy > 0 else np.nan, zz[iy][ix], zz[iy + 1][ix] if iy < S - 1 else np.nan, iy, S)
    return ((ix - R, iy - R), zz[iy][ix], (float(X1 + ix - R - X0) + sx, float(Y1 + iy - R - Y0) + sy),
            (RIM_X if rim_x else 0) | (RIM_Y if rim_y else 0))


def search(ref, mon, x0, y0, dx, dy, radius, form=None):
    """All rows -> Result of numpy arrays (the surface always).  form: "moments" / "two_pass"; None: by pixel type, as the library."""
    ref, mon = np.asarray(ref), np.asarray(mon)
    if not 1 <= radius <= MAX_RADIUS or len(x0) > MAX_ROWS or ref.dtype != mon.dtype:
        raise ValueError("zncc_search: radius 1 .. 8, at most 2^20 rows, one pixel type")
    if form is None:
        form = "two_pass" if ref.dtype == np.float32 else "moments"
    n, S = len(x0), 2 * radius + 1
    out = Result(np.zeros((n, 2), np.int32), np.full(n, np.nan), np.full((n, 2), np.nan), np.zeros(n, np.uint8), np.full((n, S, S), np.nan))
    for k in range(n):
        c = centres(x0[k], y0[k], dx[k], dy[k], ref.shape, mon.shape)
        if c is None:
            out.status[k] = SKIPPED
            continue
        z = (surface_moments if form == "moments" else surface_two_pass)(ref, mon, *c, radius)
        out.surface[k] = z
        out.offset[k], out.peak[k], out.shift[k], out.status[k] = finish(z, radius, *c)
    return out


def peaks(surface, centres_, radius):
    """The peak and parabola of given surfaces (n x S x S; centres_: n x 4 of X0, Y0, X1, Y1; a row of NaN centres is skipped):
    the numpy form of zncc_math.hpp's finish."""
    n = len(surface)
    out = Result(np.zeros((n, 2), np.int32), np.full(n, np.nan), np.full((n, 2), np.nan), np.zeros(n, np.uint8), surface)
    for k in range(n):
        if centres_[k] is None:
            out.status[k] = SKIPPED
            continue
        out.offset[k], out.peak[k], out.shift[k], out.status[k] = finish(np.asarray(surface[k], np.float64), radius, *centres_[k])
    return out


def top_two_gap(z):
    """Largest minus second-largest value of a surface (inf with fewer than two values)."""
    v = np.sort(z[~np.isnan(z)])
    return float(v[-1] - v[-2]) if v.size >= 2 else math.inf


def axis_denominators(z, offset, R):
    """(den_x, den_y) of the parabola at the peak; None for an axis whose step the rim or a missing neighbour refuses."""
    S, ix, iy = 2 * R + 1, offset[0] + R, offset[1] + R
    dens = []
    for l, r, pos in (((iy, ix - 1), (iy, ix + 1), ix), ((iy - 1, ix), (iy + 1, ix), iy)):
        if pos == 0 or pos == S - 1 or np.isnan(z[l]) or np.isnan(z[r]):
            dens.append(None)
        else:
            dens.append((float(z[l]) - 2.0 * float(z[iy, ix])) + float(z[r]))
    return dens
