"""One level and one window of the LK tracker (csrc/k_lk.hip, k_lk2.hip) in plain numpy with int64 sums - used ONLY to choose the fixtures of
tests/lk_cases.py and to prove in tests/test_lk_cases_host.py that each does what it is there for.  It is not a second oracle: what
a kernel returns is always compared with `oracle.pyr_lk`.

The template's origin is an integer pixel, so its bilinear weights are (16384, 0, 0, 0): the Q5 intensity is 32 p and Ix / Iy are the
Scharr values themselves.  The search position may be any float32 position (the level below hands one down).  Windows must lie
inside the image with one pixel to spare (template) / two (search): nothing here mirrors a border.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
FLT_SCALE = F32(1.0 / (1 << 20))
FLT_EPSILON = F32(np.finfo(np.float32).eps)
MIN_EIG = F32(1e-4)
LK_RUN = 5                      # pixels of a run (lk_device.hpp)
WRAP = 1 << 31                  # an int32 holds sums of magnitude below this


def lk_weights(a, b):
    """The bilinear weights of `lk_weights` in lk_device.hpp, float32 step by step -> (w00, w01, w10, w11)."""
    a, b = F32(a), F32(b)
    oma, omb = F32(1) - a, F32(1) - b
    t00, t01, t10 = oma * omb, a * omb, oma * b
    w00, w01, w10 = (int(np.rint(t * F32(16384))) for t in (t00, t01, t10))      # (rint: half to even, as __float2int_rn)
    return w00, w01, w10, 16384 - w00 - w01 - w10


def template_fraction(p, win, level=0):
    """(ipx, a): integer origin and float32 fraction of the template window of a key-point coordinate `p` at `level`."""
    half = F32(win - 1) * F32(0.5)
    pr = F32(p) * F32(0.5 if level else 1.0) - half
    ip = int(np.floor(pr))
    return ip, pr - F32(ip)


def scharr(img):
    """Scharr derivatives of a whole image (intensities mirrored REFLECT_101 at the border) -> (Ix, Iy) int64."""
    p = np.pad(np.asarray(img, np.int64), 1, mode="reflect")
    a00, a01, a02 = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    a10, a12 = p[1:-1, :-2], p[1:-1, 2:]
    a20, a21, a22 = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    ix = ((a02 + a22) * 3 + a12 * 10) - ((a00 + a20) * 3 + a10 * 10)
    iy = ((a20 + a22) * 3 + a21 * 10) - ((a00 + a02) * 3 + a01 * 10)
    return ix, iy


def template(img, ipx, ipy, win, deriv=None):
    """Window with integer origin (ipx, ipy) -> (I in Q5, Ix, Iy), int64 win x win.  `deriv`: `scharr(img)` computed before."""
    H, W = img.shape
    assert 0 <= ipx and ipx + win <= W and 0 <= ipy and ipy + win <= H, "window outside the image"
    ix, iy = deriv if deriv is not None else scharr(img)
    s = np.s_[ipy:ipy + win, ipx:ipx + win]
    return np.asarray(img, np.int64)[s] * 32, ix[s], iy[s]


def cut_values(iA11, iA12, iA22, win):
    """The float32 values of the eigenvalue cut of `lk_track_point` (k_lk.hip) and `lk2_track_point` (k_lk2.hip) from the integer normal matrix (int64 scalars or arrays), every step rounded on
    its own -> dict; `tracked` is the outcome of the cut `minEig < 1e-4f || D < FLT_EPSILON`."""
    A11, A12, A22 = (np.asarray(v, np.int64).astype(F32) * FLT_SCALE for v in (iA11, iA12, iA22))
    D = A11 * A22 - A12 * A12
    dA = A11 - A22
    q = dA * dA + F32(4) * A12 * A12
    min_eig = (A22 + A11 - np.sqrt(q)) / F32(2 * win * win)
    assert all(v.dtype == F32 for v in (A11, D, q, min_eig))
    return dict(A11=A11, A12=A12, A22=A22, D=D, q=q, minEig=min_eig, tracked=~((min_eig < MIN_EIG) | (D < FLT_EPSILON)))


def normal_matrix(tIx, tIy, win):
    """Integer normal matrix of one window and its `cut_values` -> dict."""
    iA11, iA12, iA22 = int((tIx * tIx).sum()), int((tIx * tIy).sum()), int((tIy * tIy).sum())
    out = {k: v[()] for k, v in cut_values(iA11, iA12, iA22, win).items()}
    out.update(iA11=iA11, iA12=iA12, iA22=iA22, tracked=bool(out["tracked"]))
    return out


def cut_map(img, win):
    """`cut_values` of every window that lies inside the image: entry [y, x] is the window whose integer origin is (x, y)."""
    ix, iy = scharr(img)

    def box(v):
        c = np.zeros((v.shape[0] + 1, v.shape[1] + 1), np.int64)
        c[1:, 1:] = v.cumsum(0).cumsum(1)
        return c[win:, win:] - c[:-win, win:] - c[win:, :-win] + c[:-win, :-win]

    return cut_values(box(ix * ix), box(ix * iy), box(iy * iy), win)


def search_values(img, nx, ny, win):
    """Q5 intensities of the search window whose float32 origin is (nx, ny) -> int64 win x win."""
    nx, ny = F32(nx), F32(ny)
    inx, iny = int(np.floor(nx)), int(np.floor(ny))
    H, W = img.shape
    assert 0 <= inx and inx + win + 1 <= W and 0 <= iny and iny + win + 1 <= H, "search window outside the image"
    w00, w01, w10, w11 = lk_weights(nx - F32(inx), ny - F32(iny))
    p = np.asarray(img, np.int64)[iny:iny + win + 1, inx:inx + win + 1]
    v = p[:-1, :-1] * w00 + p[:-1, 1:] * w01 + p[1:, :-1] * w10 + p[1:, 1:] * w11
    return (v + (1 << (14 - 5 - 1))) >> (14 - 5)


def mismatch_terms(tI, tIx, tIy, img_j, nx, ny):
    """Per-pixel terms of one iteration's mismatch vector -> (terms of ib1, terms of ib2), int64 win x win; ib = terms.sum()."""
    diff = search_values(img_j, nx, ny, tI.shape[0]) - tI
    return diff * tIx, diff * tIy


def lane_of(win):
    """Lane of every window pixel as `lk_run_desc` (lk_device.hpp) deals them: run r = t * 64 + lane, row r / rpr, columns (r % rpr) * 5 .. + 4,
    rpr = ceil(win / 5) -> (int array win x win, runs per lane NR)."""
    rpr = (win + LK_RUN - 1) // LK_RUN
    yy, xx = np.mgrid[0:win, 0:win]
    r = yy * rpr + xx // LK_RUN
    return r % 64, (win * rpr + 63) // 64


def runs_per_lane(win):
    return lane_of(win)[1]


def lane_sums(terms, win):
    """-> (largest |per-lane sum|, largest |sum over lanes 4 i .. 4 i + 3|) of per-pixel `terms`: what a lane holds in its int32 and
    what `wave_sum_split4` holds in one after its two unsplit steps."""
    lane, _ = lane_of(win)
    per = np.bincount(lane.ravel(), weights=None, minlength=64) * 0        # (int64 zeros)
    np.add.at(per, lane.ravel(), terms.ravel())
    four = per.reshape(16, 4).sum(1)
    return int(np.abs(per).max()), int(np.abs(four).max())


def theoretical_four_lane_bound(nr):
    """4 lanes x 5 NR pixels x the largest |Q5 difference| 8160 x the largest |Scharr value| 4080."""
    return 4 * 5 * nr * 8160 * 4080
