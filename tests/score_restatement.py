"""Restatement, in exact arithmetic, of the three per-key-point scores (`zncc_score`, `mutual_info_score`, `mi_score`) as
libkarios_hip.so computes them (csrc/k_zncc.hip, k_mi.hip, mi_math.hpp): the key-point rule that cuts the chips, the 32 x 32 joint
histogram of `np.histogram2d(chip_ref, chip_mon, bins=32)`, the two entropy ratios and the zero-normalised cross correlation.

This is the DEFINITION the kernels are held to (tests/test_gpu_score_edges.py, gate 1e-9); tests/test_score_host.py holds it to the
installed numpy, cell for cell, and to the recorded results of the reference (tests/golden/mutual_info.npz, zncc.npz).  Integer
pixels are binned in integer arithmetic, the entropies are summed in np.longdouble by math.fsum, the correlation is a ratio of
`fractions.Fraction` moments evaluated by `decimal` to 50 digits.  [ref] marks the reference's rule, [def] a choice of this project.

`fixtures(dtype)` are the seeded inputs shared by the CPU and the GPU tests: ranges, extremes and bin edges chosen where the
kernels' integer forms could go wrong.

Test infrastructure only: karios_amd never imports this module.
"""
from __future__ import annotations

import collections
import decimal
import functools
import math
from fractions import Fraction

import numpy as np

f32 = np.float32
ld = np.longdouble
CHIP = 57
MARGIN = 28
HALF = 21                         # the ZNCC window: the central 43 x 43 pixels of the chip
RIM = MARGIN - HALF
BINS = 32
NPX = CHIP * CHIP
INT_TYPES = (np.uint8, np.uint16, np.int16)
TYPES = INT_TYPES + (np.float32,)


# ---- the key-point rule -------------------------------------------------------------------------------------------------------------
def round_half_even_f32(v):
    """round(np.float32): to the nearest integer, ties to the even one."""
    fl = math.floor(v)
    d = v - fl                     # exact: v is a float32 held in a float64
    if d > 0.5 or (d == 0.5 and fl % 2):
        fl += 1
    return int(fl)


def chips(ref, mon, x0, y0, dx, dy):
    """[ref] `int(x0)`, `round(x0 + dx)` on the float32 sum, the four bounds tests with margin 28 on both images -> the two 57 x 57
    chips, or None (no chip: every score is NaN).  A non-finite sum gives no chip."""
    x0, y0, dx, dy = f32(x0), f32(y0), f32(dx), f32(dy)
    if not (np.isfinite(x0) and np.isfinite(y0)):
        return None
    with np.errstate(all="ignore"):
        sx, sy = f32(x0 + dx), f32(y0 + dy)
    if not (np.isfinite(sx) and np.isfinite(sy)):
        return None
    X0, Y0 = int(x0), int(y0)      # truncation toward zero
    X1, Y1 = round_half_even_f32(float(sx)), round_half_even_f32(float(sy))
    (Hr, Wr), (Hm, Wm) = ref.shape, mon.shape
    if X0 - MARGIN < 0 or Y0 - MARGIN < 0 or X1 - MARGIN < 0 or Y1 - MARGIN < 0:
        return None
    if X0 >= Wr - MARGIN or Y0 >= Hr - MARGIN or X1 >= Wm - MARGIN or Y1 >= Hm - MARGIN:
        return None
    return (ref[Y0 - MARGIN:Y0 + MARGIN + 1, X0 - MARGIN:X0 + MARGIN + 1], mon[Y1 - MARGIN:Y1 + MARGIN + 1, X1 - MARGIN:X1 + MARGIN + 1])


def window(chip):
    """The ZNCC window of a chip."""
    return chip[RIM:CHIP - RIM, RIM:CHIP - RIM]


# ---- the joint histogram ------------------------------------------------------------------------------------------------------------
def int_bins(c, rule="floor"):
    """Bins of an integer chip, in integer arithmetic: edge i of np.linspace(lo, hi, 33) is lo + i R / 32, exact in float64, so
    `edge_i <= x` is i R <= 32 (x - lo): bin = min(32 (x - lo) // R, 31); a constant chip is widened to [v - 0.5, v + 0.5]: bin 16.
    `rule` other than "floor": the deliberately wrong rules of tests/test_score_host.py (bins may then reach 32)."""
    v = c.astype(np.int64).ravel()
    lo, hi = int(v.min()), int(v.max())
    R = hi - lo
    if R == 0:
        return np.full(v.size, BINS // 2, np.int64)
    d = v - lo
    if rule == "floor":
        return np.minimum(32 * d // R, BINS - 1)
    if rule == "magic_floor":      # the kernel's multiplication with M rounded DOWN
        L = (R - 1).bit_length() if R > 1 else 0
        M = (1 << (21 + L)) // R
        return np.minimum((d * M) >> (21 + L - 5), BINS - 1)
    if rule == "round":            # to the nearest bin instead of down
        return np.minimum((2 * 32 * d + R) // (2 * R), BINS - 1)
    if rule == "no_fold":          # the maximum keeps bin 32
        return 32 * d // R
    raise ValueError(rule)


def float_bins(c):
    """numpy's rule restated on the float64 casts: edges i * step + lo with step = (hi - lo) / 32, the last edge hi itself;
    bin = searchsorted(edges, x, 'right') - 1, the maximum folded into bin 31; a constant chip widened by 0.5 on both sides."""
    v = c.astype(np.float64).ravel()
    lo, hi = float(v.min()), float(v.max())
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    step = (hi - lo) / BINS
    edges = np.array([i * step + lo for i in range(BINS)] + [hi], np.float64)
    b = np.searchsorted(edges, v, side="right") - 1
    b[v == hi] = BINS - 1
    return b.astype(np.int64)


def mi_counts(c1, c2, rule="floor"):
    """The 32 x 32 table of np.histogram2d(c1, c2, bins=32) as integers (33 x 33 under a wrong `rule`), or None: [ref] numpy raises on
    a non-finite sample in either chip and the reference scores the key point NaN."""
    c1, c2 = np.asarray(c1), np.asarray(c2)
    if c1.dtype.kind == "f":
        if not (np.isfinite(c1).all() and np.isfinite(c2).all()):
            return None
        b1, b2 = float_bins(c1), float_bins(c2)
        side = BINS
    else:
        b1, b2 = int_bins(c1, rule), int_bins(c2, rule)
        side = BINS if rule == "floor" else BINS + 1
    return np.bincount(b1 * side + b2, minlength=side * side).reshape(side, side)


def _fsum(t):
    """The sum of np.longdouble terms: each term split into two float64, both lists summed exactly by math.fsum."""
    t = np.asarray(t, ld)
    hi = t.astype(np.float64)
    low = (t - hi.astype(ld)).astype(np.float64)
    return ld(math.fsum(hi.tolist())) + ld(math.fsum(low.tolist()))


def _entropy(counts, n):
    """-sum p ln p of integer counts with total n, in np.longdouble: ln n - (1 / n) sum c ln c."""
    c = np.asarray(counts).ravel()
    c = c[c > 0].astype(ld)
    return np.log(ld(n)) - _fsum(c * np.log(c)) / ld(n)


def mi_scores(counts):
    """(studholme, nmi) of a table of counts: [ref] (H(X) + H(Y)) / H(X,Y) and 2 (H(X) + H(Y) - H(X,Y)) / (H(X) + H(Y)) (both
    ratios are independent of the logarithm's base); NaN, both, exactly when ONE joint cell is occupied (the reference's
    H(X,Y) == 0 and H(X) + H(Y) == 0), and for `None`."""
    if counts is None or int((counts > 0).sum()) == 1:
        return float("nan"), float("nan")
    n = int(counts.sum())
    hx, hy, hxy = _entropy(counts.sum(axis=1), n), _entropy(counts.sum(axis=0), n), _entropy(counts, n)
    return float((hx + hy) / hxy), float(ld(2) * (hx + hy - hxy) / (hx + hy))


# ---- the correlation ----------------------------------------------------------------------------------------------------------------
def _exact(p):
    p = np.asarray(p)
    if p.dtype.kind == "f":
        return [Fraction(float(v)) for v in p.ravel()]      # a float converts exactly
    return [int(v) for v in p.ravel()]


def zncc_exact(p1, p2):
    """mean(((p1 - m1) / s1) ((p2 - m2) / s2)) with population deviations = cv / sqrt(v1 v2) on the exact moments
    v = n S_aa - S_a^2, cv = n S_ab - S_a S_b; NaN when a window has no variance [ref] or holds a non-finite pixel."""
    p1, p2 = np.asarray(p1), np.asarray(p2)
    for p in (p1, p2):
        if p.dtype.kind == "f" and not np.isfinite(p).all():
            return float("nan")
    a, b = _exact(p1), _exact(p2)
    n = len(a)
    sa, sb = sum(a), sum(b)
    v1 = n * sum(x * x for x in a) - sa * sa
    v2 = n * sum(x * x for x in b) - sb * sb
    cv = n * sum(x * y for x, y in zip(a, b)) - sa * sb
    if v1 == 0 or v2 == 0:
        return float("nan")
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        ctx.Emax, ctx.Emin = decimal.MAX_EMAX, decimal.MIN_EMIN
        prod, cvf = Fraction(v1) * Fraction(v2), Fraction(cv)
        root = (decimal.Decimal(prod.numerator) / decimal.Decimal(prod.denominator)).sqrt()
        return float(decimal.Decimal(cvf.numerator) / decimal.Decimal(cvf.denominator) / root)


def scores(ref, mon, x0, y0, dx, dy):
    """(zncc, studholme, nmi) float64 columns of the key points, by the rules above."""
    out = np.full((3, len(x0)), np.nan, np.float64)
    for k in range(len(x0)):
        got = chips(ref, mon, x0[k], y0[k], dx[k], dy[k])
        if got is None:
            continue
        c1, c2 = got
        out[0, k] = zncc_exact(window(c1), window(c2))
        out[1, k], out[2, k] = mi_scores(mi_counts(c1, c2))
    return out


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "group name ref mon x0 y0 dx dy")


def limits(dtype):
    """(lowest, highest) value the fixtures use for a pixel type."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return -3.0e38, 3.0e38
    info = np.iinfo(dt)
    return int(info.min), int(info.max)


def tile(group, name, pairs):
    """Chips side by side: a raster 57 rows high, chip k's key point at (28 + 57 k, 28), every chip touching the first and the last
    row, the last chip ending at the raster's last element."""
    ref = np.ascontiguousarray(np.hstack([p[0] for p in pairs]))
    mon = np.ascontiguousarray(np.hstack([p[1] for p in pairs]))
    K = len(pairs)
    x0 = (MARGIN + CHIP * np.arange(K)).astype(f32)
    return Case(group, name, ref, mon, x0, np.full(K, MARGIN, f32), np.zeros(K, f32), np.zeros(K, f32))


def sweep_ranges(dtype):
    """The ranges R of the sweep: uint8 every R; 16 bit: 1 .. 600, 2^k - 1, 2^k, 2^k + 1 for k = 9 .. 15, 65534, 65535 and 300 seeded."""
    if np.dtype(dtype).itemsize == 1:
        return list(range(1, 256))
    rng = np.random.default_rng(600)
    rs = list(range(1, 601))
    for k in range(9, 16):
        rs += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    rs += [65534, 65535] + [int(v) for v in rng.integers(600, 65536, 300)]
    return list(dict.fromkeys(rs))


def sweep_samples(R, rng):
    """The 3249 offsets d of a sweep chip: ten times d = 0 and ten times d = R (on an edge for every R), for i = 1 .. 32 the integers
    around edge i (ceil(i R / 32), the one below, floor(i R / 32) + 1), the rest seeded fill; in seeded order."""
    d = [0] * 10 + [R] * 10
    for i in range(1, BINS + 1):
        up = -((-i * R) // BINS)
        d += [up, up - 1, i * R // BINS + 1]
    d = np.clip(np.array(d, np.int64), 0, R)
    d = np.concatenate([d, rng.integers(0, R + 1, NPX - d.size)])
    return rng.permutation(d)


def sweep(dtype):
    """The range sweep of the MI integer path: one chip per R; lo = the type's minimum, its maximum - R, or seeded.  The monitored
    raster carries the same chips in reversed order, each in another pixel order, so both magic constants see every R."""
    tmin, tmax = limits(dtype)
    rng = np.random.default_rng(57 + np.dtype(dtype).itemsize)
    pairs, rs = [], sweep_ranges(dtype)
    for k, R in enumerate(rs):
        lo = tmin if k % 3 == 0 else tmax - R if k % 3 == 1 else int(rng.integers(tmin, tmax - R + 1))
        pairs.append((lo + sweep_samples(R, rng)).astype(dtype).reshape(CHIP, CHIP))
    mons = [rng.permutation(c.ravel()).reshape(CHIP, CHIP) for c in reversed(pairs)]
    return tile("sweep", "sweep", list(zip(pairs, mons))), rs


def noise(dtype, rng, lo=None, hi=None):
    tmin, tmax = limits(dtype)
    lo, hi = tmin if lo is None else lo, tmax if hi is None else hi
    if np.dtype(dtype).kind == "f":
        lo, hi = float(lo), float(hi)
        return np.clip(rng.uniform(-1.0, 1.0, (CHIP, CHIP)) * 0.5 * (hi - lo) + 0.5 * (hi + lo), lo, hi).astype(dtype)
    return rng.integers(lo, hi + 1, (CHIP, CHIP)).astype(dtype)


def step_up(v, dtype):
    """The next value above v: + 1 for integers, the next float32."""
    return np.nextafter(f32(v), f32(np.inf)) if np.dtype(dtype).kind == "f" else v + 1


def bases(dtype):
    tmin, tmax = limits(dtype)
    if np.dtype(dtype).kind == "f":
        return [0.0, 1.0e6, -2.5]
    return [tmin, tmax - 1, (tmin + tmax) // 2]


def degenerate(dtype):
    """Tables with one, two or three occupied cells, and the chips whose only extreme is their first / last pixel."""
    rng = np.random.default_rng(16)
    cases, pairs = [], []

    def with_px(c, pos, v):
        c = c.copy()
        c[pos] = v
        return c
    for v in bases(dtype):
        c = np.full((CHIP, CHIP), v, dtype)
        up = step_up(v, dtype)
        two1 = np.where(rng.integers(0, 2, (CHIP, CHIP)) > 0, up, v).astype(dtype)
        two2 = np.where(rng.integers(0, 2, (CHIP, CHIP)) > 0, up, v).astype(dtype)
        pairs += [(c, c),                                                       # constant against constant: NaN
                  (c, noise(dtype, rng)), (noise(dtype, rng), c),               # constant against varying
                  (with_px(c, (30, 11), up), c), (c, with_px(c, (0, 56), up)),  # one pixel off in one chip: two cells
                  (with_px(c, (30, 11), up), with_px(c, (30, 11), up)),         # ... in both, at the same position
                  (with_px(c, (30, 11), up), with_px(c, (56, 0), up)),          # ... at different positions
                  (two1, two2), (two1, two1)]                                   # two-valued chips, R = 1
    cases.append(tile("degenerate", "cells", pairs))
    # the unique maximum only at chip pixel (56, 56) - the raster's LAST element - and the unique minimum only at (0, 0), its first
    tmin, tmax = limits(dtype)
    inner = (step_up(tmin, dtype), np.nextafter(f32(tmax), f32(0)) if np.dtype(dtype).kind == "f" else tmax - 1)
    for name, first, last in (("corner_max", None, tmax), ("corner_min", tmin, None), ("corner_both", tmin, tmax)):
        pair = []
        for _ in range(2):
            c = noise(dtype, rng, *inner)
            if first is not None:
                c[0, 0] = first
            if last is not None:
                c[CHIP - 1, CHIP - 1] = last
            pair.append(c)
        cases.append(tile("degenerate", name, [tuple(pair)]))
    return cases


def checkerboard(lo, hi, dtype):
    y, x = np.mgrid[0:CHIP, 0:CHIP]
    return np.where((x + y) % 2 == 0, lo, hi).astype(dtype)


def zncc_extremes(dtype):
    """Windows at the ends of the pixel range, windows without variance inside a chip that has some, and single pixels off by one."""
    rng = np.random.default_rng(43)
    tmin, tmax = limits(dtype)
    board, inverse = checkerboard(tmin, tmax, dtype), checkerboard(tmax, tmin, dtype)
    pairs = [(board, board), (board, inverse), (inverse, board),
             (noise(dtype, rng), noise(dtype, rng)), (noise(dtype, rng), board)]
    a = noise(dtype, rng)
    pairs.append((a, a))
    for v in bases(dtype):
        # constant inside the central 43 x 43 window, varying only in the 7-pixel rim: ZNCC NaN, both MI scores finite
        rim = noise(dtype, rng)
        rim[RIM:CHIP - RIM, RIM:CHIP - RIM] = v
        pairs += [(rim, noise(dtype, rng)), (noise(dtype, rng), rim)]
        # one pixel off by one at the window's centre and at its corners (21 +- 21 inside the window)
        for pos in ((MARGIN, MARGIN), (RIM, RIM), (RIM, CHIP - RIM - 1), (CHIP - RIM - 1, RIM), (CHIP - RIM - 1, CHIP - RIM - 1)):
            c = np.full((CHIP, CHIP), v, dtype)
            c[pos] = step_up(v, dtype)
            pairs += [(c, noise(dtype, rng)), (c, c)]
        # ... and one step OUTSIDE the window: no variance inside
        c = np.full((CHIP, CHIP), v, dtype)
        c[RIM - 1, RIM] = step_up(v, dtype)
        c[CHIP - RIM, CHIP - RIM - 1] = step_up(v, dtype)
        pairs.append((c, noise(dtype, rng)))
    return [tile("zncc", "extremes", pairs)]


NONFINITE_RIM = ((0, 0), (CHIP - 1, CHIP - 1), (3, 30), (RIM - 1, RIM - 1), (CHIP - RIM, 20))
NONFINITE_WINDOW = ((MARGIN, MARGIN), (RIM, RIM), (CHIP - RIM - 1, CHIP - RIM - 1), (20, RIM))


def nonfinite():
    """float32 chips with one NaN / +inf / -inf: in the rim (MI NaN, ZNCC finite) and in the window (all three NaN)."""
    rng = np.random.default_rng(7)
    out = []
    for group, spots in (("nonfinite_rim", NONFINITE_RIM), ("nonfinite_window", NONFINITE_WINDOW)):
        pairs = []
        for bad in (np.nan, np.inf, -np.inf):
            for pos in spots:
                for side in (0, 1):
                    pair = [noise(f32, rng, -100.0, 100.0), noise(f32, rng, 0.0, 1.0)]
                    pair[side][pos] = bad
                    pairs.append(tuple(pair))
        out.append(tile(group, group, pairs))
    return out


FLOAT_RANGES = ((0.0, 1.0), (0.1, 0.7), (-3.0e38, 3.0e38), (3.0e-45, 1.0e-40))


def float_edges():
    """float32 samples equal to float32(edge_i) of np.linspace(lo, hi, 33) and its two float32 neighbours."""
    rng = np.random.default_rng(33)
    pairs = []
    for lo, hi in FLOAT_RANGES:
        lo, hi = f32(lo), f32(hi)
        pair = []
        for _ in range(2):
            step = (float(hi) - float(lo)) / BINS
            v = [lo, hi]
            for i in range(1, BINS):
                e = f32(i * step + float(lo))
                v += [e, np.nextafter(e, f32(-np.inf)), np.nextafter(e, f32(np.inf))]
            c = noise(f32, rng, float(lo), float(hi)).ravel()
            c[:len(v)] = np.clip(np.array(v, f32), lo, hi)
            pair.append(rng.permutation(c).reshape(CHIP, CHIP))
        pairs.append(tuple(pair))
    # offset 1e6 with noise of a few float32 ulps (one ulp = 1 / 16)
    for _ in range(2):
        pairs.append(tuple((1.0e6 + rng.integers(-3, 4, (CHIP, CHIP)) / 16.0).astype(f32) for _ in range(2)))
    return [tile("float_edges", "edges", pairs)]


def placement(dtype):
    """One 64 x 70 raster pair, passed as column slices of wider arrays (row stride != width): key points at the first and last
    admissible centre and one step beyond, half-integer displacements, fractional and non-finite coordinates."""
    rng = np.random.default_rng(70)
    H, W = 64, 70
    tmin, tmax = limits(dtype)
    wide = [np.hstack([noise(dtype, rng), noise(dtype, rng)])[:, :W + 9] for _ in range(4)]
    ref = np.vstack([wide[0], wide[1]])[:H, 3:3 + W]
    mon = np.vstack([wide[2], wide[3]])[:H, 5:5 + W]
    assert ref.shape == (H, W) and mon.shape == (H, W) and ref.strides[0] != W * ref.itemsize
    pts = []
    xs, ys = (MARGIN - 1, MARGIN, W - MARGIN - 1, W - MARGIN), (MARGIN - 1, MARGIN, H - MARGIN - 1, H - MARGIN)
    for x in xs:
        for y in ys:
            pts.append((x, y, 0.0, 0.0))
    for d in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5):
        for x in (MARGIN, MARGIN + 1, 33, 34, W - MARGIN - 2, W - MARGIN - 1):
            pts.append((x, 30, d, 0.0))
        for y in (MARGIN, MARGIN + 1, 31, 32, H - MARGIN - 2, H - MARGIN - 1):
            pts.append((35, y, 0.0, d))
    for bad in (np.nan, np.inf, -np.inf):
        pts += [(35, 31, bad, 0.0), (35, 31, 0.0, bad), (bad, 31, 0.0, 0.0), (35, bad, 0.0, 0.0)]
    pts += [(28.9, 28.9, 0.0, 0.0), (27.99, 30, 0.0, 0.0), (41.99, 35.99, 0.0, 0.0), (42.0, 30, -1.0, 0.0), (30.25, 30.75, 0.25, -0.25),
            (-0.5, 30, 30.0, 0.0), (35, 31, 3.0e9, 0.0), (35, 31, -40.0, 0.0), (35, 31, 0.0, 6.0)]
    p = np.array(pts, np.float64).T.astype(f32)
    return [Case("placement", "placement", ref, mon, p[0], p[1], p[2], p[3])]


@functools.lru_cache(maxsize=None)
def fixtures(dtype):
    """Every case of a pixel type -> tuple of Case; the arrays are shared: do not write to them."""
    dt = np.dtype(dtype).type
    cases = []
    if dt is not np.float32:
        cases.append(sweep(dt)[0])
    cases += degenerate(dt) + zncc_extremes(dt) + placement(dt)
    if dt is np.float32:
        cases += nonfinite() + float_edges()
    for c in cases:
        for a in (c.ref, c.mon, c.x0, c.y0, c.dx, c.dy):
            a.flags.writeable = False
    return tuple(cases)


def groups(dtype):
    return tuple(dict.fromkeys(c.group for c in fixtures(dtype)))


@functools.lru_cache(maxsize=None)
def expected(dtype, group):
    """[(case, 3 x n float64: zncc, studholme, nmi)] of a group by the restatement - computed once, shared by the tests."""
    return tuple((c, scores(c.ref, c.mon, c.x0, c.y0, c.dx, c.dy)) for c in fixtures(dtype) if c.group == group)


# ---- ops.zncc_windows ---------------------------------------------------------------------------------------------------------------
Windows = collections.namedtuple("Windows", "name img1 img2 u1 v1 u2 v2")


@functools.lru_cache(maxsize=None)
def window_fixtures():
    """Image pairs of the other pixel types `ops.zncc_windows` reads, 47 x 49, with window centres for half-sizes 0 and 21."""
    rng = np.random.default_rng(2153)
    H, W = 47, 49
    y, x = np.mgrid[0:H, 0:W]
    out = []

    def add(name, a, b):
        u = np.array([21, 23, 25, 22, 21, 25], np.int32)
        v = np.array([21, 24, 27, 26, 27, 21], np.int32)
        out.append(Windows(name, a, b, u, v, u[::-1].copy(), v[::-1].copy()))
    add("uint32_near_2^32", ((1 << 32) - 1 - rng.integers(0, 1000, (H, W))).astype(np.uint32),
        ((1 << 32) - 1 - rng.integers(0, 3, (H, W))).astype(np.uint32))
    ends = np.where(rng.integers(0, 2, (H, W)) > 0, (1 << 31) - 1 - rng.integers(0, 100, (H, W)), -(1 << 31) + rng.integers(0, 100, (H, W)))
    add("int32_both_extremes", ends.astype(np.int32), np.where((x + y) % 2 == 0, -(1 << 31), (1 << 31) - 1).astype(np.int32))
    add("int64_within_2^53", rng.integers(-(1 << 53), (1 << 53) + 1, (H, W)), rng.integers(-(1 << 53), (1 << 53) + 1, (H, W)))
    board = np.where((x + y) % 2 == 0, 0, 255).astype(np.uint8)
    add("uint8_board_vs_float32", board, board.astype(f32))
    add("uint8_board_vs_inverse_float32", board, (255 - board).astype(f32))
    add("uint32_vs_int32", out[0].img1, out[1].img1)
    return tuple(out)


def windows_exact(w, half):
    """ZNCC of every window pair of a `Windows` case at a half-size, exact."""
    return np.array([zncc_exact(w.img1[a - half:a + half + 1, b - half:b + half + 1], w.img2[c - half:c + half + 1, d - half:d + half + 1])
                     for a, b, c, d in zip(w.u1, w.v1, w.u2, w.v2)], np.float64)
