"""The shared case list of the ZNCC search (tests/test_zncc_search_host.py: the stand-alone host program; tests/test_gpu_zncc_search.py:
the kernels, numpy in and device tensors in).  Seeded, small, and built so that every path of the kernel is taken:

rasters   96 x 120 and 128 x 160, each a window of a wider buffer (row strides 127 and 165 pixels: odd); all four pixel types
radius    1, 4, 8 (3, 9, 17 lanes per group; 21, 7, 3 groups; the last round of groups partly idle at 4 and 8)
rows      0, 1, 5, 300 (a workgroup with 1 of 4 waves at work; XCD shares of 1 and 0 workgroups; 75 workgroups over 8 XCDs)
content   "texture": smoothed noise, `mon` = `ref` moved by (+3, -2) plus noise, so surfaces have one clear peak (the float32 cases stay
          under the 1 % cap on rows without a clear peak or curvature: asserted by the host test); a flat block in `mon` (offsets
          without a value, missing neighbours) and one in `ref` (a template without variance: status 2)
          "period4": both rasters one 4 x 4 tile repeated (integer types): every value recurs 4 offsets on, exact ties
          "extreme": pixels at the ends of the type's range only: the largest moments the accumulators meet
rows of a "texture" case, in this order while they last: one plain row; the four corners of the admissible range (at radius 8 the
          square crosses each border there); skipped rows (NaN, inf, one pixel short of the 57 x 57 chip rule on each side, a sum that
          rounds out of range); a flat template; rows over the flat block of `mon`; sums at .5 (half to even); rows whose KLT
          displacement is off by more than the radius (peak on the rim); then random rows.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name dtype H W radius n kind seed")
SHIFT = (3, -2)              # `mon` is `ref` moved by this (x, y) in the "texture" cases
PAD = {120: 7, 160: 5}       # the wider buffer: W + PAD columns


def cases():
    u8, u16, i16, f32 = np.uint8, np.uint16, np.int16, np.float32
    return [Case(*c) for c in (
        ("u16_128x160_r4_n300", u16, 128, 160, 4, 300, "texture", 1),
        ("u16_96x120_r8_n300", u16, 96, 120, 8, 300, "texture", 2),
        ("u16_96x120_r1_n5", u16, 96, 120, 1, 5, "texture", 3),
        ("u8_96x120_r1_n300", u8, 96, 120, 1, 300, "texture", 4),
        ("u8_128x160_r8_n5", u8, 128, 160, 8, 5, "texture", 5),
        ("u8_96x120_r4_n1", u8, 96, 120, 4, 1, "texture", 6),
        ("i16_128x160_r4_n300", i16, 128, 160, 4, 300, "texture", 7),
        ("i16_96x120_r8_n1", i16, 96, 120, 8, 1, "texture", 8),
        ("f32_128x160_r4_n300", f32, 128, 160, 4, 300, "texture", 9),
        ("f32_96x120_r8_n300", f32, 96, 120, 8, 300, "texture", 10),
        ("f32_96x120_r1_n5", f32, 96, 120, 1, 5, "texture", 11),
        ("f32_128x160_r4_n1", f32, 128, 160, 4, 1, "texture", 12),
        ("u16_period4_r4_n5", u16, 128, 160, 4, 5, "period4", 13),
        ("u8_period4_r8_n5", u8, 96, 120, 8, 5, "period4", 14),
        ("i16_period4_r4_n5", i16, 96, 120, 4, 5, "period4", 15),
        ("u16_extreme_r4_n5", u16, 96, 120, 4, 5, "extreme", 16),
        ("i16_extreme_r8_n5", i16, 96, 120, 8, 5, "extreme", 17),
        ("u8_extreme_r1_n5", u8, 96, 120, 1, 5, "extreme", 18),
        ("u16_n0", u16, 96, 120, 4, 0, "texture", 19),
        ("f32_n0", f32, 96, 120, 8, 0, "texture", 20),
    )]


def windowed(a):
    """The same pixels as a window of a wider buffer (odd row stride), the rest poisoned with the type's largest value."""
    H, W = a.shape
    buf = np.full((H, W + PAD.get(W, 3)), np.iinfo(a.dtype).max if a.dtype.kind in "iu" else 1e30, a.dtype)
    buf[:, 2:2 + W] = a
    return buf[:, 2:2 + W]


def texture(rng, H, W):
    """Smoothed noise (3 x 3 box of unit normals), H x W, and the same field moved by SHIFT: mon[y, x] = ref[y - sy, x - sx]."""
    m = 8
    f = rng.normal(size=(H + 2 * m + 2, W + 2 * m + 2))
    f = sum(f[i:i + H + 2 * m, j:j + W + 2 * m] for i in range(3) for j in range(3)) / 3.0
    sx, sy = SHIFT
    return f[m:m + H, m:m + W], f[m - sy:m - sy + H, m - sx:m - sx + W]


def quantize(field, dtype, rng, noise):
    field = field + noise * rng.normal(size=field.shape)
    if dtype == np.float32:
        return (0.5 + 0.2 * field).astype(np.float32)
    if dtype == np.uint8:
        return np.clip(np.rint(128 + 40 * field), 0, 255).astype(np.uint8)
    if dtype == np.uint16:
        return np.clip(np.rint(20000 + 6000 * field), 0, 65535).astype(np.uint16)
    return np.clip(np.rint(3000 * field), -32768, 32767).astype(np.int16)


def rasters(case):
    rng = np.random.default_rng(case.seed)
    H, W, dt = case.H, case.W, np.dtype(case.dtype)
    if case.kind == "period4":
        lo, hi = (np.iinfo(dt).min, np.iinfo(dt).max)
        tile = rng.integers(lo // 2, hi // 2, (4, 4))
        ys, xs = np.mgrid[0:H, 0:W]
        ref = tile[ys % 4, xs % 4].astype(dt)
        mon = tile[(ys + 2) % 4, (xs - 3) % 4].astype(dt)       # mon[y, x] = ref[y + 2, x - 3]: moved by (+3, -2), and by every 4 beyond
    elif case.kind == "extreme":
        lo, hi = (np.iinfo(dt).min, np.iinfo(dt).max)
        ref = np.where(rng.random((H, W)) < 0.9, hi, lo).astype(dt)
        mon = np.where(rng.random((H, W)) < 0.9, hi, lo).astype(dt)
    else:
        a, b = texture(rng, H, W)
        ref, mon = quantize(a, dt, rng, 0.0), quantize(b, dt, rng, 0.05)
        # (float32: values whose sums are exact, so that "no variance" does not depend on the order of a summation)
        mon[0:52, 0:62] = 0.5 if dt == np.float32 else mon[0, 0]                     # offsets without a value
        ref[H - 50:, W - 50:] = 0.25 if dt == np.float32 else ref[H - 1, W - 1]      # a template without variance at (W - 29, H - 29)
    return windowed(ref), windowed(mon)


def rows(case):
    """-> float32 columns x0, y0, dx, dy of the case's rows."""
    rng = np.random.default_rng(1000 + case.seed)
    H, W, R, n = case.H, case.W, case.radius, case.n
    sx, sy = SHIFT
    lo, hx, hy = 28, W - 29, H - 29
    nan, inf = float("nan"), float("inf")
    special = [
        (70.0, 45.0, sx + 0.3, sy - 0.2),                                              # plain
        (lo, lo, 0.0, 0.0), (hx, lo, 0.0, 0.0), (lo, hy, 0.0, 0.0), (hx, hy, 0.0, 0.0),   # the four corners of the admissible range
        (hx, 40.0, 0.2, 0.0), (60.0, hy, 0.0, -0.2),                                   # the right and the lower border over texture
        (nan, 40.0, 0.0, 0.0), (50.0, 40.0, inf, 0.0), (50.0, 40.0, 0.0, -inf), (3e9, 40.0, -3e9, 0.0),
        (27.9, 40.0, 0.0, 0.0), (50.0, 27.0, 0.0, 0.0), (W - 28.0, 40.0, 0.0, 0.0), (50.0, H - 28.0, 0.0, 0.0),
        (40.0, 40.0, -13.4, 0.0), (40.0, 40.0, 0.0, H - 68.4),                         # the sum leaves the range
        (hx + 0.7, hy + 0.2, -6.0, -5.0),                                              # the flat template
        (34.0, 30.0, 0.2, -0.3), (40.0, 31.0, -2.0, 1.0), (31.0, 33.0, 4.0, 2.0),      # over the flat block of `mon`
        (60.0, 44.0, 2.5, -1.5), (61.0, 45.0, 3.5, -2.5), (62.0, 40.0, -0.5, 0.5),     # sums at .5
        (66.0, 46.0, sx - (R + 2.0), sy), (66.0, 46.0, sx, sy + R + 2.0), (58.0, 42.0, sx + R, sy - R),   # the peak beyond / on the rim
    ]
    if case.kind != "texture":
        special = [(64.0, 44.0, 0.0, 0.0), (47.0, 39.0, 1.2, -0.7), (lo, lo, 0.0, 0.0), (hx - 1.0, hy - 2.0, 0.6, 0.6), (nan, 1.0, 0.0, 0.0)]
    if n == 1:
        special = [(57.0, 41.0, sx - 0.4, sy + 1.3)]
    out = np.array(special[:n], np.float32).reshape(-1, 4)
    if n > len(out):
        m = n - len(out)
        x0 = np.floor(rng.uniform(lo + 6, hx - 6, m))
        y0 = np.floor(rng.uniform(lo + 6, hy - 6, m))
        more = np.stack([x0, y0, sx + rng.uniform(-2.5, 2.5, m), sy + rng.uniform(-2.5, 2.5, m)], axis=1).astype(np.float32)
        out = np.concatenate([out, more[np.lexsort((more[:, 1], more[:, 0]))]])       # frames are ordered by (x0, y0)
    return tuple(np.ascontiguousarray(out[:, i]) for i in range(4))


def build(case):
    """-> (ref, mon, x0, y0, dx, dy)"""
    return rasters(case) + rows(case)


# ---- how a result is held to the restatement's (`want`: zncc_search_restatement.Result with the surface; `got`: the same fields as numpy arrays)
VALUE_TOL, GAP_MIN, DEN_MIN, SHIFT_TOL, CAP = 1e-9, 2e-9, 1e-3, 1e-5, 0.01


def unclear_rows(want, radius):
    """float32: the rows whose offset or shift is NOT compared - the two largest values lie within twice the value tolerance of each
    other, or a parabola's |den| < 1e-3 (1e-9 per value moves the step by 0.5 (2e-9 + 4e-9) / 1e-3 = 3e-6 < SHIFT_TOL at that bound)."""
    import zncc_search_restatement as R
    out = np.zeros(len(want.status), bool)
    for k in np.flatnonzero((want.status & (R.SKIPPED | R.NO_VALUE)) == 0):
        dens = R.axis_denominators(want.surface[k], want.offset[k], radius)
        out[k] = R.top_two_gap(want.surface[k]) <= GAP_MIN or any(d is not None and abs(d) < DEN_MIN for d in dens)
    return out


def assert_matches(case, want, got, surface=True):
    """Integer pixel types: every output byte for byte.  float32: values within 1e-9 with the same NaN pattern; offsets and status
    equal and shifts within 1e-5 on the rows that are not `unclear_rows`, which may be at most 1 % of the case."""
    name = case.name
    assert got.offset.shape == want.offset.shape and got.offset.dtype == np.int32 and got.status.dtype == np.uint8, name
    assert got.peak.dtype == np.float64 and got.shift.dtype == np.float64 and got.shift.shape == want.shift.shape, name
    if np.dtype(case.dtype) != np.float32:
        for field in ("offset", "peak", "shift", "status") + (("surface",) if surface else ()):
            a, b = getattr(got, field), getattr(want, field)
            assert a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b, a.dtype).tobytes(), (name, field, np.argwhere(~((a == b) | ((a != a) & (b != b))))[:6])
        return
    if surface:
        assert np.array_equal(np.isnan(got.surface), np.isnan(want.surface)), name
        assert case.n == 0 or np.nanmax(np.abs(got.surface - want.surface), initial=0.0) <= VALUE_TOL, name
    assert np.array_equal(np.isnan(got.peak), np.isnan(want.peak)) and np.array_equal(np.isnan(got.shift), np.isnan(want.shift)), name
    assert np.nanmax(np.abs(got.peak - want.peak), initial=0.0) <= VALUE_TOL, name
    done = (want.status & 3) != 0
    assert np.array_equal(got.status[done], want.status[done]) and not got.offset[done].any(), name
    clear = ~unclear_rows(want, case.radius)
    assert (~clear).sum() <= CAP * case.n, (name, int((~clear).sum()))
    assert np.array_equal(got.offset[clear], want.offset[clear]) and np.array_equal(got.status[clear], want.status[clear]), name
    live = clear & ~done
    assert np.max(np.abs(got.shift[live] - want.shift[live]), initial=0.0) <= SHIFT_TOL, name
