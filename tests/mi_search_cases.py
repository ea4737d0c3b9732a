"""The shared case list of the mutual-information search (tests/test_mi_search_host.py: the stand-alone host program;
tests/test_gpu_mi_search.py: the kernels, numpy in and device tensors in).  Seeded and small: rasters of 120 x 160, each a window of a
wider buffer (row stride 165 pixels, as tests/zncc_search_cases.py pads them), at most 64 rows a case, radius 1 / 4 / 8, all four pixel
types.

content   "texture":  smoothed noise; `mon` = `ref` moved by (+3, -2) plus noise.  Both carry a constant block in their lower right
                      corner (a constant reference chip: bin 16; both chips constant: one cell, NaN at every offset, status 2) and `mon`
                      one pixel at the type's maximum and one at its minimum beside the chip of the row EXTREME: inside it at some offsets,
                      outside at others, so the range and every bin change across the surface (uint16: a range of 65535 where both are
                      inside; int16: values of both signs).  float32: one NaN in `ref` and one infinity in `mon`, each inside the chips
                      of a few rows only.
          "inverted": the same texture with the monitored copy contrast-inverted (hi - v): ZNCC is negative at the true offset.
          "binary":   two-valued rasters.
          "fullrange": uniform noise over the whole range of the type.
          "period4":  both rasters one 4 x 4 tile repeated: every chip recurs 4 offsets on, exact ties.
rows of a "texture" or "inverted" case, in this order while they last: the plain row (dx = dy = 0: the peak lands at (3, -2) from
          R = 4 on); the same texture moved beyond R (rim bits); key points exactly 28 px from each rim of `mon` (NaN columns or rows
          of the surface at every R); the row EXTREME; the constant reference chip; both chips constant; non-finite and out-of-range coordinates; rows
          one pixel short of the bounds rule; sums at .5; the rows whose chips hold the non-finite samples; then random rows.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name dtype radius n kind seed")
H, W, PAD = 120, 160, 5
SHIFT = (3, -2)              # `mon` is `ref` moved by this (x, y) in the "texture" and "inverted" cases
PLAIN = (50.0, 45.0)         # the plain row's key point: its chips lie clear of the constant blocks
EXTREME = (60.0, 75.0)       # the row beside whose monitored chip the two extreme pixels lie
BLOCK_REF, BLOCK_MON = 60, 68
NAN_AT, INF_AT = (8, 150), (100, 12)      # (row, column) of the float32 NaN in `ref` and of the infinity in `mon`


def cases():
    u8, u16, i16, f32 = np.uint8, np.uint16, np.int16, np.float32
    return [Case(*c) for c in (
        ("u16_texture_r4_n64", u16, 4, 64, "texture", 1),
        ("u16_texture_r8_n20", u16, 8, 20, "texture", 2),
        ("u16_texture_r1_n5", u16, 1, 5, "texture", 3),
        ("u8_texture_r1_n64", u8, 1, 64, "texture", 4),
        ("u8_texture_r4_n30", u8, 4, 30, "texture", 5),
        ("u8_texture_r8_n5", u8, 8, 5, "texture", 6),
        ("i16_texture_r4_n40", i16, 4, 40, "texture", 7),
        ("i16_texture_r8_n1", i16, 8, 1, "texture", 8),
        ("i16_texture_r1_n30", i16, 1, 30, "texture", 9),
        ("f32_texture_r4_n40", f32, 4, 40, "texture", 10),
        ("f32_texture_r8_n12", f32, 8, 12, "texture", 11),
        ("f32_texture_r1_n64", f32, 1, 64, "texture", 12),
        ("u16_inverted_r4_n12", u16, 4, 12, "inverted", 13),
        ("u8_inverted_r4_n5", u8, 4, 5, "inverted", 14),
        ("i16_inverted_r4_n5", i16, 4, 5, "inverted", 15),
        ("f32_inverted_r4_n5", f32, 4, 5, "inverted", 16),
        ("u8_binary_r4_n5", u8, 4, 5, "binary", 17),
        ("u16_binary_r8_n3", u16, 8, 3, "binary", 18),
        ("f32_binary_r1_n5", f32, 1, 5, "binary", 19),
        ("u16_fullrange_r4_n5", u16, 4, 5, "fullrange", 20),
        ("i16_fullrange_r4_n5", i16, 4, 5, "fullrange", 21),
        ("u8_fullrange_r1_n5", u8, 1, 5, "fullrange", 22),
        ("u16_period4_r4_n5", u16, 4, 5, "period4", 23),
        ("u8_period4_r8_n3", u8, 8, 3, "period4", 24),
        ("i16_period4_r4_n5", i16, 4, 5, "period4", 25),
        ("f32_period4_r4_n3", f32, 4, 3, "period4", 26),
        ("u16_n0", u16, 4, 0, "texture", 27),
        ("f32_n0", f32, 8, 0, "texture", 28),
    )]


def limits(dt):
    return (0.0, 1.0) if dt == np.float32 else (int(np.iinfo(dt).min), int(np.iinfo(dt).max))


def windowed(a):
    """The same pixels as a window of a wider buffer (odd row stride), the rest poisoned with the type's largest value."""
    buf = np.full((a.shape[0], a.shape[1] + PAD), np.iinfo(a.dtype).max if a.dtype.kind in "iu" else 1e30, a.dtype)
    buf[:, 2:2 + a.shape[1]] = a
    return buf[:, 2:2 + a.shape[1]]


def texture(rng):
    """Smoothed noise (3 x 3 box of unit normals), H x W, and the same field moved by SHIFT: mon[y, x] = ref[y - sy, x - sx]."""
    m = 8
    f = rng.normal(size=(H + 2 * m + 2, W + 2 * m + 2))
    f = sum(f[i:i + H + 2 * m, j:j + W + 2 * m] for i in range(3) for j in range(3)) / 3.0
    sx, sy = SHIFT
    return f[m:m + H, m:m + W], f[m - sy:m - sy + H, m - sx:m - sx + W]


def quantize(field, dtype, rng, noise):
    field = field + noise * rng.normal(size=field.shape)
    if dtype == np.float32:
        return (0.5 + 0.1 * field).astype(np.float32)
    if dtype == np.uint8:
        return np.clip(np.rint(128 + 22 * field), 0, 255).astype(np.uint8)
    if dtype == np.uint16:
        return np.clip(np.rint(30000 + 4000 * field), 0, 65535).astype(np.uint16)
    return np.clip(np.rint(3000 * field), -32768, 32767).astype(np.int16)


def rasters(case):
    rng = np.random.default_rng(case.seed)
    dt = np.dtype(case.dtype)
    lo, hi = limits(dt)
    if case.kind == "period4":
        tile = rng.integers(0, 200, (4, 4)) if dt != np.float32 else rng.integers(0, 200, (4, 4)) / 8.0
        ys, xs = np.mgrid[0:H, 0:W]
        ref = tile[ys % 4, xs % 4].astype(dt)
        mon = tile[(ys + 2) % 4, (xs - 3) % 4].astype(dt)           # mon[y, x] = ref[y + 2, x - 3]: moved by (+3, -2), and by every 4 beyond
    elif case.kind == "binary":
        a, b = texture(rng)
        v0, v1 = (0.25, 0.75) if dt == np.float32 else (lo + 3, hi - 5)
        ref, mon = np.where(a > 0, v1, v0).astype(dt), np.where(b > 0.1, v0, v1).astype(dt)
    elif case.kind == "fullrange":
        if dt == np.float32:
            ref, mon = rng.uniform(-3e38, 3e38, (H, W)).astype(dt), rng.uniform(-3e38, 3e38, (H, W)).astype(dt)
        else:
            ref, mon = rng.integers(lo, hi + 1, (H, W)).astype(dt), rng.integers(lo, hi + 1, (H, W)).astype(dt)
    else:
        a, b = texture(rng)
        ref, mon = quantize(a, dt, rng, 0.0), quantize(b, dt, rng, 0.05)
        if case.kind == "inverted":
            top = mon.max()
            mon = (top - mon).astype(dt) if dt != np.int16 else (-1 - mon).astype(dt)
        ref[H - BLOCK_REF:, W - BLOCK_REF:] = ref[H - 1, W - 1]
        mon[H - BLOCK_MON:, W - BLOCK_MON:] = mon[H - 1, W - 1]
        # beside the EXTREME row's chip (columns 32 .. 88 at offset 0): the maximum is inside from ox = 1 on, the minimum up to ox = 1
        px, py = int(EXTREME[0]), int(EXTREME[1])
        mon[py - 3, px + 29] = hi if dt != np.float32 else 2.0
        mon[py + 5, px - 27] = lo if dt != np.float32 else -1.0
        if dt == np.float32:
            ref[NAN_AT] = np.nan
            mon[INF_AT] = np.inf
    return windowed(ref), windowed(mon)


def rows(case):
    """-> float32 columns x0, y0, dx, dy of the case's rows."""
    rng = np.random.default_rng(1000 + case.seed)
    R, n = case.radius, case.n
    sx, sy = SHIFT
    lo, hx, hy = 28, W - 29, H - 29
    nan, inf = float("nan"), float("inf")
    special = [
        PLAIN + (0.0, 0.0),                                                            # plain: the peak at SHIFT from R = 4 on
        (66.0, 46.0, sx - (R + 2.0), sy), (66.0, 46.0, sx, sy + R + 2.0),              # the texture moved beyond R
        (lo, 50.0, 0.0, 0.0), (70.0, lo, 0.0, 0.0), (80.0, hy, 0.0, 0.0), (hx, 40.0, 0.0, 0.0),   # 28 px from each rim of `mon`
        EXTREME + (0.0, 0.0),                                                          # the extreme pixels enter and leave the chip
        (hx - 2.0, hy - 2.0, -(hx - 2.0 - 60.0), -(hy - 2.0 - 45.0)),                  # a constant reference chip against texture
        (hx - 2.0, hy - 2.0, 0.0, 0.0),                                                # both chips constant at every offset
        (nan, 40.0, 0.0, 0.0), (50.0, 40.0, inf, 0.0), (50.0, 40.0, 0.0, -inf), (3e9, 40.0, -3e9, 0.0), (50.0, -3e9, 0.0, 0.0),
        (27.9, 40.0, 0.0, 0.0), (50.0, 27.0, 0.0, 0.0), (W - 28.0, 40.0, 0.0, 0.0), (50.0, H - 28.0, 0.0, 0.0),
        (40.0, 40.0, -13.4, 0.0), (40.0, 40.0, 0.0, H - 68.4),                         # the sum leaves the range
        (60.0, 44.0, 2.5, -1.5), (61.0, 45.0, 3.5, -2.5), (62.0, 40.0, -0.5, 0.5),     # sums at .5
        (125.0, 30.0, -30.0, 20.0),                                                    # float32: the NaN lies in this reference chip
        (60.0, 50.0, -31.0 + R, 22.0),                                                 # float32: the infinity lies in some of these monitored chips
        (lo, lo, 0.0, 0.0), (hx, hy, -50.0, -30.0),                                    # two corners of the admissible range
    ]
    if case.kind not in ("texture", "inverted"):
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


FIELDS = ("offset", "peak", "peak_mi", "shift", "status")


def assert_matches(case, want, got, surface=True):
    """Every output byte for byte, for all four pixel types: no tolerance, no rows left out."""
    for field in FIELDS + (("surface",) if surface else ()):
        a, b = np.asarray(getattr(got, field)), np.asarray(getattr(want, field))
        assert a.dtype == b.dtype and a.shape == b.shape, (case.name, field, a.dtype, a.shape, b.shape)
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), \
            (case.name, field, np.argwhere(~((a == b) | ((a != a) & (b != b))))[:6].tolist())
