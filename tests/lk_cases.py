"""Inputs on which the LK tracker (csrc/k_lk.hip, k_lk2.hip) can be wrong without the geometry tests noticing: saturated contrast (the integer
ranges of the packed sums), windows at the eigenvalue cut, and start positions whose bilinear weights are degenerate or negative.
tests/test_lk_cases_host.py proves on the CPU that every fixture does what it is there for (with tests/lk_restatement.py),
tests/test_gpu_lk_extremes.py runs them through the kernels against `oracle.pyr_lk`.

Every fixture is a small uint8 pair (at most 160 x 200), key points and a window size.  Key points of the classes `saturated` and
`cut` sit at integer positions for odd windows and at k + 0.5 for even ones, so the template window's origin is an integer pixel and
the restatement applies.  All windows lie inside the image at both pyramid levels: a level that the oracle does not iterate on was
skipped by the cut, not by the image border.

Everything here is numpy on the CPU (the textured pair of `weights` takes its Laplacians from the oracle); nothing reads the library
under test.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import lk_restatement as R

SATURATED_WINDOWS = (25, 30, 31, 35, 36, 37, 38, 40)     # runs per lane (NR): 2 3 4 4 5 5 5 5
TAILORED_WINDOWS = (31, 33, 35)                          # NR = 4


@dataclass(frozen=True)
class Case:
    name: str
    cls: str                      # "saturated" | "cut" | "weights"
    win: int
    prev: np.ndarray              # uint8 image the key points belong to
    next: np.ndarray              # uint8 image they are tracked into
    pts: np.ndarray               # (N, 1, 2) float32
    info: dict = field(default_factory=dict, compare=False)

    def __str__(self):
        return f"{self.cls}/{self.name}/w{self.win}"


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _grid(win, ys, xs):
    """Key points whose template origin is an integer pixel: integers for odd windows, k + 0.5 for even ones."""
    off = 0.0 if win % 2 else 0.5
    return np.array([[x + off, y + off] for y in ys for x in xs], np.float32).reshape(-1, 1, 2)


# ---------------------------------------------------------------------------------------------------------------- saturated
def row_stripes(rows, h=120, w=120, brk=60, shift=2):
    """0 / 255 rows following the periodic pattern `rows`; columns >= brk are `shift` rows ahead, which gives a window across the
    break some x-gradient (it passes the eigenvalue cut)."""
    a = np.asarray(rows, np.uint8)
    r, c = np.arange(h)[:, None], np.arange(w)[None, :]
    return a[(r + shift * (c >= brk)) % len(a)]


PERIOD4 = (255, 255, 0, 0)
# Tailored to NR = 4 (winSize 31 .. 35, 7 runs per row): lanes 0 .. 3 hold runs of window rows 0, 9, 18, 27.  A row contributes the
# largest product 8160 x 4080 to the y-component when (row above, row, row below) is (255, 255, 0) or (0, 0, 255) and the search image
# holds the opposite value there; such rows can be 2 or 3 apart but not adjacent, so a period of 9 rows with contributing rows
# 0, 2, 4, 6 puts all four rows of those lanes on a contributing row for one window origin in nine.  The search image that holds
# the opposite value on exactly the contributing rows IS the pattern moved up by one row.
PERIOD9 = (255, 0, 0, 255, 255, 0, 0, 255, 255)


@functools.lru_cache(maxsize=None)
def _saturated_scenes():
    r, c = np.arange(120)[:, None], np.arange(120)[None, :]
    s4 = row_stripes(PERIOD4)
    chk = (255 * (((r // 2) + (c // 2)) % 2)).astype(np.uint8)
    blk = (np.kron(np.random.default_rng(7).integers(0, 2, (30, 30)), np.ones((4, 4), np.int64)) * 255).astype(np.uint8)
    s9 = row_stripes(PERIOD9, shift=4)
    scenes = {
        "stripes": (s4, np.roll(s4, -1, 0)),
        "stripes_t": (np.ascontiguousarray(s4.T), np.ascontiguousarray(np.roll(s4, -1, 0).T)),
        "checker": (chk, np.roll(chk, (-1, -1), (0, 1))),
        "blocks": (blk, np.roll(blk, -1, 1)),
        "stripes9": (s9, np.roll(s9, -1, 0)),
    }
    for pair in scenes.values():
        _frozen(*pair)
    return scenes


def saturated_cases():
    out = []
    for name, (a, b) in _saturated_scenes().items():
        for win in (TAILORED_WINDOWS if name == "stripes9" else SATURATED_WINDOWS):
            # nine consecutive rows: every phase of the period-4 and the period-9 rows; columns on both sides of the break
            pts = _grid(win, range(52, 61), range(52, 69, 4))
            if name == "stripes_t":
                pts = np.ascontiguousarray(pts[:, :, ::-1])
            out.append(Case(name, "saturated", win, a, b, pts))
    return out


# ---------------------------------------------------------------------------------------------------------------------- cut
CUT_H, CUT_W = 160, 200
NEAR = 0.01                        # "near the cut": restated minEig within 1 % of 1e-4


def sparse_noise(amp, lo, hi, seed):
    """Flat 128 with independent +-amp pixels whose density rises from `lo` (left) to `hi` (right)."""
    rho = np.linspace(lo, hi, CUT_W)[None, :]
    u = np.random.default_rng(seed).random((CUT_H, CUT_W))
    return (128 + np.where(u < rho / 2, -amp, np.where(u < rho, amp, 0))).astype(np.uint8)


def _inside_both_levels(win):
    """Integer template origins (x, y) of level 0 whose windows (+ the derivative's and the search's extra pixels, + 3 px of
    movement) lie inside the image at level 0 and at level 1 -> boolean map over origins, entry [y, x]."""
    half = (win - 1) / 2
    ys, xs = np.mgrid[0:CUT_H - win + 1, 0:CUT_W - win + 1]
    ok = np.ones(ys.shape, bool)
    for o, n in ((xs, CUT_W), (ys, CUT_H)):
        ok &= (o >= 5) & (o + win + 5 <= n)
        o1 = np.floor((o + half) / 2 - half)
        ok &= (o1 >= 5) & (o1 + win + 5 <= (n + 1) // 2)
    return ok


def _near_cut_points(img, win, seed, n_side=24, n_far=12):
    """Key points of `img` by restated level-0 minEig: the `n_side` windows nearest to the cut on each side of it, and `n_far` others."""
    m = R.cut_map(img, win)
    e = m["minEig"].astype(np.float64)
    ok = _inside_both_levels(win)
    rel = np.where(ok, np.abs(e / 1e-4 - 1), np.inf)
    picks = []
    for side in (m["tracked"], ~m["tracked"]):
        cand = np.argwhere(side & (rel <= NEAR))
        order = np.argsort(rel[cand[:, 0], cand[:, 1]], kind="stable")
        picks.append(cand[order[:n_side]])
    rng = np.random.default_rng(seed)
    for side in (m["tracked"], ~m["tracked"]):
        far = np.argwhere(side & ok & (rel > 10 * NEAR))
        picks.append(far[rng.choice(len(far), n_far // 2, replace=False)])
    yx = np.concatenate(picks)
    half = np.float32(win - 1) * np.float32(0.5)
    return (yx[:, ::-1].astype(np.float32) + half).reshape(-1, 1, 2)


def _by_determinant_sign(img, win, n_each=16):
    """Key points of `img` whose restated float32 determinant is negative, zero and positive: the first `n_each` of each in row order."""
    m = R.cut_map(img, win)
    ok = _inside_both_levels(win)
    yx = np.concatenate([np.argwhere(ok & sel)[:n_each] for sel in (m["D"] < 0, m["D"] == 0, m["D"] > 0)])
    return (yx[:, ::-1].astype(np.float32) + np.float32(win - 1) * np.float32(0.5)).reshape(-1, 1, 2)


def _levels_scene():
    """Random 0 / 255 blocks with a flat 31 x 31 hole around (70, 80) and nothing but 128 from column 130 on."""
    img = (np.kron(np.random.default_rng(11).integers(0, 2, (40, 50)), np.ones((4, 4), np.int64)) * 255).astype(np.uint8)
    img[80 - 15:80 + 16, 70 - 15:70 + 16] = 128
    img[:, 130:] = 128
    return img


LEVELS_POINTS = {
    "only level 1": [(69, 79), (70, 80), (71, 81)],            # the level-0 window (and its derivative ring) is inside the hole
    "both": [(40, 40), (100, 45), (45, 120), (101, 121)],
    "none": [(164, 50), (168, 80), (170, 110)],
}


@functools.lru_cache(maxsize=None)
def cut_cases():
    out = []
    for name, amp, lo, hi, win, seed in (("noise1", 1, 0.30, 0.75, 25, 5), ("noise2", 2, 0.08, 0.30, 31, 6), ("noise1", 1, 0.30, 0.75, 38, 5),
                                         ("noise2", 2, 0.08, 0.30, 30, 6)):
        img = sparse_noise(amp, lo, hi, seed)
        mon = np.roll(img, 1, 1)
        _frozen(img, mon)
        out.append(Case(name, "cut", win, img, mon, _near_cut_points(img, win, seed), {"near": True}))
    r, c = np.arange(CUT_H)[:, None], np.arange(CUT_W)[None, :]
    dots = (255 * (((r + c) // 3) % 2)).astype(np.uint8)
    dots[40:120:23, 45:150:29] ^= 1                   # about one pixel per window one grey level off: the determinant is what rounding leaves
    stripes = {
        "stripes_h": (128 + 20 * ((r // 3) % 2) + 0 * c).astype(np.uint8),
        "stripes_v": (128 + 20 * ((c // 3) % 2) + 0 * r).astype(np.uint8),
        "stripes_d": (128 + 20 * (((r + c) // 3) % 2)).astype(np.uint8),
        "stripes_d_dots": dots,
    }
    for name, img in stripes.items():
        mon = np.roll(img, (1, 1), (0, 1))
        _frozen(img, mon)
        rounding = name == "stripes_d_dots"
        pts = _by_determinant_sign(img, 25) if rounding else _grid(25, range(60, 100, 7), range(60, 130, 9))
        out.append(Case(name, "cut", 25, img, mon, pts, {"rounding": True} if rounding else {"singular": True}))
    lev = _levels_scene()
    mon = np.roll(lev, 1, 1)
    _frozen(lev, mon)
    out.append(Case("levels", "cut", 25, lev, mon, np.array(sum(LEVELS_POINTS.values(), []), np.float32).reshape(-1, 1, 2)))
    s4 = _saturated_scenes()["stripes"]
    out.append(Case("stripes4", "cut", 25, s4[0], s4[1], _grid(25, range(56, 60), range(56, 65, 4)), {"only level 0": True}))
    # the forward template is textured, the search image flat: wherever the forward pass ends, the backward template is flat
    tex = (np.kron(np.random.default_rng(12).integers(0, 2, (40, 50)), np.ones((4, 4), np.int64)) * 255).astype(np.uint8)
    flat = np.full_like(tex, 128)
    _frozen(tex, flat)
    out.append(Case("flat_return", "cut", 25, tex, flat, _grid(25, range(60, 100, 13), range(60, 140, 17)), {"flat_return": True}))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------ weights
# (a, b) in units of 2^-16 - exact in float32 when added to a key-point coordinate below 256 - and the weights they give.
# The first six have w11 == -1: the three rounded weights sum to 16385.
U = 1.0 / 65536
FRACTIONS = (
    ((35 * U, 1115 * U), (16097, 9, 279, -1)),
    ((707 * U, 75 * U), (16189, 177, 19, -1)),
    ((539 * U, 15 * U), (16246, 135, 4, -1)),
    ((35 * U, 555 * U), (16237, 9, 139, -1)),
    ((7 * U, 895 * U), (16159, 2, 224, -1)),
    ((203 * U, 215 * U), (16280, 51, 54, -1)),
    ((0.0, 0.0), (16384, 0, 0, 0)),                       # MODE 2: no interpolation
    ((100 * U, 0.0), (16359, 25, 0, 0)),                  # MODE 1: one bilinear row
    ((0.0, 100 * U), (16359, 0, 25, 0)),                  # MODE 0
) + tuple(((i / 4, j / 4), tuple(int(v * 1024) for v in ((4 - i) * (4 - j), i * (4 - j), (4 - i) * j, i * j)))
          for i in range(4) for j in range(4) if (i, j) != (0, 0))
# the example of the issue that asked for these tests (float32 values that are no multiple of 2^-16: checked as weights only)
EXAMPLE = ((0.003826478496193886, 0.0016310523496940732), (16295, 63, 27, -1))
# integer template origins: both parities per axis, so that level 1 (half the coordinate) meets fractions 0 and 1/2 plus half of (a, b)
WEIGHT_ORIGINS = tuple((x, y) for y in (48, 49, 71) for x in (58, 59, 90))
WEIGHT_WINDOWS = (25, 30, 38)


@functools.lru_cache(maxsize=None)
def _textured_pair():
    from karios_amd import synth
    from oracle import oracle as O
    mon, ref = synth.make_pair(160, 200, 0.4, -0.3, seed=20260412)
    return _frozen(O.laplacian_u8(O.to_uint8(ref), 7), O.laplacian_u8(O.to_uint8(mon), 7))


def weight_points(win):
    """-> ((N, 1, 2) float32 start positions origin + half + (a, b), the weight quadruple claimed for each at level 0)."""
    half = (win - 1) / 2
    pts, claims = [], []
    for ox, oy in WEIGHT_ORIGINS:
        for (a, b), w in FRACTIONS:
            pts.append((ox + half + a, oy + half + b))
            claims.append(w)
    if win % 2 == 0:
        # integer positions under an even window: fractions (1/2, 1/2) at level 0, and at level 1 (0, 0), (1/2, 0), (0, 1/2), (1/2, 1/2)
        # by the parities - the only way an even window meets MODE 2 and MODE 1 there
        for x, y in ((73, 63), (74, 63), (73, 64), (74, 64)):
            pts.append((x, y))
            claims.append((4096, 4096, 4096, 4096))
    return np.array(pts, np.float64).astype(np.float32).reshape(-1, 1, 2), claims


def weights_cases():
    ref, mon = _textured_pair()
    out = []
    for win in WEIGHT_WINDOWS:
        pts, claims = weight_points(win)
        out.append(Case("textured", "weights", win, ref, mon, pts, {"claims": claims}))
    return out


# -------------------------------------------------------------------------------------------------------------- raw pairs
# uint8 pairs for the entry points that start from pixels (stretch -> Laplacian -> corners -> tracker).  Pixel value 0 is "no data"
# to the automatic mask, so the dark value is 1.  Rows 1 1 255 255: the ksize-3 Laplacian 4 (a[r-1] + a[r+1] - 2 a[r]) saturates to
# 254 / 0 rows, i.e. the Laplacian images are the striped scene again; corners exist only at the phase breaks (every 64 columns).
FRAME_KSIZE = 3
RAW_WIN = 37                                     # odd: integer corners give integer template origins (the restatement applies)
UNIT_BOXES = ((0, 0, 512, 96), (8, 10, 520, 97))     # (x, y, w, h) in the raw striped pair
UNIT_MAX_CORNERS = 100                           # fewer than a unit has (112, 136)


@functools.lru_cache(maxsize=None)
def raw_stripes_pair(h=120, w=540):
    r, c = np.arange(h)[:, None], np.arange(w)[None, :]
    ref = np.where((r + 2 * ((c // 64) % 2)) % 4 < 2, 1, 255).astype(np.uint8)
    return _frozen(ref, np.roll(ref, -1, 0))


@functools.lru_cache(maxsize=None)
def raw_blocks_pair(h=160, w=200):
    ref = (np.kron(np.random.default_rng(13).integers(0, 2, (h // 4, w // 4)), np.ones((4, 4), np.int64)) * 254 + 1).astype(np.uint8)
    return _frozen(ref, np.roll(ref, 1, 1))


def all_cases():
    return saturated_cases() + list(cut_cases()) + weights_cases()


def case_ids():
    """Names of `all_cases()` without building the textured pair (which takes the oracle): for collecting parametrised tests."""
    return [str(c) for c in saturated_cases() + list(cut_cases())] + [f"weights/textured/w{w}" for w in WEIGHT_WINDOWS]


@functools.lru_cache(maxsize=None)
def _by_id():
    return {str(c): c for c in all_cases()}


def case(case_id):
    return _by_id()[case_id]


def level0_start(O, case):
    """Where the first level-0 iteration of `case` searches: twice the result of level 1 (the oracle on the two level-1 images with
    the halved key points and no further level) -> (N, 2) float32 window CENTRES."""
    p = np.asarray(case.pts, np.float32).reshape(-1, 2)
    out = O.pyr_lk(O.pyrdown_u8(case.prev), O.pyrdown_u8(case.next), p * np.float32(0.5), case.win, max_level=0)
    return out.reshape(-1, 2) * np.float32(2)
