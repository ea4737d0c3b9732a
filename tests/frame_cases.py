"""TEST INFRASTRUCTURE - named, seeded inputs of the frame stage alone (tests/test_frame_host.py, tests/test_gpu_frame.py): the places
where the forward-backward cut, the score, the compaction and the (x0, y0) placement of k_frame.hip can be wrong and where real tracker
output never lands.

A case is a list of `Call`s that run in order on ONE context; a call is what `ops.frame_from_tracks(units, n_max, cap)` takes.  Every
builder asserts its own preconditions (the ulp neighbours of the threshold occur, the ties occur, ...): a case that no longer holds
what its name says fails where it is built, not silently.  Every call stays under 100 000 rows.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

F = np.float32
THR = F(0.1)
BELOW, ABOVE = np.nextafter(THR, F(0)), np.nextafter(THR, F(1))
TINY = np.nextafter(F(0), F(1))                   # 2^-149, the smallest denormal
SUB = F(1e-40)                                    # a denormal


@dataclass
class Call:
    units: list
    n_max: int
    cap: int
    refused: bool = False                         # the library answers KM_E_UNSUPPORTED
    note: str = ""
    each_alone: bool = False                      # every unit also equals the same unit submitted alone
    facts: dict = field(default_factory=dict)


def unit(p0, p1, p0r, n=None, x_off=0, y_off=0, width=0):
    p0, p1, p0r = (np.ascontiguousarray(a, F).reshape(-1, 2) for a in (p0, p1, p0r))
    assert p0.shape == p1.shape == p0r.shape
    return {"p0": p0, "p1": p1, "p0r": p0r, "n": len(p0) if n is None else int(n), "x_off": x_off, "y_off": y_off, "width": int(width)}


def tracks(x, y, ex, ey, n=None, **kw):
    """Corners (x, y) tracked to (x + 0.5, y - 0.25) and back to (x + ex, y + ey), every sum rounded to float32."""
    x, y, ex, ey = (np.asarray(a, F) for a in np.broadcast_arrays(np.asarray(x, F), np.asarray(y, F), np.asarray(ex, F), np.asarray(ey, F)))
    with np.errstate(all="ignore"):
        p0 = np.stack([x, y], 1)
        return unit(p0, p0 + F([0.5, -0.25]), np.stack([x + ex, y + ey], 1), n, **kw)


@np.errstate(all="ignore")
def distance(u):
    """The forward-backward distance of the live rows as float32 arithmetic gives it."""
    n = len(u["p0"]) if u["n"] < 0 else min(u["n"], len(u["p0"]))
    return np.abs(u["p0"][:n] - u["p0r"][:n]).max(1)


def kept(u):
    return int((distance(u) < THR).sum())


def distinct_corners(rng, m, width, height=65536):
    """m distinct integer corners with x < width, one of them in column width - 1, in random order."""
    assert m <= width * height
    keys = np.unique(rng.integers(0, width * height, 2 * m + 64))
    while keys.size < m:
        keys = np.unique(np.concatenate([keys, rng.integers(0, width * height, 2 * m + 64)]))
    keys = rng.permutation(keys)[:m]
    x, y = keys // height, keys % height
    if not (x == width - 1).any():
        taken = set(y[x == width - 1].tolist())
        x[0], y[0] = width - 1, next(v for v in range(height) if v not in taken)
    assert len(set(zip(x.tolist(), y.tolist()))) == m
    return x.astype(F), y.astype(F)


def mixed(rng, x, y, share=0.5):
    """Errors that keep about `share` of the rows: 0.05 px for the kept ones, 0.5 px for the others, in x or in y."""
    keep = rng.random(len(x)) < share
    e = np.where(keep, F(0.05), F(0.5)) * rng.choice(F([-1, 1]), len(x))
    in_x = rng.random(len(x)) < 0.5
    return np.where(in_x, e, F(0)).astype(F), np.where(in_x, F(0), e).astype(F)


# ------------------------------------------------------------------ the cut at the threshold
def cut():
    ds = [F(0), F(-0.0), TINY, SUB, BELOW, THR, ABOVE, F(np.inf), F(np.nan)]
    x, y, ex, ey = [], [], [], []
    row = 1
    for d in ds:
        half = F(0.05) if not np.isfinite(d) else d / F(2)
        for sign in (F(1), F(-1)):
            for cx, cy, a, b in ((0, row, d, 0), (row, 0, 0, d), (0, 0, d, half), (0, 0, half, d)):     # x alone, y alone, larger first, larger second
                x.append(cx); y.append(cy); ex.append(sign * F(a)); ey.append(sign * F(b))
            row += 1
    at_zero = tracks(x, y, ex, ey)
    d0 = distance(at_zero)
    for want in (TINY, SUB, BELOW, THR, ABOVE):
        assert (d0 == want).sum() >= 8, f"distance {want!r} occurs {(d0 == want).sum()} times beside a corner at 0"
    assert np.isnan(d0).sum() >= 8 and np.isinf(d0).sum() >= 8
    # a NaN in one component beside a small finite error in the other: numpy's max returns the NaN, the row is dropped
    nan_rows = tracks([0, 0, 3, 4], [5, 6, 0, 0], [np.nan, 0.05, np.nan, 0.05], [0.05, np.nan, 0.0, np.nan])
    assert np.isnan(distance(nan_rows)).all()
    # larger corners: p0r is rounded where it is stored, the distance is what the subtraction then yields - the float32 values next to
    # corner +- 0.1f, three either side
    cx, cy, ex, ey = [], [], [], []
    for c in (1, 7, 100, 1000, 10979, 65535):
        for side in (F(1), F(-1)):
            centre = F(c) + side * THR
            near = [centre]
            for _ in range(3):
                near = [np.nextafter(near[0], F(-np.inf))] + near + [np.nextafter(near[-1], F(np.inf))]
            for k, v in enumerate(near):
                in_x = k % 2 == 0
                cx.append(c if in_x else 2 * c + k); cy.append(2 * c + k if in_x else c)
                ex.append(v - F(c) if in_x else 0); ey.append(0 if in_x else v - F(c))
    larger = tracks(cx, cy, ex, ey)
    dl = distance(larger).reshape(6, 14)
    for i, c in enumerate((1, 7, 100, 1000, 10979, 65535)):
        assert (dl[i] < THR).any() and (dl[i] >= THR).any(), f"corner {c}: the stored p0r values do not straddle the threshold"
    return [Call([at_zero], len(x), len(x), note="beside a corner at 0"), Call([nan_rows], 4, 4, note="NaN in one component"),
            Call([larger], len(cx), len(cx), note="larger corners")]


def score_sweep():
    rng = np.random.default_rng(20261)
    thr_bits = int(THR.view(np.uint32))
    last = (thr_bits - np.arange(1, 257)).astype(np.uint32).view(F)                      # the last 256 values below 0.1f
    powers = np.ldexp(F(1), np.arange(-149, -3)).astype(F)
    around = np.concatenate([np.nextafter(powers, F(0)), powers, np.nextafter(powers, F(1))])
    uniform = (rng.random(4096) * 0.1).astype(F)
    uniform = uniform[uniform < THR]
    any_bits = rng.integers(0, thr_bits, 1024).astype(np.uint32).view(F)                 # every exponent, denormals included
    d = np.concatenate([last, around, uniform, any_bits])
    assert 5500 <= d.size <= 6500 and (d < THR).all() and (d >= 0).all() and (d == BELOW).any() and (d == TINY).any() and (d == 0).any()
    in_x = np.arange(d.size) % 2 == 0
    u = tracks(0, 0, np.where(in_x, d, 0), np.where(in_x, 0, -d))
    assert np.array_equal(distance(u), d)
    return [Call([u], d.size, d.size)]


def deltas():
    z = F(0)
    rows = [  # (x0, y0, x1, y1)
        (0, 1, SUB, 1), (0, 2, -SUB, 2), (3, 0, 3, TINY), (4, 0, 4, -TINY), (0, 0, SUB, -SUB),                 # denormal results
        (5, 5, np.nan, 5), (6, 6, 6, np.nan), (7, 7, np.inf, -np.inf), (8, 8, -np.inf, 8), (9, 9, np.nan, np.inf),   # non-finite p1, rows kept
        (2.0 ** 24, 1, 2.0 ** 24 + 2, 0), (2.0 ** 24, 2, 2.0 ** 24 - 1, 2.0 ** 24), (65535, 65535, 65535.004, 65534.996),
        (1000, 2000, -1000, -2000), (12, 13, 3e38, -3e38), (16777215, 3, 16777216, 3.0000002), (z, z, -z, z),   # large, cancelling, -0.0
    ]
    a = np.array(rows, F)
    p0, p1 = a[:, :2], a[:, 2:]
    u = unit(p0, p1, p0.copy())
    with np.errstate(all="ignore"):
        dx = p1 - p0
    assert kept(u) == len(rows) and (np.abs(dx[:5]) < np.finfo(F).tiny).all() and (dx[:5] != 0).sum() == 6 and np.isnan(dx).sum() == 3
    return [Call([u], len(rows), len(rows))]


def count_word():
    rng = np.random.default_rng(20262)
    n_max = 1000
    x, y = distinct_corners(rng, n_max, 2048)
    ex, ey = mixed(rng, x, y)
    calls = []
    for n in (0, 1, 255, 256, 257, 999, 1000, 5000, -1):
        u = tracks(x, y, ex, ey, n=n, width=2048)
        live = n_max if n < 0 else min(n, n_max)
        u["p0r"][live:] = u["p0"][live:]                 # rows behind the count word would pass the cut if they were read
        assert live == n_max or kept(dict(u, n=-1)) > kept(u)
        calls.append(Call([u], n_max, n_max, note=f"n = {n}"))
    return calls


def capacity():
    rng = np.random.default_rng(20263)
    x, y = distinct_corners(rng, 1200, 4000)
    e = np.where(rng.permutation(1200) < 900, F(0.03), F(0.3))
    u = tracks(x, y, e, 0, width=4000)
    assert kept(u) == 900
    calls = [Call([u], 1200, cap, note=f"cap = {cap}") for cap in (1, 256, 899, 900, 2000)]          # (cap 2000: n_max below the capacity)
    short = dict(u, n=1000)
    calls.append(Call([short], 1200, 700, note="n = 1000, cap = 700"))
    return calls


def placement():
    rng = np.random.default_rng(20264)
    calls = []
    for m, width in ((1, 1), (255, 2048), (256, 2049), (257, 10980), (2049, 65535), (32768, 0), (32768, 65535), (2049, 2048), (300, 1), (3000, 2047)):
        extra = max(3, m // 10)                                       # dropped rows between the kept ones
        x, y = distinct_corners(rng, m + extra, width if width else 65536)
        e = np.where(rng.permutation(m + extra) < m, F(0.02), F(0.2))
        u = tracks(x, y, 0, e, width=width)
        assert kept(u) == m and min(m + extra, m) <= 32768
        calls.append(Call([u], m + extra, m, note=f"{m} kept, width {width}"))
    # the width understated: every column beyond it falls into the last bucket, the order stays exact
    x, y = distinct_corners(rng, 2000, 5000)
    calls.append(Call([tracks(x, y, 0, 0, width=100)], 2000, 2000, note="width understated"))
    # one column: the rank loop inside a bucket goes four rows at a time and ends on every tail
    for m in (601, 602, 603, 604):
        calls.append(Call([tracks(77, rng.permutation(m), 0, 0, width=128)], m, m, note=f"{m} rows in one column"))
    ys = rng.permutation(6000)
    calls.append(Call([tracks(np.where(np.arange(6000) % 2 == 0, 5, 9), ys, 0, 0, width=2048)], 6000, 6000, note="two columns of 3000 rows"))
    # list order: descending, ascending, random
    x, y = distinct_corners(rng, 1000, 300, 300)
    asc = np.lexsort((y, x))
    for name, order in (("descending", asc[::-1]), ("ascending", asc), ("random", rng.permutation(1000))):
        calls.append(Call([tracks(x[order], y[order], 0.01, 0, width=300)], 1000, 1000, note=f"{name} list order"))
    return calls


def ties():
    rng = np.random.default_rng(20265)
    gx, gy = rng.integers(0, 5, 2000), rng.integers(0, 5, 2000)
    ex, ey = mixed(rng, gx, gy, 0.8)
    dup = tracks(gx, gy, ex, ey, width=5)
    assert len(set(zip(gx.tolist(), gy.tolist()))) == 25 and kept(dup) > 1000
    calls = [Call([dup], 2000, 2000, note="2000 rows on a 5 x 5 grid")]
    # origins at which float32 no longer tells neighbouring columns / rows apart: 40 consecutive columns and rows collapse
    cols, rows = np.meshgrid(np.arange(40), np.arange(40))
    order = rng.permutation(1600)
    cx, cy = cols.ravel()[order].astype(F), rows.ravel()[order].astype(F)
    for origin in (2 ** 24 + 1, 2 ** 26, 2 ** 30):
        collapsed = len(np.unique(np.arange(40, dtype=F) + F(origin)))
        assert collapsed < 40, f"origin {origin}: 40 columns stay distinct"
        for xo, yo in ((origin, 0), (0, origin), (origin, origin)):
            calls.append(Call([tracks(cx, cy, 0, 0.05, x_off=xo, y_off=yo, width=40)], 1600, 1600, note=f"origin ({xo}, {yo})",
                              facts={"distinct": collapsed}))
    assert len(np.unique(np.arange(40, dtype=F) + F(2 ** 26))) == 6
    return calls


def radix():
    rng = np.random.default_rng(20266)
    calls = []
    for m in (32769, 40000, 70000):
        x, y = distinct_corners(rng, m, 10980, 10980)
        ex, ey = mixed(rng, x, y)
        u = tracks(x, y, ex, ey, width=10980)
        assert 0.3 < kept(u) / m < 0.7
        calls.append(Call([u], m, m, note=f"{m} rows, half kept"))
    gx, gy = rng.integers(0, 100, 40000), rng.integers(0, 100, 40000)
    ex, ey = mixed(rng, gx, gy)
    tied = tracks(gx, gy, ex, ey, width=100)
    assert 0.3 < kept(tied) / 40000 < 0.7 and len(set(zip(gx.tolist(), gy.tolist()))) <= 10000
    calls.append(Call([tied], 40000, 40000, note="40000 rows on a 100 x 100 grid"))
    x, y = distinct_corners(rng, 32769, 4096, 4096)
    full = tracks(x, y, 0, 0, width=4096)
    assert kept(full) == 32769
    calls.append(Call([full], 32769, 32769, note="32769 rows, all kept"))
    calls.append(Call([full, full], 32769, 32769, refused=True, note="two units above 32768 rows"))
    return calls


def units():
    rng = np.random.default_rng(20267)
    n_max = 1500

    def some(n, width, x_off, y_off):
        x, y = distinct_corners(rng, n_max, width if width else 3000, 4096)
        ex, ey = mixed(rng, x, y, 0.6)
        u = tracks(x, y, ex, ey, n=n, x_off=x_off, y_off=y_off, width=width)
        live = n_max if n < 0 else min(n, n_max)
        u["p0r"][live:] = u["p0"][live:]
        return u

    counts = (0, 1, 2, 255, 256, 257, 1000, n_max, 5000, -1, 63, 64, 65, 1499, 700, 1024)
    widths = (512, 1, 2048, 2049, 10980, 65535, 700, 4096, 33, 512, 2047, 5000, 16, 300, 8192, 1024)
    sixteen = [some(n, w, 1000 * k, 7 * k * k) for k, (n, w) in enumerate(zip(counts, widths))]
    calls = [Call(sixteen, n_max, n_max, each_alone=True, note="16 units")]
    calls.append(Call([some(900, 512, 0, 512), some(3, 512, 512, 0)], n_max, n_max, each_alone=True, note="2 units"))
    calls.append(Call([some(1500, 600, 0, 0), some(0, 600, 600, 0), some(1201, 0, 1200, 2 ** 26)], n_max, 1000, each_alone=True,
                      note="3 units, one of unknown width, capacity below n_max"))
    return calls


def stale_workspace():
    rng = np.random.default_rng(20268)
    calls = []
    for m in (70000, 40000, 300):
        x, y = distinct_corners(rng, m, 8000, 8000)
        ex, ey = mixed(rng, x, y)
        calls.append(Call([tracks(x, y, ex, ey, width=8000)], m, m, note=f"{m} rows"))
    return calls


CASES = {f.__name__: f for f in (cut, score_sweep, deltas, count_word, capacity, placement, ties, radix, units, stale_workspace)}
_built: dict = {}


def build(name):
    """The calls of a case, built once per process and shared (nobody changes them)."""
    if name not in _built:
        _built[name] = CASES[name]()
        for call in _built[name]:
            assert 1 <= len(call.units) <= 16 and all(len(u["p0"]) == call.n_max for u in call.units), (name, call.note)
            assert len(call.units) * call.n_max < 100000 or call.refused, (name, call.note)
            for u in call.units:
                for a in (u["p0"], u["p1"], u["p0r"]):
                    a.flags.writeable = False
    return _built[name]
