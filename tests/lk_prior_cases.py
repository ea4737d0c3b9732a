"""Inputs of the tests of the tracker under a geometric prior (tests/test_lk_prior_host.py, tests/test_gpu_lk_prior.py; the
definition: tests/lk_prior_restatement.py).  Everything here is numpy on the CPU; nothing reads the library under test.

The content is one 192 x 160 uint8 texture cut twice out of a larger canvas, so that mon(x + sx, y + sy) == ref(x, y) exactly for an
integer shift (sx, sy): blocks of 4 px smoothed twice (corners the tracker converges on), full contrast in the middle of the image and
little towards its rim - the strong corners then sit where neither a window nor the zero fill of `shift_image` reaches a border, which
is what the comparison with the reference's shift-then-track path needs.  No pixel is 0 (0 is "no data" to the automatic mask)."""
from __future__ import annotations

import functools

import numpy as np

H, W = 160, 192
PAD = 40                                   # canvas margin: integer shifts up to 40 px either way
SHIFTS = ((14, -6), (7, 3))                # (sx, sy): mon(x + sx, y + sy) == ref(x, y)
WINDOWS = (25, 21, 31)                     # the compile-time form and one generic size either side (NR 2, 2, 4)
MAX_CORNERS, QUALITY, MIN_DISTANCE, BLOCK = 40, 0.05, 9, 5


def _smooth(a):
    p = np.pad(a, 1, mode="edge")
    return (p[:-2, :-2] + p[:-2, 1:-1] + p[:-2, 2:] + p[1:-1, :-2] + p[1:-1, 1:-1] + p[1:-1, 2:] + p[2:, :-2] + p[2:, 1:-1] + p[2:, 2:]) / 9.0


@functools.lru_cache(maxsize=None)
def canvas(seed=20261021):
    rng = np.random.default_rng(seed)
    hh, ww = H + 2 * PAD, W + 2 * PAD
    t = np.kron(rng.integers(0, 256, (hh // 4 + 1, ww // 4 + 1)).astype(np.float64), np.ones((4, 4)))[:hh, :ww]
    t = _smooth(_smooth(t))
    yy, xx = np.mgrid[0:hh, 0:ww]
    r = np.maximum(np.abs(yy - (hh - 1) / 2) / (H / 2), np.abs(xx - (ww - 1) / 2) / (W / 2))      # 0 in the middle, 1 on the rim of `ref`
    env = np.clip(1.0 - (r - 0.42) / 0.2, 0.12, 1.0)
    out = np.clip(np.rint(128 + (t - 128) * env), 1, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pair(sx=0, sy=0):
    """-> (ref, mon) uint8 H x W with mon(x + sx, y + sy) == ref(x, y)."""
    c = canvas()
    ref = np.ascontiguousarray(c[PAD:PAD + H, PAD:PAD + W])
    mon = np.ascontiguousarray(c[PAD - sy:PAD - sy + H, PAD - sx:PAD - sx + W])
    for a in (ref, mon):
        a.setflags(write=False)
    return ref, mon


def rotation_prior(deg, cx=(W - 1) / 2, cy=(H - 1) / 2, sx=0.0, sy=0.0):
    """Rotation about (cx, cy) followed by a shift, as the 9 values of a prior."""
    a = np.deg2rad(deg)
    c, s = float(np.cos(a)), float(np.sin(a))
    return np.array([c, -s, cx - c * cx + s * cy + sx, s, c, cy - s * cx - c * cy + sy, 0.0, 0.0, 1.0])


def horizon_prior():
    """A projective map whose w = 1 - x / 120 is <= 0 for x >= 120: no guess on that side of the line."""
    return np.array([1.0, 0.0, 2.0, 0.0, 1.0, -1.0, -1.0 / 120.0, 0.0, 1.0])


def guess_cases(win):
    """Key points and explicit guesses of km_pyrlk_initial on `pair(7, 3)` (an odd shift: half a pixel at level 1) -> list of
    (name, pts (N, 2) float32, guesses (N, 2) float32)."""
    sx, sy = 7, 3
    half = (win - 1) / 2
    grid = np.array([[x, y] for y in (52, 77, 103) for x in (60, 95, 128)], np.float32)
    f = lambda a: np.asarray(a, np.float32).reshape(-1, 2)
    cases = [
        ("integer", grid, grid + f([sx, sy])),
        ("fractional", grid, grid + f([sx + 0.37, sy - 0.61])),
        ("fractional points", grid + f([0.25, 0.5]), grid + f([sx - 0.3, sy + 0.45])),
        # inside and outside the margin of the old (key-point centred) patch: 3 and 4 px, each axis and sign
        ("3 px", np.repeat(grid[:4], 4, 0), np.repeat(grid[:4], 4, 0) + np.tile(f([[3, 0], [-3, 0], [0, 3], [0, -3]]), (4, 1))),
        ("4 px", np.repeat(grid[:4], 4, 0), np.repeat(grid[:4], 4, 0) + np.tile(f([[4, 0], [-4, 0], [0, 4], [0, -4]]), (4, 1))),
        # the true displacement is (7, 3): from 6 px short of it the search leaves the staged patch and re-centres
        ("re-centre", grid, grid + f([sx - 6, sy + 5])),
    ]
    # search windows that cross each border (the byte-load staging path): guesses near the rims, key points well inside
    inner = f([[70, 60], [96, 80], [120, 100]])
    for name, g in (("left", [half - 2, 80]), ("top", [96, half - 3]), ("right", [W - 1 - half + 3, 80]), ("bottom", [96, H - 1 - half + 2]),
                    ("corner", [2, 1]), ("far corner", [W - 2, H - 1])):
        cases.append((f"border {name}", inner, np.tile(f(g), (3, 1)) + f([[0, 0], [0.5, 0.25], [1, 2]])))
    # the level-1 window origin floor(g / 2 - half) exactly at -win (the level iterates) and at -win - 1 (it does not), each axis
    edge = -(win + 1.0)
    cases.append(("level-1 origin -win", inner, f([[edge, 80], [96, edge], [edge, edge]])))
    cases.append(("level-1 origin -win - 1", inner, f([[edge - 2, 80], [96, edge - 2], [edge - 2, edge - 2]])))
    cases.append(("beyond the far rim", inner, f([[2 * ((W + 1) // 2) + half * 2, 80], [96, 2 * ((H + 1) // 2) + half * 2], [W + 300, H + 300]])))
    # key points whose own window crosses a border (the template is staged by byte loads), guesses inside
    cases.append(("template at the rim", f([[3, 70], [100, 2], [W - 3, 90], [90, H - 2]]), f([[3 + sx, 70 + sy], [100 + sx, 2 + sy], [W - 3 - 9, 90], [90, H - 2 - 8]])))
    return [(n, np.ascontiguousarray(p), np.ascontiguousarray(g)) for n, p, g in cases]


def mask_cases():
    """Inputs of the mask rule -> list of dicts: name, ref, mon (one pixel type), prior, base (None or uint8), nodata_ref, nodata_mon,
    x_off, y_off.  Rasters of 67 x 83 (no multiple of the kernel's 64 x 4 blocks, more than one block each way) with zeros, no-data
    values and - float32 - NaN and infinities sprinkled over both."""
    rng = np.random.default_rng(41)
    h, w = 67, 83
    out = []
    priors = [("shift", np.array([1.0, 0, 5, 0, 1.0, -3, 0, 0, 1.0])), ("half-pixel shift", np.array([1.0, 0, 2.5, 0, 1.0, 1.5, 0, 0, 1.0])),
              ("rotation 3 deg", rotation_prior(3.0, (w - 1) / 2, (h - 1) / 2)), ("horizon", np.array([1.0, 0.0, 2.0, 0.0, 1.0, -1.0, -1.0 / 50.0, 0.0, 1.0])),
              ("far away", np.array([1.0, 0, 1e6, 0, 1.0, 0, 0, 0, 1.0])), ("huge", np.array([1e300, 0, 0, 0, 1e300, 0, 0, 0, 1e-300]))]
    for dt in (np.uint8, np.uint16, np.int16, np.float32):
        def raster(seed):
            r = np.random.default_rng(seed)
            a = r.integers(1, 200, (h, w)).astype(dt)
            if dt == np.int16:
                a = (a - 100).astype(dt)
            a[r.random((h, w)) < 0.08] = 0
            a[r.random((h, w)) < 0.05] = 7                       # the no-data value of some cases
            if dt == np.float32:
                a[r.random((h, w)) < 0.04] = np.nan
                a[r.random((h, w)) < 0.02] = np.inf
                a[r.random((h, w)) < 0.02] = -np.inf
            return a
        ref, mon = raster(int(np.dtype(dt).itemsize) * 10 + 1), raster(int(np.dtype(dt).itemsize) * 10 + 2)
        for k, (pname, P) in enumerate(priors):
            nd = (7.0, 7.0) if k % 2 == 0 else ((None, 7.0) if k % 3 == 0 else (None, None))
            base = (rng.random((h, w)) < 0.7).astype(np.uint8) * (1 + k) if k in (1, 2) else None      # (any non-zero byte is "valid")
            off = (12.0, 30.0) if k in (2, 3) else (0.0, 0.0)
            if off != (0.0, 0.0) and pname == "rotation 3 deg":
                P = rotation_prior(3.0, (w - 1) / 2 + off[0], (h - 1) / 2 + off[1])
            out.append(dict(name=f"{np.dtype(dt).name} {pname}", ref=ref, mon=mon, prior=P, base=base, nodata_ref=nd[0], nodata_mon=nd[1], x_off=off[0], y_off=off[1]))
    return out


def frame_priors():
    """(name, (sx, sy) of the content, prior, (x_off, y_off, w, h) box or None) of the frame entry point's cases."""
    return [
        ("shift (14, -6)", (14, -6), np.array([1.0, 0, 14, 0, 1.0, -6, 0, 0, 1.0]), None),
        ("odd shift (7, 3)", (7, 3), np.array([1.0, 0, 7, 0, 1.0, 3, 0, 0, 1.0]), None),
        ("fractional shift", (7, 3), np.array([1.0, 0, 6.6, 0, 1.0, 3.3, 0, 0, 1.0]), None),
        ("short of the shift", (14, -6), np.array([1.0, 0, 9.0, 0, 1.0, -2.0, 0, 0, 1.0]), None),       # forward results re-centre; the backward guess leaves p0
        ("rotation 1 deg", (7, 3), rotation_prior(1.0, sx=7.0, sy=3.0), None),
        ("box", (7, 3), np.array([1.0, 0, 7, 0, 1.0, 3, 0, 0, 1.0]), (16, 8, 168, 148)),
        # guesses up to the right and upper rims of the monitored raster: search windows (forward) and template windows (backward) across them
        ("large shift (40, -30)", (40, -30), np.array([1.0, 0, 40, 0, 1.0, -30, 0, 0, 1.0]), None),
    ]
