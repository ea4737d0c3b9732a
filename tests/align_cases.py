"""Inputs of the align step's stage and degenerate-warp tests, shared by tests/test_gpu_align_stages.py, tests/test_gpu_align.py
(which run them on the GPU) and tests/test_align_host.py (which proves on the restatement alone that every input does what it is
there for: the mix of pixels of a degenerate warp, the pre-mask's decision edge, the iteration counts of the walked loops).

Test infrastructure only: karios_amd never imports this module.  References are computed once (functools.lru_cache) and returned
read-only.
"""
from __future__ import annotations

import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_restatement as R  # noqa: E402

from karios_amd import synth  # noqa: E402

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max

# (template, input) as (rows, columns): one pixel, one row, one column, reflections that wrap twice, a template lower than 16 rows
# (blocks of 1024 / hs columns), widths off the 64-column and heights off the 4-row tile, template and input of different sizes
STAGE_SHAPES = [((1, 1), (1, 1)), ((1, 9), (1, 9)), ((9, 1), (9, 1)), ((2, 2), (3, 2)), ((5, 67), (5, 67)), ((9, 300), (13, 290)),
                ((70, 131), (70, 131)), ((61, 200), (75, 190))]
GRID_STRIDE_SHAPE = ((530, 1000), (530, 1000))   # > 2048 workgroups * 256 template pixels: the iteration kernel's grid-stride path
WIDE_INPUT_SHAPE = ((2, 70), (3, 32771))         # an input wider than 32767 columns: a saturated position is one of its pixels
EDGE_MASK_MIN = 9                               # inputs of at least 9 x 9 carry the planted 243/256 and 244/256 sites


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def stage_images(shapes, dtype_name, seed=7):
    """-> (template, input) of random content; float32 content has both signs and is no multiple of anything"""
    (hs, ws), (hd, wd) = shapes
    rng = np.random.default_rng(seed + 1000 * hs + ws)
    if dtype_name == "uint8":
        return _ro(rng.integers(0, 256, (hs, ws), dtype=np.uint8), rng.integers(0, 256, (hd, wd), dtype=np.uint8))
    return _ro((rng.random((hs, ws)) * 300 - 50).astype(f32), (rng.random((hd, wd)) * 300 - 50).astype(f32))


@functools.lru_cache(maxsize=None)
def stage_mask(shape, seed=11):
    """uint8 mask of an input: ~3 % single-pixel holes, a masked strip along the top and the left border, valid values that are
    neither 0 nor 255 nor all alike, and - from 9 x 9 on - two planted sites whose blurred mask is exactly 244/256 (zeros at
    (0, +-2)) and 243/256 (the same and a corner tap at (2, 2)): the two values on either side of the pre-mask's rounding."""
    hd, wd = shape
    rng = np.random.default_rng(seed + 1000 * hd + wd)
    m = rng.integers(1, 256, (hd, wd), dtype=np.uint8)
    m[rng.random((hd, wd)) < 0.03] = 0
    if hd > 2:
        m[0] = 0
    if wd > 4:
        m[:, :2] = 0
    if min(hd, wd) >= EDGE_MASK_MIN:
        for k, (cy, cx) in enumerate(edge_sites(shape)):
            m[cy - 3:cy + 4, cx - 3:cx + 4] = rng.integers(1, 256, (7, 7), dtype=np.uint8)
            m[cy, cx - 2] = m[cy, cx + 2] = 0
            if k == 1:
                m[cy + 2, cx + 2] = 0
    return _ro(m)


def edge_sites(shape):
    """(the 244/256 site, the 243/256 site) of stage_mask"""
    hd, wd = shape
    cy = min(hd - 4, max(4, hd // 2))
    return (cy, 3 + wd // 4), (cy, 3 + wd // 4 + 8 + wd // 4)


def special_f32(shape, seed=3):
    """float32 image holding denormals, +-inf, NaN, +-FLT_MAX and signed zeros among ordinary values"""
    h, w = shape
    rng = np.random.default_rng(seed)
    a = (rng.random((h, w)) * 200 - 100).astype(f32)
    specials = np.array([1e-45, -1e-45, 1.1754942e-38, -5e-39, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX, 0.0, -0.0, 3e-41], f32)
    flat = a.reshape(-1)
    n = flat.size
    at = rng.choice(n, size=min(n, max(1, n // 25)), replace=False)
    flat[at] = specials[np.arange(at.size) % specials.size]
    if n >= 64:     # a patch of denormals only: blurs and gradients of it stay denormal
        a[h // 2:h // 2 + 6, w // 2:w // 2 + 6] = (rng.integers(-2000, 2000, a[h // 2:h // 2 + 6, w // 2:w // 2 + 6].shape) * 1e-42).astype(f32)
    return a


@functools.lru_cache(maxsize=None)
def prepared(shapes, dtype_name, masked):
    """R.ecc_prepare of stage_images (and stage_mask) -> (t, i, gx, gy, pm)"""
    t, i = stage_images(shapes, dtype_name)
    return _ro(*R.ecc_prepare(t, i, stage_mask(shapes[1]) if masked else None))


# ---- maps of the sums tests -------------------------------------------------------------------------------------------------
def sums_maps(shapes):
    """name -> float32 3 x 3 map for a template / input pair: identity, sub-pixel with perspective terms, mostly outside the input
    (N small), and a denominator x h2 + y h5 + 1 that changes sign across the template without ever being 0."""
    (hs, ws), (hd, wd) = shapes
    cross = -1.0 / (0.37 + (ws - 1) / 2.0) if ws > 1 else -1.0 / (0.37 + (hs - 1) / 2.0)
    return {
        "identity": np.eye(3, dtype=f32),
        "subpixel": np.array([[1.003, -0.004, 0.37], [0.005, 0.998, -0.61], [2e-5, -3e-5, 1]], f32),
        "outside": np.array([[1, 0, wd - 6.5], [0, 1, hd - 5.75], [0, 0, 1]], f32),
        "den_sign": np.array([[0.31, 0, 0.4], [0, 0.29, 0.3], [cross if ws > 1 else 0, cross if ws == 1 else 0, 1]], f32),
        # for WIDE_INPUT_SHAPE: columns right of 33 land 2^20 px apart, far beyond the short range: sat_short puts them on column 32767
        "sat_short": np.array([[2.0 ** 20, 0, -2.0 ** 20 * 33 + 4], [0, 1, 0.25], [0, 0, 1]], f32),
    }


def jacobian_den(shapes, mp):
    """den of ecc_jacobian for every template pixel (float32)"""
    (hs, ws), _ = shapes
    X = np.broadcast_to(np.arange(ws, dtype=f32)[None, :], (hs, ws))
    Y = np.broadcast_to(np.arange(hs, dtype=f32)[:, None], (hs, ws))
    h = np.asarray(mp, f32).reshape(9)
    return (X * h[6] + Y * h[7]) + f32(1)


def sums_masked(shapes):
    """the sums tests mask inputs of at least 9 x 9: the blur of a smaller mask with holes leaves no valid pixel"""
    return min(shapes[1]) >= EDGE_MASK_MIN


@functools.lru_cache(maxsize=None)
def exact_sums(shapes, map_name):
    """-> (exact[66], bound[66], numpy_order[66]): the correctly rounded sums (math.fsum) of the restatement's per-pixel terms of
    the float32 stage inputs (masked: sums_masked) at sums_maps(shapes)[map_name]; the bound every summation order of n exact terms obeys,
    (n - 1) 2^-53 sum |term|; and the sums in numpy's order (R.ecc_sums)."""
    terms = R.ecc_terms(*prepared(shapes, "float32", sums_masked(shapes)), sums_maps(shapes)[map_name])
    n = terms[0].size
    exact = np.array([math.fsum(t.ravel().tolist()) for t in terms])
    bound = np.array([(n - 1) * 2.0 ** -53 * math.fsum(np.abs(t).ravel().tolist()) for t in terms])
    return _ro(exact, bound, np.array([t.sum() for t in terms]))


# ---- image pairs an ECC run converges on ---------------------------------------------------------------------------------------
def _homography(tx, ty, deg, scale, p):
    th = np.radians(deg)
    return np.array([[scale * np.cos(th), -scale * np.sin(th), tx], [scale * np.sin(th), scale * np.cos(th), ty], [p[0], p[1], 1.0]])


@functools.lru_cache(maxsize=None)
def ecc_pair(shapes, seed=20260101):
    """-> (template, input, mask, initial map): Sobel magnitudes of two cuts of one smooth scene, template(x) ~ input(init A x) for
    a small homography A; the mask is the input's cut > 0 with a masked strip.  A template wider than the input hangs over it."""
    (hs, ws), (hd, wd) = shapes
    pad = 24
    n = max(hs, ws, hd, wd)
    base = synth.make_base(n, n, seed)[synth.PAD - pad:, synth.PAD - pad:]
    scene = np.clip((base - 1000.0) / 4000.0 * 255.0, 0, 255).astype(np.uint8)
    ox, oy = ((wd - ws) // 2, (hd - hs) // 2)
    A = _homography(0.8, -0.6, 0.2, 1 + 1e-3, (1e-6, -1e-6))
    T = np.array([[1, 0, pad + ox], [0, 1, pad + oy], [0, 0, 1.0]])
    inp = scene[pad:pad + hd, pad:pad + wd]
    tmpl = R.warp_perspective(scene, T @ A, (ws, hs), R.INTER_LINEAR | R.WARP_INVERSE_MAP)
    mask = np.where(inp > 0, 200, 0).astype(np.uint8)
    mask[:, :3] = 0
    init = np.array([[1, 0, ox], [0, 1, oy], [0, 0, 1]], f32)
    return _ro(R.sobel_magnitude(tmpl), R.sobel_magnitude(inp), mask, init)


LOOP_SHAPES = [((70, 131), (70, 131)), ((61, 200), (75, 190))]
LOOP_CRITERIA = (3, 200, 1e-6)


@functools.lru_cache(maxsize=None)
def loop_reference(shapes):
    """R.find_transform_ecc on ecc_pair -> (cc, map, iterations)"""
    t, i, mask, init = ecc_pair(shapes)
    return R.find_transform_ecc(t, i, init, LOOP_CRITERIA, mask, 5, return_iters=True)


def step_cases():
    """name -> (template, input, mask, map) of the one-iteration tests: an ordinary step; anti-correlated images (lambda_d <= 0:
    no convergence); a flat input (singular Hessian and an undefined correlation: no convergence); an input of vertical stripes
    (no y gradient: a singular Hessian, zeros from lu_inv_f32, with a defined correlation: the map stays as it is)."""
    shapes = LOOP_SHAPES[1]
    t, i, mask, init = ecc_pair(shapes)
    (hs, ws), (hd, wd) = shapes
    stripes_i = np.broadcast_to((np.sin(np.arange(wd) * 0.21) * 40 + 100).astype(f32)[None, :], (hd, wd)).copy()
    stripes_t = np.broadcast_to((np.sin((np.arange(ws) + init[0, 2] + 0.5) * 0.21) * 40 + 100).astype(f32)[None, :], (hs, ws)).copy()
    t70, i70, mask70, init70 = ecc_pair(LOOP_SHAPES[0])
    return {
        "ordinary": (t, i, mask, init),
        "ordinary_no_mask": (t70, i70, None, np.array([[1, 0, 0.25], [0, 1, -0.5], [1e-6, 0, 1]], f32)),
        "anticorrelated": (t70, f32(1) - t70, None, init70),
        "flat": (t, np.full((hd, wd), 0.5, f32), mask, init),
        "stripes": (stripes_t, stripes_i, None, init),
    }


# ---- Sobel magnitude ----------------------------------------------------------------------------------------------------------------
def sobel_extreme(shape=(37, 150)):
    """-> (random 0 / 255 image with the pattern of the largest possible gx^2 + gy^2 = 1020^2 + 510^2 planted, where): left column
    and upper middle 0, right column and lower middle 255 around the pixel"""
    img = (np.random.default_rng(8).integers(0, 2, shape) * 255).astype(np.uint8)
    y, x = shape[0] - 3, shape[1] - 4
    img[y - 1:y + 2, x - 1:x + 2] = np.array([[0, 0, 255], [0, 0, 255], [0, 255, 255]], np.uint8)
    return _ro(img), (y, x)


def sobel_last_pixel(shape=(70, 131)):
    """zeros but for the last pixel: only the last workgroup has a gradient, and with it the maximum"""
    img = np.zeros(shape, np.uint8)
    img[-1, -1] = 9
    return _ro(img)


# ---- warps where OpenCV's edge rules bite ---------------------------------------------------------------------------------------
BIG = 2.0 ** 31 / 32     # positions beyond this leave the int range on the 1/32 grid


def warp_cases():
    """name -> (source shape, destination shape (rows, columns), matrix, inverse flag, expectation): what the case is there for,
    checked by check_warp_case on the restatement."""
    c = {}
    I = R.WARP_INVERSE_MAP
    # W == 0 exactly on destination row 8, W > 0 above and W < 0 below it
    c["w_zero_row"] = ((20, 24), (17, 24), [[1, 0, 0], [0, 1, 0], [0, 1 / 8, -1]], I, "mix_w0")
    # W == 0 on column 16, W < 0 left of it; a 3-row destination, so the whole width is one block
    c["w_zero_col"] = ((30, 40), (3, 40), [[0.5, 0, 0], [0, 0.5, 1], [1 / 16, 0, -1]], I, "mix_w0")
    c["all_zero"] = ((9, 11), (6, 70), np.zeros((3, 3)), I, "constant")
    c["singular_forward"] = ((9, 11), (6, 70), [[1, 2, 3], [2, 4, 6], [0, 0, 1]], 0, "constant")
    # W = -1 everywhere: (x, y) -> (x + 2, y + 1)
    c["w_negative"] = ((30, 40), (20, 30), [[-1, 0, -2], [0, -1, -1], [0, 0, -1]], I, "full")
    # x beyond +-2^31 / 32 for most columns (clamp_int binds, then sat_short), y inside
    c["clamp_int_x"] = ((12, 12), (10, 70), [[BIG / 8, 0, -4 * BIG], [0, 1, 0.5], [0, 0, 1]], I, "sat_both")
    # x between 2^15 and 2^26 px: sat_short binds, clamp_int does not
    c["sat_short_x"] = ((12, 12), (10, 70), [[2.0 ** 20, 0, -2.0 ** 20 * 33 + 3.25], [0, 1, 0.25], [0, 0, 1]], I, "sat_both")
    # the same on a source wider than 32767 columns: the saturated position 32767 is INSIDE it and reads a source pixel
    c["sat_short_inside"] = ((3, 32771), (2, 70), [[2.0 ** 20, 0, -2.0 ** 20 * 33 + 3.25], [0, 1, 0.25], [0, 0, 1]], I, "sat_inside")
    c["nan_entry"] =((12, 12), (10, 70), [[1, 0, np.nan], [0, 1, 0.5], [0, 0, 1]], I, "sat_hi")
    c["nan_w"] = ((12, 12), (10, 70), [[1, 0, 0], [0, 1, 0], [np.nan, 0, 1]], I, "sat_hi")
    c["inf_entry"] = ((12, 12), (10, 70), [[1, 0, np.inf], [0, 1, 0.5], [0, 0, 1]], I, "sat_hi")
    c["neg_inf_entry"] = ((12, 12), (10, 70), [[1, 0, 0.5], [0, 1, -np.inf], [0, 0, 1]], I, "sat_lo")
    # -inf * 0 at the block's first column is NaN, and stays NaN along the block: INT_MAX, not INT_MIN
    c["inf_scale"] = ((12, 12), (10, 70), [[-np.inf, 0, 3], [0, 1, 0.5], [0, 0, 1]], I, "sat_hi")
    # 32 / 1e-300 is finite, times a position overflows to +-inf, then the clamp; column 3 maps to 0 exactly
    c["tiny_w"] = ((12, 12), (10, 70), [[1e10, 0, -3e10], [0, 1e-300, 0], [0, 0, 1e-300]], I, "sat_both")
    # every position lies exactly between two 1/32 steps, 33 x + 15.5 and 31 y + 0.5 of them: half to even goes up and down
    c["ties"] = ((20, 40), (18, 36), [[33 / 32, 0, 0.5 - 1 / 64], [0, 31 / 32, 1 / 64], [0, 0, 1]], I, "ties")
    # taps astride the last row / column and astride row / column -1, with and without a fraction
    c["edges"] = ((9, 13), (13, 17), [[1, 0, -1.75], [0, 1, -1.5], [0, 0, 1]], I, "edges")
    c["edges_whole"] = ((9, 13), (12, 16), [[1, 0, -1], [0, 1, -1], [0, 0, 1]], I, "edges")
    # sizes
    c["src_1x1"] = ((1, 1), (5, 6), [[1, 0, -2.25], [0, 1, -1.5], [0, 0, 1]], I, "edges")
    c["src_1x7"] = ((1, 7), (4, 11), [[0.9, 0.05, -1.3], [0, 0.6, -0.8], [0, 0, 1]], I, "mixed")
    c["src_7x1"] = ((7, 1), (11, 4), [[0.6, 0, -0.8], [0.05, 0.9, -1.3], [0, 0, 1]], I, "mixed")
    c["dst_1x1"] = ((9, 11), (1, 1), [[1, 0, 3.3], [0, 1, 4.6], [0, 0, 1]], I, "full")
    c["dst_1x300"] = ((9, 280), (1, 300), [[0.97, 0, -3.2], [0, 1, 4.4], [1e-4, 0, 1]], I, "mixed")
    # 3 rows: blocks of 1024 / 3 = 341 columns, not 64; the matrix of the block-relative rounding case, stretched
    c["dst_3x2000"] = ((8, 1900), (3, 2000), [[0.9, 0.0, -51.784375], [0.0, 1.0, 2.3], [0.0, 0.0, 1.0]], I, "block341")
    return {k: (s, d, np.array(m, np.float64), inv, what) for k, (s, d, m, inv, what) in c.items()}


def warp_source(shape, dtype, kind="random", seed=5):
    """a strided view (rows contiguous, row stride > width): random content without zeros or the test's border values, a 0 / 255
    checkerboard, or float32 specials"""
    h, w = shape
    rng = np.random.default_rng(seed + 100 * h + w)
    big = np.zeros((h + 3, w + 7), dtype)
    if kind == "special":
        v = special_f32(shape, seed)
    elif kind == "checker":
        v = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(dtype)
    else:
        v = rng.integers(20, 250, shape).astype(dtype) if np.dtype(dtype) == np.uint8 else (rng.random(shape) * 200 + 20).astype(dtype)
    big[1:1 + h, 2:2 + w] = v
    return big[1:1 + h, 2:2 + w]


def check_warp_case(name):
    """Assert on the restatement that warp case `name` exercises what it is listed for."""
    (sH, sW), (dH, dW), M, inv, what = warp_cases()[name]
    Mi = M if inv else R.invert3x3(M)
    src = np.arange(1, sH * sW + 1, dtype=f32).reshape(sH, sW)          # no zeros, every pixel its own value
    with np.errstate(all="ignore"):
        sx, sy, fx, fy = R.warp_taps(Mi, dH, dW, True)
        nx, ny = R.warp_taps(Mi, dH, dW, False)
        out = R.warp_perspective(src, M, (dW, dH), R.INTER_LINEAR | inv, -1.0)
        near = R.warp_perspective(src, M, (dW, dH), R.INTER_NEAREST | inv, -1.0)
    inside = (sx >= 0) & (sx + 1 < sW) & (sy >= 0) & (sy + 1 < sH)
    allout = (sx >= sW) | (sx + 1 < 0) | (sy >= sH) | (sy + 1 < 0)
    if what == "mix_w0":
        m = Mi.reshape(9)
        W = m[6] * np.arange(dW)[None, :] + m[7] * np.arange(dH)[:, None] + m[8]
        assert (W == 0).any() and (W < 0).any() and (W > 0).any()
        assert (out[W == 0] == src[0, 0]).all() and (near[W == 0] == src[0, 0]).all()      # W == 0 -> position (0, 0)
        assert (out == -1).any() and inside.any() and (near == -1).any()
        assert (inside & (W < 0)).any() or (inside & (W > 0)).any()
    elif what == "constant":
        assert not inv and not R.invert3x3(M).any() or inv and not M.any()
        assert (out == src[0, 0]).all() and (near == src[0, 0]).all()
    elif what == "full":
        assert inside.all() and (out != -1).all() and (near != -1).all()
    elif what in ("sat_both", "sat_hi", "sat_lo"):
        hi, lo = (sx == 32767) | (sy == 32767), (sx == -32768) | (sy == -32768)
        assert what != "sat_hi" or hi.all() or (hi.any() and name == "nan_w")
        assert what != "sat_lo" or lo.all()
        assert what != "sat_both" or (hi.any() and lo.any())
        if what == "sat_both":
            ok = (np.abs(sx) < 32767) & (np.abs(sy) < 32767)
            assert ok.any() and (out[ok & inside] != -1).all() and (ok & inside).any()
        assert ((nx == 32767) | (ny == 32767) | (nx == -32768) | (ny == -32768)).any()
    elif what == "sat_inside":
        at = sx == 32767
        assert at.any() and inside[at].all() and (out[at] != -1).all() and (nx == 32767).any() and (near[nx == 32767] != -1).all()
        assert (sx == -32768).any() and (out[sx == -32768] == -1).all()
    elif what == "ties":
        for P, exact in (((sx * 32 + fx)[0], 33 * np.arange(dW) + 15.5), ((sy * 32 + fy)[:, 0], 31 * np.arange(dH) + 0.5)):
            assert (np.abs(P - exact) == 0.5).all() and (P % 2 == 0).all()   # half a step off, on the even neighbour
            assert (P < exact).any() and (P > exact).any()
        assert inside.any()
    elif what == "edges":
        part = ~allout & ~inside
        assert ((sx == sW - 1) & part).any() and ((sy == sH - 1) & part).any()
        assert ((sx == -1) & part).any() and ((sy == -1) & part).any()
        assert allout.any() and (inside.any() or sH * sW == 1)
    elif what == "mixed":
        assert (~allout).any() and (out != -1).any() and (out == -1).any()
    elif what == "block341":
        assert min(1024 // min(16, dH), dW) == 341
        x = np.arange(dW, dtype=np.float64)[None, :]
        other = np.arange(dW) - np.arange(dW) % 64                      # what 64-column blocks would give
        X64 = np.rint((M[0, 0] * other + M[0, 2] + M[0, 0] * (x - other)) * 32.0).astype(np.int64)
        assert ((sx * 32 + fx)[0] != X64[0]).any() and inside.any()
    else:
        raise AssertionError(what)
