"""The definition of the align step's preprocessing (tests/prep_restatement.py) against what it restates, on the CPU: the port of
numpy's 'linear' interpolation against np.percentile / np.nanpercentile bit for bit, the restated _to_uint8 against the reference's
expression on the installed numpy, CLAHE against answers worked by hand, and against cv2 where cv2 imports."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_restatement as R  # noqa: E402

from karios_amd import ops  # noqa: E402  (lerp_linear is plain numpy: nothing here touches the GPU library)

QS = [0, 2, 33.3, 50, 98, 99.999, 100]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _arrays():
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 5, 64, 257, 1000, 4099):
        yield rng.integers(0, 256, n, dtype=np.uint8)
        yield rng.integers(0, 65536, n, dtype=np.uint16)
        yield rng.integers(-32768, 32768, n).astype(np.int16)
        yield rng.choice(np.array([-30000, -29999, 17, 29999, 30000], np.int16), n)     # b - a wraps in int16, as numpy's does
        yield (rng.standard_normal(n) * 1000).astype(np.float32)
        yield (rng.random(n).astype(np.float32) * np.float32(1e-3) + np.float32(16777216.0)) * rng.choice(np.array([1, -1, 1e-30], np.float32), n)
        yield rng.choice(np.array([0.1, 0.7, 1e7 + 1, -3.3, 1e-40], np.float32), n)      # differences that round, a denormal


def test_lerp_port_equals_numpy_percentile_bit_for_bit():
    count = 0
    for a in _arrays():
        exp = np.percentile(a, QS)
        n, v0, v1, vi = R.order_statistics(a, np.asarray(QS, np.float64) / 100)
        assert n == a.size
        for got in (R.lerp(v0, v1, vi, n, a.dtype), ops.lerp_linear(v0, v1, vi, n, a.dtype), R.percentile(a, QS)):
            assert got.dtype == np.float64
            np.testing.assert_array_equal(_bits(got), _bits(exp), err_msg=f"{a.dtype} n={a.size}")
        count += 1
    assert count >= 50


def test_lerp_port_equals_numpy_nanpercentile_bit_for_bit():
    rng = np.random.default_rng(11)
    for n in (1, 4, 333, 2048):
        a = (rng.standard_normal((n, 3)) * 50).astype(np.float32)
        a[rng.random(a.shape) < 0.2] = np.nan
        a[0, 0] = 1.5
        if n > 1:
            a[1, 1], a[1, 2] = np.inf, -np.inf
        with np.errstate(invalid="ignore"):
            exp = np.nanpercentile(a, QS)
            got = R.percentile(a, QS)
        np.testing.assert_array_equal(_bits(got), _bits(exp))
    assert np.isnan(R.percentile(np.full((2, 2), np.nan, np.float32), [2, 98])).all()     # numpy: NaN (and a RuntimeWarning)
    for dt in (np.uint16, np.int16):                                                     # integers: nanpercentile is percentile
        a = rng.integers(0, 30000, (37, 41)).astype(dt)
        np.testing.assert_array_equal(_bits(R.percentile(a, [2, 98])), _bits(np.nanpercentile(a, [2, 98])))


def _reference_to_uint8(arr):
    """karios/matcher/global_align.py:87-101, as written there, evaluated by the installed numpy."""
    if arr.dtype == np.uint8:
        return arr
    a = arr.astype(np.float32)
    finite = np.isfinite(a)
    if not finite.any():
        return np.zeros(arr.shape, dtype=np.uint8)
    lo, hi = np.percentile(a[finite], (2.0, 98.0))
    if hi > lo:
        a = np.clip(((a - lo) / (hi - lo)) * 255.0, 0, 255)
    else:
        a = np.zeros_like(a)
    return a.astype(np.uint8)


@pytest.mark.skipif(int(np.__version__.split(".")[0]) < 2, reason="the definition is numpy >= 2's float64 evaluation (NEP 50)")
@pytest.mark.parametrize("dtype", [np.uint16, np.int16, np.float32])
def test_restated_to_uint8_equals_reference_expression(dtype):
    rng = np.random.default_rng(3)
    for shape in ((1, 1), (3, 5), (97, 131), (256, 300)):
        if dtype == np.float32:
            a = (rng.standard_normal(shape) * 700 + 2000).astype(np.float32)
            a[rng.random(shape) < 0.05] = np.nan
            a[rng.random(shape) < 0.02] = np.inf
            a[rng.random(shape) < 0.02] = -np.inf
        else:
            a = rng.integers(-3000 if dtype == np.int16 else 0, 9000, shape).astype(dtype)
        with np.errstate(invalid="ignore"):
            exp = _reference_to_uint8(a)
        got = R.to_uint8_percentile(a)
        if dtype == np.float32:
            keep = ~np.isnan(a)       # NaN -> uint8 is undefined in C; the definition says 0 and x86 numpy agrees, other CPUs may not
            assert (got[~keep] == 0).all()
            np.testing.assert_array_equal(got[keep], exp[keep])
        else:
            np.testing.assert_array_equal(got, exp)
    assert (R.to_uint8_percentile(np.full((4, 4), np.nan, np.float32)) == 0).all()
    assert (R.to_uint8_percentile(np.full((4, 4), 7, dtype)) == 0).all()                  # hi <= lo
    u8 = rng.integers(0, 256, (5, 5), dtype=np.uint8)
    assert R.to_uint8_percentile(u8) is u8


def _round_half_even_sat(x):
    return int(min(255, max(0, round(x))))     # Python's round: half to even


def test_clahe_constant_image_closed_form():
    # 64 x 64 on 8 x 8: tiles of 8 x 8 = 64 px, clip = max(int(2 * 64 / 256), 1) = 1.  The one occupied bin is cut to 1, 63 are left
    # over: batch 0, residual 63, step 256 // 63 = 4 -> bins 0, 4, ..., 248 get one each.  cum(i) = min(i // 4 + 1, 63) + [i >= c];
    # every tile has the same LUT, so the blend returns LUT[c] = round(cum(c) * 255 / 64).
    for c in (0, 3, 100, 249, 255):
        img = np.full((64, 64), c, np.uint8)
        exp = _round_half_even_sat((min(c // 4 + 1, 63) + 1) * 255 / 64)
        assert (R.clahe(img, 2.0, (8, 8)) == exp).all(), c
        lut = R.clahe_luts(img, 2.0, (8, 8))[3, 5]
        assert [int(v) for v in lut[:6]] == [_round_half_even_sat((min(i // 4 + 1, 63) + (i >= c)) * 255 / 64) for i in range(6)]
    # no clipping: the LUT is the scaled cumulative histogram, a step at c
    img = np.full((64, 64), 100, np.uint8)
    assert (R.clahe(img, 0.0, (8, 8)) == 255).all()
    lut = R.clahe_luts(img, 0.0, (8, 8))[0, 0]
    assert (lut[:100] == 0).all() and (lut[100:] == 255).all()


def test_clahe_two_level_image_closed_form():
    # 64 x 64 on 2 x 2: tiles of 32 x 32 = 1024 px, clip = int(2 * 1024 / 256) = 8.  A checkerboard of a and b puts 512 of each into
    # every tile: excess 2 * 504 = 1008, batch 3, residual 240, step 1 -> bins 0 .. 239 get one more.
    a, b = 40, 200
    yy, xx = np.mgrid[0:64, 0:64]
    img = np.where((yy + xx) % 2 == 0, a, b).astype(np.uint8)

    def cum(i):
        return 3 * (i + 1) + min(i + 1, 240) + 8 * (i >= a) + 8 * (i >= b)

    assert cum(255) == 1024
    lut = R.clahe_luts(img, 2.0, (2, 2))
    for t in lut.reshape(4, 256):
        assert [int(v) for v in t] == [_round_half_even_sat(cum(i) * 255 / 1024) for i in range(256)]
    out = R.clahe(img, 2.0, (2, 2))
    assert (out[img == a] == _round_half_even_sat(cum(a) * 255 / 1024)).all()
    assert (out[img == b] == _round_half_even_sat(cum(b) * 255 / 1024)).all()


def _clahe_scalar(img, clip_limit, tiles_x, tiles_y):
    """CLAHE pixel by pixel with float32 scalars: a second, loop-shaped writing of the definition (divisible shapes only)."""
    f = np.float32
    H, W = img.shape
    th, tw = H // tiles_y, W // tiles_x
    area = th * tw
    clip = max(int(clip_limit * area / 256), 1) if clip_limit > 0 else 0
    scale = f(255.0) / f(area)
    luts = {}
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            hist = [0] * 256
            for v in img[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].reshape(-1):
                hist[int(v)] += 1
            if clip:
                excess = sum(max(h - clip, 0) for h in hist)
                hist = [min(h, clip) + excess // 256 for h in hist]
                residual = excess % 256
                if residual:
                    step = max(256 // residual, 1)
                    i = 0
                    while i < 256 and residual > 0:
                        hist[i] += 1
                        i += step
                        residual -= 1
            s, lut = 0, []
            for h in hist:
                s += h
                lut.append(f(min(255, max(0, int(np.rint(f(s) * scale))))))
            luts[ty, tx] = lut
    out = np.empty_like(img)
    for y in range(H):
        tyf = f(y) * (f(1.0) / f(th)) - f(0.5)
        ty1 = int(np.floor(tyf)); ya = tyf - f(ty1); ya1 = f(1.0) - ya
        ty2 = min(ty1 + 1, tiles_y - 1); ty1 = max(ty1, 0)
        for x in range(W):
            txf = f(x) * (f(1.0) / f(tw)) - f(0.5)
            tx1 = int(np.floor(txf)); xa = txf - f(tx1); xa1 = f(1.0) - xa
            tx2 = min(tx1 + 1, tiles_x - 1); tx1 = max(tx1, 0)
            v = int(img[y, x])
            res = (luts[ty1, tx1][v] * xa1 + luts[ty1, tx2][v] * xa) * ya1 + (luts[ty2, tx1][v] * xa1 + luts[ty2, tx2][v] * xa) * ya
            assert type(res) is np.float32
            out[y, x] = min(255, max(0, int(np.rint(res))))
    return out


def test_clahe_16x16_on_2x2_listed():
    # four 8 x 8 tiles (64 px, clip 1 when clip_limit = 2) holding ramps of different slopes
    yy, xx = np.mgrid[0:16, 0:16]
    img = ((yy * 16 + xx) * np.where(xx < 8, 1, 0.5) + np.where(yy < 8, 0, 20)).astype(np.uint8)
    for clip_limit in (2.0, 0.0, 40.0):
        out = R.clahe(img, clip_limit, (2, 2))
        np.testing.assert_array_equal(out, _clahe_scalar(img, clip_limit, 2, 2))
        lut = R.clahe_luts(img, clip_limit, (2, 2))
        # a corner pixel lies outside every tile centre: both neighbours clamp to its own tile, the blend returns that tile's LUT entry
        for (y, x), (ty, tx) in (((0, 0), (0, 0)), ((0, 15), (0, 1)), ((15, 0), (1, 0)), ((15, 15), (1, 1))):
            assert out[y, x] == lut[ty, tx, img[y, x]]
    # the top-left tile without clipping: values 0 .. 7, 16 .. 23, ..., one pixel each: LUT[v] = round(#(pixels <= v) * 255 / 64)
    lut00 = R.clahe_luts(img, 0.0, (2, 2))[0, 0]
    vals = sorted(int(v) for v in img[:8, :8].reshape(-1))
    assert [int(lut00[v]) for v in (0, 7, 8, 16, 119, 255)] == [_round_half_even_sat(sum(u <= v for u in vals) * 255 / 64) for v in (0, 7, 8, 16, 119, 255)]


def test_clahe_indivisible_shape_extends_both_dimensions():
    # 17 x 16 on 2 x 2: H is not divisible, so OpenCV extends BOTH: the bottom by 2 - 17 % 2 = 1 row and the right by a whole
    # tilesX = 2 columns (16 % 2 == 0 notwithstanding) -> 18 x 18, tiles of 9 x 9
    assert R.clahe_geometry(17, 16, 0.0, 2, 2)[:4] == (18, 18, 9, 9)
    assert R.clahe_geometry(16, 16, 0.0, 2, 2)[:4] == (16, 16, 8, 8)
    assert R.clahe_geometry(389, 517, 2.0, 8, 8)[:4] == (392, 520, 49, 65)
    assert R.clahe_geometry(512, 389, 2.0, 8, 8)[:4] == (520, 392, 65, 49)                # 512 % 8 == 0 and still extended by 8
    img = np.random.default_rng(5).integers(0, 256, (17, 16), dtype=np.uint8)
    ext = np.pad(img, ((0, 1), (0, 2)), mode="reflect")                                   # numpy's 'reflect' is BORDER_REFLECT_101
    assert ext.shape == (18, 18) and (ext[:, 16] == ext[:, 14]).all() and (ext[:, 17] == ext[:, 13]).all() and (ext[17] == ext[15]).all()
    lut = R.clahe_luts(img, 0.0, (2, 2))
    for ty in range(2):
        for tx in range(2):
            cum = np.cumsum(np.bincount(ext[ty * 9:(ty + 1) * 9, tx * 9:(tx + 1) * 9].reshape(-1), minlength=256))
            exp = [_round_half_even_sat(int(c) * 255 / 81) for c in cum]
            got = [int(v) for v in lut[ty, tx]]
            # (255 / 81 is not a float32: the definition multiplies by float32(255) / float32(81); none of these products sits on a tie)
            assert got == exp
    for bad in ((1, 16, 2, 2), (3, 3, 8, 8), (16, 16, 32, 16), (16, 16, 0, 2)):
        with pytest.raises(ValueError):
            R.clahe_geometry(bad[0], bad[1], 2.0, bad[2], bad[3])


def test_clahe_and_preprocess_equal_cv2_when_present():
    cv2 = pytest.importorskip("cv2")   # absent here: parity with cv2 stays unpinned in DESIGN section 2's sense
    rng = np.random.default_rng(9)
    for shape, grid, clip in (((512, 512), (8, 8), 2.0), ((389, 517), (8, 8), 2.0), ((512, 389), (4, 2), 40.0), ((200, 300), (16, 16), 0.0)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        np.testing.assert_array_equal(R.clahe(img, clip, grid), cv2.createCLAHE(clipLimit=clip, tileGridSize=grid).apply(img))
    raw = rng.integers(0, 9000, (389, 517)).astype(np.uint16)
    np.testing.assert_array_equal(R.preprocess(raw), cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)).apply(_reference_to_uint8(raw)))
