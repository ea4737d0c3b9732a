"""numpy restatement of KariosAPI.analyze_accuracy's arithmetic (karios/api/core.py:268-328): the valid-pixel count (:284-290) and
GeometricStat (karios/accuracy_analysis/accuracy_statistics.py:82-238) for float32 columns, as libkarios_hip.so computes them
(csrc/accuracy_math.hpp, k_accuracy.hip).

This is the DEFINITION the library is held to, bit for bit (tests/test_gpu_accuracy.py); tests/test_accuracy_host.py holds it to
the installed numpy / pandas and to the recorded results of the reference (tests/golden/accuracy.npz).  Every float32 operation
is spelled out one rounding at a time, so the definition does not move with the numpy version.  Points marked [np2] come from
knowledge of numpy 2.x's sources (umath/loops_utils.h.src `pairwise_sum`, core/_methods.py `_mean` / `_var`,
lib/_function_base_impl.py `_median`), [pd] from pandas 2.x's (`Series.gt` on a float32 column), [ref] from the reference's
expressions, [def] are choices of this project where the reference's result is not one fixed bit pattern.

Test infrastructure only: karios_amd never imports this module.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
BLOCK = 8192      # [np2] np.getbufsize(): elements the add loop sees per call of a buffered reduction
LEAF = 128        # [np2] PW_BLOCKSIZE


# ---- the sample --------------------------------------------------------------------------------------------------------------------
def threshold_as_double(t):
    """The float64 the library compares (double)score against.  [pd] `Series.gt(python float)` on a float32 column compares in
    float32 against float32(t): a score equal to float32(0.4) does not pass.  An np.float64 threshold makes the comparison float64:
    that same score passes (float32(0.4) > 0.4).  Both are one float64 comparison with the right constant."""
    if isinstance(t, np.float64):
        return float(t)
    return float(f32(t))


def sample(dx, dy, score, t, carto=False):
    """[ref :70-99] rows with score > t in row order; carto negates dy (exactly) before anything else."""
    dx, dy, score = (np.asarray(a, f32) for a in (dx, dy, score))
    keep = score.astype(np.float64) > threshold_as_double(t)
    return dx[keep], (-dy if carto else dy)[keep], score[keep]


# ---- the float32 sum ---------------------------------------------------------------------------------------------------------------
def leaf_sum(a):
    """[np2] pairwise_sum for n <= 128.  n < 8: left to right from -0 (numpy >= 1.25; the start cannot show in a result: the
    reduction's own accumulator is +0).  Else eight accumulators, ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)), the remainder left to right."""
    n = a.size
    if n < 8:
        res = f32(-0.0)
        for v in a:
            res = f32(res + v)
        return res
    m = n - n % 8
    r = a[:8].copy()
    for i in range(8, m, 8):
        r = r + a[i:i + 8]                       # float32 + float32, element by element
    res = f32(f32(f32(r[0] + r[1]) + f32(r[2] + r[3])) + f32(f32(r[4] + r[5]) + f32(r[6] + r[7])))
    for v in a[m:]:
        res = f32(res + v)
    return res


def block_sum(a):
    """[np2] pairwise_sum: above 128 elements split at n2 = n/2 - (n/2) % 8 and add the halves."""
    n = a.size
    if n <= LEAF:
        return leaf_sum(a)
    n2 = n // 2
    n2 -= n2 % 8
    return f32(block_sum(a[:n2]) + block_sum(a[n2:]))


def sum_f32(a):
    """np.add.reduce of a contiguous float32 array: [np2] the block sums of 8192 elements each, added left to right into a float32
    accumulator that starts at +0 (all-zero and all-negative-zero input give +0)."""
    a = np.ascontiguousarray(a, f32)
    acc = f32(0.0)
    with np.errstate(all="ignore"):
        for b in range(0, a.size, BLOCK):
            acc = f32(acc + block_sum(a[b:b + BLOCK]))
    return acc


def sum_left_to_right(a):
    """NOT numpy's order: what a plain loop gives (the tests show that it differs where the order matters)."""
    acc = f32(0.0)
    for v in np.asarray(a, f32):
        acc = f32(acc + v)
    return acc


# ---- mean, std, min, max, median ---------------------------------------------------------------------------------------------------
def mean_f32(a):
    """[np2 _mean] sum / float32(n): one correctly rounded float32 division."""
    with np.errstate(all="ignore"):
        return f32(sum_f32(a) / f32(a.size))


def std_f32(a):
    """[np2 _var] d = a - mean and d * d each rounded to float32, their sum as above, / float32(n), the float32 square root."""
    a = np.asarray(a, f32)
    with np.errstate(all="ignore"):
        d = a - mean_f32(a)
        return f32(np.sqrt(f32(sum_f32(d * d) / f32(a.size))))


def median_f32(a):
    """[np2 _median] odd n: the sorted element n // 2; even n: float32(float32(lo + hi) / 2).  A NaN makes it NaN."""
    a = np.asarray(a, f32)
    if np.isnan(a).any():
        return f32(np.nan)
    s = np.sort(a)
    n = s.size
    if n & 1:
        return s[n // 2]
    with np.errstate(all="ignore"):
        return f32(f32(s[n // 2 - 1] + s[n // 2]) / f32(2))


STAT_NAMES = tuple(f"{k}_{col}" for col in "xyc" for k in ("min", "max", "median", "mean", "std"))
BY_VALUE = tuple(i for i, name in enumerate(STAT_NAMES) if name.split("_")[0] in ("min", "max", "median"))   # [def] sign of a zero unpinned


def column_stats(a):
    """-> [min, max, median, mean, std] as float32 ([ref :135-151]).  A NaN poisons min / max / median / mean like numpy's."""
    a = np.asarray(a, f32)
    if np.isnan(a).any():
        lo = hi = f32(np.nan)
    else:
        lo, hi = a.min(), a.max()
    return [lo, hi, median_f32(a), mean_f32(a), std_f32(a)]


def statistics(dx, dy, score, t, carto=False):
    """-> (sample size, 15 float32 in STAT_NAMES order, or None for an empty sample [ref :133, :154-156])."""
    x, y, c = sample(dx, dy, score, t, carto)
    if x.size == 0:
        return 0, None
    return x.size, np.array(column_stats(x) + column_stats(y) + column_stats(c), f32)


# ---- CE ----------------------------------------------------------------------------------------------------------------------------
def radial(x, y, factor):
    """[ref :225-229] sqrt(x x + y y) with x = dx float32(factor), y = dy float32(factor): five float32 roundings per row."""
    fx = f32(factor)
    with np.errstate(all="ignore"):
        xs, ys = x * fx, y * fx
        return np.sqrt(xs * xs + ys * ys)


def ce_ranks(percent, n):
    """[ref :231-236] p = percent * n (float64), k = int(p) -> (k - 1 with -1 = the last, k, p - k); IndexError where k is none."""
    if n == 0:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0")
    p = float(percent) * n
    k = int(p)
    if k >= n or k < 0:
        raise IndexError(f"index {k} is out of bounds for axis 0 with size {n}")
    return (k - 1) % n, k, p - k


def ce(x, y, percent, factor):
    """compute_percentile(percent, factor) for a Python-float or float32 factor [ref :224-238]:
    float32(r[k-1] + float32(float32(r[k] - r[k-1]) * float32(p - k))) on the sorted radial errors."""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    lo, hi, frac = ce_ranks(percent, x.size)
    r = np.sort(radial(x, y, factor))
    with np.errstate(all="ignore"):
        return f32(r[lo] + f32(f32(r[hi] - r[lo]) * f32(frac)))


# ---- valid pixels ------------------------------------------------------------------------------------------------------------------
def count_valid_pixels(arr, mask=None):
    """[ref core.py:284-290] pixels that are non-zero and, with a mask, whose mask byte is non-zero.  float32 by the bits:
    (bits & 0x7fffffff) != 0 - NaN and denormals count, -0.0 does not."""
    a = np.ascontiguousarray(arr)
    nz = (a.view(np.uint32) & np.uint32(0x7FFFFFFF)) != 0 if a.dtype == np.float32 else a != 0
    if mask is not None:
        nz = nz & (np.asarray(mask) != 0)
    return int(np.count_nonzero(nz))
