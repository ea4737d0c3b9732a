"""The definition of the mutual-information search around each key point (km_mi_search, csrc/mi_search_math.hpp), in numpy and Python ints.

The reference has no such search; what it does define is every number the search is made of: `MutualInfoService._mutual_info`
(karios/matcher/mutual_info_service.py:32-63) and `ZNCCService._mutual_information` (zncc_service.py:129-151) are the two values at an
offset, both from `np.histogram2d(chip_ref, chip_mon, bins=32)` on the 57 x 57 chips, and `_compute_mutual_info` (:99-130) gives the
centres and the rule by which a row is skipped.  This file restates them:

* centres and skip rule: tests/zncc_search_restatement.py `centres` (= tests/score_restatement.py `chips`), unchanged;
* the table of counts: tests/score_restatement.py `mi_counts` (`int_bins`, `float_bins`) - the reference chip's bins fixed per row, the
  monitored chip's range and bins taken anew at every offset;
* from counts to value, exactly: T[c] = round_half_even(c ln c 2^36) as Python ints (`decimal`, 60 digits), L = T[3249],
  num = 2 L - Sx - Sy, den = L - Sxy with Sx, Sy, Sxy the sums of T over the row marginals, the column marginals and the cells;
  Studholme's NMI = float(num) / float(den), NaN iff den == 0; the `mi_score` formula = float(2 (num - den)) / float(num), NaN iff
  num == 0.  Every integer stays below 2^53, so each value is ONE correctly rounded float64 division: a function of the pixels alone;
* peak and sub-pixel step: tests/zncc_search_restatement.py `finish`, unchanged, on the Studholme surface.
"""
import decimal
import functools
from collections import namedtuple

import numpy as np

import score_restatement as SR
import zncc_search_restatement as ZR
from zncc_search_restatement import MAX_RADIUS, MAX_ROWS, NO_VALUE, RIM_X, RIM_Y, SKIPPED, centres  # noqa: F401

CHIP, MARGIN, NPX, BINS, SCALE_BITS = 57, 28, 57 * 57, 32, 36
Result = namedtuple("Result", "offset peak peak_mi shift status surface surface_mi")


@functools.lru_cache(maxsize=None)
def table():
    """T[c] for c = 0 .. 3249 as Python ints."""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        scale = decimal.Decimal(1 << SCALE_BITS)
        return tuple([0, 0] + [int((decimal.Decimal(c) * decimal.Decimal(c).ln() * scale).to_integral_value(rounding=decimal.ROUND_HALF_EVEN))
                               for c in range(2, NPX + 1)])


@functools.lru_cache(maxsize=None)
def _table_array():
    return np.array(table(), np.int64)


def sums(counts):
    """(num, den) of a 32 x 32 table of counts, as Python ints."""
    T = _table_array()
    counts = np.asarray(counts, np.int64)
    L = int(T[NPX])
    Sx, Sy, Sxy = int(T[counts.sum(axis=1)].sum()), int(T[counts.sum(axis=0)].sum()), int(T[counts].sum())
    return 2 * L - Sx - Sy, L - Sxy


def values(counts):
    """(Studholme's NMI, the mi_score formula) of a table of counts; (NaN, NaN) for None."""
    if counts is None:
        return float("nan"), float("nan")
    num, den = sums(counts)
    assert 0 <= den <= num < 2 ** 53 and 0 <= 2 * (num - den) < 2 ** 53
    return (float(num) / float(den) if den else float("nan")), (float(2 * (num - den)) / float(num) if num else float("nan"))


def chip_inside(x, y, shape):
    """The reference's bounds rule for a chip centred at column x, row y."""
    return not (x - MARGIN < 0 or y - MARGIN < 0 or x >= shape[1] - MARGIN or y >= shape[0] - MARGIN)


def chip(img, x, y):
    return img[y - MARGIN:y + MARGIN + 1, x - MARGIN:x + MARGIN + 1]


def bins(c):
    """Bins of one chip by the existing rules, or None for a float32 chip with a non-finite sample."""
    c = np.asarray(c)
    if c.dtype.kind == "f":
        return SR.float_bins(c) if np.isfinite(c).all() else None
    return SR.int_bins(c)


def surfaces(ref, mon, X0, Y0, X1, Y1, R):
    """Both values at every offset -> (S x S Studholme, S x S mi_score formula)."""
    S = 2 * R + 1
    z, zmi = np.full((S, S), np.nan), np.full((S, S), np.nan)
    b1 = bins(chip(ref, X0, Y0))
    if b1 is None:                                               # a non-finite sample in the reference chip: the whole row
        return z, zmi
    for oy in range(-R, R + 1):
        for ox in range(-R, R + 1):
            x, y = X1 + ox, Y1 + oy
            if not chip_inside(x, y, mon.shape):
                continue
            b2 = bins(chip(mon, x, y))                           # the monitored chip's range and bins: anew at every offset
            if b2 is None:
                continue
            counts = np.bincount(b1 * BINS + b2, minlength=BINS * BINS).reshape(BINS, BINS)
            z[oy + R, ox + R], zmi[oy + R, ox + R] = values(counts)
    return z, zmi


def search(ref, mon, x0, y0, dx, dy, radius):
    """All rows -> Result of numpy arrays (both surfaces always)."""
    ref, mon = np.asarray(ref), np.asarray(mon)
    if not 1 <= radius <= MAX_RADIUS or len(x0) > MAX_ROWS or ref.dtype != mon.dtype or ref.dtype not in [np.dtype(t) for t in SR.TYPES]:
        raise ValueError("mi_search: radius 1 .. 8, at most 2^20 rows, one pixel type of uint8, uint16, int16, float32")
    n, S = len(x0), 2 * radius + 1
    out = Result(np.zeros((n, 2), np.int32), np.full(n, np.nan), np.full(n, np.nan), np.full((n, 2), np.nan), np.zeros(n, np.uint8),
                 np.full((n, S, S), np.nan), np.full((n, S, S), np.nan))
    for k in range(n):
        c = centres(x0[k], y0[k], dx[k], dy[k], ref.shape, mon.shape)
        if c is None:
            out.status[k] = SKIPPED
            continue
        z, zmi = surfaces(ref, mon, *c, radius)
        out.surface[k], out.surface_mi[k] = z, zmi
        out.offset[k], out.peak[k], out.shift[k], out.status[k] = ZR.finish(z, radius, *c)
        if not out.status[k] & NO_VALUE:
            out.peak_mi[k] = zmi[out.offset[k, 1] + radius, out.offset[k, 0] + radius]
    return out
