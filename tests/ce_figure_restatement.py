"""numpy restatement of the numbers `CircularErrorPlot._plot` hands to matplotlib (karios/report/circular_error_plot.py:181-228,
254-303, 305-357, 359-368) for float32 columns and a Python-float resolution, as libkarios_hip.so computes them (csrc/ce_math.hpp,
k_ce.hip) around the two host steps that stay numpy's and scipy's own: `np.linspace` for the bin edges and the spline FIT.

This is the DEFINITION the library is held to, bit for bit (tests/test_gpu_ce_figure.py); tests/test_ce_figure_host.py holds it to
the installed numpy / scipy and to the recorded results of the reference (tests/golden/ce_figure.npz).  Every float operation is
one rounding per line.  Points marked [np2] come from numpy 2.x's sources (lib/_histograms_impl.py `_get_outer_edges`,
`_get_bin_edges`, `_hist_bin_sqrt`, `histogram`, `histogramdd`), [fp] from FITPACK's (`bispeu`, `fpbisp`, `fpbspl`, as scipy's
`RectBivariateSpline.ev` calls them), [sp] from scipy's `interpn(method="splinef2d")`, [ref] from the reference's expressions,
[def] are choices of this project where the reference's result is not one fixed bit pattern.

Test infrastructure only: karios_amd never imports this module.
"""
from __future__ import annotations

import numpy as np

import accuracy_restatement as A

f32 = np.float32
f64 = np.float64
GRID = 10            # [ref :267] bins of the density per axis
LDS_BINS = 4095      # csrc/ce_math.hpp: bins of an axis histogram a workgroup keeps in LDS
MAX_BINS = 65536     # ... and bins the device form takes (KM_CE_MAX_BINS)


# ---- the sample ---------------------------------------------------------------------------------------------------------------------
def scaled_sample(dx, dy, score, t, res, carto=False):
    """[ref :204, :257-258] -> (dx, +-dy, x, y) of the rows with score > t: x = dx * float32(res), one float32 product each (NEP 50:
    `res` is a Python float)."""
    u, v, _c = A.sample(dx, dy, score, t, carto)
    if u.size == 0:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")     # [ref :185] np.max of nothing
    r = f32(res)
    with np.errstate(all="ignore"):
        return u, v, u * r, v * r


# ---- the axis histograms --------------------------------------------------------------------------------------------------------------
def axis_range(v, res):
    """[ref :185, :206] the range from the UNSCALED column: v_max = max(|max|, |min|) in float32, (-v_max * res, v_max * res)."""
    v_max = max(f32(abs(v.max())), f32(abs(v.min())))
    last = f32(v_max * f32(res))
    return f32(-last), last


def axis_edges(x, first, last):
    """[np2 _get_bin_edges, bins="sqrt"] -> (first, last, float32 edges).  Equal bounds widen by 0.5; the width is a float64 (np.sqrt of
    a Python int); the edges are numpy's own linspace."""
    if first == last:
        first, last = f32(first - f32(0.5)), f32(last + f32(0.5))
    assert bool(np.all((x >= first) & (x <= last)))              # rounding is monotonic: the scaled column lies inside the scaled range
    ptp = f32(x.max() - x.min())
    width = f64(ptp) / np.sqrt(f64(x.size))
    n_bins = int(np.ceil(f64(f32(last - first)) / width)) if width else 1
    edges = np.linspace(first, last, n_bins + 1, endpoint=True, dtype=f32)
    if np.any(edges[:-1] >= edges[1:]):
        raise ValueError(f"Too many bins for data range. Cannot create {n_bins} finite-sized bins.")
    return first, last, edges


def axis_counts(x, first, last, edges):
    """[np2 histogram, uniform bins] the float32 index with numpy's three corrections -> int64 counts."""
    nb = edges.size - 1
    denom = f32(last - first)
    d = x - first
    q = d / denom
    f = q * f32(nb)
    idx = f.astype(np.intp)
    idx[idx == nb] -= 1
    idx[x < edges[idx]] -= 1
    idx[(x >= edges[idx + 1]) & (idx != nb - 1)] += 1
    return np.bincount(idx, minlength=nb).astype(np.int64)


def axis_histogram(v, x, res):
    """`_compute_histogram` [ref :181-228] for the unscaled column v and its scaled x -> (int64 counts, float32 edges)."""
    first, last, edges = axis_edges(x, *axis_range(v, res))
    return axis_counts(x, first, last, edges), edges


def gaussian(x):
    """[ref :335-336] np.mean and np.std of the SCALED column, in float32."""
    return A.mean_f32(x), A.std_f32(x)


# ---- the density of the scatter -----------------------------------------------------------------------------------------------------
def grid_edges(v):
    """[np2 histogramdd] GRID + 1 float32 edges over [min, max], widened by 0.5 when they are equal; numpy's own linspace."""
    lo, hi = v.min(), v.max()
    if lo == hi:
        lo, hi = f32(lo - f32(0.5)), f32(hi + f32(0.5))
    e = np.linspace(lo, hi, GRID + 1)
    assert e.dtype == f32
    return e


def grid_bin(v, e):
    """[np2 histogramdd] searchsorted(e, v, side="right"), the value on the last edge pulled into the last bin -> bin 0 .. GRID - 1."""
    k = (e[None, :] <= v[:, None]).sum(axis=1)
    k[v == e[-1]] -= 1
    return k - 1


def grid_counts(x, y, ex, ey):
    bx, by = grid_bin(x, ex), grid_bin(y, ey)
    ok = (bx >= 0) & (bx < GRID) & (by >= 0) & (by < GRID)
    return np.bincount(bx[ok] * GRID + by[ok], minlength=GRID * GRID).reshape(GRID, GRID).astype(f64)


def centres(e):
    """[ref :271] 0.5 * (e[1:] + e[:-1]) in float32."""
    return f32(0.5) * (e[1:] + e[:-1])


def fit(cx, cy, counts):
    """The spline FIT is scipy's own (100 numbers in; 14 + 14 knots and 100 coefficients out); whatever it raises passes through."""
    from scipy.interpolate import RectBivariateSpline
    tx, ty, c = RectBivariateSpline(cx, cy, counts).tck
    return np.asarray(tx, f64), np.asarray(ty, f64), np.asarray(c, f64)


def _bspline4(t, x):
    """[fp fpbisp + fpbspl, k = 3] clamp to [t[3], t[n - 4]], the interval by a linear search from the left, de Boor's recurrence with
    the Fortran text's operand order -> (l - 4, h[4]) per point, float64."""
    n = t.size
    arg = np.where(x < t[3], t[3], x)
    arg = np.where(arg > t[n - 4], t[n - 4], arg)
    l = np.full(x.shape, 4, np.intp)                      # FITPACK's one-based l
    go = np.ones(x.shape, bool)
    for j in range(4, n - 4):                             # while not (arg < t(l + 1) or l == n - 4): l += 1
        go = go & ~(arg < t[j])
        l = l + go
    h = np.zeros((4,) + x.shape, f64)
    h[0] = 1.0
    for j in range(1, 4):
        hh = h[:j].copy()
        h[0] = 0.0
        for i in range(1, j + 1):
            tli, tlj = t[l + i - 1], t[l + i - j - 1]
            same = tli == tlj
            with np.errstate(all="ignore"):
                f = hh[i - 1] / (tli - tlj)
                a = f * (tli - arg)
                a = h[i - 1] + a
                b = f * (arg - tlj)
            h[i - 1] = np.where(same, h[i - 1], a)
            h[i] = np.where(same, 0.0, b)
    return l - 4, h


def bispeu(tx, ty, c, x, y):
    """[fp fpbisp] sp = sp + c * wx[i] * wy[j], i outer, j inner, from 0; float64."""
    lx, wx = _bspline4(tx, x)
    ly, wy = _bspline4(ty, y)
    sp = np.zeros(x.shape, f64)
    for i in range(4):
        for j in range(4):
            term = c[(lx + i) * GRID + ly + j] * wx[i]
            term = term * wy[j]
            sp = sp + term
    return sp


def density(tx, ty, c, cx, cy, x, y):
    """[sp interpn] the spline inside [cx[0], cx[-1]] x [cy[0], cy[-1]] (float32 comparisons), NaN outside, rounded to float32."""
    inside = (cx[0] <= x) & (x <= cx[-1]) & (cy[0] <= y) & (y <= cy[-1])
    z = np.full(x.shape, np.nan, f32)
    z[inside] = bispeu(tx, ty, c, x[inside].astype(f64), y[inside].astype(f64)).astype(f32)
    return z


def drawing_order(z):
    """[def] numpy's `z.argsort()` is not stable; the definition is the stable ascending order by (z, row), -0 equal to +0, NaN last."""
    return np.argsort(z, kind="stable")


# ---- the whole figure -----------------------------------------------------------------------------------------------------------------
class Figure:
    pass


def figure(dx, dy, score, t, res, carto=False):
    """Everything `_plot` hands to matplotlib, by the names of ops.ce_figure's result."""
    u, v, x, y = scaled_sample(dx, dy, score, t, res, carto)
    r = Figure()
    r.sample = int(x.size)
    r.hist_x, r.bins_x = axis_histogram(u, x, res)
    r.hist_y, r.bins_y = axis_histogram(v, y, res)
    (r.mu_x, r.sigma_x), (r.mu_y, r.sigma_y) = gaussian(x), gaussian(y)
    r.x_edges, r.y_edges = grid_edges(x), grid_edges(y)
    r.counts2d = grid_counts(x, y, r.x_edges, r.y_edges)
    cx, cy = centres(r.x_edges), centres(r.y_edges)
    z = density(*fit(cx, cy, r.counts2d), cx, cy, x, y)
    idx = drawing_order(z)
    r.scatter_x, r.scatter_y, r.scatter_z = x[idx], y[idx], z[idx]
    r.radial = np.sort(A.radial(u, v, res))                     # [ref :363] == sqrt(x x + y y): the same five float32 roundings
    r.plot_limit = max(np.abs(x).max(), np.abs(y).max())        # [ref :262-265]
    r.ce90, r.ce95 = A.ce(u, v, 0.9, res), A.ce(u, v, 0.95, res)
    return r


FIELDS = ("hist_x", "bins_x", "hist_y", "bins_y", "mu_x", "sigma_x", "mu_y", "sigma_y", "scatter_x", "scatter_y", "scatter_z", "counts2d",
          "x_edges", "y_edges", "radial", "plot_limit", "ce90", "ce95")
