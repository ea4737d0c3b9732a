"""Inputs and comparisons the CPU and the GPU tests of the circular-error figure's numbers share (tests/test_ce_figure_host.py,
tests/test_gpu_ce_figure.py): fresh frames by kind, the reference's expressions written out on numpy / scipy, comparison by bits.

Test infrastructure only: karios_amd never imports this module."""
import warnings

import numpy as np

import ce_figure_restatement as R

f32 = np.float32
THRESHOLD = 0.4
KINDS = ("normal", "quantised", "far", "equal", "carto")


def fresh(kind, n_sample, seed=0):
    """-> (dx, dy, score, carto): exactly `n_sample` rows lie above THRESHOLD, the others (one in three, mixed in) below.
    normal: noise around a small offset.  quantised: displacements on a grid of 1 / 8, so that points sit exactly on edges.  far: a
    narrow sample far from zero (many bins: thousands for a few hundred rows).  equal: one value.  carto: normal, dy negated."""
    rng = np.random.default_rng(1000 * seed + n_sample + 17 * KINDS.index(kind))
    n = n_sample + n_sample // 2 + 2
    score = np.full(n, f32(0.25))
    score[rng.permutation(n)[:n_sample]] = (rng.integers(27, 65, n_sample) / 64).astype(f32)
    if kind == "quantised":
        dx, dy = np.round(rng.standard_normal(n) * 2 * 8) / 8, np.round(rng.standard_normal(n) * 3 * 8) / 8
    elif kind == "far":
        dx, dy = 20 + rng.standard_normal(n) * 0.02, -7 + rng.standard_normal(n) * 0.01
    elif kind == "equal":
        dx, dy = np.full(n, 0.25), np.full(n, -0.5)
    else:
        dx, dy = rng.standard_normal(n) * 1.5 + 0.2, rng.standard_normal(n) * 0.8 - 0.1
    return dx.astype(f32), dy.astype(f32), score, kind == "carto"


def beyond_the_cap(n_sample=100):
    """A sample whose x histogram has more bins than the device takes (2 * 1000 * sqrt(100) / 0.1 = 200 000); y stays small."""
    dx, dy, score, _ = fresh("normal", n_sample, seed=5)
    dx = (1000 + np.linspace(-0.05, 0.05, dx.size)).astype(f32)
    return dx, dy, score, False


def numpy_figure(dx, dy, score, t, res, carto=False):
    """The reference's expressions (circular_error_plot.py:185-207, 256-280, 335-336, 360-368; accuracy_statistics.py:224-238),
    written out on the installed numpy / scipy; the drawing order is the definition's stable one."""
    from scipy.interpolate import interpn
    keep = score > t
    vx, vy = dx[keep], (-dy if carto else dy)[keep]
    r = R.Figure()
    r.sample = int(vx.size)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for axis, vect in (("x", vx), ("y", vy)):
            v_max = np.max([np.abs(np.max(vect)), np.abs(np.min(vect))])
            hist, bins = np.histogram(vect * res, bins="sqrt", range=(-v_max * res, v_max * res))
            setattr(r, f"hist_{axis}", hist), setattr(r, f"bins_{axis}", bins)
            setattr(r, f"mu_{axis}", np.mean(vect * res)), setattr(r, f"sigma_{axis}", np.std(vect * res))
        x, y = vx * res, vy * res
        r.plot_limit = np.max([np.max(np.abs(x)), np.max(np.abs(y))])
        r.counts2d, r.x_edges, r.y_edges = np.histogram2d(x, y, bins=10)
        z = interpn((0.5 * (r.x_edges[1:] + r.x_edges[:-1]), 0.5 * (r.y_edges[1:] + r.y_edges[:-1])), r.counts2d, np.vstack([x, y]).T,
                    method="splinef2d", bounds_error=False)
        idx = np.argsort(z, kind="stable")
        r.scatter_x, r.scatter_y, r.scatter_z = x[idx], y[idx], z[idx]
        v = np.sort(np.sqrt(x * x + y * y))
        r.radial = v
        ce = []
        for percent in (0.9, 0.95):
            p = percent * v.size
            k = int(p)
            ce.append(v[k - 1] + (v[k] - v[k - 1]) * (p - k))
        r.ce90, r.ce95 = ce
    return r


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def same(a, b):
    """Same dtype, shape and bits; NaN equals NaN."""
    a, b = host(a), host(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        nan = np.isnan(a)
        return bool(np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes())
    return a.tobytes() == b.tobytes()


def differing(got, want, fields=R.FIELDS):
    """The fields of two figures that are not the same by bits."""
    return [f for f in fields if not same(getattr(got, f), getattr(want, f))] + ([] if got.sample == want.sample else ["sample"])
