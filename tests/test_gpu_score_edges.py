"""The score kernels (k_zncc.hip, k_mi.hip) at pixel extremes and bin boundaries, against the exact restatement
(tests/score_restatement.py; tests/test_score_host.py holds that to numpy and to the reference's recorded results).

Every fixture group of every pixel type through `ops.zncc_batch` and `ops.mi_batch`, the window fixtures through `ops.zncc_windows`:
the NaN pattern must be identical, the values within 1e-9 - the gate of every score test of this suite.  The observed maximum of each
group is printed (pytest -s) and recorded in CHANGELOG.md.  The range sweep runs once more through `ResidentPair.score_frame`
(resident rasters, page-locked key points) and must deliver bit-equal columns.
"""
import numpy as np
import pandas as pd
import pytest

import score_restatement as R

pytestmark = pytest.mark.gpu

GATE = 1e-9
INT_GROUPS = ("sweep", "degenerate", "zncc", "placement")
FLOAT_GROUPS = ("degenerate", "zncc", "placement", "nonfinite_rim", "nonfinite_window", "float_edges")
CASES = [(np.dtype(t).name, g) for t in R.INT_TYPES for g in INT_GROUPS] + [("float32", g) for g in FLOAT_GROUPS]


def worst(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.flatnonzero(np.isnan(got) != np.isnan(want))[:10])
    d = np.abs(got - want)[~np.isnan(want)]
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize("dtype,group", CASES)
def test_scores_equal_the_exact_restatement(ops, dtype, group):
    assert group in R.groups(dtype)
    top = [0.0, 0.0, 0.0]
    for c, want in R.expected(dtype, group):
        z = ops.zncc_batch(c.ref, c.mon, c.x0, c.y0, c.dx, c.dy)
        st, nmi = ops.mi_batch(c.ref, c.mon, c.x0, c.y0, c.dx, c.dy)
        for i, got in enumerate((z, st, nmi)):
            top[i] = max(top[i], worst(got, want[i], (c.name, ("zncc", "studholme", "nmi")[i])))
    print(f"kernels vs restatement [{dtype} {group}]: zncc {top[0]:.3g} studholme {top[1]:.3g} nmi {top[2]:.3g}")
    assert max(top) <= GATE, top


@pytest.mark.parametrize("half", [0, 21])
def test_zncc_windows_equal_the_exact_restatement(ops, half):
    top = 0.0
    for w in R.window_fixtures():
        got, outside = ops.zncc_windows(w.img1, w.img2, w.u1, w.v1, w.u2, w.v2, half)
        assert not outside.any()
        top = max(top, worst(got, R.windows_exact(w, half), w.name))
    print(f"zncc_windows vs restatement [half {half}]: {top:.3g}")
    assert top <= GATE


@pytest.mark.parametrize("dtype", [np.dtype(t).name for t in R.INT_TYPES])
def test_sweep_through_score_frame_is_bit_equal(ops, dtype):
    from karios_amd.resident import ResidentPair
    (c, want), = R.expected(dtype, "sweep")
    n = len(c.x0)
    score = np.where(np.arange(n) % 5 == 3, 0.25, 0.75).astype(np.float32)          # every fifth row is below the threshold: NaN
    frame = pd.DataFrame({"x0": c.x0, "y0": c.y0, "dx": c.dx, "dy": c.dy, "score": score})
    pair = ResidentPair.upload(c.mon, c.ref)
    got = pair.score_frame(frame, 0.4, mutual_info=True)
    keep = score >= np.float32(0.4)
    z = ops.zncc_batch(c.ref, c.mon, c.x0, c.y0, c.dx, c.dy)
    st, nmi = ops.mi_batch(c.ref, c.mon, c.x0, c.y0, c.dx, c.dy)
    for col, direct, exact in (("zncc_score", z, want[0]), ("mutual_info_score", st, want[1]), ("mi_score", nmi, want[2])):
        v = got[col].to_numpy()
        assert np.isnan(v[~keep]).all() and np.array_equal(v[keep].view(np.uint64), direct[keep].view(np.uint64)), col
        assert worst(v[keep], exact[keep], col) <= GATE
