"""TEST INFRASTRUCTURE - the tail of the reference's tracker restated in numpy and pandas, for the frame stage alone
(tests/test_frame_host.py, tests/test_gpu_frame.py; cases in tests/frame_cases.py).

What the reference does between `calcOpticalFlowPyrLK` and the frame a tile yields (`karios/matcher/klt.py:142-168`, `341-348`), in
the reference's order and with its operators, on `(N, 1, 2)` float32 point lists:

    1. `abs(p0 - p0r)` in float32, reshaped to rows of two, and the row maximum (numpy's `max`: a NaN in either component wins);
    2. the comparison with the Python float `0.1` (float32 against a Python scalar compares in float32);
    3. the boolean selection of p0, p1 and d;
    4. `1 - d / 0.1` (float32);
    5. `DataFrame.from_dict` of x0, y0, x1 - x0, y1 - y0, score;
    6. the tile origin added to x0 and y0, in float32;
    7. `sort_values(by=["x0", "y0"], inplace=True)` - pandas orders several keys with a stable sort, and the index keeps each row's
       position before the sort.

The library's own rules, which the reference does not have (its lists have no capacity), each applied where the device applies it:

    a. a unit's count word `n` says how many rows of its lists are live; rows behind it are never read;
    b. `n` is clamped to `n_max`; a unit without a count word (`n < 0`) has `n_max` live rows;
    c. at most `cap` kept rows survive: the first `cap` in list order (between steps 3 and 4);
    d. `n_init == 0` (no live row) gives `None` instead of a frame; header word 1 carries `n_init`, word 0 the rows of the frame.
"""
from __future__ import annotations

import numpy as np
from pandas import DataFrame

COLUMNS = ("x0", "y0", "dx", "dy", "score")
QUIET_NAN = np.uint32(0x7FC00000)


def live_rows(n: int, n_max: int) -> int:
    """Rules a and b."""
    return n_max if n < 0 else min(int(n), n_max)


@np.errstate(all="ignore")       # (the cases hold NaN, infinities and denormals on purpose)
def frame_of_tracks(p0, p1, p0r, n: int, x_off, y_off, n_max: int, cap: int):
    """-> (frame or None, rows, n_init)."""
    n_init = live_rows(n, n_max)
    if n_init == 0:                                                  # rule d
        return None, 0, 0
    p0, p1, p0r = (np.asarray(a, np.float32).reshape(-1, 1, 2)[:n_init] for a in (p0, p1, p0r))    # rule a
    d = abs(p0 - p0r).reshape(-1, 2).max(-1)                         # 1
    assert d.dtype == np.float32
    back_threshold = 0.1
    st = d < back_threshold                                          # 2
    p0, p1, d = p0[st][:cap], p1[st][:cap], d[st][:cap]              # 3, rule c
    score = 1 - d / back_threshold                                   # 4
    assert score.dtype == np.float32
    x0, y0 = p0[:, 0, 0].reshape(len(p0)), p0[:, 0, 1].reshape(len(p0))
    x1, y1 = p1[:, 0, 0].reshape(len(p1)), p1[:, 0, 1].reshape(len(p1))
    points = DataFrame.from_dict({"x0": x0, "y0": y0, "dx": x1 - x0, "dy": y1 - y0, "score": score})     # 5
    points["x0"] = points["x0"] + np.float32(x_off)                  # 6
    points["y0"] = points["y0"] + np.float32(y_off)
    assert all(points[c].dtype == np.float32 for c in COLUMNS)
    points.sort_values(by=["x0", "y0"], inplace=True)                # 7
    return points, len(points), n_init


def bits(column) -> np.ndarray:
    """A float32 column as its uint32 words: -0.0 differs from 0.0, a denormal from zero; NaN counts by position (one word for all)."""
    a = np.ascontiguousarray(column, np.float32)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = QUIET_NAN
    return u


def assert_same_frame(got, want, what=""):
    """Columns word for word, index labels exactly."""
    if want is None or got is None:
        assert got is None and want is None, f"{what}: {'no frame' if got is None else 'a frame'} instead of {'none' if want is None else 'one'}"
        return
    assert tuple(got.columns) == COLUMNS == tuple(want.columns), f"{what}: columns {tuple(got.columns)}"
    assert len(got) == len(want), f"{what}: {len(got)} rows, expected {len(want)}"
    for c in COLUMNS:
        g, w = got[c].to_numpy(), want[c].to_numpy()
        assert g.dtype == np.float32 and w.dtype == np.float32, f"{what}: column {c} is {g.dtype} / {w.dtype}"
        bad = np.flatnonzero(bits(g) != bits(w))
        assert bad.size == 0, f"{what}: column {c} differs in {bad.size} rows, first at row {bad[0]}: {g[bad[0]]!r} instead of {w[bad[0]]!r}"
    gi, wi = np.asarray(got.index, np.int64), np.asarray(want.index, np.int64)
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, f"{what}: index labels differ in {bad.size} rows, first at row {bad[0]}: {gi[bad[0]]} instead of {wi[bad[0]]}"


def frames_of(units, n_max: int, cap: int):
    """What `ops.frame_from_tracks(units, n_max, cap)` has to return, per unit: (frame or None, rows, n_init)."""
    return [frame_of_tracks(u["p0"], u["p1"], u["p0r"], u["n"], u["x_off"], u["y_off"], n_max, cap) for u in units]
