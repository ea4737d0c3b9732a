"""numpy restatement of the tracker's iterative outlier clip (karios/matcher/klt.py:52-71) for float32 displacement columns, as
libkarios_hip.so computes it (csrc/clip_math.hpp, k_clip.hip).

This is the DEFINITION the library is held to (tests/test_gpu_clip.py, the sanitized host program of tests/test_clip_host.py);
tests/test_clip_host.py holds it to `karios_amd.frames.sigma_clip` on the installed numpy and to the reference's recorded result
(tests/golden/outliers.npz).  Every float32 operation is one rounding on tests/accuracy_restatement.py's sums, so the definition does
not move with the numpy version.

Test infrastructure only: karios_amd never imports this module.
"""
from __future__ import annotations

import numpy as np

import accuracy_restatement as A

f32 = np.float32
N_SIGMA = f32(3.0)       # [ref klt.py:58-61] `3 * std`: a Python number times a float32 scalar is a float32 product
LIMIT = f32(20.0)        # [ref] pixels; the comparison is in float32 and strict
MAX_ROWS = 32768         # rows the device form takes (csrc/clip_math.hpp cl::MAX_ROWS)


def round_keep(u, v, mean=A.mean_f32, std=A.std_f32):
    """The rows one round keeps.  `mean` / `std`: the float32 statistics (the tests swap in left-to-right sums to show that the
    summation order decides)."""
    with np.errstate(all="ignore"):
        mu, mv = mean(u), mean(v)
        lu, lv = f32(N_SIGMA * std(u)), f32(N_SIGMA * std(v))
        ou, ov = np.abs(u - mu), np.abs(v - mv)                  # float32 - float32, element by element
        return (ou < lu) & (ov < lv) & (ou < LIMIT) & (ov < LIMIT)   # NaN compares false


def sigma_clip(dx, dy, mean=A.mean_f32, std=A.std_f32):
    """-> (indices of the survivors in row order, rounds computed).  Stops when a round keeps every row or no row is left; the
    statistics of a round are taken on the COMPACTED arrays of the round before."""
    u, v = np.ascontiguousarray(dx, f32), np.ascontiguousarray(dy, f32)
    alive = np.arange(u.size)
    rounds = 0
    while alive.size:
        keep = round_keep(u, v, mean, std)
        rounds += 1
        if keep.all():
            break
        alive, u, v = alive[keep], u[keep], v[keep]
    return alive, rounds


def mean_left_to_right(a):
    """NOT numpy's: the mean on a plain loop's sum."""
    with np.errstate(all="ignore"):
        return f32(A.sum_left_to_right(a) / f32(a.size))


def std_left_to_right(a):
    """NOT numpy's: the standard deviation on plain loops' sums."""
    a = np.asarray(a, f32)
    with np.errstate(all="ignore"):
        d = a - mean_left_to_right(a)
        return f32(np.sqrt(f32(A.sum_left_to_right(d * d) / f32(a.size))))


def sigma_clip_left_to_right(dx, dy):
    return sigma_clip(dx, dy, mean_left_to_right, std_left_to_right)


def clip_block(block, cap):
    """The clip of a frame block (`karios_amd.frames.block_to_frame`'s layout: 4 int32 {rows, Ninit, flags, candidates}, then six float32
    columns of `cap` entries, column 5 = the row's position in the kept list as int bits) -> (clipped block, rounds).  Rows stay in
    (x0, y0) order, column 5 becomes the position among the survivors, header words 1..3 stay; rows behind the new count are
    unspecified (here: zero)."""
    block = np.array(block, f32, copy=True)
    hdr = block[:4].view(np.int32)
    rows = int(hdr[0])
    body = block[4:4 + 6 * cap].reshape(6, cap)
    label = body[5, :rows].view(np.int32)
    u, v = np.empty(rows, f32), np.empty(rows, f32)
    u[label], v[label] = body[2, :rows], body[3, :rows]          # the kept list in corner order
    alive, rounds = sigma_clip(u, v)
    if alive.size == rows:
        return block, rounds
    new_label = np.full(rows, -1, np.int64)
    new_label[alive] = np.arange(alive.size)
    kept = new_label[label] >= 0                                  # frame rows that survive, in frame order
    out = np.zeros_like(block)
    out[:4] = block[:4]
    ob = out[4:4 + 6 * cap].reshape(6, cap)
    ob[:5, :alive.size] = body[:5, :rows][:, kept]
    ob[5, :alive.size] = new_label[label][kept].astype(np.int32).view(f32)
    out[:1].view(np.int32)[0] = alive.size
    out[4 + 6 * cap:] = block[4 + 6 * cap:]
    return out, rounds


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 7, 8, 9, 127, 128, 129, 255, 256, 257, 1000, 8191, 8192, 8193, 8969, 12000, 20000, 32768)
KINDS = ("tails", "offset", "far")


def scene(kind, n, seed):
    """float32 (dx, dy) of n rows.  tails: Student-t, 3 degrees of freedom; offset: the same around (1000, -750), where the sum's
    rounding error is of the size of a row's distance to the 3-sigma limit; far: a second population more than 20 px away."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    t = rng.standard_t(3, size=(2, n))
    if kind == "tails":
        dx, dy = 0.4 * t[0], 0.4 * t[1]
    elif kind == "offset":
        dx, dy = 1000 + 0.3 * t[0], -750 + 0.3 * t[1]
    else:
        dx, dy = 0.2 * rng.standard_normal(n), 0.2 * rng.standard_normal(n)
        far = rng.random(n) < 0.08
        dx = dx + np.where(far, 23.0, 0.0)
        dy = dy - np.where(far, 31.0, 0.0)
    return dx.astype(f32), dy.astype(f32)


# order-sensitive fixtures: (n, seed) of the `offset` family whose survivors differ when the sums run left to right (found by a search
# over seeds on the CPU; tests/test_clip_host.py asserts for each that it still discriminates)
ORDER_SENSITIVE = ((8969, 2), (8969, 6), (8969, 12), (12000, 2), (12000, 5), (12000, 9))


def order_sensitive(n, seed):
    return scene("offset", n, seed)


def special_cases():
    """name -> (dx, dy): a constant column, a NaN row, a row exactly 20 px off the mean (kept by `<=`, dropped by the strict `<`)."""
    rng = np.random.default_rng(5)
    base = (0.25 * rng.standard_normal(300)).astype(f32)
    const = np.full(300, 1.5, f32)
    nan_row = base.copy()
    nan_row[17] = np.nan
    # four each of +-0.5 and +-20: every sum is exact, the mean is 0, the deviations are exactly 0.5 or 20 and 3 std = 42.4: only the
    # strict 20-px rule drops the +-20 rows (8 of 16 survive, in two rounds)
    exact = np.tile(np.array([0.5, 20.0, -20.0, -0.5], f32), 4)
    return {"constant_dx": (const, base), "constant_dy": (base, const), "nan_dx": (nan_row, base), "nan_dy": (base, nan_row),
            "exactly_20": (exact, np.zeros(16, f32) + (np.arange(16) % 2).astype(f32)), "single": (base[:1], base[:1]),
            "empty": (base[:0], base[:0])}


def fixtures():
    """Every fixture of the suite as (name, dx, dy)."""
    out = []
    for kind in KINDS:
        for n in SIZES:
            out.append((f"{kind}_{n}", *scene(kind, n, 1)))
    for n, seed in ORDER_SENSITIVE:
        out.append((f"order_{n}_{seed}", *order_sensitive(n, seed)))
    for name, (dx, dy) in special_cases().items():
        out.append((name, dx, dy))
    return out
