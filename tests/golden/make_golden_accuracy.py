#!/usr/bin/env python3
"""Golden vectors for `analyze_accuracy`, produced by the REFERENCE's own `GeometricStat`
(karios/accuracy_analysis/accuracy_statistics.py) and the count expression of `KariosAPI.analyze_accuracy`
(karios/api/core.py:284-290), imported from /root/reference (build container only).

Run here, never on the GPU box:   python tests/golden/make_golden_accuracy.py      -> tests/golden/accuracy.npz
Only DATA is written: the score columns, the dx / dy columns of the small cases, a checksum of every column (the large dx / dy
columns are rebuilt by `frame` below, integer arithmetic only, and held to the checksum), tiny rasters with masks, and the
reference's results (statistics, CE, counts, the line of correl_res.txt).  No reference source is copied.

`frame`, `raster` and the lists below are imported by the tests; nothing at module level touches the reference.
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 2, 7, 8, 9, 127, 128, 129, 136, 1000, 8191, 8192, 8193, 16389, 20000)     # rows above the Python-float threshold
FACTORS = (1.0, 10.0, 0.3)
PERCENTS = (0.9, 0.95)
THRESHOLD = 0.4
STORE_COLUMNS_UP_TO = 1000
DTYPES = ("uint8", "uint16", "int16", "float32")
T32 = np.float32(THRESHOLD)
ULP_ROWS = (T32, np.nextafter(T32, np.float32(1)), np.nextafter(T32, np.float32(0)))   # at the threshold, one ulp above, one below


def _hash(n, seed):
    """n 32-bit words from the row index: integer arithmetic only, the same everywhere."""
    u = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed) * np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    u ^= u >> np.uint64(15)
    u = (u * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    u ^= u >> np.uint64(13)
    u = (u * np.uint64(3266489917)) & np.uint64(0xFFFFFFFF)
    u ^= u >> np.uint64(16)
    return u


def _unit(n, seed):
    return _hash(n, seed).astype(np.float64) / 4294967296.0


def frame(n_sample, seed=0):
    """-> dx, dy, score (float32): exactly n_sample rows have score > float32(0.4), one of them by a single ulp; among the others
    one sits AT float32(0.4) (it passes a float64 comparison with 0.4) and one an ulp below; scores otherwise lie on a grid of
    1 / 64.  dx is noise around 0.37, dy around 1000 with a spread of 0.01 (sums that depend on their order)."""
    n_fail = n_sample // 3 + 3
    n = n_sample + n_fail
    score = np.empty(n, np.float32)
    k = _hash(n, 3 * seed + 1)
    score[:n_sample] = ((k[:n_sample] % np.uint64(39)) + np.uint64(26)).astype(np.float32) / np.float32(64)      # 26/64 .. 64/64
    score[n_sample:] = (k[n_sample:] % np.uint64(26)).astype(np.float32) / np.float32(64)                        # 0 .. 25/64
    score[0] = ULP_ROWS[1]
    score[n_sample], score[n_sample + 1] = ULP_ROWS[0], ULP_ROWS[2]
    order = np.argsort(_hash(n, 3 * seed + 2), kind="stable")
    dx = ((_unit(n, 3 * seed + 3) - 0.5) * 6.0 + 0.37).astype(np.float32)
    dy = (1000.0 + (_unit(n, 3 * seed + 4) - 0.5) * 0.04).astype(np.float32)
    return dx[order], dy[order], score[order]


def raster(dtype, H=13, W=17, seed=0):
    """-> tiny raster of `dtype` with zeros, and a uint8 mask; int16 with negatives, float32 with NaN, -0.0 and denormals."""
    dt = np.dtype(dtype)
    u = _hash(H * W, 11 + seed).reshape(H, W)
    v = (u % np.uint64(5)).astype(np.int64) * ((u >> np.uint64(8)) % np.uint64(200)).astype(np.int64)      # 1 in 5 is zero
    if dt == np.int16:
        v = np.where((u >> np.uint64(20)) % np.uint64(2) == 0, v, -v)
    a = v.astype(dt)
    if dt == np.float32:
        flat = a.reshape(-1).view(np.uint32)
        flat[3], flat[10], flat[20], flat[30], flat[40] = 0x7FC00000, 0x80000000, 0x00000001, 0x807FFFFF, 0xFFC00001
        flat[50] = 0x80000000
    mask = ((_hash(H * W, 12 + seed) % np.uint64(3)).astype(np.uint8) * np.uint8(100)).reshape(H, W)             # 1 in 3 is zero
    return a, mask


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def main():
    import tempfile
    import types

    import pandas as pd
    sys.path.insert(0, HERE)
    from make_golden import import_reference
    import_reference()
    from karios.accuracy_analysis.accuracy_statistics import GeometricStat

    out = {"sizes": np.array(SIZES), "factors": np.array(FACTORS), "percents": np.array(PERCENTS)}
    names = ["min_x", "max_x", "median_x", "mean_x", "std_x", "min_y", "max_y", "median_y", "mean_y", "std_y", "min_c", "max_c", "median_c",
             "mean_c", "std_c"]
    lines = []
    for i, n in enumerate(SIZES):
        dx, dy, score = frame(n, i)
        out[f"score_{n}"] = score
        out[f"crc_{n}"] = np.array([crc(dx), crc(dy), crc(score)], np.uint32)
        if n <= STORE_COLUMNS_UP_TO:
            out[f"dx_{n}"], out[f"dy_{n}"] = dx, dy
        points = pd.DataFrame({"dx": dx, "dy": dy, "score": score})
        for thr_tag, thr in (("py", THRESHOLD), ("f64", np.float64(THRESHOLD))):
            for carto in (False, True):
                st = GeometricStat(types.SimpleNamespace(confidence_threshold=thr), points, carto)
                st.compute_stats(1000 + n)
                tag = f"{n}_{thr_tag}_{int(carto)}"
                assert st.valid and all(type(getattr(st, k)) is np.float32 for k in names)
                out[f"sample_{tag}"] = np.array(st.sample_pixel)
                out[f"stats_{tag}"] = np.array([getattr(st, k) for k in names], np.float32)
                ce = [st.compute_percentile(p, f) for f in FACTORS for p in PERCENTS]
                assert all(type(v) is np.float32 for v in ce)
                out[f"ce_{tag}"] = np.array(ce, np.float32)
                ce32 = [st.compute_percentile(p, np.float32(f)) for f in FACTORS for p in PERCENTS]
                assert np.array_equal(np.array(ce32, np.float32).view(np.uint32), out[f"ce_{tag}"].view(np.uint32))
                if thr_tag == "py" and not carto:
                    with tempfile.TemporaryDirectory() as td:
                        path = os.path.join(td, "correl_res.txt")
                        st.update_statistic_file("ref.tif", "mon.tif", path)
                        st.update_statistic_file("ref.tif", "mon.tif", path)
                        lines.append(open(path, encoding="utf-8").read())
    out["correl_res"] = np.array(lines)
    # nothing above the threshold
    st = GeometricStat(types.SimpleNamespace(confidence_threshold=2.0), pd.DataFrame(dict(zip(("dx", "dy", "score"), frame(9, 0)))), False)
    st.compute_stats(5)
    assert not st.valid and st.sample_pixel == 0
    try:
        st.compute_percentile(0.9, 1.0)
        raise SystemExit("the reference did not raise on an empty sample")
    except IndexError:
        pass
    # ---- the count expression of analyze_accuracy (core.py:284-290)
    for dt in DTYPES:
        a, mask = raster(dt)
        out[f"raster_{dt}"], out[f"mask_{dt}"] = a, mask
        masked_image = np.copy(a)
        masked_image[mask == 0] = 0
        out[f"count_{dt}"] = np.array([np.count_nonzero(a), np.count_nonzero(masked_image)])
    path = os.path.join(HERE, "accuracy.npz")
    np.savez_compressed(path, **out)
    print("accuracy.npz written:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
