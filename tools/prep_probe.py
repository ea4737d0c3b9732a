"""Times of the align step's preprocessing at Sentinel-2 size (10980^2) next to a byte model per entry point.

    python tools/prep_probe.py [--n 10980] [--reps 10] [--cpu] [--out profiles/prep_probe_10980.json]

Synthetic uint16 raster generated on the device (karios_amd.synth.make_pair_torch).  Every call goes through a _dev entry point on
resident buffers; each figure is the median wall time of --reps calls (the library's stream drained after each), so it includes the
launches and, for the order statistics, the one copy of the results.  --cpu adds the numpy times of the same calls on this host
(np.nanpercentile, the reference's _to_uint8), one thread, once each.  With a development build of the library (KARIOS_HIP_LIB
pointing at libkarios_hip_dev.so) the order statistics are also timed with one LDS atomic per pixel ("prep_hist_plain"), the form the
run-aggregated histogram was measured against.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from karios_amd import _lib, ops, synth  # noqa: E402


def _vp(t):
    return C.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10980)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--out", default="profiles/prep_probe_10980.json")
    a = ap.parse_args()
    import torch

    n = a.n
    c = _lib.default_context()
    lib, h = c.lib, c.handle
    mon16, _ref = synth.make_pair_torch(n, n, 0.5, 0.25, seed=20261016, device="cuda")
    del _ref
    mon32 = mon16.to(torch.float32)
    u8 = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    eq = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def timed(fn):
        ts = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            fn()
            c.sync()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts[1:]) * 1e3

    pd = C.POINTER(C.c_double)
    q = np.array([0.02, 0.98])
    cnt = C.c_int64()
    v0, v1, vi = np.zeros(2), np.zeros(2), np.zeros(2)

    def stats(t, code, exclude):
        c.check(lib.km_order_statistics_dev(h, _vp(t), code, n, n, n, exclude, 2, q.ctypes.data_as(pd), C.byref(cnt), v0.ctypes.data_as(pd),
                                            v1.ctypes.data_as(pd), vi.ctypes.data_as(pd)), "order_statistics")

    ms = {}
    ms["order_statistics_u16"] = timed(lambda: stats(mon16, _lib.KM_U16, 0))
    lo, hi = ops.lerp_linear(v0, v1, vi, cnt.value, np.uint16)
    ms["order_statistics_f32"] = timed(lambda: stats(mon32, _lib.KM_F32, 1))
    ms["stretch_u16"] = timed(lambda: c.check(lib.km_stretch_percentile_u8_dev(h, _vp(mon16), _lib.KM_U16, n, n, n, float(lo), float(hi), _vp(u8),
                                                                               n), "stretch"))
    ms["stretch_f32"] = timed(lambda: c.check(lib.km_stretch_percentile_u8_dev(h, _vp(mon32), _lib.KM_F32, n, n, n, float(lo), float(hi), _vp(u8),
                                                                               n), "stretch"))
    ms["clahe_8x8"] = timed(lambda: c.check(lib.km_clahe_dev(h, _vp(u8), n, n, n, 2.0, 8, 8, _vp(eq), n), "clahe"))
    ms["clahe_16x16"] = timed(lambda: c.check(lib.km_clahe_dev(h, _vp(u8), n, n, n, 2.0, 16, 16, _vp(eq), n), "clahe"))
    if lib.km_is_dev_build():
        c.set_option("prep_hist_plain", 1)
        ms["order_statistics_u16_plain_atomics"] = timed(lambda: stats(mon16, _lib.KM_U16, 0))
        c.set_option("prep_hist_plain", 0)
        const = torch.full((n, n), 1234, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        ms["order_statistics_u16_constant"] = timed(lambda: stats(const, _lib.KM_U16, 0))
        c.set_option("prep_hist_plain", 1)
        ms["order_statistics_u16_constant_plain_atomics"] = timed(lambda: stats(const, _lib.KM_U16, 0))
        c.set_option("prep_hist_plain", 0)

    px = n * n
    bytes_per_px = {  # DRAM bytes the kernels must move per pixel
        "order_statistics_u16": 3 * 2, "order_statistics_f32": 3 * 4,     # three passes over the raster
        "stretch_u16": 2 + 1, "stretch_f32": 4 + 1,
        "clahe_8x8": 1 + 1 + 1, "clahe_16x16": 1 + 1 + 1,                 # histogram pass; apply: read + write
    }
    rec = {"n": n, "reps": a.reps, "dev_build": bool(lib.km_is_dev_build()), "ms": {k: round(v, 4) for k, v in ms.items()},
           "percentiles_2_98": [float(lo), float(hi)],
           "byte_model_GB": {k: round(v * px / 1e9, 3) for k, v in bytes_per_px.items()},
           "effective_TB_per_s": {k: round(v * px / (ms[k] * 1e-3) / 1e12, 2) for k, v in bytes_per_px.items()}}
    if a.cpu:
        host = mon16.cpu().numpy().view(np.uint16)
        t0 = time.perf_counter()
        ref = np.nanpercentile(host, [2, 98])
        t1 = time.perf_counter()
        f = host.astype(np.float32)
        plo, phi = np.percentile(f[np.isfinite(f)], (2.0, 98.0))
        np.clip(((f - plo) / (phi - plo)) * 255.0, 0, 255).astype(np.uint8)
        t2 = time.perf_counter()
        rec["cpu_numpy_ms"] = {"nanpercentile_u16": round((t1 - t0) * 1e3, 1), "to_uint8_u16": round((t2 - t1) * 1e3, 1)}
        rec["cpu_numpy_percentiles_2_98"] = [float(ref[0]), float(ref[1])]
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
