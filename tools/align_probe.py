"""Times of the global align step at Sentinel-2 size (10980^2) next to a byte model per kernel.

    python tools/align_probe.py [--n 10980] [--reps 10] [--out profiles/align_probe_10980.json]

Synthetic pair generated on the device (karios_amd.synth._base_torch, mon = the scene under a known homography, warped by the
library).  Every call goes through a _dev entry point on resident buffers; each figure is the median wall time of --reps calls
(the library's stream drained after each), so it includes the launch and, for ECC, the per-iteration copy of the 66 sums.
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
from karios_amd import _lib, synth  # noqa: E402


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _dp(a):
    return np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10980)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="profiles/align_probe_10980.json")
    a = ap.parse_args()
    import torch

    n, pad = a.n, synth.PAD
    c = _lib.default_context()
    lib, h = c.lib, c.handle
    base = synth._base_torch(n, n, 20261016, "cuda").contiguous()
    th = np.radians(0.005)
    A = np.array([[np.cos(th), -np.sin(th), 1.3], [np.sin(th), np.cos(th), -0.9], [2e-10, -2e-10, 1.0]])
    T = np.array([[1, 0, pad], [0, 1, pad], [0, 0, 1.0]]) @ A
    mon32 = torch.empty((n, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    c.check(lib.km_warp_perspective_dev(h, _vp(base), _lib.KM_F32, base.shape[0], base.shape[1], base.stride(0), _vp(mon32), n, n, n, 1, 1,
                                        0.0, _dp(T)), "synth")
    c.sync()
    ref32 = base[pad:pad + n, pad:pad + n].round().clamp(1, 16000).contiguous()
    mon32 = mon32.round().clamp(1, 16000)
    ref8 = ((ref32 - 1000.0) * (255.0 / 4000.0)).clamp(0, 255).to(torch.uint8)
    mon8 = ((mon32 - 1000.0) * (255.0 / 4000.0)).clamp(0, 255).to(torch.uint8)
    del base
    torch.cuda.synchronize()

    def timed(fn):
        ts = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            fn()
            c.sync()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts[1:]) * 1e3

    M = np.linalg.inv(A)
    dst8 = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    dst32 = torch.empty((n, n), dtype=torch.float32, device="cuda")
    sob = torch.empty((n, n), dtype=torch.float32, device="cuda")
    ms = {}
    ms["warp_u8_linear"] = timed(lambda: c.check(lib.km_warp_perspective_dev(h, _vp(mon8), _lib.KM_U8, n, n, n, _vp(dst8), n, n, n, 1, 0, 0.0,
                                                                             _dp(M)), "warp u8"))
    ms["warp_f32_linear"] = timed(lambda: c.check(lib.km_warp_perspective_dev(h, _vp(mon32), _lib.KM_F32, n, n, n, _vp(dst32), n, n, n, 1, 0,
                                                                              0.0, _dp(M)), "warp f32"))
    ms["warp_u8_nearest"] = timed(lambda: c.check(lib.km_warp_perspective_dev(h, _vp(mon8), _lib.KM_U8, n, n, n, _vp(dst8), n, n, n, 0, 0, 0.0,
                                                                              _dp(M)), "warp nearest"))
    ms["sobel_magnitude"] = timed(lambda: c.check(lib.km_sobel_magnitude_dev(h, _vp(ref8), n, n, n, _vp(sob)), "sobel"))
    c.check(lib.km_sobel_magnitude_dev(h, _vp(mon8), n, n, n, _vp(dst32)), "sobel mon")
    c.sync()

    def ecc(iters):
        mp = np.eye(3, dtype=np.float32)
        cc, it = C.c_double(), C.c_int()
        c.check(lib.km_find_transform_ecc_dev(h, _vp(sob), _vp(dst32), _lib.KM_F32, n, n, n, n, n, n, _vp(mon8), n, mp.ctypes.data_as(C.c_void_p),
                                              iters, -1.0, 5, C.byref(cc), C.byref(it)), "ecc")
        return it.value
    ms["ecc_prep"] = timed(lambda: ecc(0))
    k = 5
    ms[f"ecc_prep_plus_{k}_iterations"] = timed(lambda: ecc(k))
    ms["ecc_iteration"] = (ms[f"ecc_prep_plus_{k}_iterations"] - ms["ecc_prep"]) / k

    inits = np.ascontiguousarray(np.array([[[1, 0, 1.0], [0, 1, -0.75], [0, 0, 1]], np.eye(3)], np.float64).reshape(2, 9))
    fin = np.empty((2, 9)); res = np.empty((2, 9), np.float32); ccs = np.empty(2)
    its = np.empty(2, np.int32); valid = np.empty(2, np.int64); st = np.empty(2, np.int32)
    P = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731

    def refine():
        c.check(lib.km_refine_ecc_candidates_dev(h, _vp(mon8), n, n, n, _vp(ref8), n, n, n, 2, P(inits), 200, 1e-6, P(fin), P(res), P(ccs),
                                                 P(its), P(valid), P(st)), "refine")
    ms["refine_two_candidates"] = timed(refine)

    px = n * n
    bytes_per_px = {  # DRAM bytes the kernels must move per destination / template pixel (taps of neighbouring pixels hit in L2)
        "warp_u8_linear": 2, "warp_f32_linear": 8, "warp_u8_nearest": 2,
        "sobel_magnitude": 1 + 4 + 8,                       # u8 read, magnitude write, then read + write for the divide
        "ecc_prep": 8 + 8 + 8 + 5 + 8 + 8 + 16,             # template blur (2 passes), input blur, pre-mask blur, plane (reads + 16 B write)
        "ecc_iteration": 4 + 16,                            # template + one float4 per pixel of the input plane
    }
    rec = {"n": n, "reps": a.reps, "ms": {k2: round(v, 4) for k2, v in ms.items()},
           "iterations_per_candidate": [int(x) for x in its], "status": [int(x) for x in st], "cc": [float(x) for x in ccs],
           "byte_model_GB": {k2: round(v * px / 1e9, 3) for k2, v in bytes_per_px.items()},
           "effective_TB_per_s": {k2: round(v * px / (ms[k2] * 1e-3) / 1e12, 2) for k2, v in bytes_per_px.items()}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
