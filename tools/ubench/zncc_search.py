#!/usr/bin/env python3
"""Timing of the ZNCC search around each key point: 32 000 key points on a 10980 x 10980 uint16 pair, radius 2, 4
and 8, the search kernel (`ops.zncc_search`, device tensors in) against the only other route to the same surface - `ops.zncc_windows`
over n (2R+1)^2 window pairs, the generic `_zncc2` kernel, one wavefront per window, every window read from global memory twice.

Both are timed by the library's own events around the kernel (the "zncc" stage under `set_profiling`), after a warm-up call, the two
routes alternating within the run; the generic route's uploads of both rasters and of its window list are outside its events, and its
wall time per call is recorded beside.  The surfaces of the two routes are compared on the first call (integer pixels: the exact-moment
value against the two-pass value, within 1e-9).  Operation and byte counts come from the shapes.  Recorded, not gated.

    python tools/ubench/zncc_search.py [--out profiles/zncc_search.json] [--side 10980] [--points 32000] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from karios_amd import ops, synth  # noqa: E402

SIDE, HW = 43, 21


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zncc_search.json"))
    ap.add_argument("--side", type=int, default=10980)
    ap.add_argument("--points", type=int, default=32000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--radii", type=int, nargs="+", default=[2, 4, 8])
    args = ap.parse_args()
    side, n = args.side, args.points
    ctx = ops.default_context()
    mon_t, ref_t = synth.make_pair_torch(side, side, 0.4, -0.3, seed=7, device="cuda")
    mon_t, ref_t = mon_t.view(torch.uint16), ref_t.view(torch.uint16)
    torch.cuda.synchronize()
    mon, ref = (t.view(torch.int16).cpu().numpy().view(np.uint16) for t in (mon_t, ref_t))
    rng = np.random.default_rng(11)
    x0, y0 = np.floor(rng.uniform(40, side - 40, n)), np.floor(rng.uniform(40, side - 40, n))
    order = np.lexsort((y0, x0))                                   # frames are ordered by (x0, y0)
    cols = [np.ascontiguousarray(v[order], np.float32) for v in (x0, y0, 0.4 + rng.normal(0, 0.5, n), -0.3 + rng.normal(0, 0.5, n))]
    cols_t = [torch.from_numpy(c).cuda() for c in cols]
    X0, Y0 = cols[0].astype(np.int64), cols[1].astype(np.int64)
    X1, Y1 = np.rint(cols[0] + cols[2]).astype(np.int64), np.rint(cols[1] + cols[3]).astype(np.int64)
    rec = {"device": torch.cuda.get_device_name(0), "side": side, "points": n, "repeats": args.repeats, "pixel_type": "uint16", "radii": {}}

    def stage():
        return ctx.stage_ms()["zncc"]

    for R in args.radii:
        S, RW = 2 * R + 1, SIDE + 2 * R
        o = np.arange(-R, R + 1)
        u2 = np.broadcast_to(Y1[:, None, None] + o[None, :, None], (n, S, S)).ravel()
        v2 = np.broadcast_to(X1[:, None, None] + o[None, None, :], (n, S, S)).ravel()
        u1, v1 = np.repeat(Y0, S * S), np.repeat(X0, S * S)

        def search():
            return ops.zncc_search(ref_t, mon_t, *cols_t, radius=R, surface=True)

        def windows():
            return ops.zncc_windows(ref, mon, u1, v1, u2, v2, HW)

        new = search()                                             # warm-up of both routes, and the comparison
        old, outside = windows()
        surface = new.surface.cpu().numpy().reshape(-1)
        if outside.any() or not np.array_equal(np.isnan(surface), np.isnan(old)) or np.nanmax(np.abs(surface - old)) > 1e-9:
            raise SystemExit(f"radius {R}: the two routes differ")
        t_new, t_old, wall_old, wall_new = [], [], [], []
        ctx.set_profiling(True)
        try:
            for _ in range(args.repeats):                          # alternating
                t0 = time.perf_counter()
                search()
                wall_new.append((time.perf_counter() - t0) * 1e3)
                t_new.append(stage())
                t0 = time.perf_counter()
                windows()
                wall_old.append((time.perf_counter() - t0) * 1e3)
                t_old.append(stage())
        finally:
            ctx.set_profiling(False)
        offsets = n * S * S
        row = {
            "offsets": offsets,
            "search_kernel_ms_median": statistics.median(t_new), "search_kernel_ms_min": min(t_new), "search_call_wall_ms_median": statistics.median(wall_new),
            "windows_kernel_ms_median": statistics.median(t_old), "windows_kernel_ms_min": min(t_old), "windows_call_wall_ms_median": statistics.median(wall_old),
            "kernel_speedup": statistics.median(t_old) / statistics.median(t_new),
            # from the shapes: multiply-accumulates of the correlation sums (S_b, S_bb, S_ab per pixel and offset), the bytes the search
            # stages once per key point, the bytes the generic route reads (two windows, two passes), the surface written
            "macs": 3 * offsets * SIDE * SIDE,
            "search_bytes_staged": n * (RW * RW + SIDE * SIDE) * 2, "windows_bytes_read": offsets * 2 * 2 * SIDE * SIDE * 2, "surface_bytes": offsets * 8,
            "search_lds_bytes_read": offsets * 2 * SIDE * SIDE * 2,
        }
        row["search_Gmac_per_s"] = row["macs"] / 1e6 / row["search_kernel_ms_median"]
        rec["radii"][str(R)] = row
        print(R, row, flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
