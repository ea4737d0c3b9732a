#!/usr/bin/env python3
"""Timing of the mutual-information search around each key point: 32 000 key points ordered by (x0, y0) on a resident
10980 x 10980 uint16 pair, radius 2, 4 and 8, the search kernel (`km_mi_search_dev`) against the only other route to the same surface
the library has - `km_mi_batch_dev` over n (2R+1)^2 fabricated rows with dx' = X1 + ox - x0, dy' = Y1 + oy - y0, which re-reads both
chips from global memory and re-bins the reference chip once per offset.

Both are timed by the library's own events around the kernel (the "mutual_info" stage under `set_profiling`), after a warm-up call, the
two routes alternating within the run, median of the repeats.  The surfaces of the two routes are compared on the first call (within
1e-9, the gate `km_mi_batch` is held to).  Operation and byte counts come from the shapes.  Recorded, not gated.

    python tools/ubench/mi_search.py [--out profiles/mi_search.json] [--side 10980] [--points 32000] [--repeats 5]
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

from karios_amd import _lib, ops, synth  # noqa: E402

CHIP = 57


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mi_search.json"))
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
    rng = np.random.default_rng(11)
    x0, y0 = np.floor(rng.uniform(40, side - 40, n)), np.floor(rng.uniform(40, side - 40, n))
    order = np.lexsort((y0, x0))                                   # frames are ordered by (x0, y0)
    cols = [np.ascontiguousarray(v[order], np.float32) for v in (x0, y0, 0.4 + rng.normal(0, 0.5, n), -0.3 + rng.normal(0, 0.5, n))]
    cols_t = [torch.from_numpy(c).cuda() for c in cols]
    X1, Y1 = np.rint(cols[0] + cols[2]).astype(np.int64), np.rint(cols[1] + cols[3]).astype(np.int64)
    rec = {"device": torch.cuda.get_device_name(0), "side": side, "points": n, "repeats": args.repeats, "pixel_type": "uint16", "radii": {}}
    code = _lib._DTYPES[np.dtype(np.uint16)]

    def stage():
        return ctx.stage_ms()["mutual_info"]

    for R in args.radii:
        S, RW = 2 * R + 1, CHIP + 2 * R
        o = np.arange(-R, R + 1)
        # the fabricated rows: the same x0, y0 (the same reference chip), a displacement whose float32 sum is the offset's centre exactly
        fx0, fy0 = np.repeat(cols[0], S * S), np.repeat(cols[1], S * S)
        fdx = (np.broadcast_to(X1[:, None, None] + o[None, None, :], (n, S, S)).ravel() - fx0).astype(np.float32)
        fdy = (np.broadcast_to(Y1[:, None, None] + o[None, :, None], (n, S, S)).ravel() - fy0).astype(np.float32)
        fab_t = [torch.from_numpy(np.ascontiguousarray(c, np.float32)).cuda() for c in (fx0, fy0, fdx, fdy)]
        out_t = torch.empty(n * S * S, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def search():
            return ops.mi_search(ref_t, mon_t, *cols_t, radius=R, surface=True)

        def batch():
            ctx.check(ctx.lib.km_mi_batch_dev(ctx.handle, ref_t.data_ptr(), mon_t.data_ptr(), code, side, side, side, side, side, side,
                                              *(c.data_ptr() for c in fab_t), n * S * S, out_t.data_ptr(), None), "km_mi_batch_dev")
            ctx.sync()

        new = search()                                             # warm-up of both routes, and the comparison
        batch()
        surface, old = new.surface.cpu().numpy().reshape(-1), out_t.cpu().numpy()
        if not np.array_equal(np.isnan(surface), np.isnan(old)) or np.nanmax(np.abs(surface - old)) > 1e-9:
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
                batch()
                wall_old.append((time.perf_counter() - t0) * 1e3)
                t_old.append(stage())
        finally:
            ctx.set_profiling(False)
        offsets = n * S * S
        row = {
            "offsets": offsets,
            "search_kernel_ms_median": statistics.median(t_new), "search_kernel_ms_min": min(t_new), "search_call_wall_ms_median": statistics.median(wall_new),
            "batch_kernel_ms_median": statistics.median(t_old), "batch_kernel_ms_min": min(t_old), "batch_call_wall_ms_median": statistics.median(wall_old),
            "kernel_speedup": statistics.median(t_old) / statistics.median(t_new),
            # from the shapes: LDS atomics (one per pixel and offset), the bytes the search stages once per key point, the bytes the generic
            # route reads (two chips per offset), the surface written
            "lds_atomics": offsets * CHIP * CHIP,
            "search_bytes_staged": n * (RW * RW + CHIP * CHIP) * 2, "batch_bytes_read": offsets * 2 * CHIP * CHIP * 2, "surface_bytes": offsets * 8,
            "search_lds_bytes_per_workgroup": 16 * S * S + 4096 + ((2 * RW * RW + 15) // 16) * 16,
        }
        row["search_ns_per_offset"] = row["search_kernel_ms_median"] * 1e6 / offsets
        row["batch_ns_per_offset"] = row["batch_kernel_ms_median"] * 1e6 / offsets
        rec["radii"][str(R)] = row
        print(R, row, flush=True)
        del fab_t, out_t

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
