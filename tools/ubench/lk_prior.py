#!/usr/bin/env python3
"""Timing of the seeded tracker launch: 20 000 key points of a resident 10980 x 10980 uint16 pair whose monitored
raster lies (+14, -6) px off the reference, tracked under the prior `from_shift(-6, 14)` on the rasters as they are, against the unseeded
launch on the pre-shifted pair - what the reference's `shift_image` route hands the tracker.  Both are whole tile calls
(`ResidentPair.match_tile`); the figure is the library's own "lk_fwd_bwd" stage span (events around the tracker launch, `set_profiling`), median
of the repeats, the two routes alternating.  Beside it: what the seeded route adds (the mask pass under the prior, timed as a call of
`ops.prior_mask` on device tensors) and what it no longer needs (the 241 MB shifted copy, `km_shift_image_dev`).  The bilinear warp a
homography needs in the reference's route is not timed here: km_warp_perspective_dev serves uint8 / float32 rasters, not this pair's
uint16 (profiles/align_probe_10980.json holds its figures).  Recorded, not gated.

    python tools/ubench/lk_prior.py [--out profiles/lk_prior.json] [--side 10980] [--points 20000] [--repeats 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from karios_amd import ops, synth  # noqa: E402
from karios_amd.core import KLTConfiguration  # noqa: E402
from karios_amd.matcher import prior as prior_mod  # noqa: E402
from karios_amd.resident import ResidentPair  # noqa: E402

SX, SY = 14, -6


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lk_prior.json"))
    ap.add_argument("--side", type=int, default=10980)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    side = args.side
    ctx = ops.default_context()
    mon, ref = synth.make_pair_torch(side, side, 0.4, -0.3, seed=7, device="cuda")
    raw = torch.roll(mon, shifts=(SY, SX), dims=(0, 1)).contiguous()            # raw(x + SX, y + SY) == mon(x, y)
    torch.cuda.synchronize()
    conf = KLTConfiguration(maxCorners=args.points)
    P = prior_mod.from_shift(SY, SX)
    wrap = lambda m: ResidentPair.from_device_pointers(m.data_ptr(), ref.data_ptr(), np.uint16, side, side, ctx=ctx, keepalive=(m, ref))
    seeded_pair, shifted_pair = wrap(raw), wrap(mon)

    def seeded():
        return seeded_pair.match_tile(conf, zncc_threshold=0.4, prior=P)

    def unseeded():
        return shifted_pair.match_tile(conf, zncc_threshold=0.4)

    a, b = seeded(), unseeded()                                                  # warm-up, and what the two routes found
    rec = {"device": torch.cuda.get_device_name(0), "side": side, "max_corners": args.points, "repeats": args.repeats, "pixel_type": "uint16",
           "shift": [SX, SY], "seeded_rows": len(a), "unseeded_rows": len(b), "seeded_corners": int(a.attrs["Ninit"]), "unseeded_corners": int(b.attrs["Ninit"]),
           "seeded_median_dx_dy": [float(a["dx"].median()), float(a["dy"].median())], "unseeded_median_dx_dy": [float(b["dx"].median()), float(b["dy"].median())]}
    lk = {"seeded": [], "unseeded": []}
    ctx.set_profiling(True)
    try:
        for _ in range(args.repeats):
            seeded()
            lk["seeded"].append(ctx.stage_ms()["lk_fwd_bwd"])
            unseeded()
            lk["unseeded"].append(ctx.stage_ms()["lk_fwd_bwd"])
    finally:
        ctx.set_profiling(False)
    rec["lk_ms"] = {k: {"median": statistics.median(v), "min": min(v), "all": v} for k, v in lk.items()}
    rec["seeded_over_unseeded"] = rec["lk_ms"]["seeded"]["median"] / rec["lk_ms"]["unseeded"]["median"]

    def wall(fn):
        out = []
        for _ in range(args.repeats + 1):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out[1:])

    u16 = lambda t: t                                                            # (int16 storage of uint16 pixels)
    rec["prior_mask_call_ms"] = wall(lambda: ops.prior_mask(u16(ref), u16(raw), P, dtype=np.uint16))
    dst = torch.empty_like(raw)
    shift = lambda: ctx.check(ctx.lib.km_shift_image_dev(ctx.handle, C.c_void_p(raw.data_ptr()), 2, side, side, side, SY, SX, C.c_void_p(dst.data_ptr())),
                              "km_shift_image_dev")
    rec["shift_copy_ms"] = wall(shift)
    rec["shift_copy_bytes"] = int(raw.numel() * 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))
    print("written", args.out)


if __name__ == "__main__":
    main()
