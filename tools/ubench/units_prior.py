#!/usr/bin/env python3
"""Timing of the batched submission under priors: four distinct resident 10980 x 10980 uint16 pairs whose monitored
rasters lie off the reference by four different integer shifts, 20 000 corners each, three routes to their frame blocks:

  (a) ONE km_klt_units_frame_prior_submit for the four pairs (`submit_units(priors=)`), and a pipelined stream of such submissions
      ("units_pipeline" 1, six in a row, at most three in flight);
  (b) the only prior route of the parent: four km_klt_tile_frame_prior_dev calls, one after the other (`_prior_tile_raw`, no DataFrame);
  (c) the reference's route on this library: four km_shift_image_dev copies + one unseeded batch on the copies, without scores (the
      reference skips them there).

Wall time of the submitting thread from the first call to the last block's arrival, the context synchronised in front (the library
works on streams of its own, so an event of the caller's stream brackets nothing); median of the repeats after a warm-up, the routes
alternating.  Per route: ms per pair and the stage spans of one submission (`km_frame_stage_ms`; (b): of the last tile call).  The
prior-mask launch of the batch has no entry point of its own, so its cost is given by a PROXY: four km_prior_mask_dev calls (the
single-unit kernel, the same item) into a preallocated mask, wall time with the context's synchronisation - four call overheads more
than the batched launch, none of its grid's empty workgroups.  Recorded, not gated.

    python tools/ubench/units_prior.py [--out profiles/units_prior.json] [--side 10980] [--points 20000] [--repeats 5]
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
from karios_amd.resident import ResidentPair, submit_units  # noqa: E402

SHIFTS = [(14, -6), (7, 3), (-9, 12), (20, 5)]          # (sx, sy) per pair: raw(x + sx, y + sy) == mon(x, y)
THRESHOLD = 0.4


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "units_prior.json"))
    ap.add_argument("--side", type=int, default=10980)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    side, n = args.side, len(SHIFTS)
    ctx = ops.default_context()
    conf = KLTConfiguration(maxCorners=args.points)
    raws, refs, copies, priors = [], [], [], []
    for k, (sx, sy) in enumerate(SHIFTS):
        mon, ref = synth.make_pair_torch(side, side, 0.4, -0.3, seed=7 + k, device="cuda")
        raws.append(torch.roll(mon, shifts=(sy, sx), dims=(0, 1)).contiguous())
        refs.append(ref)
        copies.append(torch.empty_like(mon))
        priors.append(prior_mod.from_shift(sy, sx))
        del mon
    torch.cuda.synchronize()
    wrap = lambda m, r: ResidentPair.from_device_pointers(m.data_ptr(), r.data_ptr(), np.uint16, side, side, ctx=ctx, keepalive=(m, r))
    raw_pairs = [wrap(m, r) for m, r in zip(raws, refs)]
    copy_pairs = [wrap(m, r) for m, r in zip(copies, refs)]
    raw_units, copy_units = [(p, None, None) for p in raw_pairs], [(p, None, None) for p in copy_pairs]

    def route_a():
        pend = submit_units(raw_units, conf, THRESHOLD, priors=priors)
        pend.wait()
        return pend

    def route_a_stream(count=6):
        ctx.set_option("units_pipeline", 1)
        try:
            pend = []
            for _ in range(count):
                pend.append(submit_units(raw_units, conf, THRESHOLD, priors=priors))
                if len(pend) >= 3:
                    pend[-3].wait()
            for p in pend:
                p.wait()
        finally:
            ctx.set_option("units_pipeline", 0)
        return count

    def route_b():
        return [p._prior_tile_raw(conf, None, 0, 0, P, THRESHOLD) for p, P in zip(raw_pairs, priors)]

    def route_c():
        for raw, dst, (sx, sy) in zip(raws, copies, SHIFTS):
            ctx.check(ctx.lib.km_shift_image_dev(ctx.handle, C.c_void_p(raw.data_ptr()), 2, side, side, side, sy, sx, C.c_void_p(dst.data_ptr())),
                      "km_shift_image_dev")
        pend = submit_units(copy_units, conf, None)
        pend.wait()
        return pend

    def masks():
        out = torch.empty((side, side), dtype=torch.uint8, device="cuda")
        for raw, ref, P in zip(raws, refs, priors):
            ctx.check(ctx.lib.km_prior_mask_dev(ctx.handle, C.c_void_p(ref.data_ptr()), C.c_void_p(raw.data_ptr()), raw_pairs[0].code, side, side, side, side, None, 0,
                                                None, None, P.ctypes.data_as(C.POINTER(C.c_double)), 0.0, 0.0, C.c_void_p(out.data_ptr())), "km_prior_mask_dev")

    def wall(fn):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    routes = {"a_batched_prior": route_a, "b_tile_prior_calls": route_b, "c_shift_copies_unseeded_batch": route_c}
    rec = {"device": torch.cuda.get_device_name(0), "side": side, "pairs": n, "max_corners": args.points, "repeats": args.repeats, "pixel_type": "uint16",
           "shifts": SHIFTS, "threshold": THRESHOLD}
    rows = {}
    for name, fn in routes.items():                                              # warm-up, and what every route found
        out = fn()
        raws_out = out.wait() if hasattr(out, "wait") else out
        rows[name] = [r.n_rows for r in raws_out]
    route_a_stream(3)
    masks()
    rec["rows"] = rows
    times = {k: [] for k in list(routes) + ["a_pipelined_stream", "prior_masks_proxy_four_single_calls"]}
    for _ in range(args.repeats):
        for name, fn in routes.items():
            times[name].append(wall(fn)[0] / n)
        t, count = wall(route_a_stream)
        times["a_pipelined_stream"].append(t / count / n)
        times["prior_masks_proxy_four_single_calls"].append(wall(masks)[0] / n)
    rec["ms_per_pair"] = {k: {"median": statistics.median(v), "min": min(v), "all": v} for k, v in times.items()}
    ctx.set_profiling(True)
    try:
        spans = {"a_batched_prior": route_a().stage_ms(), "c_shift_copies_unseeded_batch": route_c().stage_ms()}
        route_b()
        spans["b_tile_prior_calls_last_tile"] = ctx.stage_ms()
    finally:
        ctx.set_profiling(False)
    rec["stage_ms"] = spans
    step = rec["ms_per_pair"]["a_batched_prior"]["median"]
    rec["mask_proxy_share_of_batched_step"] = rec["ms_per_pair"]["prior_masks_proxy_four_single_calls"]["median"] / step
    rec["a_over_b"] = step / rec["ms_per_pair"]["b_tile_prior_calls"]["median"]
    rec["a_over_c"] = step / rec["ms_per_pair"]["c_shift_copies_unseeded_batch"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))
    print("written", args.out)


if __name__ == "__main__":
    main()
