#!/usr/bin/env python3
"""Timing of the vector-mask burn on a full-size grid: `ops.rasterize_polygons` into a resident 10980 x 10980
uint8 plane, the fill and the line pass separately, by events on the library's stream (km_mask_pass_ms) after warm-up:

  (a) a 4-vertex oblique quadrilateral - the line pass is four long sequential walks;
  (b) a 4096-vertex polygon with one hole.

Beside them, taken in the same run: the page-locked upload of a mask of that size through the copy `ResidentPair.upload` makes of its
mask (DeviceBuffer.upload_image_async from `pinned_empty` memory, then the context's sync) - the cost the burn replaces - and the fill's
byte model (side^2 bytes written once).  The rasters are checked: two calls give the same bytes, the count of ones lies within one and
a half perimeters of the polygon's area.  Recorded, not gated.

    python tools/ubench/mask_rasterize.py [--out profiles/mask_rasterize.json] [--side 10980] [--calls 10]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from karios_amd import ops, pinned_empty  # noqa: E402
from karios_amd.resident import DeviceBuffer  # noqa: E402


def ring_of(n, cx, cy, r, wobble, phase=0.0):
    pts = [(cx + r * (1.0 + wobble * math.sin(7 * a + phase)) * math.cos(a), cy + r * (1.0 + wobble * math.sin(7 * a + phase)) * math.sin(a))
           for a in (2.0 * math.pi * k / n for k in range(n))]
    return pts + [pts[0]]


def area_and_perimeter(rings):
    area = perimeter = 0.0
    for k, ring in enumerate(rings):
        a = 0.5 * sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(ring[:-1], ring[1:]))
        area += abs(a) if k == 0 else -abs(a)
        perimeter += sum(math.hypot(q[0] - p[0], q[1] - p[1]) for p, q in zip(ring[:-1], ring[1:]))
    return area, perimeter


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_rasterize.json"))
    ap.add_argument("--side", type=int, default=10980)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    side, s = args.side, args.side / 10980.0
    ctx = ops.default_context()
    rec = {"device": torch.cuda.get_device_name(0), "side": side, "calls": args.calls, "model_MB": side * side / 1e6}
    quad = [[(1200.3 * s, 800.7 * s), (9800.6 * s, 1500.2 * s), (10100.4 * s, 9900.9 * s), (700.8 * s, 9100.5 * s), (1200.3 * s, 800.7 * s)]]
    big = [ring_of(3071, 5490.2 * s, 5490.7 * s, 4700.0 * s, 0.08), ring_of(1023, 5200.4 * s, 5600.1 * s, 1500.0 * s, 0.05, 1.0)[::-1]]
    out = torch.empty((side, side), dtype=torch.uint8, device="cuda")
    for name, rings in (("quadrilateral_4", quad), ("polygon_4096_one_hole", big)):
        vertices = sum(len(r) for r in rings)
        ops.rasterize_polygons([rings], (side, side), out=out)                    # warm-up: workspace growth, first launch
        first = out.clone()
        ctx.set_profiling(True)
        fill, lines, wall = [], [], []
        try:
            for _ in range(args.calls):
                t0 = time.perf_counter()
                ops.rasterize_polygons([rings], (side, side), out=out)
                wall.append((time.perf_counter() - t0) * 1e3)
                f, l = ctx.mask_pass_ms()
                fill.append(f)
                lines.append(l)
        finally:
            ctx.set_profiling(False)
        if not torch.equal(first, out):
            raise SystemExit(f"{name}: two calls differ")
        ones = int(out.sum(dtype=torch.int64))
        area, perimeter = area_and_perimeter(rings)
        if abs(ones - area) > 1.5 * perimeter + 4:          # (all-touched adds at most |dx| + |dy| pixels per edge)
            raise SystemExit(f"{name}: {ones} ones for an area of {area:.0f} and a perimeter of {perimeter:.0f}")
        row = {"case": name, "vertices": vertices, "ones": ones, "area": area, "fill_ms_median": statistics.median(fill), "fill_ms_min": min(fill),
               "lines_ms_median": statistics.median(lines), "lines_ms_min": min(lines), "call_wall_ms_median": statistics.median(wall),
               "fill_TB_per_s": side * side / 1e9 / statistics.median(fill)}
        rec[name] = row
        print(row, flush=True)

    # the yardstick: the same plane from page-locked host memory
    host = pinned_empty((side, side), np.uint8, ctx)
    host[:] = 1
    buf = DeviceBuffer(ctx, host.nbytes)
    t = []
    for k in range(args.calls + 1):
        t0 = time.perf_counter()
        keep = buf.upload_image_async(host)
        ctx.sync()
        if k:
            t.append((time.perf_counter() - t0) * 1e3)
    del keep
    rec["pinned_upload"] = {"ms_median": statistics.median(t), "ms_min": min(t), "GB_per_s": side * side / 1e6 / statistics.median(t)}
    print("pinned_upload", rec["pinned_upload"], flush=True)
    buf.free()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
