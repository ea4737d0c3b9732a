#!/usr/bin/env python3
"""Timing and full-size check of analyze_accuracy's device entry points on resident data.

  * km_count_valid_pixels_dev on a 10980 x 10980 uint16 raster with a mask: the result against torch.count_nonzero of the same
    device tensors, the median of 10 calls against the byte model (3 B / px);
  * km_accuracy_stats_dev at n = 80 000 and 3 000 000 rows: the median of 10 calls beside the same numpy / pandas expressions
    (accuracy_statistics.py:82-238) timed on this machine's host.

    python tools/accuracy_probe.py [--out profiles/accuracy_probe.json] [--side 10980]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from karios_amd import ops  # noqa: E402


def median_ms(fn, calls=10):
    fn()                                                   # warm-up: workspace growth, first launch
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def host_statistics(points, confidence=0.4):
    """The reference's expressions, on the host."""
    vx, vy, vc = points["dx"], points["dy"], points["score"]
    mas = vc.gt(confidence)
    x, y, c = np.array(vx[mas]), np.array(vy[mas]), np.array(vc[mas])
    out = [f(v) for v in (x, y, c) for f in (np.min, np.max, np.median, np.mean, np.std)]
    for percent in (0.9, 0.95):
        v_s = np.sort(np.sqrt(x * x + y * y))
        p = percent * v_s.shape[0]
        k = int(p)
        out.append(v_s[k - 1] + (v_s[k] - v_s[k - 1]) * (p - k))
    return x.size, out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accuracy_probe.json"))
    ap.add_argument("--side", type=int, default=10980)
    args = ap.parse_args()
    dev = torch.device("cuda")
    rec = {"device": torch.cuda.get_device_name(0), "side": args.side}

    # ---- the count
    side = args.side
    g = torch.Generator(device=dev).manual_seed(1)
    img16 = torch.randint(-3, 4, (side, side), dtype=torch.int16, device=dev, generator=g)          # one pixel in seven is zero
    mask = (torch.rand((side, side), device=dev, generator=g) < 0.8).to(torch.uint8)
    want = int(torch.count_nonzero((img16 != 0) & (mask != 0)))
    img = img16.view(torch.uint16)
    got = ops.count_valid_pixels(img, mask)
    if got != want:
        raise SystemExit(f"count_valid_pixels {got} != torch.count_nonzero {want}")
    ms = median_ms(lambda: ops.count_valid_pixels(img, mask))
    ms_nomask = median_ms(lambda: ops.count_valid_pixels(img))
    gb = side * side * 3 / 1e9
    rec["count"] = {"valid": got, "total": side * side, "ms_median_of_10": ms, "model_GB": gb, "TB_per_s": gb / ms, "ms_no_mask": ms_nomask,
                    "TB_per_s_no_mask": side * side * 2 / 1e9 / ms_nomask, "checked_against": "torch.count_nonzero"}
    print("count", rec["count"], flush=True)
    del img, img16, mask

    # ---- the statistics
    rec["statistics"] = []
    rng = np.random.default_rng(2)
    for n in (80_000, 3_000_000):
        dx = (0.4 + 0.3 * rng.standard_normal(n)).astype(np.float32)
        dy = (-0.3 + 0.3 * rng.standard_normal(n)).astype(np.float32)
        score = rng.random(n).astype(np.float32)
        points = pd.DataFrame({"dx": dx, "dy": dy, "score": score})
        cols = [torch.from_numpy(a).to(dev) for a in (dx, dy, score)]
        res = ops.accuracy_statistics(*cols, 0.4)
        sample, host = host_statistics(points)
        names = list(ops.ACCURACY_STAT_NAMES)
        dev_vals = [res.stats[k] for k in names] + list(res.ce)
        same = res.sample == sample and all(np.float32(a) == np.float32(b) for a, b in zip(dev_vals, host))
        if not same:
            raise SystemExit(f"statistics at n = {n} differ from numpy's: {dev_vals} != {host}")
        row = {"n": n, "sample": sample, "device_ms_median_of_10": median_ms(lambda: ops.accuracy_statistics(*cols, 0.4)),
               "host_numpy_pandas_ms_median_of_10": median_ms(lambda: host_statistics(points)), "equal_to_numpy": True}
        rec["statistics"].append(row)
        print("statistics", row, flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
