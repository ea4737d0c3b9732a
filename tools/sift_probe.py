"""Stage times of the align step's SIFT next to a byte model of its dense stages.

    python tools/sift_probe.py [--size 10980] [--reps 10] [--limit 600] [--out profiles/sift_probe.json]

A synthetic raster of karios_amd.synth (the bench texture, seed 11) goes through ops.preprocess (percentile stretch + CLAHE) and
stays on the device.  --reps calls of km_sift_detect_and_compute_dev on it; per stage the median over the calls of the device time
the call itself reports (stream events around the stages, summed over the octaves and listed per octave), the host time of the
final order, and the whole call by the host clock next to the sum of its stages - the difference is what the host adds between
the stages (the allocation of the planes, the copy of the records to the host).  The calls run in a child process under --limit
seconds (default 600): a call that hangs is killed there and the probe ends with status 124, nothing is started behind it.

The byte model (bytes that must cross HBM at the least, P = samples of the octave's plane, float32):
  base      the uint8 raster once (P / 4 bytes), the doubled image written and read (8 P), the two blur passes (16 P)
  blur_dog  per level: row pass read + write (8 P), column pass read, the level below read for the DoG, level and DoG written
            (16 P); n + 2 levels; the decimation reads every second row and writes a quarter plane (3 P)
  scan      the n + 2 DoG planes once (4 P each)
The sparse stages (refine, orient, describe) are bound by their sequential per-lane loops, not by bytes: no model.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_LAYERS = 3


def model_bytes(h, w, n_octaves):
    out = {"base": 0.25 * h * w + 24.0 * 4 * h * w, "blur_dog": [], "scan": []}
    hh, ww = 2 * h, 2 * w
    for _ in range(n_octaves):
        p = float(hh * ww)
        out["blur_dog"].append((N_LAYERS + 2) * 24 * p + 3 * p)
        out["scan"].append((N_LAYERS + 2) * 4 * p if hh > 10 and ww > 10 else 0.0)
        hh, ww = hh // 2, ww // 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10980)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=600, help="seconds for the whole run of the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift_probe.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    # this process never opens the GPU: it only waits for the child, and kills it when the limit runs out
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--size", str(a.size), "--reps", str(a.reps),
                              "--out", a.out], timeout=a.limit)
    except subprocess.TimeoutExpired:
        sys.stderr.write(f"sift_probe: no result within {a.limit} s; the child process was killed\n")
        return 124
    return out.returncode


def worker(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from karios_amd import _lib, ops, synth
    ctx = _lib.default_context()
    dev = torch.device("cuda", ctx.device)
    n = a.size
    raw = synth._base_torch(n, n, 11, dev)[synth.PAD:synth.PAD + n, synth.PAD:synth.PAD + n].cpu().numpy()
    d_img = torch.from_numpy(ops.preprocess(raw)).to(dev)
    del raw
    runs = []
    for rep in range(a.reps + 1):                                    # the first call sizes the lists: not counted
        t0 = time.perf_counter()
        kp, desc, st = ops.sift_detect_and_compute(d_img, descriptor_dtype=np.uint8, return_stats=True)
        st["wrapper_s"] = time.perf_counter() - t0
        del kp, desc
        if rep:
            runs.append(st)
    med = lambda f: statistics.median(f(r) for r in runs)            # noqa: E731
    n_oct = runs[0]["octaves"]
    model = model_bytes(n, n, n_oct)
    rec = {"size": n, "reps": a.reps, "octaves": n_oct, "count": runs[0]["count"], "before_dedup": runs[0]["before_dedup"],
           "candidates": runs[0]["candidates"], "refined": runs[0]["refined"], "keypoints": runs[0]["keypoints"],
           "workspace_gb": round(runs[0]["workspace_bytes"] / 1e9, 3), "stages_ms": {}, "per_octave_ms": {}, "model": {}}
    rec["stages_ms"]["base"] = round(med(lambda r: r["times_us"]["base"]) / 1e3, 3)
    for name in ops.SIFT_STAGES:
        rec["stages_ms"][name] = round(med(lambda r: sum(r["times_us"][name])) / 1e3, 3)
        rec["per_octave_ms"][name] = [round(med(lambda r, o=o: r["times_us"][name][o]) / 1e3, 3) for o in range(n_oct)]
    rec["stages_ms"]["sort_host"] = round(med(lambda r: r["times_us"]["sort_host"]) / 1e3, 3)
    rec["stages_ms"]["gather"] = round(med(lambda r: r["times_us"]["gather"]) / 1e3, 3)
    rec["sum_of_stages_ms"] = round(sum(rec["stages_ms"].values()), 3)
    rec["call_ms"] = round(med(lambda r: r["times_us"]["call_host"]) / 1e3, 3)
    rec["call_minus_stages_ms"] = round(rec["call_ms"] - rec["sum_of_stages_ms"], 3)
    rec["wrapper_call_ms"] = round(med(lambda r: r["wrapper_s"]) * 1e3, 3)
    rec["wrapper_calls"] = runs[0]["calls"]
    rec["regrows"] = list(runs[0]["regrows"])
    for name, byts, ms in (("base", model["base"], rec["stages_ms"]["base"]), ("blur_dog", sum(model["blur_dog"]), rec["stages_ms"]["blur_dog"]),
                           ("scan", sum(model["scan"]), rec["stages_ms"]["scan"]),
                           ("blur_dog_octave0", model["blur_dog"][0], rec["per_octave_ms"]["blur_dog"][0]),
                           ("scan_octave0", model["scan"][0], rec["per_octave_ms"]["scan"][0])):
        rec["model"][name] = {"bytes": int(byts), "ms": ms, "tb_per_s": round(byts / (ms * 1e-3) / 1e12, 3) if ms else None}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
