#!/usr/bin/env python3
"""What the tracker's outlier filter (`outliers_filtering`) costs at 10980^2, in the headline's form - four distinct pairs per batched
submission, pipelined, ZNCC on: ms per pair with the filter on, with it off, and through the host path a user had before the device
clip (`ResidentPair._match_tile_host_clip`: a blocking call, three copies of point lists, numpy's clip and sort, a second scoring call).
Then the clip kernel alone on 20 000 rows.  python tools/clip_probe.py [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from karios_amd import frames, ops, synth
from karios_amd._lib import Context
from karios_amd.core import KLTConfiguration
from karios_amd.resident import ResidentPair
from karios_amd.stream import FrameStream

S = int(os.environ.get("KARIOS_PROBE_SIDE", 10980))
N = 4                                   # pairs per submission
out_path = sys.argv[1] if len(sys.argv) > 1 else "clip_probe.json"
dev = torch.device("cuda", 0)
ctx = Context(0)
on, off = KLTConfiguration(outliers_filtering=True), KLTConfiguration()
pairs = []
for b in range(N):
    mon, ref = synth.make_pair_torch(S, S, 0.5, 0.25, seed=20260101 + 10 * b, device=dev)
    torch.cuda.synchronize()
    pairs.append(ResidentPair.from_device_pointers(mon.data_ptr(), ref.data_ptr(), np.uint16, S, S, ctx=ctx, keepalive=(mon, ref)))
record = {"device": torch.cuda.get_device_name(0), "side": S, "pairs_per_submission": N, "max_corners": on.maxCorners}

# ---- the pipelined loop, windows alternating between the two settings
steps = int(os.environ.get("KARIOS_PROBE_SUBS", 12))
windows = {True: [], False: []}
rows = {}
with FrameStream(0.4, depth=2) as s:
    def go(conf, count):
        got = 0
        for _ in range(count):
            got += sum(d.raw.n_rows for d in s.submit_many([(p, None, None) for p in pairs], conf))
        got += sum(d.raw.n_rows for d in s.drain())
        ctx.sync()
        return got
    go(on, 4), go(off, 4)
    for rep in range(5):
        for flag in ((True, False) if rep % 2 == 0 else (False, True)):
            t0 = time.perf_counter()
            got = go(on if flag else off, steps)
            windows[flag].append((time.perf_counter() - t0) / (steps * N) * 1e3)
            rows[flag] = got // (steps * N)
    redone = s.units_redone
for flag, name in ((True, "filter_on"), (False, "filter_off")):
    w = sorted(windows[flag])
    record[name] = {"ms_per_pair_median_of_5_windows": w[2], "windows": [round(v, 4) for v in windows[flag]], "rows_per_pair": rows[flag]}
record["filter_on_over_off"] = record["filter_on"]["ms_per_pair_median_of_5_windows"] / record["filter_off"]["ms_per_pair_median_of_5_windows"]
record["units_redone"] = redone

# ---- the host path: what `match_tile(conf(outliers_filtering=True), zncc_threshold=...)` ran before the device clip
host = []
for rep in range(3):
    for p in pairs:
        t0 = time.perf_counter()
        f = p._match_tile_host_clip(on, None, 0, 0, 0.4)
        host.append((time.perf_counter() - t0) * 1e3)
record["host_path"] = {"ms_per_pair_median_of_12": float(np.median(host)), "median_without_the_first_round": float(np.median(host[N:])), "rows": len(f)}
# the two paths deliver the same frame
dev_frame = pairs[-1].match_tile(on, zncc_threshold=0.4)
record["device_frame_equals_host_frame"] = bool(dev_frame.index.equals(f.index) and all(
    np.array_equal(dev_frame[c].to_numpy(), f[c].to_numpy(), equal_nan=True) for c in ("x0", "y0", "dx", "dy", "score", "zncc_score")))

# ---- the kernel alone, 20 000 rows
def back_to_back(tdx, tdy, reps=20):
    """ms per km_sigma_clip_dev: `reps` calls enqueued one behind the other, one synchronise at the end (the launches overlap the kernels)."""
    import ctypes as C
    n = tdx.numel()
    keep, res = torch.empty(n, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    tab = lambda p: (C.c_void_p * 1)(p)
    args = (tab(tdx.data_ptr()), tab(tdy.data_ptr()), (C.c_int * 1)(n), 1, tab(keep.data_ptr()), C.c_void_p(res.data_ptr()))
    torch.cuda.synchronize()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.check(ctx.lib.km_sigma_clip_dev(ctx.handle, *args), "km_sigma_clip_dev")
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def kernel_alone(dx, dy, reps=30):
    tdx, tdy = torch.from_numpy(dx).to(dev), torch.from_numpy(dy).to(dev)
    keep, rounds = ops.sigma_clip(tdx, tdy, ctx=ctx, return_rounds=True)
    queued = sorted(back_to_back(tdx, tdy) for _ in range(5))[2]
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ops.sigma_clip(tdx, tdy, ctx=ctx)
        times.append((time.perf_counter() - t0) * 1e3)
    t_np = []
    for _ in range(5):
        t0 = time.perf_counter()
        want = frames.sigma_clip(dx, dy)
        t_np.append((time.perf_counter() - t0) * 1e3)
    return {"n": int(dx.size), "survivors": int(keep.numel()), "rounds": rounds, "kernel_ms_20_calls_back_to_back_median_of_5": queued,
            "us_per_round": 1e3 * queued / max(rounds, 1), "call_ms_median_of_30": float(np.median(times)),
            "numpy_ms_median_of_5": float(np.median(t_np)), "equal_to_numpy": bool(np.array_equal(keep.cpu().numpy(), want)),
            "note": "call_ms: host clock around ops.sigma_clip - the call, its synchronise, the result copy and the tensor bookkeeping"}

rng = np.random.default_rng(1)
t = rng.standard_t(3, size=(2, 20000))
record["kernel_heavy_tails"] = kernel_alone((0.4 * t[0]).astype(np.float32), (0.4 * t[1]).astype(np.float32))
plain = pairs[0].match_tile(off)
order = np.argsort(plain.index.to_numpy())
record["kernel_fb_kept_list"] = kernel_alone(plain["dx"].to_numpy()[order].copy(), plain["dy"].to_numpy()[order].copy())
with open(out_path, "w") as fh:
    json.dump(record, fh, indent=1)
print(json.dumps(record))
