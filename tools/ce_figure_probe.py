"""Wall clock of the circular-error figure's numbers next to numpy / scipy on the same machine's host.

    python tools/ce_figure_probe.py [--sizes 80000,3000000] [--reps 10] [--out profiles/ce_figure_probe.json]

Per size: a synthetic frame (normal displacements, two rows in three above the threshold) resident on the device; the median wall
time of --reps calls of `ops.ce_figure` on the device columns after one warm-up call (three library calls, numpy's linspace and scipy's
spline fit between them, the stream drained by each), and of the reference's numpy / scipy expressions on host copies
(tests/ce_figure_cases.py `numpy_figure`: both np.histogram, np.histogram2d, interpn, argsort, sort, mean / std, the percentiles).
One process; every GPU step runs under a time limit of its own (an alarm that ends the process: nothing is started behind a step that
hung).  The host figure is one machine's, with whatever else runs on it.
"""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from karios_amd import ops  # noqa: E402

THRESHOLD, RES = 0.4, 10.0


class step_limit:
    """with step_limit(seconds, what): the process ends (status 124) when the step takes longer."""

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _expired(self, *_):
        sys.stderr.write(f"ce_figure_probe: step '{self.what}' exceeded {self.seconds} s; stopping\n")
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def frame(n):
    rng = np.random.default_rng(n)
    score = (rng.integers(10, 65, n) / 64).astype(np.float32)
    return (rng.standard_normal(n) * 1.5 + 0.2).astype(np.float32), (rng.standard_normal(n) * 0.8 - 0.1).astype(np.float32), score


def median_ms(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="80000,3000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_figure_probe.json"))
    args = ap.parse_args()
    import torch
    import ce_figure_cases as K
    records = []
    for n in (int(s) for s in args.sizes.split(",")):
        dx, dy, score = frame(n)
        with step_limit(120, f"upload and warm-up of {n} rows"):
            cols = tuple(torch.from_numpy(a).cuda() for a in (dx, dy, score))
            fig = ops.ce_figure(*cols, THRESHOLD, RES)
            torch.cuda.synchronize()
        with step_limit(300, f"{args.reps} device calls of {n} rows"):
            dev = median_ms(lambda: ops.ce_figure(*cols, THRESHOLD, RES), args.reps)
        want = K.numpy_figure(dx, dy, score, THRESHOLD, RES)
        host = median_ms(lambda: K.numpy_figure(dx, dy, score, THRESHOLD, RES), args.reps)
        rec = {"rows": n, "sample": fig.sample, "bins_x": int(fig.bins_x.size - 1), "bins_y": int(fig.bins_y.size - 1), "n_outside": fig.n_outside,
               "path": fig.path, "equal_to_numpy_scipy": not K.differing(fig, want), "reps": args.reps,
               "device_ms": {"median": dev[0], "min": dev[1], "max": dev[2]}, "host_numpy_scipy_ms": {"median": host[0], "min": host[1], "max": host[2]}}
        print(json.dumps(rec), flush=True)
        records.append(rec)
    out = {"tool": "tools/ce_figure_probe.py", "device": torch.cuda.get_device_name(0), "host_cpus_usable": len(os.sched_getaffinity(0)),
           "threshold": THRESHOLD, "img_res": RES, "records": records}
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
