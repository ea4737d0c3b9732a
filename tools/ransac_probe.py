"""Times of the align step's RANSAC homography next to its operation model.

    python tools/ransac_probe.py [--sizes 20000:0.5,200000:0.2,1000000:0.1] [--reps 10] [--cpu-evals 2e9]
                                 [--out profiles/ransac_probe.json]

Planted scenes of karios_amd.synth.homography_scene (sigma 0.4 px, seed 7), resident on the device.  Per (n, inlier share): the
median wall time of --reps calls of km_find_homography_ransac_dev - pack, the copy back of the pairs, every batch's subsets, launches
and count copies, the winner's mask, the solve on the inliers and the Levenberg-Marquardt refinement on the host, all included - with
the call's statistics.  One process; every GPU step runs under a time limit of its own (an alarm that ends the process: nothing is
started behind a step that hung).
--cpu-evals: the host restatement (tests/ransac_restatement.py: a Python loop with numpy scoring, NOT OpenCV) is timed once where
n * iterations run does not exceed it, and its outcome compared.
--merge-into FILE --kernel-stats CSV_OR_DIR --sizes ONE_SIZE: no GPU work; the kernel_stats CSV or database of a `rocprofv3
--kernel-trace --stats -- python tools/ransac_probe.py --sizes ONE_SIZE --out ''` run of this probe is read, its kernel times are
added to that size's record in FILE, and the scoring kernel's time is set against the operation model.

The operation model: the scoring loop of k_ransac.hip is VALU_PER_WAVE_ITERATION instructions per (wave, iteration) for 4 pairs a
lane (counted in the compiled code), so n * iterations / 256 * VALU_PER_WAVE_ITERATION wave-instructions, issued at
CYCLES_PER_WAVE_INSTRUCTION per SIMD on 256 CUs x 4 SIMDs at 2.4 GHz.
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
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
from karios_amd import _lib, synth  # noqa: E402
from karios_amd.ops import RANSAC_STATS  # noqa: E402

VALU_PER_WAVE_ITERATION = 95        # score_kernel's loop body: 4 pairs a lane (packed float32 multiplies and adds, 4 exact divisions)
PAIRS_PER_WAVE = 256
CYCLES_PER_WAVE_INSTRUCTION = 4.3
SIMDS, CLOCK_HZ = 256 * 4, 2.4e9
KERNELS = ("score_kernel", "solve_kernel", "mask_kernel", "pack_kernel")


def model_ms(n, iterations):
    return n * iterations / PAIRS_PER_WAVE * VALU_PER_WAVE_ITERATION * CYCLES_PER_WAVE_INSTRUCTION / (SIMDS * CLOCK_HZ) * 1e3


class step_limit:
    """with step_limit(seconds, what): the process ends (status 124) when the step takes longer."""

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _expired(self, *_):
        sys.stderr.write(f"ransac_probe: step '{self.what}' exceeded {self.seconds} s; stopping\n")
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def kernel_stats(path):
    """Calls, average and total duration per kernel of this feature from rocprofv3's output: a *kernel_stats.csv, or the rocpd
    database (*.db) newer versions write by default (its `kernels` view holds one row per dispatch)."""
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)) or \
            sorted(glob.glob(os.path.join(path, "**", "*.db"), recursive=True))
    else:
        found = [path]
    rows = []                                        # (name, calls, average ns)
    for f in found:
        if f.endswith(".db"):
            import sqlite3
            db = sqlite3.connect(f)
            rows += list(db.execute("select name, count(*), avg(duration) from kernels group by name"))
        else:
            rows += [(r.get("Name", ""), int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(f))]
    out = {}
    for name, calls, avg in rows:
        for key in KERNELS:
            if key in name:
                out[key] = {"calls": int(calls), "average_us": round(float(avg) / 1e3, 1), "total_ms": round(float(avg) * int(calls) / 1e6, 3)}
    return out


def parse_sizes(text):
    return [(int(s.split(":")[0]), float(s.split(":")[1])) for s in text.split(",")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000:0.5,200000:0.2,1000000:0.1")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-evals", type=float, default=2e9)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--merge-into", default="", help="no GPU work: add --kernel-stats to the record of --sizes in this JSON file")
    ap.add_argument("--out", default="profiles/ransac_probe.json")
    a = ap.parse_args()
    if a.merge_into:
        (n, w), = parse_sizes(a.sizes)
        doc = json.load(open(a.merge_into))
        for rec in doc["sizes"]:
            if (rec["n"], rec["inlier_share"]) == (n, w):
                ks = kernel_stats(a.kernel_stats)
                rec["kernel_trace"] = ks
                if "score_kernel" in ks:
                    # the traced run makes reps + 1 identical calls: the scoring kernel's time of ONE call against the model
                    per_call = ks["score_kernel"]["total_ms"] / (rec["reps"] + 1)
                    rec["score_kernel_ms_per_call"] = round(per_call, 3)
                    rec["score_kernel_over_model"] = round(per_call / rec["model_ms_evaluated"], 2)
        with open(a.merge_into, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    c = _lib.default_context()
    lib, h = c.lib, c.handle
    records = []
    for n, w in parse_sizes(a.sizes):
        src, dst, planted, _H = synth.homography_scene(n, w, 0.4, 7)
        bufs = []

        def dev(nbytes):
            p, cap = c.dev_alloc(nbytes)
            bufs.append((p, cap))
            return C.c_void_p(p)

        with step_limit(120, f"upload {n}"):
            d_src, d_dst, d_mask = dev(src.nbytes), dev(dst.nbytes), dev(n)
            c.check(lib.km_h2d(h, d_src, _lib.ptr(src), src.nbytes), "km_h2d")
            c.check(lib.km_h2d(h, d_dst, _lib.ptr(dst), dst.nbytes), "km_h2d")
        H, found, stats = np.zeros(9), C.c_int(0), (C.c_int64 * 8)()

        def call():
            c.check(lib.km_find_homography_ransac_dev(h, d_src, 2, d_dst, 2, n, 3.0, 10000, 0.999, H.ctypes.data_as(C.POINTER(C.c_double)), d_mask,
                                                      C.byref(found), stats, None, None), "km_find_homography_ransac_dev")

        ts = []
        for _ in range(a.reps + 1):
            with step_limit(300, f"find_homography {n}:{w}"):
                t0 = time.perf_counter()
                call()
                c.sync()
                ts.append(time.perf_counter() - t0)
        st = dict(zip(RANSAC_STATS, (int(v) for v in stats)))
        mask = np.zeros(n, np.uint8)
        c.check(lib.km_d2h(h, _lib.ptr(mask), d_mask, n), "km_d2h")
        rec = {"n": n, "inlier_share": w, "reps": a.reps, "found": int(found.value), "stats": st,
               "planted_inliers": int(planted.sum()), "mask_equals_planted": bool(np.array_equal(mask != 0, planted)),
               "find_homography_ransac_dev_ms": round(statistics.median(ts[1:]) * 1e3, 3),
               "evaluations": n * st["evaluated"],
               "model_ms_evaluated": round(model_ms(n, st["evaluated"]), 4), "model_ms_sequential": round(model_ms(n, st["ran"]), 4)}
        if float(n) * st["ran"] <= a.cpu_evals:
            import ransac_restatement as R
            info = {}
            t0 = time.perf_counter()
            Hw, maskw = R.find_homography(src, dst, 3.0, 10000, 0.999, info=info)
            rec["host_restatement_python_loop_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            rec["equals_restatement"] = bool(Hw is not None and np.array_equal(Hw.reshape(-1).view(np.uint64), H.view(np.uint64))
                                             and np.array_equal(maskw[:, 0], mask) and info["ran"] == st["ran"])
        for p, cap in bufs:
            c.dev_release(p, cap)
        records.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"valu_per_wave_iteration": VALU_PER_WAVE_ITERATION, "cycles_per_wave_instruction": CYCLES_PER_WAVE_INSTRUCTION,
                       "simds": SIMDS, "clock_hz": CLOCK_HZ, "sizes": records}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
