"""Times of the align step's descriptor matching next to its operation model.

    python tools/match_probe.py [--sizes 20000x30000,200000x200000,1000000x1000000] [--reps 10] [--cpu-cells 1e9]
                                [--out profiles/match_probe.json]

Synthetic SIFT-like descriptors (karios_amd.synth.descriptor_scene: 40 % planted pairs, 6 % rivals, sigma 30), resident on the device.
Per size: the median wall time of --reps calls of km_match_lowe_mutual_dev (pack, both directions, filter, the copy of the counters)
and of km_knn_match_u8_dev for (mon, ref, 2) and (ref, mon, 1) alone, the library's stream drained after each call.  One process;
every GPU step runs under a time limit of its own (an alarm that ends the process: nothing is started behind a step that hung).
--cpu-cells: the host restatement (tests/match_restatement.py) is timed once where n_mon * n_ref does not exceed it.
--merge-into FILE --kernel-stats CSV_OR_DIR --sizes ONE_SIZE: no GPU work; the kernel_stats CSV or database of a `rocprofv3 --kernel-trace --stats --
python tools/match_probe.py --sizes ONE_SIZE --out ''` run of this probe is read and its average kernel times are added to that
size's record in FILE.
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

I8_DENSE_OPS_PER_S = 5.0e15     # MI355X dense int8 MFMA rate (twice the bf16 form's 2.5e15), the yardstick of the operation model


class step_limit:
    """with step_limit(seconds, what): the process ends (status 124) when the step takes longer."""

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _expired(self, *_):
        sys.stderr.write(f"match_probe: step '{self.what}' exceeded {self.seconds} s; stopping\n")
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


KERNELS = ("knn_kernel<1>", "knn_kernel<2>", "knn_merge_kernel<1>", "knn_merge_kernel<2>", "pack_kernel", "filter_flag_kernel",
           "filter_scatter_kernel")


def kernel_stats(path):
    """Average duration per kernel of this feature from rocprofv3's output: a *kernel_stats.csv, or the rocpd database (*.db) newer
    versions write by default (its `kernels` view holds one row per dispatch)."""
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
            if key in name or key.replace("<", "ILi").replace(">", "E") in name:
                out[key] = {"calls": int(calls), "average_us": round(float(avg) / 1e3, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000x30000,200000x200000,1000000x1000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-cells", type=float, default=1e9)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--merge-into", default="", help="no GPU work: add --kernel-stats to the record of --sizes in this JSON file")
    ap.add_argument("--out", default="profiles/match_probe.json")
    a = ap.parse_args()
    if a.merge_into:
        n, m = (int(v) for v in a.sizes.split("x"))
        doc = json.load(open(a.merge_into))
        for rec in doc["sizes"]:
            if (rec["n_mon"], rec["n_ref"]) == (n, m):
                rec["kernel_trace"] = kernel_stats(a.kernel_stats)
        with open(a.merge_into, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    c = _lib.default_context()
    lib, h = c.lib, c.handle
    records = []
    for size in a.sizes.split(","):
        n, m = (int(v) for v in size.split("x"))
        mon, ref = synth.descriptor_scene(n, m, min(n, m) * 2 // 5, min(n, m) * 3 // 50, 30, 1)
        bufs = []

        def dev(nbytes):
            p, cap = c.dev_alloc(nbytes)
            bufs.append((p, cap))
            return C.c_void_p(p)

        with step_limit(120, f"upload {size}"):
            d_mon, d_ref = dev(mon.nbytes), dev(ref.nbytes)
            c.check(lib.km_h2d(h, d_mon, _lib.ptr(mon), mon.nbytes), "km_h2d")
            c.check(lib.km_h2d(h, d_ref, _lib.ptr(ref), ref.nbytes), "km_h2d")
            d_qi, d_ti, d_dist = dev(4 * n), dev(4 * n), dev(4 * n)
            d_idx, d_d = dev(8 * max(n, m)), dev(8 * max(n, m))
        counts = (C.c_int * 3)()

        def timed(fn, what):
            ts = []
            for _ in range(a.reps + 1):
                with step_limit(120, f"{what} {size}"):
                    t0 = time.perf_counter()
                    fn()
                    c.sync()
                    ts.append(time.perf_counter() - t0)
            return round(statistics.median(ts[1:]) * 1e3, 3)

        ms = {
            "match_lowe_mutual_dev": timed(lambda: c.check(lib.km_match_lowe_mutual_dev(h, d_mon, n, 128, d_ref, m, 128, _lib.KM_U8, 128, 0.75, n,
                                                                                        d_qi, d_ti, d_dist, counts), "match"), "match"),
            "knn_mon_ref_2_dev": timed(lambda: c.check(lib.km_knn_match_u8_dev(h, d_mon, n, 128, d_ref, m, 128, 128, 2, d_idx, d_d), "knn"), "knn 2"),
            "knn_ref_mon_1_dev": timed(lambda: c.check(lib.km_knn_match_u8_dev(h, d_ref, m, 128, d_mon, n, 128, 128, 1, d_idx, d_d), "knn"), "knn 1"),
        }
        ops_dir = 2.0 * n * m * 128
        rec = {"n_mon": n, "n_ref": m, "reps": a.reps, "counts": list(counts), "ms": ms,
               "integer_ops_per_direction": ops_dir,
               "model_ms_per_direction_at_i8_dense_rate": round(ops_dir / I8_DENSE_OPS_PER_S * 1e3, 3),
               "achieved_Tops_per_s": {k: round(ops_dir / (ms[k] * 1e-3) / 1e12, 1) for k in ("knn_mon_ref_2_dev", "knn_ref_mon_1_dev")}}
        if float(n) * m <= a.cpu_cells:
            import match_restatement as R
            t0 = time.perf_counter()
            want = R.match_lowe_mutual(mon, ref)
            rec["host_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            rec["counts_equal_restatement"] = list(want[3]) == list(counts)
        for p, cap in bufs:
            c.dev_release(p, cap)
        records.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"i8_dense_ops_per_s_yardstick": I8_DENSE_OPS_PER_S, "sizes": records}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
