"""Driver of tests/test_sift_host.py part 1: csrc/sift_math.hpp, compiled by g++ under the address and undefined-behaviour
sanitizers into the shared object named on the command line, against tests/sift_restatement.py - bit for bit.  Runs in a subprocess
with libasan preloaded; prints SIFT-HOST OK at the end."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sift_restatement as S  # noqa: E402
from karios_amd import synth  # noqa: E402

lib = C.CDLL(sys.argv[1])
vp, ci, cd, cf, sz = C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_ssize_t
lib.sf_exp.argtypes = [ci, vp, vp]
lib.sf_sincos.argtypes = [ci, vp, vp, vp]
lib.sf_atan2.argtypes = [ci, vp, vp, vp]
lib.sf_kernel.argtypes, lib.sf_kernel.restype = [cd, vp], ci
lib.sf_level_sigma.argtypes, lib.sf_level_sigma.restype = [cd, ci, ci], cd
lib.sf_base_sigma.argtypes, lib.sf_base_sigma.restype = [cd], cf
lib.sf_n_octaves.argtypes, lib.sf_n_octaves.restype = [ci, ci], ci
lib.sf_refine_many.argtypes = [vp, C.c_size_t, sz, ci, ci, ci, ci, vp, ci, cd, cd, cd, vp, vp, vp]
lib.sf_orient.argtypes, lib.sf_orient.restype = [vp, sz, ci, ci, ci, ci, cf, ci, vp], ci
lib.sf_describe.argtypes = [vp, sz, ci, ci, cf, cf, cf, cf, vp]


def p(a):
    return a.ctypes.data_as(vp)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the four transcendentals over dense grids, endpoints and special values included
x = np.concatenate([np.linspace(-710, 40, 300001), [-700.0, -700.0000001, 0.0, -0.0, 1.0, -1.0, 5e-324, -745.0],
                    (np.arange(-1000, 50) + 0.5) * S.LN2, np.float32(np.linspace(-30, 0, 50001)).astype(np.float64)])
out = np.zeros_like(x)
lib.sf_exp(len(x), p(x), p(out))
assert same(out, S.exp64(x)), "exp differs"
ok = x > -700
assert np.abs(out[ok] / np.exp(x[ok]) - 1).max() < 4e-16
a = np.concatenate([np.linspace(0, 360, 400001), [0, 45, 90, 135, 180, 225, 270, 315, 360, 44.999996, 45.000004]]).astype(np.float32)
co, si = np.zeros_like(a), np.zeros_like(a)
lib.sf_sincos(len(a), p(a), p(co), p(si))
wc, ws = S.sincos_deg(a)
assert same(co, wc) and same(si, ws), "sin / cos differ"
assert np.abs(co - np.cos(np.deg2rad(a.astype(np.float64)))).max() < 6e-8
rng = np.random.default_rng(2)
yy = np.concatenate([rng.normal(size=200000), np.zeros(8), [1, -1, 1, -1, 0, 0, 1e-30, 255], rng.integers(-255, 256, 100000) / 2]).astype(np.float32)
xx = np.concatenate([rng.normal(size=200000), [0, 1, -1, 0, 0, 1, -1, 0], [1, 1, -1, -1, 1, -1, 1e-30, -255], rng.integers(-255, 256, 100000) / 2]).astype(np.float32)
at = np.zeros_like(yy)
lib.sf_atan2(len(yy), p(yy), p(xx), p(at))
assert same(at, S.atan2_deg(yy, xx)), "atan2 differs"

# ---- scalars of the dense part
for sigma in [S.level_sigmas(1.6, 3)[i] for i in range(6)] + [float(lib.sf_base_sigma(1.6)), 0.3, 2.0, 3.9]:
    taps = np.zeros(65, np.float32)
    n = lib.sf_kernel(sigma, p(taps))
    assert same(taps[:n], S.gaussian_kernel(sigma)), sigma
assert [lib.sf_level_sigma(1.6, 3, i) for i in range(1, 6)] == S.level_sigmas(1.6, 3)[1:]
assert [lib.sf_level_sigma(1.2, 4, i) for i in range(1, 7)] == S.level_sigmas(1.2, 4)[1:]
for m in list(range(1, 200)) + [1024, 1449, 1448, 21960, 21961, 46340]:
    assert lib.sf_n_octaves(m, m + 3) == S.n_octaves(m, m + 3), m

# ---- refinement, orientations and descriptors of two scenes, every candidate and every key point
REC = np.dtype([("layer", np.int32), ("r", np.int32), ("c", np.int32), ("octave", np.int32), ("x", np.float32), ("y", np.float32),
                ("size", np.float32), ("response", np.float32)])
n_cand = n_kp = 0
for scene, params in ((synth.sift_scene(160, 5), (0.02, 10.0)), (synth.sift_scene(128, 9)[:96], (0.04, 5.0))):
    info = {}
    kp, desc = S.detect_and_compute(scene, *params, info=info)
    tr = info["trace"]
    for o in range(info["stats"]["octaves"]):
        cand, ok_want = tr["cand"][o]
        if not len(cand):
            continue
        D = np.ascontiguousarray(np.stack(tr["dog"][o]))
        rows, cols = D.shape[1:]
        c32 = np.ascontiguousarray(cand, np.int32)
        ok = np.zeros(len(cand), np.int32)
        rec = np.zeros(len(cand), REC)
        lib.sf_refine_many(p(D), rows * cols, cols, rows, cols, o, len(cand), p(c32), 3, params[0], params[1], 1.6, p(ok), p(rec), None)
        assert np.array_equal(ok != 0, ok_want), "refinement outcome differs"
        fields, layer, r, c = tr["refined"][o]
        got = rec[ok != 0]
        assert np.array_equal(got["layer"], layer) and np.array_equal(got["r"], r) and np.array_equal(got["c"], c)
        for name in ("x", "y", "size", "response", "octave"):
            assert same(got[name], fields[name]), name
        n_cand += len(cand)
        # orientations: the angles of every refined key point, in order, are the octave's key points
        kp_o, desc_o = tr["kp"][o]
        angles, owner = [], []
        buf = np.zeros(36, np.float32)
        for k in range(len(got)):
            img = tr["gauss"][o][got["layer"][k]]
            cnt = lib.sf_orient(p(img), cols, rows, cols, int(got["r"][k]), int(got["c"][k]), float(got["size"][k]), o, p(buf))
            angles += list(buf[:cnt])
            owner += [k] * cnt
        assert same(np.array(angles, np.float32), kp_o["angle"]), "angles differ"
        assert same(fields["x"][owner], kp_o["x"]) and same(fields["octave"][owner], kp_o["octave"])
        inv = np.float32(1) / np.float32(1 << o)
        row = np.zeros(128, np.uint8)
        for k in range(len(kp_o)):
            q = kp_o[k]
            img = tr["gauss"][o][(int(q["octave"]) >> 8) & 255]
            lib.sf_describe(p(img), cols, rows, cols, float(q["x"] * inv), float(q["y"] * inv), float(q["angle"]), float(q["size"] * inv * np.float32(0.5)),
                            p(row))
            assert same(row, desc_o[k]), ("descriptor differs", o, k)
        n_kp += len(kp_o)
assert n_cand >= 200 and n_kp >= 200, (n_cand, n_kp)
print("candidates", n_cand, "key points", n_kp)
print("SIFT-HOST OK")
