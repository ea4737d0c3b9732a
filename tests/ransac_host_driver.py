"""Driver of tests/test_ransac_host.py part 2: csrc/ransac_math.hpp, compiled by g++ under the address and undefined-behaviour
sanitizers into the shared object named on the command line, against tests/ransac_restatement.py - bit for bit.  Runs in a
subprocess with libasan preloaded; prints RANSAC-HOST OK at the end."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ransac_restatement as R  # noqa: E402
from karios_amd import synth  # noqa: E402

lib = C.CDLL(sys.argv[1])
vp, ci, cd = C.c_void_p, C.c_int, C.c_double
lib.rs_rng.argtypes = [ci, vp]
lib.rs_subsets.argtypes, lib.rs_subsets.restype = [vp, ci, ci, vp], ci
lib.rs_check_subset.argtypes, lib.rs_check_subset.restype = [vp, vp], ci
lib.rs_update.argtypes, lib.rs_update.restype = [cd, cd, ci, ci], ci
lib.rs_dlt.argtypes, lib.rs_dlt.restype = [vp, vp, ci, vp], ci
lib.rs_dlt4_many.argtypes = [vp, vp, ci, vp, vp]
lib.rs_jacobi.argtypes, lib.rs_jacobi.restype = [vp, ci, vp, vp], ci
lib.rs_err.argtypes = [vp, vp, ci, vp]
lib.rs_count.argtypes, lib.rs_count.restype = [vp, vp, ci, cd], ci
lib.rs_replay.argtypes = [vp, vp, ci, ci, cd, ci, vp]
lib.rs_refine.argtypes, lib.rs_refine.restype = [vp, vp, ci, vp], ci


def p(a):
    return a.ctypes.data_as(vp)


def pairs_of(src, dst):
    return np.ascontiguousarray(np.concatenate([src, dst], 1), np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def c_subsets(src, dst, k):
    idx = np.zeros((k, 4), np.int32)
    return idx, lib.rs_subsets(p(pairs_of(src, dst)), len(src), k, p(idx))


# ---- the random stream and the subsets of the first 10 000 iterations on two scenes
out = np.zeros(8, np.uint32)
lib.rs_rng(8, p(out))
rng = R.RNG()
assert out.tolist() == [rng.next() for _ in range(8)]
scenes = [synth.homography_scene(400, 0.6, 0.3, 7), synth.homography_scene(3000, 0.2, 0.4, 7), synth.homography_scene(2000, 0.1, 0.5, 7)]
for src, dst, _planted, _H in scenes[:2]:
    its = R.Iterations(src, dst, 3.0)
    rng, want = R.RNG(), []
    for _ in range(10000):
        want.append(R.get_subset(src, dst, rng))
    idx, drawn = c_subsets(src, dst, 10000)
    assert drawn == 10000 and np.array_equal(idx, np.array(want)), "subsets differ"
# checkSubset on degenerate quadruples, getSubset's failure on a collinear scene
line = np.stack([np.arange(50, dtype=np.float32) * 3, np.arange(50, dtype=np.float32) * 7 + 1], 1)
idx, drawn = c_subsets(line, line, 5)
assert drawn == 0 and R.get_subset(line, line, R.RNG()) is None
rs = np.random.default_rng(3)
for _ in range(2000):
    a, b = rs.uniform(0, 100, (4, 2)).astype(np.float32), rs.uniform(0, 100, (4, 2)).astype(np.float32)
    if rs.random() < 0.3:
        a[3] = a[0] + (a[1] - a[0]) * np.float32(0.5)
    assert bool(lib.rs_check_subset(p(a), p(b))) == R.check_subset(a, b)
for w in (0.5, 0.3, 0.2, 0.17, 0.1, 0.0, 1.0, 0.999):
    for cap in (10000, 100, 1):
        assert lib.rs_update(0.999, 1 - w, 4, cap) == R.update_num_iters(0.999, 1 - w, 4, cap)

# ---- Jacobi, and the 4-point matrices of 2 000 subsets
A = rs.normal(size=(40, 9, 9))
A = A + A.transpose(0, 2, 1)
Wb, Vb, rotb = R.jacobi_batch(A)
for i in range(len(A)):
    W, V = np.zeros(9), np.zeros((9, 9))
    rot = lib.rs_jacobi(p(A[i].copy()), 9, p(W), p(V))
    w, v, it = R.jacobi(A[i])
    assert rot == it == rotb[i] and np.array_equal(bits(W), bits(w)) and np.array_equal(bits(V), bits(v))
    assert np.array_equal(bits(Wb[i]), bits(w)) and np.array_equal(bits(Vb[i]), bits(v)), "the batched restatement differs from the scalar one"
src, dst, _planted, _H = scenes[1]
idx, _ = c_subsets(src, dst, 2000)
dst2 = dst.copy()
dst2[idx[9]] = dst2[idx[9][0]]                                 # four pairs with one image point: the scale test refuses
H = np.zeros((2000, 9))
ok = np.zeros(2000, np.int32)
lib.rs_dlt4_many(p(pairs_of(src, dst2)), p(idx), 2000, p(H), p(ok))
Hr, okr = R.run_kernel4_batch(src[idx], dst2[idx])
assert not okr[9] and okr.sum() >= 1990 and np.array_equal(ok != 0, okr)
assert np.array_equal(bits(H.reshape(-1, 3, 3)), bits(Hr)), "4-point matrices differ"
for i in (0, 5, 77):
    one = R.run_kernel(src[idx[i]], dst2[idx[i]])
    assert np.array_equal(bits(one), bits(Hr[i]))

# ---- the scoring expression on 1e5 (hypothesis, point) pairs, a part of them at the threshold
thr = R.threshold_sq(3.0)
hyp = rs.integers(0, 2000, 100000)
hyp[okr[hyp] == 0] = 0
pt = rs.integers(0, len(src), 100000)
Hf = Hr[hyp].astype(np.float32).reshape(-1, 9)
x, y = src[pt, 0], src[pt, 1]
mx, my = dst[pt, 0].copy(), dst[pt, 1].copy()
edge = np.arange(100000) % 4 == 0
ww = np.float32(1) / (Hf[:, 6] * x + Hf[:, 7] * y + np.float32(1))
px, py = (Hf[:, 0] * x + Hf[:, 1] * y + Hf[:, 2]) * ww, (Hf[:, 3] * x + Hf[:, 4] * y + Hf[:, 5]) * ww
t = (px - np.float32(3))[edge]
step = rs.integers(-1, 2, t.size)
mx[edge] = np.where(step < 0, np.nextafter(t, np.float32(-np.inf)), np.where(step > 0, np.nextafter(t, np.float32(np.inf)), t))
my[edge] = py[edge]
quad = np.ascontiguousarray(np.stack([x, y, mx, my], 1), np.float32)
err = np.zeros(100000, np.float32)
lib.rs_err(p(np.ascontiguousarray(Hf)), p(quad), 100000, p(err))
want = np.array([R.reproj_err(Hr[h], quad[i:i + 1, :2], quad[i:i + 1, 2:])[0] for i, h in enumerate(hyp[:3000])])
assert np.array_equal(err[:3000].view(np.uint32), want.view(np.uint32))
hs = np.unique(hyp)
for h in hs[:200]:
    sel = np.nonzero(hyp == h)[0]
    assert np.array_equal(err[sel].view(np.uint32), R.reproj_err(Hr[h], quad[sel, :2], quad[sel, 2:]).view(np.uint32))
e = err[edge]
near = np.abs(e.view(np.int32).astype(np.int64) - np.float32(thr).view(np.int32)) <= 64
assert (e == thr).sum() > 10 and (near & (e < thr)).sum() > 10 and (near & (e > thr)).sum() > 10, "no pairs at the threshold"

# ---- the replay, the n-point DLT and the LM result on three scenes
for (src, dst, _planted, _H), max_iters in zip(scenes, (10000, 10000, 3000)):
    info = {}
    Hw, maskw = R.find_homography(src, dst, 3.0, max_iters, 0.999, info=info)
    its = info["its"]
    k = len(its.idx)
    idx, drawn = c_subsets(src, dst, k)
    assert drawn == k and np.array_equal(idx, its.idx)
    pr = pairs_of(src, dst)
    H4, ok = np.zeros((k, 9)), np.zeros(k, np.int32)
    lib.rs_dlt4_many(p(pr), p(idx), k, p(H4), p(ok))
    assert np.array_equal(bits(H4.reshape(-1, 3, 3)), bits(its.H)) and np.array_equal(ok != 0, its.valid)
    counts = np.array([lib.rs_count(p(pr), p(np.ascontiguousarray(H4[i])), len(src), 3.0) if ok[i] else 0 for i in range(k)], np.int32)
    assert np.array_equal(counts, its.count)
    out = np.zeros(4, np.int32)
    lib.rs_replay(p(counts), p(ok), k, len(src), 0.999, max_iters, p(out))
    assert out.tolist()[1:] == [info["best_count"], info["best_iter"], info["ran"]], (out, info)
    keep = maskw[:, 0] != 0
    assert keep.sum() == info["best_count"]
    Hc = np.ascontiguousarray(H4[info["best_iter"]])
    lm = lib.rs_refine(p(np.ascontiguousarray(src[keep])), p(np.ascontiguousarray(dst[keep])), int(keep.sum()), p(Hc))
    assert lm == info["lm_iters"] and np.array_equal(bits(Hc.reshape(3, 3)), bits(Hw)), (lm, info["lm_iters"], Hc, Hw)
    # the n-point solve alone
    Hn = np.zeros(9)
    assert lib.rs_dlt(p(np.ascontiguousarray(src[keep])), p(np.ascontiguousarray(dst[keep])), int(keep.sum()), p(Hn)) == 1
    assert np.array_equal(bits(Hn.reshape(3, 3)), bits(R.run_kernel(src[keep], dst[keep])))
print("RANSAC-HOST OK")
