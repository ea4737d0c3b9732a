"""Second driver of the host-only sanitizer build (run by tests/test_host_asan.py in a subprocess with libasan preloaded): the
entry points of the align step - api_align.hip, api_prep.hip, api_match.hip, api_ransac.hip, api_sift.hip.

Loads tests/hoststub/_build/libkarios_host_asan.so through the product's ctypes signatures (karios_amd._lib.SIGNATURES), as
driver.py does.  The RANSAC and SIFT stand-ins are ransac_math.hpp / sift_math.hpp (stub_kernels_align.cpp), so
km_find_homography_ransac* and km_sift_detect_and_compute* run end to end on the CPU and are compared with
tests/ransac_restatement.py / tests/sift_restatement.py bit for bit: batch loop, replay and refinement of RANSAC, both repeat paths,
the grown lists and the capacity protocol of SIFT.  Prep, match and align have do-little stand-ins: what is walked there is the host
side - argument checks, slot layouts, the grouping of quantiles, ecc_step / lu_inv_f32, every copy in and out.
Prints 'HOST-ASAN ALIGN OK' at the end; any sanitizer report aborts the process.
"""
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ransac_restatement as R  # noqa: E402
import sift_restatement as S  # noqa: E402
from sift_scenes import scene  # noqa: E402

from karios_amd import synth  # noqa: E402
from karios_amd._lib import _DTYPES, SIGNATURES  # noqa: E402  (signatures only: the product library is NOT loaded)
from karios_amd.ops import sift_capacity_estimate  # noqa: E402

lib = C.CDLL(os.path.join(ROOT, "tests", "hoststub", "_build", "libkarios_host_asan.so"))
for name, (res, args) in SIGNATURES.items():
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = res, args
lib.stub_counters.argtypes = [C.POINTER(C.c_long)]
lib.stub_fail_malloc_after.argtypes = [C.c_int]

KM_E_ARG, KM_E_NOMEM, KM_E_UNSUPPORTED, KM_E_NO_CONVERGENCE, KM_E_CAPACITY = -1, -3, -4, -7, -8
ECC_CONVERGED, ECC_SKIPPED, ECC_NO_CONVERGENCE = 0, 1, 2
U8, U16, I16, F32 = (_DTYPES[np.dtype(t)] for t in ("uint8", "uint16", "int16", "float32"))
# quantiles of one selection, from the header: the cases below are "exactly one group" and "two groups" whatever its value
KP_MAX_Q = int(re.search(r"^#define KP_MAX_Q (\d+)", open(os.path.join(ROOT, "karios_amd", "csrc", "k_prep.hpp")).read(), re.M).group(1))


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def ok(rc, what):
    assert rc == 0, f"{what}: status {rc}: {lib.km_last_error(ctx).decode()}"


def err(rc, what, code=KM_E_ARG, text=None):
    msg = lib.km_last_error(ctx).decode()
    assert rc == code and (text is None or text in msg), f"{what}: expected {code} ({text}), got {rc}: {msg}"


def to_dev(a):
    a = np.ascontiguousarray(a)
    d = C.c_void_p()
    ok(lib.km_dev_alloc(ctx, max(a.nbytes, 1), C.byref(d)), "dev_alloc")
    if a.nbytes:
        ok(lib.km_h2d(ctx, d, P(a), a.nbytes), "h2d")
    return d


def from_dev(d, shape, dtype, free=True):
    out = np.zeros(shape, dtype)
    if out.nbytes:
        ok(lib.km_d2h(ctx, P(out), d, out.nbytes), "d2h")
    if free:
        ok(lib.km_dev_free(ctx, d), "dev_free")
    return out


def nomem(call, what):
    """One allocation failure inside `call`: KM_E_NOMEM comes back, and the same call works afterwards."""
    lib.stub_fail_malloc_after(0)
    err(call(), what + " under allocation failure", KM_E_NOMEM, "hipMalloc")
    ok(call(), what + " after the failure")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def strided(a, pad, fill=0):
    """`a` as a view of a wider array: (view, row stride in elements)"""
    wide = np.full((a.shape[0], a.shape[1] + pad), fill, a.dtype)
    wide[:, :a.shape[1]] = a
    return wide[:, :a.shape[1]], wide.shape[1]


rng = np.random.default_rng(5)
ctx = C.c_void_p()
ok(lib.km_ctx_create(0, C.byref(ctx)), "ctx_create")

# ================================================================== RANSAC: bit for bit against the restatement
def ransac(src, dst, n, dev=False, stride=2, max_iters=10000, iterations=False):
    H, found, stats = np.full(9, 7.0), C.c_int(-1), (C.c_int64 * 8)()
    mask = np.full(max(n, 1), 9, np.uint8)
    counts, valid = (np.full(max_iters, -5, np.int32), np.full(max_iters, -5, np.int32)) if iterations else (None, None)
    a, b = (np.zeros((max(n, 1), stride), np.float32) for _ in range(2))
    a[:n, :2], b[:n, :2] = src[:n], dst[:n]
    tail = (n, 3.0, max_iters, 0.999, H.ctypes.data_as(C.POINTER(C.c_double)))
    if dev:
        da, db, dm = to_dev(a), to_dev(b), to_dev(mask)
        rc = lib.km_find_homography_ransac_dev(ctx, da, stride, db, stride, *tail, dm, C.byref(found), stats, P(counts), P(valid))
        mask = from_dev(dm, mask.shape, np.uint8)
        for d in (da, db):
            ok(lib.km_dev_free(ctx, d), "dev_free")
    else:
        rc = lib.km_find_homography_ransac(ctx, P(a), stride, P(b), stride, *tail, P(mask), C.byref(found), stats, P(counts), P(valid))
    return rc, H.reshape(3, 3), mask[:n].reshape(n, 1), found.value, [int(v) for v in stats], counts, valid


src, dst, _planted, _H = synth.homography_scene(400, 0.6, 0.3, 7)
nomem(lambda: ransac(src, dst, 400)[0], "find_homography_ransac")
for (n, inl, noise, seed), (want_ran, want_inliers) in (((400, 0.6, 0.3, 7), (50, 240)), ((300, 0.3, 0.4, 3), (849, 90)), ((64, 0.5, 0.3, 1), (107, 32))):
    src, dst, _planted, _H = synth.homography_scene(n, inl, noise, seed)
    info = {}
    Hw, maskw = R.find_homography(src, dst, 3.0, 10000, 0.999, info=info)
    assert (info["ran"], info["best_count"], int(maskw.sum())) == (want_ran, want_inliers, want_inliers), info
    for first_batch in (16, 0):                                   # 0: the default schedule
        ok(lib.km_set_option(ctx, b"ransac_first_batch", first_batch), "ransac_first_batch")
        for dev, stride in ((False, 3), (True, 2), (True, 5)):
            rc, H, mask, found, st, counts, valid = ransac(src, dst, n, dev, stride, iterations=True)
            ok(rc, "find_homography_ransac")
            what = f"scene {n}/{seed}, first batch {first_batch}, dev {dev}"
            assert found == 1 and np.array_equal(bits(H), bits(Hw)) and np.array_equal(mask, maskw), what
            assert st[0] == info["ran"] and st[2] == info["best_iter"] and st[3] == info["best_count"] and st[4] == info["lm_iters"], (what, st, info)
            assert st[5] == (first_batch or st[5]) and st[0] <= st[1] <= max(st[5], 2 * st[0]), (what, st)
            its = info["its"]
            assert np.array_equal(counts[:st[0]], its.count[:st[0]]) and np.array_equal(valid[:st[0]] != 0, its.valid[:st[0]]), what
            assert (counts[st[1]:] == -5).all() and (valid[st[1]:] == -5).all() and len(counts) == 10000, what
# four pairs: one solve, a mask of ones; three: an error
Hw, maskw = R.find_homography(src[:4], dst[:4])
for dev in (False, True):
    rc, H, mask, found, st, _c, _v = ransac(src, dst, 4, dev)
    ok(rc, "four pairs")
    assert found == 1 and np.array_equal(bits(H), bits(Hw)) and (mask == 1).all()
    err(ransac(src, dst, 3, dev)[0], "three pairs", KM_E_ARG, "at least 4")
bad = dst.copy()
bad[17, 1] = np.nan
err(ransac(src, bad, 64)[0], "NaN coordinate", KM_E_ARG, "dst point 17")
err(ransac(src, bad, 64, True)[0], "NaN coordinate (dev)", KM_E_ARG, "dst point 17 has a coordinate that is not finite (y)")
line = np.stack([np.arange(50, dtype=np.float32) * 3, np.arange(50, dtype=np.float32) * 7 + 1], 1)      # getSubset never finds a subset
for dev in (False, True):
    rc, H, mask, found, st, _c, _v = ransac(line, line, 50, dev)
    ok(rc, "collinear scene")
    assert found == 0 and not mask.any() and not H.any() and st[0] == 0
H9, found = np.zeros(9), C.c_int()
Hp = H9.ctypes.data_as(C.POINTER(C.c_double))
m64 = np.zeros(64, np.uint8)
err(lib.km_find_homography_ransac(ctx, None, 2, P(dst), 2, 64, 3.0, 100, 0.999, Hp, P(m64), C.byref(found), None, None, None), "null src")
err(lib.km_find_homography_ransac(ctx, P(src), 2, P(dst), 2, 64, 3.0, 100, 0.999, Hp, None, C.byref(found), None, None, None), "null mask")
err(lib.km_find_homography_ransac(ctx, P(src), 1, P(dst), 2, 64, 3.0, 100, 0.999, Hp, P(m64), C.byref(found), None, None, None), "row stride 1")
err(lib.km_find_homography_ransac(ctx, P(src), 2, P(dst), 2, 64, 3.0, 100, 1.0, Hp, P(m64), C.byref(found), None, None, None), "confidence 1")
err(lib.km_find_homography_ransac_dev(ctx, P(src), 2, P(dst), 2, 64, 3.0, (1 << 24) + 1, 0.5, Hp, P(m64), C.byref(found), None, None, None), "max_iters")

# ================================================================== SIFT: bit for bit against the restatement
def sift(img, stride, cap, ddt=np.uint8, dev=False, desc_stride=128, nfeatures=0, null_out=False):
    H, W = img.shape
    room = max(cap, 1)
    fields, desc = np.full((6, room), -3, np.float32), np.full((room, desc_stride), 201, ddt)
    count, stats = C.c_int(-1), (C.c_int64 * 160)()
    head = (H, W, stride, nfeatures, 3, 0.02, 10.0, 1.6, cap)
    tail = (_DTYPES[np.dtype(ddt)], desc_stride, C.byref(count), stats)
    if null_out:
        fn, image = (lib.km_sift_detect_and_compute_dev, to_dev(np.ascontiguousarray(img))) if dev else (lib.km_sift_detect_and_compute, P(img))
        rc = fn(ctx, image, H, W, W if dev else stride, *head[3:], *([None] * 7), *tail)
        if dev:
            ok(lib.km_dev_free(ctx, image), "dev_free")
    elif dev:
        d_img, d_f, d_desc = to_dev(np.ascontiguousarray(img)), to_dev(fields), to_dev(desc)
        fp = [C.c_void_p(d_f.value + 4 * room * k) for k in range(6)]
        rc = lib.km_sift_detect_and_compute_dev(ctx, d_img, H, W, W, *head[3:], *fp, d_desc, *tail)
        fields, desc = from_dev(d_f, fields.shape, np.float32), from_dev(d_desc, desc.shape, ddt)
        ok(lib.km_dev_free(ctx, d_img), "dev_free")
    else:
        rc = lib.km_sift_detect_and_compute(ctx, P(img), *head, *[P(fields[k]) for k in range(6)], P(desc), *tail)
    return rc, count.value, fields, desc, stats


def sift_same(got, want, n_rows, what):
    """count, the six fields, the descriptors and the stats' counts of a call against the restatement's (kp, desc, stats)"""
    rc, count, fields, desc, stats = got
    kp, wdesc, wstats = want
    assert count == len(kp), (what, count, len(kp))
    for k, name in enumerate(S.KP_DTYPE.names):
        assert np.array_equal(fields[k, :n_rows].view(np.uint32), np.ascontiguousarray(kp[name][:n_rows]).view(np.uint32)), (what, name)
    assert (fields[:, n_rows:] == -3).all() and (desc[n_rows:] == 201).all() and (desc[:, 128:] == 201).all(), what + ": written beyond the rows"
    if n_rows:
        assert np.array_equal(desc[:n_rows, :128], wdesc[:n_rows].astype(desc.dtype)), what + ": descriptors"
    n = wstats["octaves"]
    assert stats[0] == n and (stats[1], stats[2]) == (wstats["before_dedup"], wstats["after_dedup"]), what
    per = [int(v) for v in stats[4:4 + 3 * n]]
    assert (per[0::3], per[1::3], per[2::3]) == (wstats["candidates"], wstats["refined"], wstats["keypoints"]), what


def restated(img):
    info = {}
    kp, desc = S.detect_and_compute(img, info=info)
    return kp, desc, info["stats"]


# grow_keep's copy: on a context whose lists are still small, the second octave of the 128 x 128 scene needs longer key-point and
# descriptor lists than the first left behind (km_ws gives a slot 1/16 + 256 bytes of head-room), so both are retired and their live
# prefix, the first octave's records (24 bytes a key point, 128 a descriptor), is copied over.  Each form on a context of its own: a list that has grown stays grown.
multi = synth.sift_scene(128, 9)
want = restated(multi)
ref0, ref1, kp0, kp1 = *want[2]["refined"][:2], *want[2]["keypoints"][:2]
assert kp0 and kp1 and kp1 <= 2 * ref1 + 64 and (kp0 + 2 * ref1 + 64) * 24 > (2 * ref0 + 64) * 24 * 17 // 16 + 256 and (kp0 + kp1) * 128 > kp0 * 128 * 17 // 16 + 256, want[2]
shared_ctx = ctx
for dev in (False, True):
    ctx = C.c_void_p()
    ok(lib.km_ctx_create(0, C.byref(ctx)), "ctx_create")
    got = sift(multi, 128, len(want[0]), np.uint8, dev)
    ok(got[0], "128 x 128 on a fresh context")
    sift_same(got, want, len(want[0]), f"128 x 128 on a fresh context, dev {dev}")
    ok(lib.km_ctx_destroy(ctx), "ctx_destroy")
ctx = shared_ctx

# the 90 x 90 dot lattice, with an allocation failure deep inside its first call: both lists overflow and the wrapper's estimate too
lattice = scene("lattice", 90, 90)
want = restated(lattice)
n = len(want[0])
estimate = sift_capacity_estimate(90, 90)
assert want[2]["candidates"][0] > max(256, 180 * 180 * 3 // 256) and want[2]["keypoints"][0] > 2 * want[2]["refined"][0] + 64 and n > estimate
assert (want[2]["candidates"][0], n, estimate) == (588, 783, 762)
lib.stub_fail_malloc_after(9)
err(sift(lattice, 90, estimate)[0], "sift under allocation failure", KM_E_NOMEM, "hipMalloc")
for dev in (False, True):
    for ddt in (np.uint8, np.float32):
        got = sift(lattice, 90, estimate, ddt, dev)
        err(got[0], "lattice at the estimate", KM_E_CAPACITY, f"{n} key points, room for {estimate}")
        assert got[4][136] >= 1 and got[4][137] >= 1, ("regrows", got[4][136], got[4][137])
        sift_same(got, want, estimate, f"lattice at the estimate, dev {dev}")
        got = sift(lattice, 90, got[1], ddt, dev, desc_stride=136 if dev else 128)
        ok(got[0], "lattice at the true count")
        assert got[4][136] >= 1 and got[4][137] >= 1
        sift_same(got, want, n, f"lattice at the true count, dev {dev}")
textured, stride = strided(scene("textured", 97, 131), 37, 255)
for what, img, stride, n_want, before in (("128 x 128", synth.sift_scene(128, 9), 128, 64, 65), ("97 x 131 of a wider array", textured, stride, 60, None),
                                          ("flat 9 x 9", scene("flat", 9, 9), 9, 0, None)):
    want = restated(img)
    n = len(want[0])
    assert n == n_want and (before is None or want[2]["before_dedup"] == before), (what, n, want[2])
    for dev in (False, True):
        got = sift(img, stride, n + 5, np.uint8, dev)
        ok(got[0], what)
        sift_same(got, want, n, f"{what}, dev {dev}")
        got = sift(img, stride, n // 3, np.float32, dev)
        assert got[0] == (KM_E_CAPACITY if n else 0), (what, got[0])
        sift_same(got, want, n // 3, f"{what}, a third of the room, dev {dev}")
        got = sift(img, stride, 0, np.uint8, dev, null_out=True)
        assert got[0] == (KM_E_CAPACITY if n else 0) and got[1] == n, (what, got[:2])
img = synth.sift_scene(128, 9)
err(sift(img, 128, 10, nfeatures=100)[0], "nfeatures", KM_E_UNSUPPORTED, "nfeatures = 100")
err(sift(img, 128, 10, null_out=True)[0], "null outputs with room", KM_E_ARG)
err(sift(img, 100, 10)[0], "row stride below the width", KM_E_ARG)
err(sift(img, 128, 10, desc_stride=130)[0], "host form with a descriptor stride", KM_E_ARG, "dense descriptor rows")
err(sift(img, 128, -1)[0], "negative room", KM_E_ARG)
err(lib.km_sift_detect_and_compute(ctx, None, 128, 128, 128, 0, 3, 0.02, 10.0, 1.6, 0, *([None] * 7), U8, 128, C.byref(C.c_int()), None), "null image", KM_E_ARG)

# ================================================================== match
def knn(q, sq, t, st, k, dev=False):
    n_q, n_t = len(q), len(t)
    idx, dist = np.full((max(n_q, 1), k), -9, np.int32), np.full((max(n_q, 1), k), -9, np.float32)
    if dev:
        dq, dt, di, dd = to_dev(q.base if q.base is not None else q), to_dev(t.base if t.base is not None else t), to_dev(idx), to_dev(dist)
        rc = lib.km_knn_match_u8_dev(ctx, dq, n_q, sq, dt, n_t, st, 128, k, di, dd)
        idx, dist = from_dev(di, idx.shape, np.int32), from_dev(dd, dist.shape, np.float32)
        for d in (dq, dt):
            ok(lib.km_dev_free(ctx, d), "dev_free")
    else:
        rc = lib.km_knn_match_u8(ctx, P(q), n_q, sq, P(t), n_t, st, 128, k, P(idx), P(dist))
    return rc, idx, dist


def lowe(mon, sm, ref, sr, dtype, cap, dev=False, ratio=0.75):
    qi, ti, dist, counts = np.full(max(cap, 1), -9, np.int32), np.full(max(cap, 1), -9, np.int32), np.full(max(cap, 1), -9, np.float32), np.zeros(3, np.int32)
    cp = counts.ctypes.data_as(C.POINTER(C.c_int))
    if dev:
        ds = [to_dev(a.base if a.base is not None else a) for a in (mon, ref)] + [to_dev(a) for a in (qi, ti, dist)]
        rc = lib.km_match_lowe_mutual_dev(ctx, ds[0], len(mon), sm, ds[1], len(ref), sr, dtype, 128, ratio, cap, ds[2], ds[3], ds[4], cp)
        qi, ti, dist = from_dev(ds[2], qi.shape, np.int32), from_dev(ds[3], ti.shape, np.int32), from_dev(ds[4], dist.shape, np.float32)
        for d in ds[:2]:
            ok(lib.km_dev_free(ctx, d), "dev_free")
    else:
        rc = lib.km_match_lowe_mutual(ctx, P(mon), len(mon), sm, P(ref), len(ref), sr, dtype, 128, ratio, cap, P(qi), P(ti), P(dist), cp)
    return rc, qi, ti, dist, counts


ref_d = rng.integers(0, 256, (300, 128), dtype=np.uint8)
mon_d = ref_d[rng.permutation(300)[:170]].copy()
mon_d[:, :7] ^= 1                                                  # every mon row has its ref row as a close first neighbour
mon_v, sm = strided(mon_d, 32)
ref_v, sr = strided(ref_d, 7)
nomem(lambda: knn(mon_v, sm, ref_v, sr, 2)[0], "knn_match_u8")
d2 = ((mon_d.astype(np.int64)[:, None, :] - ref_d.astype(np.int64)[None, :, :]) ** 2).sum(2)
for dev in (False, True):
    for k in (1, 2):
        rc, idx, dist = knn(mon_v, sm, ref_v, sr, k, dev)
        ok(rc, "knn_match_u8")
        assert np.array_equal(idx[:, 0], d2.argmin(1)) and np.array_equal(dist[:, 0], np.sqrt(d2.min(1).astype(np.float32))), (k, dev)
    ok(knn(mon_v[:0], sm, ref_v, sr, 2, dev)[0], "knn: empty query set")
rc, idx, dist = knn(mon_v, sm, ref_v[:0], sr, 2)
ok(rc, "knn: empty train set")
assert (idx == -1).all() and np.isposinf(dist).all()
err(knn(mon_v, sm, ref_v, sr, 3)[0], "knn k = 3")
err(knn(mon_v, 100, ref_v, sr, 2)[0], "knn row stride")
err(lib.km_knn_match_u8(ctx, None, 5, 128, P(ref_d), 300, 128, 128, 1, P(idx), P(dist)), "knn null query")
err(lib.km_knn_match_u8(ctx, P(mon_d), 5, 128, P(ref_d), 300, 128, 64, 1, P(idx), P(dist)), "knn dim", KM_E_UNSUPPORTED)
for dtype, cast in ((U8, np.uint8), (F32, np.float32)):
    mon_c, _ = strided(mon_d.astype(cast), 32)
    ref_c, _ = strided(ref_d.astype(cast), 7)
    for dev in (False, True):
        rc, qi, ti, dist, counts = lowe(mon_c, sm, ref_c, sr, dtype, 170, dev)
        ok(rc, "match_lowe_mutual")
        m = counts[2]
        assert counts[0] == 170 and m == counts[1] == 170 and np.array_equal(qi[:m], np.arange(170)) and np.array_equal(ti[:m], d2.argmin(1)), counts
        rc, qi, ti, dist, counts = lowe(mon_c, sm, ref_c, sr, dtype, 50, dev)
        err(rc, "match_lowe_mutual with little room", KM_E_ARG, "170 mutual matches, room for 50")
        assert counts[2] == 170 and (qi[:50] == np.arange(50)).all() if dev else counts[2] == 170
        rc, _q, _t, _d, counts = lowe(mon_c[:0], sm, ref_c, sr, dtype, 10, dev)
        assert rc == 0 and counts.tolist() == [0, 0, 0]
        rc, _q, _t, _d, counts = lowe(mon_c, sm, ref_c[:0], sr, dtype, 10, dev)
        assert rc == 0 and counts.tolist() == [170, 0, 0]
mon_f, _ = strided(mon_d.astype(np.float32), 32)
ref_f, _ = strided(ref_d.astype(np.float32), 7)
ref_f[5, 9] = 0.5
ref_f[200, 3] = 300.0
for dev in (False, True):
    err(lowe(mon_f, sm, ref_f, sr, F32, 170, dev)[0], "descriptors that are no bytes", KM_E_ARG, "ref descriptors hold 2 elements that are no integers in 0 .. 255, the first at (row 5, column 9)")
nomem(lambda: lowe(np.tile(mon_d, (3, 1)), 128, ref_d, 128, U8, 600)[0], "match_lowe_mutual")
err(lowe(mon_v, sm, ref_v, sr, U16, 170)[0], "match dtype")
err(lowe(mon_v, sm, ref_v, sr, U8, 170, ratio=float("nan"))[0], "match ratio")
err(lowe(mon_v, sm, ref_v, sr, U8, -1)[0], "match negative room")
err(lib.km_match_lowe_mutual(ctx, P(mon_d), 170, 128, P(ref_d), 300, 128, U8, 128, 0.75, 10, None, None, None, None), "match null outputs")

# ================================================================== prep
def order_stats(img, stride, dtype, q, dev=False, exclude=0):
    q = np.asarray(q, np.float64)
    n, v0, v1, vi = C.c_int64(-1), np.full(max(len(q), 1), -7.0), np.full(max(len(q), 1), -7.0), np.full(max(len(q), 1), -7.0)
    pd = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in (q if len(q) else np.zeros(1), v0, v1, vi)]
    src = to_dev(img.base) if dev else P(img)
    fn = lib.km_order_statistics_dev if dev else lib.km_order_statistics
    rc = fn(ctx, src, dtype, img.shape[0], img.shape[1], stride, exclude, len(q), pd[0], C.byref(n), pd[1], pd[2], pd[3])
    if dev:
        ok(lib.km_dev_free(ctx, src), "dev_free")
    return rc, n.value, v0, v1, vi


big = rng.integers(0, 255, (260, 301)).astype(np.float32)
nomem(lambda: order_stats(*strided(big, 11), F32, [0.5])[0], "order_statistics")
for dtype, cast in ((U8, np.uint8), (U16, np.uint16), (I16, np.int16), (F32, np.float32)):
    a = (rng.integers(0, 250, (61, 83)) - (100 if cast in (np.int16, np.float32) else 0)).astype(cast)
    view, stride = strided(a, 9)
    flat = np.sort(a.reshape(-1).astype(np.float64))
    for n_q in (1, KP_MAX_Q, KP_MAX_Q + 3):                        # the last: two groups through the select
        q = np.linspace(0.02, 1.0, n_q)
        for dev in (False, True):
            rc, n, v0, v1, vi = order_stats(view, stride, dtype, q, dev)
            ok(rc, "order_statistics")
            lo = (q * (a.size - 1)).astype(np.int64)
            assert n == a.size and np.array_equal(vi, q * (a.size - 1)) and np.array_equal(v0, flat[lo]) and np.array_equal(v1, flat[np.minimum(lo + 1, a.size - 1)]), (dtype, n_q, dev)
view, stride = strided(np.full((20, 30), np.nan, np.float32), 4)
for dev in (False, True):
    rc, n, v0, v1, vi = order_stats(view, stride, F32, np.linspace(0, 1, KP_MAX_Q + 3), dev)
    assert rc == 0 and n == 0 and (v0 == -7).all() and (v1 == -7).all() and (vi == -7).all(), "no value kept: the outputs stay as they were"
    rc, n, v0, v1, vi = order_stats(view, stride, F32, [], dev, exclude=1)
    assert rc == 0 and n == 0
view, stride = strided(a, 9)
err(order_stats(view, stride, F32, [0.1, 1.5])[0], "quantile outside [0, 1]", KM_E_ARG, "quantile 1 = 1.5")
err(order_stats(view, stride, 4, [0.5])[0], "order_statistics dtype")
err(order_stats(view, stride, F32, [0.5], exclude=2)[0], "order_statistics exclude")
err(order_stats(view, 10, F32, [0.5])[0], "order_statistics stride")
err(lib.km_order_statistics(ctx, None, F32, 5, 5, 5, 0, 0, None, C.byref(C.c_int64()), None, None, None), "order_statistics null image")
err(lib.km_order_statistics(ctx, P(a), F32, 5, 5, 5, 0, 0, None, None, None, None, None), "order_statistics null count")
for dtype, cast in ((U8, np.uint8), (U16, np.uint16), (I16, np.int16), (F32, np.float32)):
    a = rng.integers(0, 250, (61, 83)).astype(cast)
    view, stride = strided(a, 9)
    want = np.clip((a.astype(np.float64) - 20.0) / 180.0 * 255.0, 0, 255).astype(np.uint8)
    out = np.zeros((61, 83), np.uint8)
    ok(lib.km_stretch_percentile_u8(ctx, P(view), dtype, 61, 83, stride, 20.0, 200.0, P(out)), "stretch_percentile_u8")
    assert np.array_equal(out, want), dtype
    d_in, d_out = to_dev(view.base), to_dev(np.full((61, 100), 77, np.uint8))
    ok(lib.km_stretch_percentile_u8_dev(ctx, d_in, dtype, 61, 83, stride, 20.0, 200.0, d_out, 100), "stretch_percentile_u8_dev")
    out = from_dev(d_out, (61, 100), np.uint8)
    assert np.array_equal(out[:, :83], want) and (out[:, 83:] == 77).all(), dtype
    ok(lib.km_dev_free(ctx, d_in), "dev_free")
err(lib.km_stretch_percentile_u8(ctx, P(view), 4, 61, 83, stride, 20.0, 200.0, P(out)), "stretch dtype")
err(lib.km_stretch_percentile_u8(ctx, P(view), F32, 61, 83, stride, 20.0, 200.0, None), "stretch null output")
a = rng.integers(0, 256, (61, 83), dtype=np.uint8)
view, stride = strided(a, 9)
out = np.zeros((61, 83), np.uint8)
ok(lib.km_clahe(ctx, P(view), 61, 83, stride, 2.0, 8, 8, P(out)), "clahe")
assert np.array_equal(out, a)                                      # (the stand-in's LUTs are the identity)
d_in, d_out = to_dev(view.base), to_dev(np.full((61, 100), 77, np.uint8))
ok(lib.km_clahe_dev(ctx, d_in, 61, 83, stride, 2.0, 8, 8, d_out, 100), "clahe_dev")
got = from_dev(d_out, (61, 100), np.uint8)
assert np.array_equal(got[:, :83], a) and (got[:, 83:] == 77).all()
# (kp_clahe_geometry is host code of k_prep.hip, outside this build: the message is the stand-in's, the case walks km_clahe's way out)
err(lib.km_clahe(ctx, P(view), 61, 83, stride, 2.0, 0, 8, P(out)), "clahe tile grid", KM_E_ARG, "tile grid 0 x 8")
err(lib.km_clahe(ctx, P(view), 61, 83, stride, float("nan"), 8, 8, P(out)), "clahe clip limit")
err(lib.km_clahe_dev(ctx, d_in, 61, 83, stride, 2.0, 8, 8, None, 100), "clahe null output")
err(lib.km_clahe_dev(ctx, d_in, 61, 83, stride, 2.0, 8, 8, d_in, 80), "clahe output stride")
ok(lib.km_dev_free(ctx, d_in), "dev_free")

# ================================================================== align
ident = np.eye(3).reshape(-1)
Mp = ident.ctypes.data_as(C.POINTER(C.c_double))
a = rng.integers(1, 256, (300, 400), dtype=np.uint8)
nomem(lambda: lib.km_warp_perspective(ctx, P(a), U8, 300, 400, 400, P(np.zeros((300, 400), np.uint8)), 300, 400, 1, 0, 0.0, Mp), "warp_perspective")
for dtype, cast in ((U8, np.uint8), (F32, np.float32)):
    a = rng.integers(1, 256, (70, 90)).astype(cast)
    view, stride = strided(a, 6)
    for linear in (1, 0):
        for inverse in (0, 1):
            out = np.zeros((50, 64), cast)
            ok(lib.km_warp_perspective(ctx, P(view), dtype, 70, 90, stride, P(out), 50, 64, linear, inverse, 0.0, Mp), "warp_perspective")
            assert np.array_equal(out, a[:50, :64])                # (the stand-in copies, whatever the map)
            d_in, d_out = to_dev(view.base), to_dev(np.full((50, 80), 77, cast))
            ok(lib.km_warp_perspective_dev(ctx, d_in, dtype, 70, 90, stride, d_out, 50, 64, 80, linear, inverse, 0.0, Mp), "warp_perspective_dev")
            got = from_dev(d_out, (50, 80), cast)
            assert np.array_equal(got[:, :64], a[:50, :64]) and (got[:, 64:] == 77).all()
            ok(lib.km_dev_free(ctx, d_in), "dev_free")
err(lib.km_warp_perspective(ctx, P(view), U16, 70, 90, stride, P(out), 50, 64, 1, 0, 0.0, Mp), "warp dtype", KM_E_UNSUPPORTED)
err(lib.km_warp_perspective(ctx, P(view), F32, 70, 90, stride, P(out), 50, 64, 2, 0, 0.0, Mp), "warp interpolation", KM_E_UNSUPPORTED)
err(lib.km_warp_perspective(ctx, P(view), F32, 70, 90, stride, P(out), 50, 64, 1, 0, 0.0, None), "warp null matrix")
err(lib.km_warp_perspective(ctx, None, F32, 70, 90, stride, P(out), 50, 64, 1, 0, 0.0, Mp), "warp null source")
err(lib.km_warp_perspective(ctx, P(view), F32, 70, 90, 80, P(out), 50, 64, 1, 0, 0.0, Mp), "warp source stride")
a = rng.integers(0, 256, (70, 90), dtype=np.uint8)
view, stride = strided(a, 6)
out = np.zeros((70, 90), np.float32)
ok(lib.km_sobel_magnitude(ctx, P(view), 70, 90, stride, P(out)), "sobel_magnitude")
assert np.array_equal(out, a.astype(np.float32))
d_in, d_out = to_dev(view.base), to_dev(out * 0)
ok(lib.km_sobel_magnitude_dev(ctx, d_in, 70, 90, stride, d_out), "sobel_magnitude_dev")
assert np.array_equal(from_dev(d_out, (70, 90), np.float32), a.astype(np.float32))
err(lib.km_sobel_magnitude_dev(ctx, d_in, 70, 90, stride, None), "sobel null output")
err(lib.km_sobel_magnitude(ctx, P(view), 70, 0, stride, P(out)), "sobel empty image")
ok(lib.km_dev_free(ctx, d_in), "dev_free")


def ecc(tmpl, inp, dtype, max_iter, eps, mask=None, dev=False, gauss=5):
    """The stand-in gives the sums of a well-conditioned system (a Hessian whose LU takes a row swap), of a singular one for an input without variance."""
    warp, cc, iters = np.eye(3, dtype=np.float32).reshape(-1), C.c_double(-5), C.c_int(-5)
    (t, st), (i, si) = strided(tmpl, 3), strided(inp, 5)
    m, sm = strided(mask, 2) if mask is not None else (None, 0)
    hs, ws, hd, wd = *tmpl.shape, *inp.shape
    if dev:
        ds = [to_dev(x.base) if x is not None else None for x in (t, i, m)]
        rc = lib.km_find_transform_ecc_dev(ctx, ds[0], ds[1], dtype, hs, ws, st, hd, wd, si, ds[2], sm, P(warp), max_iter, eps, gauss, C.byref(cc), C.byref(iters))
        for d in ds:
            if d is not None:
                ok(lib.km_dev_free(ctx, d), "dev_free")
    else:
        rc = lib.km_find_transform_ecc(ctx, P(t), P(i), dtype, hs, ws, st, hd, wd, si, P(m), sm, P(warp), max_iter, eps, gauss, C.byref(cc), C.byref(iters))
    return rc, warp, cc.value, iters.value


tmpl = rng.integers(0, 200, (64, 64)).astype(np.float32)
inp = tmpl + rng.integers(0, 9, (64, 64)).astype(np.float32)
ones = np.ones((64, 64), np.uint8)
for dev in (False, True):
    for dtype, cast, mask in ((F32, np.float32, None), (U8, np.uint8, ones)):
        rc, warp, cc, iters = ecc(tmpl.astype(cast), inp.astype(cast), dtype, 6, 0.0, mask, dev)      # eps 0: to the stop at max_iters
        ok(rc, "find_transform_ecc")
        assert iters == 6 and 0.9 < cc <= 1.0 and not np.array_equal(warp, np.eye(3, dtype=np.float32).reshape(-1)) and np.isfinite(warp).all(), (cc, iters, warp)
        rc, warp, cc, iters = ecc(tmpl.astype(cast), inp.astype(cast), dtype, 50, 1e-3, mask, dev)    # the stand-in's correlation does not move: two iterations
        assert rc == 0 and iters == 2, (rc, iters)
        rc, warp, cc, iters = ecc(tmpl.astype(cast), np.full((64, 64), 4, cast), dtype, 6, 0.0, mask, dev)
        err(rc, "find_transform_ecc on a singular system", KM_E_NO_CONVERGENCE, "iteration 1")
        assert iters == 1
    ok(ecc(tmpl, inp[:50, :60], F32, 3, 0.0, None, dev)[0], "find_transform_ecc, shapes that differ")
err(ecc(tmpl, inp, F32, 6, 0.0, gauss=3)[0], "ecc gaussFiltSize", KM_E_UNSUPPORTED)
err(ecc(tmpl.astype(np.uint16), inp.astype(np.uint16), U16, 6, 0.0)[0], "ecc dtype", KM_E_UNSUPPORTED)
err(ecc(tmpl, inp, F32, -1, 0.0)[0], "ecc max_iter")
err(lib.km_find_transform_ecc(ctx, P(tmpl), P(inp), F32, 64, 64, 64, 64, 64, 64, None, 0, None, 5, 0.0, 5, C.byref(C.c_double()), C.byref(C.c_int())), "ecc null map")
err(lib.km_find_transform_ecc(ctx, None, P(inp), F32, 64, 64, 64, 64, 64, 64, None, 0, P(warp), 5, 0.0, 5, C.byref(C.c_double()), C.byref(C.c_int())), "ecc null template")


def refine(mon, ref, inits, max_iter, eps, dev=False):
    n = len(inits)
    inits = np.ascontiguousarray(inits, np.float64)
    final, resid, cc = np.full((n, 9), -5.0), np.full((n, 9), -5, np.float32), np.full(n, -5.0)
    iters, valid, status = np.full(n, -5, np.int32), np.full(n, -5, np.int64), np.full(n, -5, np.int32)
    (m, sm), (r, sr) = strided(mon, 3), strided(ref, 5)
    tail = (n, P(inits), max_iter, eps, P(final), P(resid), P(cc), P(iters), P(valid), P(status))
    if dev:
        dm, dr = to_dev(m.base), to_dev(r.base)
        rc = lib.km_refine_ecc_candidates_dev(ctx, dm, *mon.shape, sm, dr, *ref.shape, sr, *tail)
        for d in (dm, dr):
            ok(lib.km_dev_free(ctx, d), "dev_free")
    else:
        rc = lib.km_refine_ecc_candidates(ctx, P(m), *mon.shape, sm, P(r), *ref.shape, sr, *tail)
    return rc, final, resid, cc, iters, valid, status


ref8 = rng.integers(1, 200, (64, 64)).astype(np.uint8)
mon8 = (ref8 + rng.integers(0, 9, (64, 64))).astype(np.uint8)
shift = np.array([1, 0, 2.5, 0, 1, -1.25, 0, 0, 1.0])
for dev in (False, True):
    rc, final, resid, cc, iters, valid, status = refine(mon8, ref8, [ident, shift], 4, 0.0, dev)      # two candidates in one call
    ok(rc, "refine_ecc_candidates")
    assert (status == ECC_CONVERGED).all() and (iters == 4).all() and (valid == 64 * 64).all() and ((cc > 0.9) & (cc <= 1)).all(), (status, iters, valid, cc)
    for k, init in enumerate((ident, shift)):
        assert np.allclose(final[k].reshape(3, 3), resid[k].astype(np.float64).reshape(3, 3) @ init.reshape(3, 3), rtol=1e-12, atol=0)
    rc, final, resid, cc, iters, valid, status = refine(np.full((64, 64), 4, np.uint8), ref8, [ident, shift], 4, 0.0, dev)
    assert rc == 0 and (status == ECC_NO_CONVERGENCE).all() and np.isnan(final).all() and np.isnan(cc).all(), (rc, status)
    sparse = np.zeros((64, 64), np.uint8)
    sparse[:15, :] = mon8[:15, :]                                  # 960 pixels: below the 1000 the refinement asks for
    rc, final, resid, cc, iters, valid, status = refine(sparse, ref8, [ident], 4, 0.0, dev)
    assert rc == 0 and status[0] == ECC_SKIPPED and valid[0] == 960 and iters[0] == 0 and np.isnan(final).all(), (rc, status, valid)
    ok(refine(mon8, ref8, np.zeros((0, 9)), 4, 0.0, dev)[0], "refine_ecc_candidates: no candidate")
err(refine(mon8, ref8, [ident], -1, 0.0)[0], "refine max_iter")
err(lib.km_refine_ecc_candidates(ctx, P(mon8), 64, 64, 64, P(ref8), 64, 64, 64, 1, None, 4, 0.0, None, None, None, None, None, None), "refine null arrays")
err(lib.km_refine_ecc_candidates(ctx, None, 64, 64, 64, P(ref8), 64, 64, 64, 0, None, 4, 0.0, None, None, None, None, None, None), "refine null image")

ok(lib.km_ctx_destroy(ctx), "ctx_destroy")
cnt = (C.c_long * 3)()
lib.stub_counters(cnt)
assert cnt[0] == 0 and cnt[1] == 0, f"HIP allocations left behind: device {cnt[0]}, page-locked {cnt[1]}"
assert cnt[2] == 0, f"{cnt[2]} asynchronous runtime copies touched PAGEABLE memory"
print("HOST-ASAN ALIGN OK")
