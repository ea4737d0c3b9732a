"""cv2.SIFT detectAndCompute of the align step on the GPU (k_sift.hip, api_sift.hip, sift_math.hpp) against its definition,
tests/sift_restatement.py: the number of key points, their order, all six fields by their bits, the descriptors byte for byte and
the stats counts.  Nothing is excluded and nothing has a tolerance."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the full-size case runs this file as a script
import sift_restatement as S  # noqa: E402
from sift_scenes import scene  # noqa: E402

from karios_amd import _lib, synth  # noqa: E402
from karios_amd.matcher import Sift, global_align  # noqa: E402
from karios_amd.ops import SIFT_FIELDS, sift_detect_and_compute  # noqa: E402  (the feature's names: the file fails without them)

pytestmark = pytest.mark.gpu
_cache = {}


def restated(kind, h, w, contrast=0.02, edge=10.0):
    """The restatement's outcome on a scene (kept per module: its Python loops are the expensive part)."""
    key = (kind, h, w, contrast, edge)
    if key not in _cache:
        info = {}
        kp, desc = S.detect_and_compute(scene(kind, h, w), contrast, edge, info=info)
        _cache[key] = (kp, desc, info["stats"])
    return _cache[key]


def assert_same(got_kp, got_desc, got_stats, want):
    kp, desc, stats = want
    assert len(got_kp["x"]) == len(kp)
    for name in SIFT_FIELDS:
        a, b = np.ascontiguousarray(got_kp[name]), np.ascontiguousarray(kp[name])
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=name)
    if desc is None:
        assert len(got_desc) == 0
    else:
        np.testing.assert_array_equal(got_desc, desc.astype(got_desc.dtype))
    if got_stats is not None:
        n = stats["octaves"]
        assert got_stats["octaves"] == n
        for name in ("candidates", "refined", "keypoints"):
            assert got_stats[name][:n] == stats[name], name
        assert (got_stats["before_dedup"], got_stats["after_dedup"]) == (stats["before_dedup"], stats["after_dedup"])
        assert got_stats["count"] == len(kp) == sum(stats["keypoints"]) - (stats["before_dedup"] - stats["after_dedup"])


CASES = [("textured", 64, 64), ("textured", 97, 131), ("textured", 200, 257), ("textured", 512, 512), ("textured", 333, 768),
         ("textured", 12, 40), ("flat", 97, 131), ("binary", 97, 131), ("binary", 64, 64), ("blob", 64, 64), ("blob", 200, 257), ("flat", 9, 9), ("lattice", 120, 120)]


@pytest.mark.parametrize("kind,h,w", CASES)
def test_bit_identical_to_the_restatement(kind, h, w):
    want = restated(kind, h, w)
    kp, desc, stats = sift_detect_and_compute(scene(kind, h, w), descriptor_dtype=np.uint8, return_stats=True)
    print(kind, h, w, "key points", len(kp), "stats", {k: stats[k] for k in ("candidates", "refined", "keypoints")})
    assert_same(kp, desc, stats, want)
    if kind == "textured" and h >= 200:
        assert len(kp) > 100


def test_non_default_parameters():
    want = restated("textured", 200, 257, 0.04, 5.0)
    assert len(want[0]) < len(restated("textured", 200, 257)[0])
    kp, desc, stats = sift_detect_and_compute(scene("textured", 200, 257), contrast_threshold=0.04, edge_threshold=5, descriptor_dtype=np.uint8,
                                              return_stats=True)
    assert_same(kp, desc, stats, want)


def test_both_descriptor_dtypes_hold_the_same_values():
    img = scene("textured", 200, 257)
    kp8, d8 = sift_detect_and_compute(img, descriptor_dtype=np.uint8)
    kpf, df = sift_detect_and_compute(img)
    assert d8.dtype == np.uint8 and df.dtype == np.float32 and df.shape == d8.shape == (len(kp8), 128)
    np.testing.assert_array_equal(df, d8.astype(np.float32))
    assert kp8.tobytes() == kpf.tobytes()


def test_strided_host_view_never_reads_the_padding():
    img = scene("textured", 97, 131)
    wide = np.full((97, 131 + 37), 255, np.uint8)
    wide[:, :131] = img
    kp, desc, stats = sift_detect_and_compute(wide[:, :131], descriptor_dtype=np.uint8, return_stats=True)
    assert_same(kp, desc, stats, restated("textured", 97, 131))


def test_device_form_on_torch_tensors_equals_the_host_form_and_repeats():
    import torch
    ctx = _lib.default_context()
    dev = torch.device("cuda", ctx.device)
    img = scene("textured", 333, 768)
    wide = torch.full((333, 800), 255, dtype=torch.uint8, device=dev)
    wide[:, :768] = torch.from_numpy(img).to(dev)
    runs = [sift_detect_and_compute(wide[:, :768], descriptor_dtype=np.uint8, return_stats=True) for _ in range(2)]
    host = sift_detect_and_compute(img, descriptor_dtype=np.uint8)
    for kp, desc, stats in runs:
        assert desc.is_cuda and all(kp[name].is_cuda for name in SIFT_FIELDS)
        rec = {name: kp[name].cpu().numpy() for name in SIFT_FIELDS}
        assert_same(rec, desc.cpu().numpy(), stats, restated("textured", 333, 768))
        for name in SIFT_FIELDS:
            assert rec[name].tobytes() == np.ascontiguousarray(host[0][name]).tobytes()
        np.testing.assert_array_equal(desc.cpu().numpy(), host[1])


def test_capacity_protocol():
    img = scene("textured", 200, 257)
    want_kp, want_desc, _stats = restated("textured", 200, 257)
    n = len(want_kp)
    cap = n // 3
    kp, desc, stats = sift_detect_and_compute(img, descriptor_dtype=np.uint8, return_stats=True, capacity=cap)
    assert stats["count"] == n and len(kp) == cap
    assert kp.tobytes() == want_kp[:cap].tobytes()
    np.testing.assert_array_equal(desc, want_desc[:cap])
    # the status itself, and nfeatures
    ctx = _lib.default_context()
    fields = np.zeros((6, cap), np.float32)
    d = np.zeros((cap, 128), np.uint8)
    count = C.c_int(0)
    args = [_lib.ptr(fields[k]) for k in range(6)] + [_lib.ptr(d), _lib._DTYPES[np.dtype("uint8")], 128, C.byref(count), None]
    rc = ctx.lib.km_sift_detect_and_compute(ctx.handle, _lib.ptr(img), 200, 257, 257, 0, 3, 0.02, 10.0, 1.6, cap, *args)
    assert rc == _lib.E_CAPACITY and count.value == n
    np.testing.assert_array_equal(d, want_desc[:cap])
    rc = ctx.lib.km_sift_detect_and_compute(ctx.handle, _lib.ptr(img), 200, 257, 257, 100, 3, 0.02, 10.0, 1.6, cap, *args)
    assert rc == _lib.E_UNSUPPORTED


def test_lists_that_overflow_run_their_stage_again_and_the_wrapper_calls_twice():
    """The dot lattice has more extrema than the candidate list's first size (0.4 % of samples x layers), more than two orientations
    per refined key point (the key-point list's first room is 2 n + 64) and more key points than the wrapper's estimate: all three
    repeat paths run, and the outcome is still the restatement's."""
    from karios_amd.ops import sift_capacity_estimate
    want = restated("lattice", 120, 120)
    stats = want[2]
    assert stats["candidates"][0] > max(256, 240 * 240 * 3 // 256)
    assert stats["keypoints"][0] > 2 * stats["refined"][0] + 64
    assert len(want[0]) > sift_capacity_estimate(120, 120)
    kp, desc, got = sift_detect_and_compute(scene("lattice", 120, 120), descriptor_dtype=np.uint8, return_stats=True)
    print("lattice: key points", len(kp), "regrows", got["regrows"], "calls", got["calls"])
    assert got["calls"] == 2 and got["regrows"][0] >= 1 and got["regrows"][1] >= 1
    assert_same(kp, desc, got, want)
    import torch
    dev = torch.device("cuda", _lib.default_context().device)
    kpd, descd, gotd = sift_detect_and_compute(torch.from_numpy(scene("lattice", 120, 120)).to(dev), descriptor_dtype=np.uint8, return_stats=True)
    assert gotd["calls"] == 2
    assert_same({name: kpd[name].cpu().numpy() for name in SIFT_FIELDS}, descd.cpu().numpy(), gotd, want)


def corners_error(H, planted, h, w):
    c = np.array([[0, 0, 1], [w - 1, 0, 1], [w - 1, h - 1, 1], [0, h - 1, 1]], np.float64)
    a, b = c @ np.asarray(H, np.float64).T, c @ planted.T
    return np.abs(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:]).max()


PLANTED = np.array([[1.002, -0.004, 3.5], [0.003, 0.998, -2.25], [1e-6, -5e-7, 1.0]])


def warped(ref_f32, n):
    """mon: `ref` seen through the inverse of PLANTED (dst(x) = src(M^-1 x)), so that mon -> ref is PLANTED."""
    from karios_amd import ops
    return ops.warp_perspective(ref_f32, np.linalg.inv(PLANTED), (n, n), flags=ops.INTER_LINEAR, border_value=0.0)


def planted_pair(n, seed):
    ref = synth.sift_scene(n, seed)
    return np.clip(np.rint(warped(ref.astype(np.float32), n)), 0, 255).astype(np.uint8), ref


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_whole_chain_through_detect_global_alignment():
    n = 1024
    mon, ref = planted_pair(n, 21)
    got = global_align.detect_global_alignment(mon, ref, sift=Sift())
    # the pieces, one by one
    sift = Sift()
    mon_u8, ref_u8 = global_align._preprocess(mon), global_align._preprocess(ref)
    kp_mon, desc_mon = sift.detectAndCompute(mon_u8, None)
    kp_ref, desc_ref = sift.detectAndCompute(ref_u8, None)
    assert len(kp_mon) > 500 and len(kp_ref) > 500 and desc_mon.dtype == np.float32
    assert kp_mon[0].pt == (float(kp_mon.records["x"][0]), float(kp_mon.records["y"][0]))
    s, d = global_align.match_descriptors(kp_mon, desc_mon, kp_ref, desc_ref)
    matrix, n_inliers = global_align.estimate_homography(s, d)
    print("chain: key points", len(kp_mon), len(kp_ref), "matches", len(s), "inliers", n_inliers, "corner error", corners_error(matrix, PLANTED, n, n))
    assert corners_error(matrix, PLANTED, n, n) <= global_align.RANSAC_THRESHOLD_PX
    want = global_align.refine_global_alignment(mon_u8, ref_u8, matrix, n_inliers, len(s))
    assert (got.n_matches, got.n_inliers) == (len(s), n_inliers)
    np.testing.assert_array_equal(bits(got.matrix), bits(want.matrix))
    assert [c[0] for c in got.candidates] == [c[0] for c in want.candidates]
    for a, b in zip(got.candidates, want.candidates):
        np.testing.assert_array_equal(bits(a[1]), bits(b[1]))


FULLSIZE_LIMIT_S = 600   # the child process (scene, two preprocess calls, three SIFT calls, one match, RANSAC) takes 7 s on an MI355X: ample


def test_sentinel2_size_call_on_a_resident_raster():
    """The full-size case in a process of its own, under its own time limit: a hang ends there, not in the suite."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--fullsize"], capture_output=True, text=True, timeout=FULLSIZE_LIMIT_S)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "FULLSIZE OK" in out.stdout, out.stdout[-3000:] + out.stderr[-6000:]


def fullsize_case():
    """10980 x 10980: the call finishes, repeats itself, keeps every point inside the image, and its count is the stats' sum; the
    planted homography of a full-size pair comes back within 3 px at the corners."""
    import torch
    ctx = _lib.default_context()
    dev = torch.device("cuda", ctx.device)
    n = 10980
    ref = synth._base_torch(n, n, 11, dev)[synth.PAD:synth.PAD + n, synth.PAD:synth.PAD + n].cpu().numpy()
    mon = warped(ref, n)
    mon_u8, ref_u8 = global_align._preprocess(mon), global_align._preprocess(ref)
    d_mon = torch.from_numpy(mon_u8).to(dev)
    t0 = time.perf_counter()
    kp, desc, stats = sift_detect_and_compute(d_mon, return_stats=True)
    t1 = time.perf_counter()
    kp2, desc2, stats2 = sift_detect_and_compute(d_mon, return_stats=True)
    t2 = time.perf_counter()
    print("10980^2: key points", stats["count"], "seconds", t1 - t0, t2 - t1, "stats", stats)
    count = stats["count"]
    assert count == len(desc) == sum(stats["keypoints"]) - (stats["before_dedup"] - stats["after_dedup"]) and count > 100000
    times, times2 = stats.pop("times_us"), stats2.pop("times_us")
    print("10980^2 times (us)", times, times2)
    assert stats == stats2 and torch.equal(desc, desc2) and all(torch.equal(kp[name], kp2[name]) for name in SIFT_FIELDS)
    x, y = kp["x"].cpu().numpy(), kp["y"].cpu().numpy()
    assert x.min() >= 0 and y.min() >= 0 and x.max() <= n - 1 and y.max() <= n - 1
    del desc2, kp2
    # the pair: the strongest key points of both images carry the match (the matcher's cost is quadratic in their number)
    sift = Sift()
    kp_ref, desc_ref = sift.detectAndCompute(ref_u8, None)
    keep = 60000
    top_m = np.sort(np.argsort(-kp["response"].cpu().numpy(), kind="stable")[:keep])
    top_r = np.sort(np.argsort(-kp_ref.records["response"], kind="stable")[:keep])
    pts_m = np.stack([x, y], 1)[top_m]
    s, d = global_align.match_descriptors(pts_m, desc.cpu().numpy()[top_m], np.asarray(kp_ref)[top_r], desc_ref[top_r])
    matrix, n_inliers = global_align.estimate_homography(s, d)
    err = corners_error(matrix, PLANTED, n, n)
    print("10980^2 pair: matches", len(s), "inliers", n_inliers, "corner error", err)
    assert err <= global_align.RANSAC_THRESHOLD_PX
    print("FULLSIZE OK")


if __name__ == "__main__":
    assert sys.argv[1:] == ["--fullsize"]
    fullsize_case()
