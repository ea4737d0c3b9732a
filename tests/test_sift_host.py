"""CPU suite: SIFT detectAndCompute of the align step (cv2.SIFT_create(nfeatures=0, contrastThreshold=0.02, edgeThreshold=10),
karios/matcher/global_align.py:48-50, 160-166).

1. csrc/sift_math.hpp - the text the kernels and the library's host side compile - built by g++ with -ffp-contract=off under the
   address and undefined-behaviour sanitizers and compared with tests/sift_restatement.py bit for bit (tests/sift_host_driver.py, in
   a subprocess with libasan preloaded).  csrc/sift_order.hpp - the final order on the host - built the same way and held to one
   stable sort on the stated order.
2. Known answers that tie the restatement to SIFT rather than to itself.
3. The chain on the CPU: restatement SIFT -> match_restatement -> ransac_restatement recovers a planted homography.
4. The ABI carries the two entry points; the argument checks of ops.sift_detect_and_compute and Sift.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import align_restatement as A
import match_restatement as M
import ransac_restatement as R
import sanitizer_harness as san
import sift_restatement as S

from karios_amd import _lib, ops, synth
from karios_amd.matcher import Sift, global_align
from karios_amd.ops import sift_detect_and_compute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the shared header ---------------------------------------------------------------------------------------------------------------
SHIM = r"""
#include "sift_math.hpp"
extern "C" {
void sf_exp(int n, const double *x, double *out) { for (int i = 0; i < n; i++) out[i] = sf::exp64(x[i]); }
void sf_sincos(int n, const float *a, float *c, float *s) { for (int i = 0; i < n; i++) sf::sincos_deg(a[i], c[i], s[i]); }
void sf_atan2(int n, const float *y, const float *x, float *out) { for (int i = 0; i < n; i++) out[i] = sf::atan2_deg(y[i], x[i]); }
int sf_kernel(double sigma, float *taps) { return sf::gaussian_kernel(sigma, taps, 2 * sf::MAX_RADIUS + 1); }
double sf_level_sigma(double sigma, int n_layers, int i) { return sf::level_sigma(sigma, n_layers, i); }
float sf_base_sigma(double sigma) { return sf::base_sigma(sigma); }
int sf_n_octaves(int h2, int w2) { return sf::n_octaves(h2, w2); }
void sf_refine_many(const float *dog, size_t plane, ptrdiff_t stride, int rows, int cols, int octv, int n, const int *cand, int n_layers,
                    double contrast, double edge, double sigma, int *ok, sf::Refined *out, void *)
{
    for (int i = 0; i < n; i++)
        ok[i] = sf::refine(dog, plane, stride, rows, cols, octv, cand[3 * i], cand[3 * i + 1], cand[3 * i + 2], n_layers, contrast, edge, sigma, out[i]);
}
int sf_orient(const float *img, ptrdiff_t stride, int rows, int cols, int r, int c, float size, int octv, float *angles)
{
    return sf::orientations(img, stride, rows, cols, r, c, size, octv, angles);
}
void sf_describe(const float *img, ptrdiff_t stride, int rows, int cols, float px, float py, float angle, float scl, uint8_t *out)
{
    float hist[sf::D_HIST];
    sf::descriptor<1>(img, stride, rows, cols, px, py, angle, scl, hist, out);
}
}
"""


def test_shared_header_matches_the_restatement_under_sanitizers(tmp_path):
    env = san.san_env()
    src, so = tmp_path / "sift_shim.cpp", tmp_path / "libsift_shim.so"
    src.write_text(SHIM)
    san.build(src, so)
    out = san.run([sys.executable, os.path.join(ROOT, "tests", "sift_host_driver.py"), str(so)], "SIFT-HOST OK", 1500, env)
    cand, kps = re.search(r"candidates (\d+) key points (\d+)", out.stdout).groups()
    assert int(cand) >= 200 and int(kps) >= 200


ORDER_MAIN = r"""
#include "sift_order.hpp"
#include <cstdio>
int main(int argc, char **argv)       // keys file -> file of the indices that stay, in the final order
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<sf::Key> keys;
    sf::Key k;
    while (fread(&k, sizeof k, 1, f) == 1) keys.push_back(k);
    fclose(f);
    std::vector<int> perm;
    sf::final_order(keys.data(), keys.size(), perm);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!perm.empty() && fwrite(perm.data(), sizeof(int), perm.size(), f) != perm.size()) return 2;
    return fclose(f) ? 2 : 0;
}
"""


def test_final_order_of_the_library_is_the_stated_total_order(tmp_path):
    """csrc/sift_order.hpp (a radix sort on (x, y), sf::key_less inside the runs of one point) against one stable sort on the stated
    order - x, y ascending, size descending, angle ascending, response and octave descending - and the duplicate rule, on records
    with ties at every depth; the records that are not positive and finite take the header's other path."""
    src, exe = tmp_path / "order_main.cpp", tmp_path / "order_main"
    src.write_text(ORDER_MAIN)
    san.build(src, exe, shared=False)
    rng = np.random.default_rng(4)

    def records(n, lowest):
        k = np.zeros(n, S.KP_DTYPE)
        k["x"] = np.float32(lowest) + rng.integers(0, 40, n).astype(np.float32) * np.float32(547.25) + rng.integers(0, 3, n).astype(np.float32) / 8
        k["y"] = np.float32(lowest) + rng.integers(0, 40, n).astype(np.float32) * np.float32(0.37)
        k["size"] = rng.choice(np.float32([2.1, 3.3, 9.0]), n)
        k["angle"] = rng.choice(np.float32([0.0, 10.5, 200.25, 359.9]), n)
        k["response"] = rng.choice(np.float32([0.01, 0.02]), n)
        k["octave"] = rng.choice(np.int32([0x10100, 0x10200, 0x802ff]), n)
        return k

    assert S.KP_DTYPE.names == ("x", "y", "size", "angle", "response", "octave") and S.KP_DTYPE.itemsize == 24
    for case, k in (("ties", records(30000, 5.0)), ("wide", np.concatenate([records(5000, 5.0), records(5000, 20000.0)])),
                    ("zero and negative", records(3000, -2.0)), ("one", records(1, 5.0)), ("none", records(0, 5.0))):
        fin, fout = tmp_path / "keys.bin", tmp_path / "perm.bin"
        fin.write_bytes(k.tobytes())
        subprocess.check_call([str(exe), str(fin), str(fout)], timeout=120)
        got = np.fromfile(fout, np.int32)
        order = np.lexsort((-k["octave"].astype(np.int64), -k["response"], k["angle"], -k["size"], k["y"], k["x"]))
        s = k[order]
        keep = np.ones(len(s), bool)
        keep[1:] = ~((s["x"][1:] == s["x"][:-1]) & (s["y"][1:] == s["y"][:-1]) & (s["size"][1:] == s["size"][:-1]) & (s["angle"][1:] == s["angle"][:-1]))
        assert np.array_equal(got, order[keep]), case
        if case == "ties":
            assert 100 < keep.sum() < len(k) - 100          # duplicates were there, and not everything was one


# ---- 2. known answers -------------------------------------------------------------------------------------------------------------------
def test_kernel_sizes_and_unit_sums_of_the_default_sigmas():
    sig = S.level_sigmas(1.6, 3)
    assert sig[0] == 1.6 and abs(sig[1] - 1.6 * np.sqrt(2 ** (2 / 3) - 1)) < 1e-12 and abs(sig[5] / sig[2] - 2.0) < 1e-12
    base = np.sqrt(np.float32(1.6) * np.float32(1.6) - np.float32(1.0))
    sizes = []
    for s in [float(base)] + sig[1:]:
        k = S.gaussian_kernel(s)
        sizes.append(len(k))
        assert k.dtype == np.float32 and len(k) % 2 == 1 and np.array_equal(k, k[::-1]) and k.argmax() == len(k) // 2
        assert abs(float(k.astype(np.float64).sum()) - 1.0) <= len(k) * 2.0 ** -24       # each tap rounds by half an ulp of a value < 1
    assert sizes == [11, 11, 13, 17, 21, 27]
    assert S.n_octaves(2 * 10980, 2 * 10980) == 13 and S.n_octaves(1024, 1024) == 9 and S.n_octaves(2, 2) == 0


def test_flat_and_tiny_images_give_nothing():
    for img in (np.full((64, 80), 93, np.uint8), np.zeros((128, 128), np.uint8), np.full((4, 4), 7, np.uint8), synth.sift_scene(8, 1)[:3, :4]):
        kp, desc = S.detect_and_compute(img)
        assert len(kp) == 0 and desc is None and kp.dtype == S.KP_DTYPE


@pytest.mark.parametrize("s", [3, 5, 8])
def test_one_gaussian_blob(s):
    n = 128
    yy, xx = np.mgrid[0:n, 0:n]
    img = np.rint(40 + 180 * np.exp(-((yy - 64) ** 2 + (xx - 64) ** 2) / (2.0 * s * s))).astype(np.uint8)
    kp, desc = S.detect_and_compute(img)
    assert len(kp) >= 1
    best = kp[np.argmax(kp["response"])]
    print("blob", s, "strongest", best, "of", len(kp))
    assert abs(float(best["x"]) - 64) <= 1e-3 and abs(float(best["y"]) - 64) <= 1e-3
    step = 2.0 ** (1.0 / 3.0)
    assert s / step <= float(best["size"]) / 2 <= s * step


@pytest.fixture(scope="module")
def scene512():
    info = {}
    kp, desc = S.detect_and_compute(synth.sift_scene(512, 1), info=info)
    return kp, desc, info["stats"]


def test_scene_has_enough_key_points_and_well_formed_descriptors(scene512):
    kp, desc, stats = scene512
    assert len(kp) >= 500 and desc.shape == (len(kp), 128) and desc.dtype == np.uint8
    norms = np.sqrt((desc.astype(np.float64) ** 2).sum(1))
    print("key points", len(kp), "descriptor norms", norms.min(), norms.max())
    assert np.abs(norms - 512).max() <= 0.5 * np.sqrt(128)
    assert stats["after_dedup"] == len(kp) <= stats["before_dedup"] == sum(stats["keypoints"])
    assert (kp["x"] >= 0).all() and (kp["y"] >= 0).all() and (kp["x"] <= 511).all() and (kp["y"] <= 511).all()
    assert ((kp["angle"] >= 0) & (kp["angle"] < 360)).all() and (kp["response"] * 3 >= 0.02).all()
    layer, octave = (kp["octave"] >> 8) & 255, kp["octave"] & 255
    assert ((layer >= 1) & (layer <= 3)).all() and set(np.unique(octave)) <= {255, 0, 1, 2, 3, 4, 5, 6, 7}


def test_no_two_key_points_are_equal_and_the_order_is_the_stated_one(scene512):
    kp = scene512[0]
    assert len(np.unique(kp)) == len(kp)
    rows = [(float(k["x"]), float(k["y"]), -float(k["size"]), float(k["angle"]), -float(k["response"]), -int(k["octave"])) for k in kp]
    # the order was fixed before the octave byte was decremented: undo that for the comparison
    rows = [r[:5] + (-(((-r[5]) & ~255) | (((-r[5]) + 1) & 255)),) for r in rows]
    assert rows == sorted(rows)
    head = [r[:4] for r in rows]
    assert len(set(head)) == len(head)                                     # no two share (x, y, size, angle)


# ---- 3. the chain on the CPU --------------------------------------------------------------------------------------------------------------
def test_the_chain_recovers_a_planted_homography():
    n = 256
    planted = np.array([[1.002, -0.004, 3.5], [0.003, 0.998, -2.25], [1e-6, -5e-7, 1.0]])
    ref = synth.sift_scene(n, 21)
    mon = A.warp_perspective(ref, np.linalg.inv(planted), (n, n))         # dst(x) = src(M^-1 x): mon -> ref is `planted`
    kp_mon, desc_mon = S.detect_and_compute(mon)
    kp_ref, desc_ref = S.detect_and_compute(ref)
    qi, ti, _dist, counts = M.match_lowe_mutual(desc_mon, desc_ref, global_align.LOWE_RATIO)
    src, dst = np.stack([kp_mon["x"], kp_mon["y"]], 1)[qi], np.stack([kp_ref["x"], kp_ref["y"]], 1)[ti]
    H, mask = R.find_homography(src, dst, global_align.RANSAC_THRESHOLD_PX, global_align.RANSAC_MAX_ITERS, global_align.RANSAC_CONFIDENCE)
    c = np.array([[0, 0, 1], [n - 1, 0, 1], [n - 1, n - 1, 1], [0, n - 1, 1]], np.float64)
    a, b = c @ H.T, c @ planted.T
    err = np.abs(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:]).max()
    print("key points", len(kp_mon), len(kp_ref), "matches", counts, "inliers", int(mask.sum()), "corner error", err)
    assert err <= global_align.RANSAC_THRESHOLD_PX


# ---- 4. plumbing ------------------------------------------------------------------------------------------------------------------------
def test_header_and_signature_table_carry_the_entry_points():
    header = open(os.path.join(ROOT, "include", "karios_hip.h")).read()
    for name in ("km_sift_detect_and_compute", "km_sift_detect_and_compute_dev"):
        assert re.search(rf"\bint {name}\s*\(", header) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == 22
    assert "KM_E_CAPACITY = -8" in header and _lib.E_CAPACITY == -8 and "global_align.py:48-50" in header
    assert hasattr(_lib.load(), "km_sift_detect_and_compute_dev")
    # nothing of the product imports the restatement
    for dirpath, _, files in os.walk(os.path.join(ROOT, "karios_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "sift_restatement" not in open(os.path.join(dirpath, f)).read(), f


def test_argument_checks_need_no_device():
    with pytest.raises(ValueError, match="expected a uint8 image"):
        sift_detect_and_compute(np.zeros((32, 32), np.float32))
    with pytest.raises(ValueError, match="expected a uint8 image"):
        sift_detect_and_compute(np.zeros((32, 32), np.uint16))
    with pytest.raises(ValueError, match="descriptor_dtype"):
        sift_detect_and_compute(np.zeros((32, 32), np.uint8), descriptor_dtype=np.float64)
    with pytest.raises(_lib.KariosHipError, match="2-D"):
        sift_detect_and_compute(np.zeros((32, 32, 3), np.uint8))
    with pytest.raises(NotImplementedError, match="nfeatures"):
        Sift(nfeatures=500)
    with pytest.raises(NotImplementedError, match="mask"):
        Sift().detectAndCompute(np.zeros((32, 32), np.uint8), np.ones((32, 32), np.uint8))
    s = Sift()
    assert (s.contrast_threshold, s.edge_threshold) == (global_align.SIFT_CONTRAST_THRESHOLD, global_align.SIFT_EDGE_THRESHOLD) == (0.02, 10)


def test_sift_object_and_key_point_container(monkeypatch):
    rec = np.zeros(3, ops.SIFT_KEYPOINT_DTYPE)
    rec["x"], rec["y"], rec["size"], rec["octave"] = [1.5, 2.5, 3.5], [4, 5, 6], [2, 3, 4], [511, 767, 1023]
    desc = np.arange(3 * 128, dtype=np.float32).reshape(3, 128) % 256
    seen = {}

    def fake(image, **kw):
        seen.update(kw, image=image)
        return (rec, desc) if seen.get("some", True) else (rec[:0], desc[:0])

    monkeypatch.setattr(ops, "sift_detect_and_compute", fake)
    img = np.zeros((16, 16), np.uint8)
    kp, d = Sift(0.03, 7).detectAndCompute(img, None)
    assert seen["image"] is img and (seen["contrast_threshold"], seen["edge_threshold"]) == (0.03, 7.0)
    assert d is desc and len(kp) == 3 and kp[1].pt == (2.5, 5.0) and kp[2].size == 4.0 and kp[0].octave == 511
    assert [k.pt for k in kp] == [(1.5, 4.0), (2.5, 5.0), (3.5, 6.0)]
    pts = global_align._points(kp)
    assert type(pts) is np.ndarray and pts.dtype == np.float32 and pts.tolist() == [[1.5, 4.0], [2.5, 5.0], [3.5, 6.0]]
    assert np.asarray(kp[np.array([2, 0])]).tolist() == [[3.5, 6.0], [1.5, 4.0]] and len(kp[:2]) == 2
    seen["some"] = False
    kp, d = Sift().detectAndCompute(img)
    assert len(kp) == 0 and d is None
    with pytest.raises(RuntimeError, match="SIFT found no descriptors"):
        global_align.match_descriptors(kp, d, kp, d)
