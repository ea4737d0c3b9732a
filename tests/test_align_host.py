"""Global align step on the CPU: the numpy restatement (tests/align_restatement.py) is the definition of the warp and ECC
arithmetic; karios_amd.matcher.global_align's glue runs with karios_amd.ops replaced by that restatement."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_restatement as R  # noqa: E402

from karios_amd import _lib, ops, synth  # noqa: E402


def _scene(n, pad=32, seed=20260101):
    base = synth.make_base(n + 2 * pad, n + 2 * pad, seed)[: n + 2 * pad, : n + 2 * pad]
    return np.clip((base - 1000.0) / 4000.0 * 255.0, 0, 255).astype(np.uint8)


def _homography(tx=2.3, ty=-1.7, deg=0.05, scale=1 + 2e-4, p=(1e-7, -1e-7)):
    th = np.radians(deg)
    return np.array([[scale * np.cos(th), -scale * np.sin(th), tx], [scale * np.sin(th), scale * np.cos(th), ty], [p[0], p[1], 1.0]])


def _corners(M, n):
    c = np.array([[0, 0, 1], [n - 1, 0, 1], [0, n - 1, 1], [n - 1, n - 1, 1]], float).T
    q = np.asarray(M, float) @ c
    return q[:2] / q[2]


def test_restatement_warp_integer_translation_is_a_shift():
    img = _scene(64, pad=0)
    for dtype in (np.uint8, np.float32):
        a = img.astype(dtype)
        M = np.array([[1, 0, 3], [0, 1, -2], [0, 0, 1]], float)   # dst(x, y) = src(x + 3, y - 2)
        for flags in (R.INTER_LINEAR, R.INTER_NEAREST):
            out = R.warp_perspective(a, M, (64, 64), flags | R.WARP_INVERSE_MAP, 0.0)
            exp = np.zeros_like(a)
            exp[2:, :61] = a[:62, 3:]
            np.testing.assert_array_equal(out, exp)


def test_restatement_forward_mode_is_inverse_mode_of_the_closed_form_inverse():
    rng = np.random.default_rng(5)
    img = rng.random((57, 83)).astype(np.float32)
    M = _homography(4.2, -3.1, 1.5, 1.01, (2e-4, -1e-4))
    inv = R.invert3x3(M)
    np.testing.assert_allclose(inv @ M, np.eye(3), atol=1e-12)
    for flags in (R.INTER_LINEAR, R.INTER_NEAREST):
        a = R.warp_perspective(img, M, (90, 40), flags, 0.5)
        b = R.warp_perspective(img, inv, (90, 40), flags | R.WARP_INVERSE_MAP, 0.5)
        np.testing.assert_array_equal(a, b)


def test_restatement_ecc_recovers_a_known_homography_in_the_documented_direction():
    """template(x) ~ input(W x): with mon(x) = scene(A x) and ref = scene, ECC(ref, mon) returns W = A^-1."""
    n, pad = 320, 32
    big = _scene(n, pad)
    A = _homography()
    T = np.array([[1, 0, pad], [0, 1, pad], [0, 0, 1.0]])
    ref = big[pad:pad + n, pad:pad + n]
    mon = R.warp_perspective(big, T @ A, (n, n), R.INTER_LINEAR | R.WARP_INVERSE_MAP)
    cc, W, it = R.find_transform_ecc(R.sobel_magnitude(ref), R.sobel_magnitude(mon), np.eye(3, dtype=np.float32), (3, 200, 1e-6),
                                     None, 5, return_iters=True)
    assert cc > 0.99 and 1 < it < 200
    err = np.abs(_corners(W.astype(float), n) - _corners(np.linalg.inv(A), n)).max()
    assert err <= 0.05, err
    assert np.abs(_corners(W.astype(float), n) - _corners(A, n)).max() > 1.0


def test_reference_composition_applies_the_residual_in_the_opposite_direction():
    """_refine_with_ecc composes residual @ init.  On a pure translation the mon -> ref map is t, the ECC residual from
    init = I is W = t^-1 (the test above), so the reference's final is t^-1 and W^-1 @ init would be t: documented in
    INTEGRATION.md section 6; the mirror keeps the reference's arithmetic."""
    n, pad = 256, 32
    big = _scene(n, pad, seed=7)
    t = np.array([[1, 0, 1.5], [0, 1, -2.25], [0, 0, 1.0]])       # mon -> ref: ref(x) = mon(x - (1.5, -2.25))
    ref = big[pad:pad + n, pad:pad + n]
    mon = R.warp_perspective(big, np.array([[1, 0, pad + 1.5], [0, 1, pad - 2.25], [0, 0, 1.0]]), (n, n),
                             R.INTER_LINEAR | R.WARP_INVERSE_MAP)   # mon(x) = scene(x + (1.5, -2.25))
    (final, cc, _it, _nv, status, residual), = R.refine_ecc_candidates(mon, ref, [np.eye(3)])
    assert status == R.ST_CONVERGED and cc > 0.9
    assert np.abs(final[:2, 2] - (-t[:2, 2])).max() < 0.05            # what the reference returns
    assert np.abs(np.linalg.inv(residual.astype(float))[:2, 2] - t[:2, 2]).max() < 0.05


# ---- the glue of karios_amd.matcher.global_align with ops replaced by the restatement --------------------------------------
@pytest.fixture
def restated(monkeypatch):
    monkeypatch.setattr(ops, "refine_ecc_candidates", lambda mon, ref, inits, it=200, eps=1e-6, ctx=None:
                        R.refine_ecc_candidates(mon, ref, inits, it, eps))
    monkeypatch.setattr(ops, "warp_perspective", lambda src, M, dsize, flags=1, border_value=0.0, ctx=None:
                        R.warp_perspective(src, M, dsize, flags, border_value))
    monkeypatch.setattr(ops, "sobel_magnitude", lambda img, ctx=None: R.sobel_magnitude(img))
    from karios_amd.matcher import global_align
    return global_align


def test_glue_refine_with_ecc_composes_like_the_reference(restated):
    n, pad = 192, 32
    big = _scene(n, pad, seed=11)
    ref = big[pad:pad + n, pad:pad + n]
    mon = R.warp_perspective(big, np.array([[1, 0, pad + 0.75], [0, 1, pad + 0.5], [0, 0, 1.0]]), (n, n), R.INTER_LINEAR | 16)
    init = np.array([[1, 0, -0.5], [0, 1, -0.25], [0, 0, 1.0]])
    m, cc = restated._refine_with_ecc(mon, ref, init)
    (final, cc_r, _i, _v, _s, residual), = R.refine_ecc_candidates(mon, ref, [init])
    np.testing.assert_array_equal(m, residual.astype(np.float64) @ init.astype(np.float64))
    np.testing.assert_array_equal(m, final)
    assert cc == cc_r


def test_glue_skip_below_1000_valid_pixels_and_anticorrelation_raises(restated):
    rng = np.random.default_rng(3)
    ref = rng.integers(1, 255, (96, 96), dtype=np.uint8)
    far = np.array([[1, 0, 90.0], [0, 1, 90.0], [0, 0, 1]])            # 6 x 6 valid pixels left: skipped
    m, cc = restated._refine_with_ecc(ref, ref, far)
    assert m is None and np.isnan(cc)
    t = R.sobel_magnitude(ref)
    with pytest.raises(R.EccNoConvergence):   # anti-correlated: lambda_d <= 0 at the first iteration
        R.find_transform_ecc(t, np.float32(1) - t, np.eye(3, dtype=np.float32), (3, 200, 1e-6))


def test_glue_no_convergence_gives_none_nan(monkeypatch, restated):
    monkeypatch.setattr(ops, "refine_ecc_candidates", lambda mon, ref, inits, it=200, eps=1e-6, ctx=None:
                        [(None, float("nan"), 0, 5000, _lib.ECC_NO_CONVERGENCE, None)])
    m, cc = restated._refine_with_ecc(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8), np.eye(3))
    assert m is None and np.isnan(cc)


def test_glue_candidate_selection_is_strict_and_keeps_ransac_when_nothing_converges(monkeypatch, restated):
    a, b = np.eye(3), np.diag([1.0, 1.0, 1.0]) + np.array([[0, 0, 0.5], [0, 0, 0], [0, 0, 0]])
    res = np.eye(3, dtype=np.float32)
    S = _lib.ECC_CONVERGED

    def fake(scores):
        return lambda mon, ref, inits, it=200, eps=1e-6, ctx=None: [
            (None, float("nan"), 0, 0, _lib.ECC_NO_CONVERGENCE, None) if s is None else (None, s, 3, 5000, S, res) for s in scores]
    img = np.zeros((8, 8), np.uint8)
    monkeypatch.setattr(ops, "refine_ecc_candidates", fake([0.8, 0.8]))
    al = restated.refine_global_alignment(img, img, a, 40, 50, prior=b)
    assert al.matrix is al.candidates[0][1] and [c[0] for c in al.candidates] == ["RANSAC", "prior"]   # tie: the first stays
    monkeypatch.setattr(ops, "refine_ecc_candidates", fake([0.7, 0.8]))
    al = restated.refine_global_alignment(img, img, a, 40, 50, prior=b)
    np.testing.assert_array_equal(al.matrix, res.astype(np.float64) @ b)
    monkeypatch.setattr(ops, "refine_ecc_candidates", fake([None, None]))
    al = restated.refine_global_alignment(img, img, a, 40, 50, prior=b)
    assert al.matrix is a and al.candidates == [] and al.score == 0.8


def test_glue_render_skips_candidates_close_to_the_chosen_matrix(restated):
    rng = np.random.default_rng(9)
    mon = rng.integers(0, 4000, (40, 50)).astype(np.uint16)
    ref = np.zeros((36, 44), np.uint16)
    chosen = _homography(1.25, -0.5, 0.3, 1.001, (1e-5, 0))
    al = restated.GlobalAlignment(chosen, 10, 12, [("RANSAC", chosen + 1e-12, 0.9), ("prior", chosen + 0.01, 0.8)])
    mask = (mon > 2000).astype(np.uint8)
    out, out_mask, alts = restated.render_global_alignment(mon, ref, mask, al)
    np.testing.assert_array_equal(out, R.warp_perspective(mon.astype(np.float32), chosen, (44, 36), 1, 0.0).astype(np.uint16))
    np.testing.assert_array_equal(out_mask, R.warp_perspective(mask, chosen, (44, 36), 0, 0))
    assert list(alts) == ["prior"]
    np.testing.assert_array_equal(alts["prior"], R.warp_perspective(mon.astype(np.float32), (chosen + 0.01).astype(np.float32),
                                                                    (44, 36), 1, 0.0).astype(np.uint16))


def test_decompose_string():
    from karios_amd.matcher.global_align import _decompose
    assert _decompose(np.eye(3)) == "rot=+0.000°  sx=1.0000 sy=1.0000  tx=+0.00 ty=+0.00  persp=0.000000"


def test_restatement_positions_are_block_relative():
    """WarpPerspectiveInvoker computes X0 at the first column of a 64-column block and adds M[0] * x1: for this matrix that
    rounds differently from the absolute position at hundreds of pixels, so the GPU case using it pins the block rule."""
    M = np.array([[0.9, 0.0, -51.784375], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    sx, sy, fx, fy = R.warp_taps(M, 20, 260, True)
    x = np.arange(260, dtype=np.float64)[None, :]
    absolute = np.rint((0.9 * x + -51.784375) * 32.0).astype(np.int64)
    assert ((sx * 32 + fx) != absolute).sum() > 100


def test_prior_from_georefs():
    from karios_amd.matcher.global_align import _prior_from_georefs

    class SR:
        def __init__(self, same):
            self.same = same

        def IsSame(self, other):
            if self.same is None:
                raise RuntimeError("no CRS")
            return self.same

    class Img:
        def __init__(self, proj, sr, x_res, y_res, x_min, y_max):
            self.projection, self.spatial_ref = proj, sr
            self.x_res, self.y_res, self.x_min, self.y_max = x_res, y_res, x_min, y_max
    ref = Img("EPSG:32631", SR(True), 10.0, -10.0, 300000.0, 5000000.0)
    mon = Img("EPSG:32631", SR(True), 20.0, -20.0, 300040.0, 4999970.0)
    np.testing.assert_array_equal(_prior_from_georefs(mon, ref), [[2.0, 0, 4.0], [0, 2.0, 3.0], [0, 0, 1]])
    assert _prior_from_georefs(Img("", SR(True), 10, -10, 0, 0), ref) is None
    assert _prior_from_georefs(Img("x", SR(False), 10, -10, 0, 0), ref) is None
    assert _prior_from_georefs(Img("x", SR(None), 10, -10, 0, 0), ref) is None

