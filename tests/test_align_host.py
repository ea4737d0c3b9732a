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



# ---- the inputs of the stage and degenerate-warp GPU tests (tests/align_cases.py) do what they are there for ------------------------
import align_cases as A  # noqa: E402


@pytest.mark.parametrize("name", list(A.warp_cases()))
def test_warp_case_reaches_the_rule_it_is_listed_for(name):
    A.check_warp_case(name)


def test_special_float_source_holds_every_special_value():
    a = A.warp_source((33, 41), np.float32, "special")
    tiny = np.finfo(np.float32).tiny
    assert np.isnan(a).any() and (a == np.inf).any() and (a == -np.inf).any() and (a == A.FLT_MAX).any() and (a == -A.FLT_MAX).any()
    assert ((a != 0) & (np.abs(a) < tiny)).any() and (np.signbit(a) & (a == 0)).any() and a.strides[0] > a.shape[1] * 4


@pytest.mark.parametrize("shapes", [s for s in A.STAGE_SHAPES if min(s[1]) >= A.EDGE_MASK_MIN], ids=str)
def test_stage_mask_hits_both_sides_of_the_premask_rounding(shapes):
    m = A.stage_mask(shapes[1])
    valid = m[m > 0]
    assert (m == 0).any() and not m[0].any() and not m[:, :2].any() and ((valid != 255).any() and len(np.unique(valid)) > 2)
    blur = R.gauss5((m > 0).astype(np.float32))
    pm = R.ecc_premask(m, m.shape)
    one, zero = A.edge_sites(shapes[1])
    assert blur[one] == np.float32(244 / 256) and pm[one] == 1 and blur[zero] == np.float32(243 / 256) and pm[zero] == 0
    k = np.float32(0.5 / 0.95)
    assert np.float32(243 / 256) * k < 0.5 < np.float32(244 / 256) * k       # no value of the n / 256 grid lies between them
    assert pm.min() == 0 and pm.max() == 1 and pm.dtype == np.uint8


@pytest.mark.parametrize("shapes", A.LOOP_SHAPES, ids=str)
def test_loop_cases_converge_inside_the_iteration_cap(shapes):
    cc, mp, it = A.loop_reference(shapes)
    assert 1 < it < 200 and cc > 0.9


def test_step_cases_are_what_they_are_named():
    for name, (t, i, mask, mp) in A.step_cases().items():
        s = R.ecc_sums(*R.ecc_prepare(t, i, mask), mp)
        H = np.zeros((8, 8), np.float32)
        H[np.triu_indices(8)] = s[6:42]
        H = H + np.triu(H, 1).T
        singular = not R.lu_inv_f32(H).any()
        if name in ("anticorrelated", "flat"):
            with pytest.raises(R.EccNoConvergence, match="minimized" if name == "anticorrelated" else "NaN"):
                R.ecc_step(s, mp)
        else:
            rho, new = R.ecc_step(s, mp)
            assert 0.5 < rho < 1 and np.array_equal(new, np.asarray(mp, np.float32)) == (name == "stripes")
        assert singular == (name in ("flat", "stripes")), name


SUMS_HOST_SHAPES = [A.STAGE_SHAPES[6], A.STAGE_SHAPES[7]]


@pytest.mark.parametrize("name", ["identity", "subpixel", "outside", "den_sign"])
@pytest.mark.parametrize("shapes", SUMS_HOST_SHAPES, ids=str)
def test_numpy_order_sums_lie_inside_the_exact_sum_bound_and_one_pixel_does_not(shapes, name):
    exact, bound, numpy_order = A.exact_sums(shapes, name)
    assert np.isfinite(exact).all() and (np.abs(numpy_order - exact) <= bound).all()
    assert (np.abs(numpy_order - exact) <= 0.05 * bound).all()               # far inside: the bound is no tight fit to one order
    terms = R.ecc_terms(*A.prepared(shapes, "float32", True), A.sums_maps(shapes)[name])
    n_valid = int(exact[0])
    (hs, ws), (hd, wd) = shapes
    assert n_valid == terms[0].sum()
    assert 0 < n_valid < 40 if name == "outside" else n_valid > (100 if name == "den_sign" else hs * ws // 4)
    if name == "den_sign":
        den = A.jacobian_den(shapes, A.sums_maps(shapes)[name])
        assert (den > 0).any() and (den < 0).any() and (den != 0).all()
    for k in range(66):                                                        # leaving one median pixel out is far outside the bound
        mag = np.abs(terms[k][terms[k] != 0])
        assert mag.size and np.median(mag) > 1e4 * bound[k], (k, np.median(mag), bound[k])


def test_wide_input_sums_case_counts_pixels_at_the_saturated_position():
    shapes = A.WIDE_INPUT_SHAPE
    (hs, ws), (hd, wd) = shapes
    mp = A.sums_maps(shapes)["sat_short"]
    sx, sy, fx, fy = R.warp_taps(mp.astype(np.float64), hs, ws, True)
    nx, ny = R.warp_taps(mp.astype(np.float64), hs, ws, False)
    assert wd > 32768 and (sx == 32767).sum() == (nx == 32767).sum() == hs * (ws - 34) and (sx == -32768).any()
    exact, bound, numpy_order = A.exact_sums(shapes, "sat_short")
    assert exact[0] == (sx >= 0).sum() == hs * (ws - 33) and (np.abs(numpy_order - exact) <= bound).all()    # N: column 33 and the saturated ones
    terms = R.ecc_terms(*A.prepared(shapes, "float32", False), mp)
    assert (terms[1][sx == 32767] != 0).all()                                 # ... each with the image's value at column 32767


def test_ecc_sums_is_the_numpy_sum_of_ecc_terms():
    shapes = A.STAGE_SHAPES[5]
    parts = A.prepared(shapes, "float32", True)
    mp = A.sums_maps(shapes)["subpixel"]
    terms = R.ecc_terms(*parts, mp)
    assert len(terms) == 66 and all(t.shape == shapes[0] and t.dtype == np.float64 for t in terms)
    np.testing.assert_array_equal(R.ecc_sums(*parts, mp), [t.sum() for t in terms])
    m, T = terms[0], parts[0].astype(np.float64)
    assert set(np.unique(m)) <= {0.0, 1.0}
    np.testing.assert_array_equal(terms[3], m * T)
    np.testing.assert_array_equal(terms[4], m * T * T)


def _pad101(a, r):
    for axis in (0, 1):
        pad = [(0, 0), (0, 0)]
        pad[axis] = (r, r)
        a = np.pad(a, pad, mode="reflect" if a.shape[axis] > 1 else "edge")
    return a


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 2), (5, 67), (13, 29)])
def test_gauss5_is_the_5x5_binomial_correlation_with_reflect_101(shape):
    """on integer images every float32 step of R.gauss5 is exact, so it must equal the plain fp64 correlation"""
    a = np.random.default_rng(shape[0] * 100 + shape[1]).integers(0, 256, shape).astype(np.float64)
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    p = _pad101(a, 2)
    exp = np.zeros(shape)
    for dy in range(5):
        for dx in range(5):
            exp += k[dy] * k[dx] * p[dy:dy + shape[0], dx:dx + shape[1]]
    got = R.gauss5(a.astype(np.float32))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.astype(np.float64), exp)


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 2), (13, 29)])
def test_ecc_gradients_are_plain_central_differences_times_the_premask(shape):
    rng = np.random.default_rng(shape[0] * 10 + shape[1])
    a = (rng.random(shape) * 255).astype(np.float32)
    pm = (rng.random(shape) < 0.7).astype(np.uint8)
    p = _pad101(a.astype(np.float64), 1)
    H, W = shape
    ex = (p[1:1 + H, 2:2 + W] - p[1:1 + H, 0:W]) / 2 * pm        # exact in fp64, one rounding to float32
    ey = (p[2:2 + H, 1:1 + W] - p[0:H, 1:1 + W]) / 2 * pm
    gx, gy = R.ecc_gradients(a, pm)
    assert gx.dtype == gy.dtype == np.float32
    np.testing.assert_array_equal(gx, ex.astype(np.float32))
    np.testing.assert_array_equal(gy, ey.astype(np.float32))


def _plain_sobel_sq(img):
    p = _pad101(np.asarray(img, np.int64), 1)
    H, W = img.shape
    s = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]   # noqa: E731
    gx = (s(-1, 1) - s(-1, -1)) + 2 * (s(0, 1) - s(0, -1)) + (s(1, 1) - s(1, -1))
    gy = (s(1, -1) - s(-1, -1)) + 2 * (s(1, 0) - s(-1, 0)) + (s(1, 1) - s(-1, 1))
    return gx * gx + gy * gy


def test_sobel_extreme_patterns_reach_the_largest_gradient_and_the_last_workgroup():
    img, at = A.sobel_extreme()
    sq = _plain_sobel_sq(img)
    assert sq.max() == 1020 ** 2 + 510 ** 2 == sq[at] and set(np.unique(img)) == {0, 255}     # the largest gx^2 + gy^2 of 8-bit pixels
    out = R.sobel_magnitude(img)
    assert out[at] == 1.0 and out.max() == 1.0
    np.testing.assert_array_equal(out, np.sqrt(sq.astype(np.float32)) / np.float32(np.sqrt(np.float32(sq.max()))))
    last = A.sobel_last_pixel()
    H, W = last.shape
    sq = _plain_sobel_sq(last)
    ys, xs = np.nonzero(sq)
    assert ys.size and (ys >= (H - 1) // 4 * 4).all() and (xs >= (W - 1) // 64 * 64).all()     # only the last 4 x 64 workgroup sees it
