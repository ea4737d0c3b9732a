"""Both hand-written FFTs of the large-offset pre-aligner on content WITHOUT a clean peak (tests/phase_cases.py; the fixtures and
the tolerances are proven on the CPU by tests/test_phase_cases_host.py):

  * k_fft.hip (float32): shift, `path == 1` and the margin (largest - second largest) / largest against the float64 reference
    surface, within the tolerance derived from a complex64 scipy FFT - in every form the options and shapes select;
  * k_phase.hip: the 1 % rule - float32 answers above it, complex128 decides below it;
  * k_fft64.hip (complex128): the arg-max on near-ties whose two peaks are 1e-8 .. 2e-6 apart, for every plan kind and every
    pair / half / plain form - a transform with float32 accuracy, a chirp with lost phase precision or a mis-indexed Hermitian
    partner picks the wrong peak about every second time;
  * one-pixel-wide, 2 x 2 and odd x odd images in both precisions.
"""
import ctypes as C

import numpy as np
import pytest

import phase_cases as pc

pytestmark = pytest.mark.gpu

F64_FORMS = ((0, 1, 1), (0, 1, 0), (0, 0, 0), (1, 1, 1))          # (f64_plain, f64_pair, f64_half)
DEFAULTS = {"phase_fp64": 0, "fft61": 1, "fft_herm": 1, "f64_plain": 0, "f64_pair": 1, "f64_half": 1}


@pytest.fixture
def ctx(ops):
    """The default context; every option a test may have set is back at its default afterwards."""
    c = ops._lib.default_context()
    try:
        yield c
    finally:
        for name, value in DEFAULTS.items():
            c.set_option(name, value)


@pytest.fixture(scope="module")
def tolerances():
    return pc.load_tolerances()


def _plan(n, along_columns):
    from karios_amd import _lib
    levels = (C.c_int * 32)()
    nl, blue = C.c_int(-1), C.c_int(-1)
    assert _lib.load().km_phase_plan(n, along_columns, levels, 16, C.byref(nl), C.byref(blue), None) == 0
    return [(levels[2 * i], levels[2 * i + 1]) for i in range(nl.value)], blue.value


@pytest.mark.parametrize("shape", pc.FAST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_margin_and_shift_on_split_peaks(ops, ctx, tolerances, shape):
    """uint16 / uint8 / int16 / float32 pixels, sigma 0 and 0.5, reference margin in [0.03, 0.3]: the float32 path answers, with
    the reference's shift and the reference's margin to within tol = 16 max|complex64 surface - float64 surface| / v1 (3e-5 .. 3e-4,
    tests/golden/phase_margin_tolerances.npz) - in the default form, with the Stockham rows instead of the 61 * M rows, with the
    full-plane instead of the Hermitian inverse, wherever the shape has such a form (122 x 96 fuses the cross-power step into
    the first inverse pass, 96 x 122 and the generic shapes run it as a kernel of its own)."""
    forms = pc.fast_forms(shape)
    assert len(forms) == 1 + (pc.is_61m(shape[0]) or pc.is_61m(shape[1])) + (pc.is_61m(shape[0]) and pc.is_61m(shape[1]))
    failures = []
    for case in pc.margin_cases(shape):
        tol = tolerances[case.key]
        for name, opts in forms:
            for k, v in {**DEFAULTS, **opts}.items():
                ctx.set_option(k, v)
            got = ops.phase_cross_correlation(case.b, case.a)
            path, margin = ctx.phase_info()
            print(f"{case.key:36s} {name:22s} path {path} shift {got} margin {margin:.6f} reference {case.margin:.6f} "
                  f"diff {abs(margin - case.margin):.2e} tol {tol:.2e}")
            if path != 1 or not np.array_equal(got, case.shift) or not abs(margin - case.margin) <= tol:
                failures.append((case.key, name, path, got.tolist(), case.shift.tolist(), margin, case.margin, tol))
    assert not failures, failures


@pytest.mark.parametrize("shape", pc.DECISION_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_percent_rule_hands_weak_peaks_to_complex128(ops, ctx, shape):
    """k_phase.hip: a reference margin of 0.1 .. 0.6 % (still eleven orders above float64 error) -> the float32 margin is under 1 %
    and complex128 decides (`path == 2`); 2 .. 20 % -> float32 answers (`path == 1`).  The reference's arg-max either way."""
    for case, want_path in pc.decision_cases(shape):
        got = ops.phase_cross_correlation(case.b, case.a)
        path, margin = ctx.phase_info()
        print(f"{case.key} reference margin {case.margin:.5f}: path {path}, float32 margin {margin:.5f}, shift {got}")
        assert path == want_path, (case.key, path, margin, case.margin)
        np.testing.assert_array_equal(got, case.shift, err_msg=case.key)


PLAN_KINDS = {       # kind -> what km_phase_plan must say about (H along columns, W along rows)
    "smooth": lambda ph, pw: not ph[1] and not pw[1] and all(k == 0 for _, k in ph[0] + pw[0]) and len(ph[0]) == 1 and len(pw[0]) == 1,
    "prime_on_w": lambda ph, pw: not pw[1] and any(k == 1 for _, k in pw[0]) and not ph[1],
    "prime_on_h": lambda ph, pw: not ph[1] and any(k == 1 for _, k in ph[0]) and not pw[1],
    "bluestein_h": lambda ph, pw: ph[1] > 0 and not pw[1],
    "bluestein_w": lambda ph, pw: pw[1] > 0 and not ph[1],
    "bluestein_both": lambda ph, pw: ph[1] > 0 and pw[1] > 0,
    "two_column_levels": lambda ph, pw: not ph[1] and len(ph[0]) == 2 and all(k == 0 for _, k in ph[0]),
    "long_rows": lambda ph, pw: not pw[1] and len(pw[0]) == 2 and all(k == 0 for _, k in pw[0]),
}


@pytest.mark.parametrize("kind", list(pc.NEAR_TIE_SHAPES))
def test_complex128_picks_the_larger_of_two_peaks_one_part_in_ten_million_apart(ops, ctx, kind):
    """k_fft64.hip on six near-ties per plan kind (two planted peaks 1e-8 .. 2e-6 apart, float32 pixels): the reference's arg-max
    in every (f64_plain, f64_pair, f64_half) form under `phase_fp64`, and again without it - the float32 margin is ~0 there, so the
    1 % rule must hand the pair to complex128 (`path == 2`) with the same answer."""
    shape = pc.NEAR_TIE_SHAPES[kind]
    ph, pw = _plan(shape[0], 1), _plan(shape[1], 0)
    assert PLAN_KINDS[kind](ph, pw), (kind, ph, pw)
    wrong = []
    for seed in pc.near_tie_seeds(shape):
        case = pc.near_tie_pair(shape, seed)
        other = [s for s in case.planted if tuple(case.shift) != s]
        for plain, pair, half in F64_FORMS:
            for k, v in (("phase_fp64", 1), ("f64_plain", plain), ("f64_pair", pair), ("f64_half", half)):
                ctx.set_option(k, v)
            got = ops.phase_cross_correlation(case.b, case.a)
            assert ctx.phase_info()[0] == 2
            if not np.array_equal(got, case.shift):
                wrong.append((case.key, (plain, pair, half), got.tolist(), case.shift.tolist(), other))
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)
        got = ops.phase_cross_correlation(case.b, case.a)
        path, margin = ctx.phase_info()
        assert path == 2 and margin < 0.01, (case.key, path, margin)
        if not np.array_equal(got, case.shift):
            wrong.append((case.key, "phase_fp64=0", got.tolist(), case.shift.tolist(), other))
    assert not wrong, wrong


def _noisy_shifted_pair(shape, dtype, seed):
    """One crop and a shifted crop of the same scene with noise (sigma 0.5) - sides too small for two planted shifts."""
    H, W = shape
    base = pc._scene(H, W, 77 + seed)
    rng = np.random.default_rng([H, W, seed])
    s = (0 if H == 1 else int(rng.integers(1, max(2, min(30, H // 8) + 1))), 0 if W == 1 else -int(rng.integers(1, max(2, min(30, W // 8) + 1))))
    a = pc._cast(pc._in_pixel_units(pc._crop(base, H, W, (0, 0)), dtype), dtype)
    b = pc._cast(pc._in_pixel_units(pc._crop(base, H, W, s) + 0.5 * float(base.std()) * rng.standard_normal(shape), dtype), dtype)
    return a, b


@pytest.mark.parametrize("shape", [(1, 300), (300, 1), (1, 61), (2, 2), (3, 5), (45, 35)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sides_at_the_edges_of_the_rule_in_both_precisions(ops, ctx, shape):
    """W = 1 or H = 1: complex128 only (`path == 2` whatever the options say); 2 x 2, 3 x 5 and an odd x odd pair with noise: the
    float32 path runs and answers unless its margin is under 1 %.  The reference's arg-max wherever the reference margin is not
    itself a matter of rounding (> 1e-6), from both precisions."""
    for seed, dtype in enumerate(pc.DTYPES):
        a, b = _noisy_shifted_pair(shape, dtype, seed)
        cc = pc.surface64(b, a)
        flat, _, _, ref_margin = pc.top2(cc)
        want = pc.shift_of(flat, shape)
        for fp64 in (0, 1):
            ctx.set_option("phase_fp64", fp64)
            got = ops.phase_cross_correlation(b, a)
            path, margin = ctx.phase_info()
            print(f"{shape} {np.dtype(dtype).name} phase_fp64 {fp64}: path {path} margin {margin:.5f} reference {ref_margin:.5f} shift {got} want {want}")
            if fp64 or min(shape) == 1:
                assert path == 2
            elif ref_margin >= 0.02:
                assert path == 1, (shape, dtype, path, margin, ref_margin)
            elif ref_margin <= 0.006:
                assert path == 2
            if ref_margin > 1e-6:
                np.testing.assert_array_equal(got, want, err_msg=f"{shape} {np.dtype(dtype).name} phase_fp64={fp64}")
        ctx.set_option("phase_fp64", 0)
