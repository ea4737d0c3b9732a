"""CPU proofs for tests/phase_cases.py, so that a failure of tests/test_gpu_phase_accuracy.py can never be the fixture's fault:
the float64 reference surface against a long-double DFT, the float32 margin tolerance and the conditions that keep it from hiding
a failure, two injected defects that the tolerance must catch at every shape, and the builders' conditions for every committed
(shape, pixel type, seed)."""
import numpy as np
import pytest

import phase_cases as pc


def _dft_matrix(n, sign):
    """exp(sign 2 pi i k m / n) in long double: phases reduced as (k m mod n) in integers, pi from arctan in long double."""
    pi = 4 * np.arctan(np.longdouble(1))
    km = (np.arange(n, dtype=np.int64)[:, None] * np.arange(n, dtype=np.int64)[None, :]) % n
    ang = (2 * pi / np.longdouble(n)) * km.astype(np.longdouble)
    return np.cos(ang) + (1j * sign) * np.sin(ang)


@pytest.mark.parametrize("shape", [(45, 35), (131, 200)])
def test_reference_surface_equals_a_long_double_dft(shape):
    """surface64 (scipy.fft, float64) against the same expression with DFT matrices in long double: <= 1e-13 of the peak
    (measured 2e-15 .. 4e-15), on a margin case with noise - no clean peak."""
    c = pc.pair_with_margin(shape, np.uint16, pc.MARGIN_WINDOW, 0.5, pc.SCENE_SEED.get(shape, 0))
    H, W = shape
    Fh, Fw = _dft_matrix(H, -1), _dft_matrix(W, -1)
    src = Fh @ c.b.astype(np.longdouble) @ Fw
    tgt = Fh @ c.a.astype(np.longdouble) @ Fw
    prod = src * np.conj(tgt)
    prod = prod / np.maximum(np.abs(prod), 100 * np.finfo(np.float64).eps)
    cc = np.abs(np.conj(Fh) @ prod @ np.conj(Fw)) / (H * W)
    dev = float(np.abs(cc - c.cc).max() / cc.max())
    print(f"{shape}: max deviation {dev:.2e} of the peak")
    assert dev <= 1e-13
    assert int(np.argmax(cc)) == c.flat


def test_top2_and_shift_follow_the_library_definition():
    cc = np.array([[1.0, 5.0, 5.0], [0.0, 4.0, 2.0]])
    assert pc.top2(cc) == (1, 5.0, 5.0, 0.0)                        # first arg-max; only the peak's own sample is excluded
    assert pc.top2(np.array([[2.0, 8.0], [6.0, 1.0]]))[1:] == (8.0, 6.0, 0.25)
    np.testing.assert_array_equal(pc.shift_of(5 * 7 + 6, (6, 7)), [-1, -1])
    np.testing.assert_array_equal(pc.shift_of(3 * 7 + 3, (6, 7)), [3, 3])
    np.testing.assert_array_equal(pc.shift_of(4, (1, 7)), [0, -3])
    assert pc.flat_of((-1, -1), (6, 7)) == 41


@pytest.fixture(scope="module")
def tolerances():
    return pc.load_tolerances()


@pytest.mark.parametrize("shape", pc.FAST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_margin_cases_their_tolerance_and_the_injected_defects(shape, tolerances):
    """Every float32-margin case of the shape: the reference margin lies in the window with the peak on the planted shift; the
    committed tolerance is 8 * 2 * max|complex64 surface - float64 surface| / v1 of this very case, at most 1e-3 and a tenth of the
    margin, and the complex64 emulation (a correct float32 FFT) meets it eight times over.  Both injected defects - 0.01 rad phase
    errors, one spectrum column in five dropped - break the bound in at least one case of the shape."""
    caught = {"phase": 0, "columns": 0}
    for c in pc.margin_cases(shape):
        assert pc.MARGIN_WINDOW[0] <= c.margin <= pc.MARGIN_WINDOW[1] and tuple(c.shift) == c.planted[0], c.key
        assert c.a.dtype == c.b.dtype and c.a.shape == shape
        s32 = pc.surface32_emulated(c.b, c.a)
        tol = tolerances[c.key]
        fresh = pc.margin_tolerance(s32, c.cc)
        assert 0.5 * fresh <= tol <= 2.0 * fresh, (c.key, tol, fresh)           # the committed figure is this formula's (FFT builds differ in the last bits)
        assert tol <= 1e-3 and tol <= c.margin / 10, (c.key, tol, c.margin)
        i32, _, _, m32 = pc.top2(s32)
        assert i32 == c.flat and abs(m32 - c.margin) <= tol / 8, (c.key, m32, c.margin, tol)
        for name, defect in (("phase", pc.inject_phase_noise), ("columns", pc.inject_dropped_columns)):
            i, _, _, m = pc.top2(pc.surface32_emulated(c.b, c.a, defect))
            caught[name] += i != c.flat or abs(m - c.margin) > tol
    print(shape, caught)
    assert caught["phase"] >= 1 and caught["columns"] >= 1, caught
    assert len(tolerances) == 8 * len(pc.FAST_SHAPES)


def test_margin_shapes_reach_every_float32_form():
    """The forms of k_fft.hip the shapes and options select (the GPU test runs every one of them)."""
    reached = set()
    for shape in pc.FAST_SHAPES:
        h61, w61 = pc.is_61m(shape[0]), pc.is_61m(shape[1])
        for _, opts in pc.fast_forms(shape):
            on = opts.get("fft61", 1)
            h, w = h61 and on, w61 and on
            fused = h
            herm = h and w and fused and opts.get("fft_herm", 1)
            reached.add(("rows61" if w else "stockham", "cols61" if h else "stockham",
                         "hermitian" if herm else "fused_cross" if fused else "cross_kernel", "top2_rows" if w else "argmax_kernel"))
            if herm:
                reached.add(("hermitian", "odd_rows" if shape[0] % 2 else "even_rows"))
    for want in (("rows61", "cols61", "hermitian", "top2_rows"), ("hermitian", "odd_rows"), ("hermitian", "even_rows"),
                 ("rows61", "cols61", "fused_cross", "top2_rows"),
                 ("stockham", "stockham", "cross_kernel", "argmax_kernel"), ("stockham", "cols61", "fused_cross", "argmax_kernel"),
                 ("rows61", "stockham", "cross_kernel", "top2_rows")):
        assert want in reached, want
    assert pc.is_61m(732) and not pc.is_61m(61) and not pc.is_61m(61 * 61 * 2) and not pc.is_61m(61 * 11)


@pytest.mark.parametrize("shape", pc.DECISION_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decision_cases_lie_on_their_side_of_the_one_percent_rule(shape):
    seen = set()
    for c, path in pc.decision_cases(shape):
        lo, hi = pc.DECIDE_F64_WINDOW if path == 2 else pc.DECIDE_F32_WINDOW
        assert lo <= c.margin <= hi and tuple(c.shift) == c.planted[0], (c.key, c.margin)
        # the complex64 emulation stays on the same side of 1 % with room to spare: the rule's outcome is not a matter of rounding
        m32 = pc.top2(pc.surface32_emulated(c.b, c.a))[3]
        assert (m32 < 0.008) if path == 2 else (m32 > 0.015), (c.key, m32)
        seen.add(path)
    assert seen == {1, 2}


@pytest.mark.parametrize("kind", list(pc.NEAR_TIE_SHAPES))
def test_near_tie_cases_hold_their_conditions(kind):
    """>= 6 near-ties per plan kind: the two planted peaks are the two largest samples 1e-8 .. 2e-6 apart (eight orders above
    float64 error), the third is <= 0.9 of the first, and numpy's FFT agrees with scipy's on the arg-max."""
    shape = pc.NEAR_TIE_SHAPES[kind]
    seeds = pc.near_tie_seeds(shape)
    assert len(seeds) >= 6
    for seed in seeds:
        c = pc.near_tie_pair(shape, seed)
        assert c.a.dtype == np.float32 and c.b.dtype == np.float32
        gap = pc.check_near_tie(c)
        assert pc.NEAR_TIE_GAP[0] <= gap <= pc.NEAR_TIE_GAP[1]
        prod = np.fft.fft2(c.b.astype(np.float64)) * np.fft.fft2(c.a.astype(np.float64)).conj()
        cc = np.abs(np.fft.ifft2(prod / np.maximum(np.abs(prod), 100 * np.finfo(np.float64).eps)))
        assert int(np.argmax(cc)) == c.flat, (kind, seed)


def test_builders_refuse_what_they_cannot_build():
    with pytest.raises(ValueError):
        pc.pair_with_margin((2, 2), np.uint16, pc.MARGIN_WINDOW, 0.0)       # no room for two shifts
    with pytest.raises(ValueError):
        pc.near_tie_pair((244, 183), 4)                                      # the frame's (0, 0) sample outranks the planted peaks
