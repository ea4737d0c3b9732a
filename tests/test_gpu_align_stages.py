"""findTransformECC's stages on the MI355X, one by one, against the numpy restatement (tests/align_restatement.py) through
ops.ecc_stages: the blurred template and the {image, gx, gy, pre-mask} plane bit for bit; the 66 sums of an iteration against
their exactly rounded value within the bound every summation order obeys; the host algebra of a step and the whole loop bitwise
on the GPU's own sums.  tests/test_align_host.py proves on the CPU that the inputs (tests/align_cases.py) reach the edges they
are there for."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_cases as A  # noqa: E402
import align_restatement as R  # noqa: E402

from karios_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu

IDENTITY = np.eye(3, dtype=np.float32)
ONE_ITERATION = (ops.TERM_CRITERIA_COUNT, 1, 0.0)


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))   # bitwise, signed zeros included


def _same_but_nan(a, b):
    """NaN at the same places (its payload and sign are not defined by IEEE arithmetic), every other element bitwise"""
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    np.testing.assert_array_equal(a.view(np.uint32)[ok], b.view(np.uint32)[ok])


# ---- a. the prepared planes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("shapes", A.STAGE_SHAPES, ids=str)
def test_prepared_planes_bit_identical(shapes, dtype, masked):
    t, i = A.stage_images(shapes, dtype)
    mask = A.stage_mask(shapes[1]) if masked else None
    t_blur, plane, _ = ops.ecc_stages(t, i, IDENTITY, mask)
    et, ei, egx, egy, epm = A.prepared(shapes, dtype, masked)
    _same(t_blur, et)
    for ch, exp in enumerate((ei, egx, egy, epm.astype(np.float32))):
        _same(np.ascontiguousarray(plane[..., ch]), exp)
    if masked and min(shapes[1]) >= A.EDGE_MASK_MIN:
        # the decision edge of the pre-mask (asserted on the restatement alone in test_align_host.py): 244/256 -> 1, 243/256 -> 0
        one, zero = A.edge_sites(shapes[1])
        assert plane[one][3] == 1.0 and plane[zero][3] == 0.0


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shapes", [A.STAGE_SHAPES[3], A.STAGE_SHAPES[5], A.STAGE_SHAPES[7]], ids=str)
def test_prepared_planes_of_denormals_infinities_and_nan(shapes, masked):
    """the build keeps denormals: a blur or gradient flushed to zero differs from the restatement in its bits"""
    t, i = A.special_f32(shapes[0], 3), A.special_f32(shapes[1], 4)
    mask = A.stage_mask(shapes[1]) if masked else None
    t_blur, plane, _ = ops.ecc_stages(t, i, IDENTITY, mask)
    with np.errstate(all="ignore"):
        et, ei, egx, egy, epm = R.ecc_prepare(t, i, mask)
    if t.size >= 64:
        tiny = np.abs(et[np.isfinite(et)])
        assert ((tiny > 0) & (tiny < np.finfo(np.float32).tiny)).any()            # denormal results exist
    _same_but_nan(t_blur, et)
    for ch, exp in enumerate((ei, egx, egy, epm.astype(np.float32))):
        _same_but_nan(np.ascontiguousarray(plane[..., ch]), exp)


# ---- b. the 66 sums -----------------------------------------------------------------------------------------------------------
def _check_sums(shapes, name):
    t, i = A.stage_images(shapes, "float32")
    mask, mp = A.stage_mask(shapes[1]) if A.sums_masked(shapes) else None, A.sums_maps(shapes)[name]
    exact, bound, _ = A.exact_sums(shapes, name)
    got = ops.ecc_stages(t, i, mp, mask)[2]
    assert got.shape == (66,) and got.dtype == np.float64
    for k in range(66):
        print(f"sum {k}: got {got[k]!r} exact {exact[k]!r} |diff| {abs(got[k] - exact[k]):.3e} bound {bound[k]:.3e}")
    assert got[0] == exact[0]                                                      # N: an integer count
    bad = [k for k in range(66) if not abs(got[k] - exact[k]) <= bound[k]]
    assert not bad, bad
    again = ops.ecc_stages(t, i, mp, mask)[2]
    np.testing.assert_array_equal(again.view(np.uint64), got.view(np.uint64))


@pytest.mark.parametrize("name", ["identity", "subpixel", "outside", "den_sign"])
@pytest.mark.parametrize("shapes", A.STAGE_SHAPES, ids=str)
def test_sums_against_the_exact_sum(shapes, name):
    _check_sums(shapes, name)


def test_sums_against_the_exact_sum_grid_stride():
    _check_sums(A.GRID_STRIDE_SHAPE, "subpixel")


def test_sums_against_the_exact_sum_at_saturated_positions():
    """positions beyond the short range saturate to column 32767, a pixel of this input: it counts in N and in every sum"""
    _check_sums(A.WIDE_INPUT_SHAPE, "sat_short")


# ---- c. the host algebra of one iteration on the GPU's own sums ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.step_cases()))
def test_one_iteration_is_the_restated_step_on_the_gpu_sums(name):
    t, i, mask, m0 = A.step_cases()[name]
    sums = ops.ecc_stages(t, i, m0, mask)[2]
    try:
        exp = R.ecc_step(sums, m0)
    except R.EccNoConvergence:
        exp = None
    assert (exp is None) == (name in ("anticorrelated", "flat"))
    if exp is None:
        with pytest.raises(_lib.KariosHipError) as e:
            ops.find_transform_ecc(t, i, m0, ONE_ITERATION, mask)
        assert e.value.code == _lib.E_NO_CONVERGENCE
        return
    cc, W, it = ops.find_transform_ecc(t, i, m0, ONE_ITERATION, mask, return_iterations=True)
    assert it == 1 and np.float64(cc).view(np.uint64) == np.float64(exp[0]).view(np.uint64)
    _same(W, exp[1])
    if name == "stripes":     # singular Hessian: lu_inv_f32 returns zeros and the map stays
        _same(W, np.asarray(m0, np.float32))


# ---- d. the loop, walked in Python on the GPU's sums ---------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", A.LOOP_SHAPES, ids=str)
def test_loop_walked_on_the_gpu_sums(shapes):
    t, i, mask, init = A.ecc_pair(shapes)
    _, n_it, eps = A.LOOP_CRITERIA
    mp = np.array(init, np.float32)
    rho, last, it = -1.0, -eps, 0
    while it + 1 <= n_it and abs(rho - last) >= eps:          # find_transform_ecc's termination rule
        it += 1
        last = rho
        rho, mp = R.ecc_step(ops.ecc_stages(t, i, mp, mask)[2], mp)
    cc, W, n = ops.find_transform_ecc(t, i, init, A.LOOP_CRITERIA, mask, return_iterations=True)
    assert n == it and 1 < it < 200
    assert np.float64(cc).view(np.uint64) == np.float64(rho).view(np.uint64)
    _same(W, mp)
    assert it == A.loop_reference(shapes)[2]


def test_ecc_stages_argument_checks():
    t, i = A.stage_images(A.STAGE_SHAPES[4], "float32")
    with pytest.raises(_lib.KariosHipError):
        ops.ecc_stages(t, i.astype(np.uint8), IDENTITY)
    with pytest.raises(_lib.KariosHipError):
        ops.ecc_stages(t, i, IDENTITY, np.ones((3, 3), np.uint8))
    c = _lib.default_context()
    sums = np.empty(66)
    rc = c.lib.km_ecc_stages(c.handle, _lib.ptr(t), _lib.ptr(i), _lib.KM_F32, 5, 67, 67, 5, 67, 67, None, 0, _lib.ptr(IDENTITY), None, None,
                             sums.ctypes.data_as(_lib._pd))
    assert rc == _lib.E_ARG
    t_blur, plane = np.empty((5, 67), np.float32), np.empty((5, 67, 4), np.float32)
    rc = c.lib.km_ecc_stages(c.handle, _lib.ptr(t), _lib.ptr(i), _lib.KM_U16, 5, 67, 67, 5, 67, 67, None, 0, _lib.ptr(IDENTITY),
                             _lib.ptr(t_blur), _lib.ptr(plane), sums.ctypes.data_as(_lib._pd))
    assert rc == _lib.E_UNSUPPORTED
    rc = c.lib.km_ecc_stages(c.handle, _lib.ptr(t), _lib.ptr(i), _lib.KM_F32, 5, 67, 67, 5, 67, 67, None, 0, None,
                             _lib.ptr(t_blur), _lib.ptr(plane), sums.ctypes.data_as(_lib._pd))
    assert rc == _lib.E_ARG
