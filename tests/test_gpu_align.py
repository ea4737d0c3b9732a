"""Global align step on the MI355X against the numpy restatement (tests/align_restatement.py): warps and the Sobel magnitude bit
for bit, findTransformECC / _refine_with_ecc to fp64 summation order (same iteration count, maps within 1e-3 px at the template
corners, cc within 1e-6), bitwise identical run to run."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_cases as A  # noqa: E402
import align_restatement as R  # noqa: E402

import ctypes as C  # noqa: E402

from karios_amd import _lib, ops, synth  # noqa: E402

pytestmark = pytest.mark.gpu


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


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))   # bitwise, NaN and signed zeros included


CASES = [  # (src H, W, dst H, W, matrix)
    (97, 131, 70, 150, _homography(-20.5, 13.25, 7.0, 1.07, (3e-4, -2e-4))),
    (64, 64, 64, 64, _homography(0.4, -0.3, 0.0, 1.0, (0, 0))),
    (200, 257, 211, 193, _homography(35.0, -41.0, -12.0, 0.93, (-1e-4, 5e-4))),
    (33, 5, 17, 9, _homography(1.5, 2.5, 20.0, 1.3, (1e-3, 0))),
    (40, 400, 5, 300, _homography(150.25, 10.5, 3.0, 1.02, (1e-4, 0))),      # dH < 16: blocks of 1024 / 5 = 204 columns
    (30, 260, 20, 260, np.array([[0.9, 0.0, -51.784375], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])),   # block-relative != absolute rounding
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_warp_perspective_bit_identical(case, dtype):
    sH, sW, dH, dW, M = CASES[case]
    rng = np.random.default_rng(case)
    big = (rng.random((sH + 3, sW + 7)) * 255).astype(dtype)
    src = big[1:1 + sH, 2:2 + sW]                        # strided input
    for flags in (ops.INTER_LINEAR, ops.INTER_NEAREST):
        for inv in (0, ops.WARP_INVERSE_MAP):
            for border in (0.0, 7.3, float("nan")):
                got = ops.warp_perspective(src, M, (dW, dH), flags | inv, border)
                exp = R.warp_perspective(src, M, (dW, dH), flags | inv, border)
                _same(got, exp)


def _same_but_nan(a, b):
    """NaN at the same places (its payload and sign are not defined by IEEE arithmetic), every other element bitwise"""
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    np.testing.assert_array_equal(a.view(np.uint32)[ok], b.view(np.uint32)[ok])


def _warp_both_ways(src, M, dsize, inverse_flags=(0, ops.WARP_INVERSE_MAP), same=_same):
    for flags in (ops.INTER_LINEAR, ops.INTER_NEAREST):
        for inv in inverse_flags:
            for border in (0.0, 7.3, float("nan")):
                got = ops.warp_perspective(src, M, dsize, flags | inv, border)
                with np.errstate(all="ignore"):
                    exp = R.warp_perspective(src, M, dsize, flags | inv, border)
                (same if border == border or src.dtype == np.uint8 else _same_but_nan)(got, exp)


@pytest.mark.parametrize("name", list(A.warp_cases()))
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_warp_perspective_where_the_edge_rules_bite(name, dtype):
    """W == 0 and W < 0, singular and all-zero matrices, positions beyond the int and the short range, non-finite entries, exact
    ties on the 1/32 grid, taps astride the source's edges, tiny sources and destinations: tests/align_cases.py, each with the
    condition it is there for (also asserted on the CPU in test_align_host.py)"""
    A.check_warp_case(name)
    (sH, sW), (dH, dW), M, inv, _ = A.warp_cases()[name]
    _warp_both_ways(A.warp_source((sH, sW), dtype), M, (dW, dH), (inv,))


@pytest.mark.parametrize("name", ["edges", "w_zero_row", "ties", "src_1x7"])
def test_warp_perspective_float32_specials_and_uint8_full_scale(name):
    (sH, sW), (dH, dW), M, inv, _ = A.warp_cases()[name]
    _warp_both_ways(A.warp_source((sH, sW), np.float32, "special"), M, (dW, dH), (inv,), _same_but_nan)
    _warp_both_ways(A.warp_source((sH, sW), np.uint8, "checker"), M, (dW, dH), (inv,))


def test_warp_perspective_checkerboard_half_pixel_blend():
    """0 / 255 at weights 16/32 x 16/32 and at every other fraction: the 8-bit blend's rounding at full scale"""
    src = A.warp_source((40, 50), np.uint8, "checker")
    for M in ([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]], [[1 + 1 / 32, 0, -1.25], [0, 1 - 1 / 32, -0.75], [0, 0, 1]]):
        exp = R.warp_perspective(src, np.array(M), (56, 44), R.INTER_LINEAR | R.WARP_INVERSE_MAP, 255.0)
        assert (exp == 128).any() if M[0][0] == 1 else len(np.unique(exp)) > 30    # 127.5 rounds up; many fractions
        _warp_both_ways(src, np.array(M, np.float64), (56, 44), (ops.WARP_INVERSE_MAP,))


def test_warp_perspective_float32_matrix_and_dev_entry_point():
    import torch
    src = (np.random.default_rng(1).random((300, 400)) * 4000).astype(np.float32)
    M = _homography(3.3, -7.1, 0.4, 1.0003, (2e-7, -1e-7)).astype(np.float32)
    exp = R.warp_perspective(src, M, (380, 290), ops.INTER_LINEAR, -1.0)
    _same(ops.warp_perspective(src, M, (380, 290), ops.INTER_LINEAR, -1.0), exp)
    c = _lib.default_context()
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.empty((290, 384), dtype=torch.float32, device="cuda")
    m = np.ascontiguousarray(M, np.float64)
    import ctypes as C
    torch.cuda.synchronize()
    c.check(c.lib.km_warp_perspective_dev(c.handle, C.c_void_p(d_src.data_ptr()), _lib.KM_F32, 300, 400, 400, C.c_void_p(d_dst.data_ptr()),
                                          290, 380, 384, 1, 0, -1.0, m.ctypes.data_as(C.POINTER(C.c_double))), "warp_dev")
    c.sync()
    _same(d_dst[:, :380].cpu().numpy().copy(), exp)


@pytest.mark.parametrize("shape", [(64, 64), (129, 77), (1, 9), (512, 700), (9, 1), (1, 1), (2, 2), (4, 65)])
def test_sobel_magnitude_bit_identical(shape):
    img = np.random.default_rng(shape[0]).integers(0, 256, shape, dtype=np.uint8)
    _same(ops.sobel_magnitude(img), R.sobel_magnitude(img))
    flat = np.full(shape, 7, np.uint8)
    _same(ops.sobel_magnitude(flat), R.sobel_magnitude(flat))


def test_sobel_magnitude_largest_gradient_and_maximum_in_the_last_workgroup():
    img, at = A.sobel_extreme()                  # gx^2 + gy^2 = 1020^2 + 510^2 at `at` (test_align_host.py)
    got = ops.sobel_magnitude(img)
    assert got[at] == 1.0
    _same(got, R.sobel_magnitude(img))
    last = A.sobel_last_pixel()
    got = ops.sobel_magnitude(last)
    assert got.max() == 1.0 and got[-1, -2] > 0
    _same(got, R.sobel_magnitude(last))


def _pair(n, A, pad=32, seed=20260101):
    big = _scene(n, pad, seed)
    T = np.array([[1, 0, pad], [0, 1, pad], [0, 0, 1.0]])
    return big[pad:pad + n, pad:pad + n], R.warp_perspective(big, T @ A, (n, n), R.INTER_LINEAR | R.WARP_INVERSE_MAP)


@pytest.mark.parametrize("n", [512, 2048])
def test_find_transform_ecc_matches_restatement_and_recovers_the_warp(n):
    A = _homography()
    ref, mon = _pair(n, A)
    t, i = R.sobel_magnitude(ref), R.sobel_magnitude(mon)
    mask = (mon > 0).astype(np.uint8) * 255
    crit = (3, 200, 1e-6)
    cc, W, it = ops.find_transform_ecc(t, i, np.eye(3, dtype=np.float32), crit, mask, 5, return_iterations=True)
    cc_r, W_r, it_r = R.find_transform_ecc(t, i, np.eye(3, dtype=np.float32), crit, mask, 5, return_iters=True)
    assert it == it_r and 1 < it < 200
    assert abs(cc - cc_r) <= 1e-6
    assert np.abs(_corners(W.astype(float), n) - _corners(W_r.astype(float), n)).max() <= 1e-3
    assert np.abs(_corners(W.astype(float), n) - _corners(np.linalg.inv(A), n)).max() <= 0.05   # template(x) ~ input(W x)
    cc2, W2, it2 = ops.find_transform_ecc(t, i, np.eye(3, dtype=np.float32), crit, mask, 5, return_iterations=True)
    assert (cc2, it2) == (cc, it) and np.array_equal(W2.view(np.uint32), W.view(np.uint32))


def test_find_transform_ecc_no_convergence_where_the_restatement_raises():
    ref, _ = _pair(512, np.eye(3))
    t = R.sobel_magnitude(ref)
    with pytest.raises(R.EccNoConvergence):
        R.find_transform_ecc(t, np.float32(1) - t, np.eye(3, dtype=np.float32), (3, 200, 1e-6))
    with pytest.raises(_lib.KariosHipError) as e:
        ops.find_transform_ecc(t, np.float32(1) - t, np.eye(3, dtype=np.float32), (3, 200, 1e-6))
    assert e.value.code == _lib.E_NO_CONVERGENCE
    with pytest.raises(_lib.KariosHipError) as e:
        ops.find_transform_ecc(t, t, np.eye(3, dtype=np.float32), (3, 200, 1e-6), gauss_filt_size=3)
    assert e.value.code == _lib.E_UNSUPPORTED


def test_refine_ecc_candidates_match_restatement_skip_and_repeat():
    n = 512
    A = _homography(1.75, -2.5, 0.08, 1 + 3e-4, (5e-8, 1e-7))
    ref, mon = _pair(n, A, seed=99)
    inits = [np.eye(3), np.array([[1, 0, 0.5], [0, 1, -0.5], [0, 0, 1.0]]), np.array([[1, 0, 500.0], [0, 1, 500.0], [0, 0, 1]])]
    got = ops.refine_ecc_candidates(mon, ref, inits)
    exp = R.refine_ecc_candidates(mon, ref, inits)
    for g, e in zip(got, exp):
        assert g[4] == e[4] and g[3] == e[3]
        if e[4] == R.ST_CONVERGED:
            assert g[2] == e[2] and abs(g[1] - e[1]) <= 1e-6
            assert np.abs(_corners(g[0], n) - _corners(e[0], n)).max() <= 1e-3
    assert [g[4] for g in got] == [_lib.ECC_CONVERGED, _lib.ECC_CONVERGED, _lib.ECC_SKIPPED]
    again = ops.refine_ecc_candidates(mon, ref, inits)
    for g, h in zip(got, again):
        assert g[1:5] == h[1:5] or (np.isnan(g[1]) and np.isnan(h[1]) and g[2:5] == h[2:5])
        if g[0] is not None:
            assert np.array_equal(g[0], h[0]) and np.array_equal(g[5], h[5])


def test_refine_and_render_global_alignment():
    from karios_amd.matcher import refine_global_alignment, render_global_alignment
    n = 768
    A = _homography(2.0, 1.25, -0.03, 1 - 1e-4, (0, 0))
    ref, mon = _pair(n, A, seed=5)
    ransac = np.array([[1, 0, -1.5], [0, 1, -1.0], [0, 0, 1.0]])
    prior = np.eye(3)
    al = refine_global_alignment(mon, ref, ransac, 30, 40, prior=prior)
    assert len(al.candidates) == 2
    best = max(al.candidates, key=lambda c: c[2])
    assert al.matrix is best[1]
    # from init = I the reference's composition gives the ECC residual W itself, template(x) ~ input(W x): W ~ A^-1
    prior_m = [c[1] for c in al.candidates if c[0] == "prior"][0]
    assert np.abs(_corners(prior_m, n) - _corners(np.linalg.inv(A), n)).max() <= 0.05
    mon16 = (mon.astype(np.uint16) * 40 + 3)
    out, out_mask, alts = render_global_alignment(mon16, ref, (mon > 100).astype(np.uint8), al)
    rows = np.arange(0, n, 97)
    exp = R.warp_perspective(mon16.astype(np.float32), al.matrix, (n, n), R.INTER_LINEAR, 0.0, rows=rows).astype(np.uint16)
    np.testing.assert_array_equal(out[rows], exp)
    exp_m = R.warp_perspective((mon > 100).astype(np.uint8), al.matrix, (n, n), R.INTER_NEAREST, 0, rows=rows)
    np.testing.assert_array_equal(out_mask[rows], exp_m)
    for name, cand, _ in al.candidates:
        if name in alts:
            e = R.warp_perspective(mon16.astype(np.float32), cand.astype(np.float32), (n, n), R.INTER_LINEAR, 0.0, rows=rows)
            np.testing.assert_array_equal(alts[name][rows], e.astype(np.uint16))


# ---- the _dev entry points on strided device buffers, bitwise against the host forms --------------------------------------------
def _vp(t):
    return C.c_void_p(t.data_ptr())


def _strided(torch, a, dy=3, dx=5):
    """device copy of a (rows contiguous, row stride > width): a view into a larger buffer"""
    big = torch.zeros((a.shape[0] + dy, a.shape[1] + dx), dtype=getattr(torch, a.dtype.name), device="cuda")
    v = big[dy:, dx:]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def test_sobel_magnitude_dev_strided_matches_host():
    import torch
    img = np.random.default_rng(4).integers(0, 256, (301, 517), dtype=np.uint8)
    d_img = _strided(torch, img)
    d_out = torch.empty(img.shape, dtype=torch.float32, device="cuda")
    c = _lib.default_context()
    torch.cuda.synchronize()
    c.check(c.lib.km_sobel_magnitude_dev(c.handle, _vp(d_img), img.shape[0], img.shape[1], d_img.stride(0), _vp(d_out)), "sobel_dev")
    c.sync()
    _same(d_out.cpu().numpy(), ops.sobel_magnitude(img))


def test_find_transform_ecc_template_and_input_of_different_sizes():
    """the template covers part of the input: hs x ws != hd x wd; host form against the restatement, _dev form (strided) bitwise"""
    import torch
    big = _scene(640, 0, seed=21)[:600, :640]
    A = _homography(3.25, -1.5, 0.1, 1 + 4e-4, (1e-7, 2e-7))
    inp = big                                                           # 600 x 640
    tmpl = R.warp_perspective(big, np.array([[1, 0, 40.0], [0, 1, 30.0], [0, 0, 1]]) @ A, (520, 480),
                              R.INTER_LINEAR | R.WARP_INVERSE_MAP)      # 480 x 520: tmpl(x) = inp(T A x)
    t, i = R.sobel_magnitude(tmpl), R.sobel_magnitude(inp)
    mask = np.ones(inp.shape, np.uint8)
    mask[:, :7] = 0
    init = np.array([[1, 0, 40.0], [0, 1, 30.0], [0, 0, 1]], np.float32)
    crit = (3, 200, 1e-6)
    cc, W, it = ops.find_transform_ecc(t, i, init, crit, mask, 5, return_iterations=True)
    cc_r, W_r, it_r = R.find_transform_ecc(t, i, init, crit, mask, 5, return_iters=True)
    assert it == it_r and 1 < it < 200 and abs(cc - cc_r) <= 1e-6
    assert np.abs(_corners(W.astype(float), 480) - _corners(W_r.astype(float), 480)).max() <= 1e-3
    exp_w = np.array([[1, 0, 40.0], [0, 1, 30.0], [0, 0, 1]]) @ A
    assert np.abs(_corners(W.astype(float), 480) - _corners(exp_w, 480)).max() <= 0.05
    d_t, d_i, d_m = _strided(torch, t), _strided(torch, i, 1, 9), _strided(torch, mask, 2, 3)
    mp = np.array(init, np.float32)
    cc_d, it_d = C.c_double(), C.c_int()
    c = _lib.default_context()
    torch.cuda.synchronize()
    c.check(c.lib.km_find_transform_ecc_dev(c.handle, _vp(d_t), _vp(d_i), _lib.KM_F32, 480, 520, d_t.stride(0), 600, 640, d_i.stride(0),
                                            _vp(d_m), d_m.stride(0), mp.ctypes.data_as(C.c_void_p), 200, 1e-6, 5, C.byref(cc_d),
                                            C.byref(it_d)), "ecc_dev")
    assert it_d.value == it and cc_d.value == cc and np.array_equal(mp.view(np.uint32), W.view(np.uint32))


def _refine_dev(c, torch, d_mon, d_ref, inits):
    n = len(inits)
    ini = np.ascontiguousarray(np.array(inits, np.float64).reshape(n, 9))
    fin = np.empty((n, 9)); res = np.empty((n, 9), np.float32); cc = np.empty(n)
    it = np.empty(n, np.int32); valid = np.empty(n, np.int64); st = np.empty(n, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    torch.cuda.synchronize()
    c.check(c.lib.km_refine_ecc_candidates_dev(c.handle, _vp(d_mon), d_mon.shape[0], d_mon.shape[1], d_mon.stride(0), _vp(d_ref),
                                               d_ref.shape[0], d_ref.shape[1], d_ref.stride(0), n, P(ini), 200, 1e-6, P(fin), P(res),
                                               P(cc), P(it), P(valid), P(st)), "refine_dev")
    return fin, res, cc, it, valid, st


def _same_refine(dev, host):
    fin, res, cc, it, valid, st = dev
    for k, h in enumerate(host):
        assert (st[k], valid[k], it[k]) == (h[4], h[3], h[2])
        assert np.array_equal(np.float64(cc[k]), np.float64(h[1]), equal_nan=True)
        if h[0] is not None:
            assert np.array_equal(fin[k].reshape(3, 3), h[0]) and np.array_equal(res[k].reshape(3, 3).view(np.uint32), h[5].view(np.uint32))


def test_refine_ecc_candidates_dev_strided_matches_host():
    import torch
    n = 512
    ref, mon = _pair(n, _homography(-1.25, 0.75, -0.05, 1 - 2e-4, (0, 1e-7)), seed=31)
    mon = mon[:500, :490]                                              # mon and ref of different sizes
    inits = [np.eye(3), np.array([[1, 0, 1.0], [0, 1, -0.5], [0, 0, 1]]), np.array([[1, 0, 600.0], [0, 1, 0], [0, 0, 1]])]
    host = ops.refine_ecc_candidates(mon, ref, inits)
    assert [h[4] for h in host] == [_lib.ECC_CONVERGED, _lib.ECC_CONVERGED, _lib.ECC_SKIPPED]
    _same_refine(_refine_dev(_lib.default_context(), torch, _strided(torch, mon), _strided(torch, ref, 1, 11), inits), host)


def _s2_pair(torch, n, A, seed):
    """synthetic uint16 Sentinel-2-sized pair generated on the device: ref = the scene, mon(x) = scene(A x) (f32 warp by the
    library itself, then quantised); both stretched to uint8 as the caller's preprocessing would"""
    pad = synth.PAD
    base = synth._base_torch(n, n, seed, "cuda").contiguous()
    ref16 = base[pad:pad + n, pad:pad + n].round().clamp(1, 16000)
    mon32 = torch.empty((n, n), dtype=torch.float32, device="cuda")
    T = np.array([[1, 0, pad], [0, 1, pad], [0, 0, 1.0]]) @ A
    c = _lib.default_context()
    torch.cuda.synchronize()
    c.check(c.lib.km_warp_perspective_dev(c.handle, _vp(base), _lib.KM_F32, base.shape[0], base.shape[1], base.stride(0), _vp(mon32), n, n,
                                          n, 1, 1, 0.0, np.ascontiguousarray(T).ctypes.data_as(C.POINTER(C.c_double))), "synth warp")
    c.sync()
    mon16 = mon32.round().clamp(1, 16000)   # uint16 values, held as float32 on the device

    def u8(a):
        return ((a - 1000.0) * (255.0 / 4000.0)).clamp(0, 255).to(torch.uint8)
    return ref16, mon16, u8(ref16), u8(mon16)


def test_sentinel2_size_refine_render_and_dev_forms():
    import torch
    n = 10980
    A = _homography(1.3, -0.9, 0.005, 1 + 5e-5, (2e-10, -2e-10))
    ref16, mon16, d_ref8, d_mon8 = _s2_pair(torch, n, A, 20261016)
    ref8, mon8 = d_ref8.cpu().numpy(), d_mon8.cpu().numpy()
    from karios_amd.matcher import refine_global_alignment, render_global_alignment
    ransac = np.array([[1, 0, 1.0], [0, 1, -0.75], [0, 0, 1.0]])
    prior = np.eye(3)
    al = refine_global_alignment(mon8, ref8, ransac, 100, 120, prior=prior)
    assert [cand[0] for cand in al.candidates] == ["RANSAC", "prior"]
    assert al.matrix is max(al.candidates, key=lambda cand: cand[2])[1]
    Ai = np.linalg.inv(A)
    for name, m, cc in al.candidates:
        R0 = ransac if name == "RANSAC" else prior
        # template(x) ~ input(W x) with input = mon pre-warped by R0: W = R0 A^-1, and the reference's final W @ R0
        assert cc > 0.9 and np.abs(_corners(m, n) - _corners(R0 @ Ai @ R0, n)).max() <= 0.1, (name, cc)
    # the _dev form on the device rasters (strided views) against the host form, bitwise
    host = ops.refine_ecc_candidates(mon8, ref8, [ransac, prior])
    big = torch.zeros((n, n + 64), dtype=torch.uint8, device="cuda")
    big[:, 64:].copy_(d_mon8)
    _same_refine(_refine_dev(_lib.default_context(), torch, big[:, 64:], d_ref8, [ransac, prior]), host)
    del big
    # the renders against the restatement on row bands
    mon_np = mon16.cpu().numpy().astype(np.uint16)
    mask = (mon8 > 128).astype(np.uint8)
    out, out_mask, alts = render_global_alignment(mon_np, ref8, mask, al)
    assert out.dtype == np.uint16 and out.shape == (n, n)
    rows = np.concatenate([np.arange(0, 16), np.arange(5000, 5016), np.arange(n - 16, n)])
    src32 = mon_np.astype(np.float32)
    exp = R.warp_perspective(src32, al.matrix, (n, n), R.INTER_LINEAR, 0.0, rows=rows).astype(np.uint16)
    np.testing.assert_array_equal(out[rows], exp)
    np.testing.assert_array_equal(out_mask[rows], R.warp_perspective(mask, al.matrix, (n, n), R.INTER_NEAREST, 0, rows=rows))
    for name, m, _ in al.candidates:
        if name in alts:
            e = R.warp_perspective(src32, m.astype(np.float32), (n, n), R.INTER_LINEAR, 0.0, rows=rows).astype(np.uint16)
            np.testing.assert_array_equal(alts[name][rows], e)

