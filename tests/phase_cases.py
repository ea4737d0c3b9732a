"""Phase-correlation content WITHOUT a clean peak, and the references that go with it (tests/test_phase_cases_host.py proves the
fixtures on the CPU, tests/test_gpu_phase_accuracy.py runs them through k_fft.hip / k_fft64.hip / k_phase.hip).

A noise-free shifted copy gives one dominant peak, the input on which a wrong transform is hardest to see: an independent 0.05 rad
phase error on every bin, or every fifth spectrum column missing, leaves the arg-max alone and moves the margin in the third
digit.  Here the moving image is a crop `a` of one synthetic scene and the reference image a BLEND of two crops at different
integer shifts plus noise,

    b = w * b1 + (1 - w) * b2 + sigma * std(scene) * N(0, 1)        (rounded and cast to the pixel type)

so that the correlation surface carries two planted peaks whose heights cross as `w` passes the tie.  `w` is bisected on the
float64 reference surface until the margin (largest - second largest) / largest sits in a requested window, or - float32 pixels
only - until the two planted peaks are 1e-8 .. 2e-6 apart.

Everything here is numpy / scipy on the CPU; nothing reads the library under test.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import scipy.fft as sfft

from karios_amd import synth

GOLDEN_TOLERANCES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phase_margin_tolerances.npz")
BORDER = 40                       # the scene is (H + 80) x (W + 80): crops may move by +-40

DTYPES = (np.uint16, np.uint8, np.int16, np.float32)
SIGMAS = (0.0, 0.5)

# float32 path (k_fft.hip): smallest shapes that reach each form.  61 * M sides take the wave-local rows (`fft61`), everything else
# (and 61 * M under fft61 = 0) the generic Stockham rows.
FAST_SHAPES = (
    (122, 183),    # both sides 61 M, even row count: Hermitian half-plane inverse, two rows per transform
    (183, 122),    # ... odd row count: the last pair has one member
    (244, 183),    # ... M = 4 (one radix-4 stage) x M = 3
    (96, 250),     # generic rows, radices 2 3 / 2 5
    (64, 112),     # generic rows, radix 7
    (122, 96),     # only H is 61 M: the cross-power step rides on the first inverse pass' load
    (96, 122),     # only W is 61 M: separate cross_power_f32_kernel, top2 reported by the rows
    (48, 732),     # 61 * 12: the M-point transform has a radix-4 and a radix-3 stage
)
MARGIN_WINDOW = (0.03, 0.3)       # float32 answers, margin compared with the reference
DECIDE_F64_WINDOW = (0.001, 0.006)   # below the 1 % rule: complex128 decides
DECIDE_F32_WINDOW = (0.02, 0.2)      # above it: float32 answers
DECISION_SHAPES = ((122, 183), (96, 250), (96, 122), (45, 35))
# scene seed per shape: on small crops the frame itself correlates at shift (0, 0) and can outrank the planted peaks; the builders
# raise then, and these are seeds at which every case of the shape builds (tests/test_phase_cases_host.py proves it)
SCENE_SEED = {(64, 112): 2, (122, 96): 1, (96, 122): 8, (48, 732): 0, (45, 35): 4}

# complex128 path (k_fft64.hip): one shape per plan kind (km_phase_plan tells which), >= 6 near-ties each
NEAR_TIE_SHAPES = {
    "smooth": (96, 250),
    "prime_on_w": (244, 183),
    "prime_on_h": (183, 244),
    "bluestein_h": (131, 200),
    "bluestein_w": (200, 131),
    "bluestein_both": (257, 263),
    "two_column_levels": (512, 96),
    "long_rows": (64, 4096),
}
NEAR_TIE_SEEDS = {(244, 183): (0, 1, 2, 3, 6, 7)}      # (seeds 4 and 5: the frame's own (0, 0) sample outranks the planted peaks)


def near_tie_seeds(shape):
    return NEAR_TIE_SEEDS.get(shape, tuple(range(6)))
NEAR_TIE_GAP = (1e-8, 2e-6)


# ---------------------------------------------------------------------------------------------------- surfaces
def surface64(reference_image, moving_image):
    """|cc| of oracle/oracle.py::phase_cross_correlation (skimage 0.24 defaults, normalization='phase'), float64."""
    src = sfft.fftn(np.asarray(reference_image, np.float64))
    tgt = sfft.fftn(np.asarray(moving_image, np.float64))
    prod = src * tgt.conj()
    eps = np.finfo(prod.real.dtype).eps
    prod /= np.maximum(np.abs(prod), 100 * eps)
    return np.abs(sfft.ifftn(prod))


def top2(cc):
    """-> (flat arg-max (first one), largest, second largest, margin) with the library's definition: the second largest is taken
    over every sample but the peak's own, margin = (largest - second) / largest."""
    flat = np.asarray(cc).ravel()
    i1 = int(np.argmax(flat))
    v1 = float(flat[i1])
    rest = flat.copy()
    rest[i1] = -np.inf
    v2 = float(rest.max()) if flat.size > 1 else 0.0
    return i1, v1, v2, ((v1 - v2) / v1 if v1 > 0 else 0.0)


def shift_of(flat, shape):
    """Integer shift of a flat arg-max as skimage reports it (oracle.py:471-477)."""
    H, W = shape
    r, c = divmod(int(flat), W)
    if r > H // 2:
        r -= H
    if c > W // 2:
        c -= W
    return np.array([0 if H == 1 else r, 0 if W == 1 else c], np.float64)


def flat_of(shift, shape):
    return (int(shift[0]) % shape[0]) * shape[1] + int(shift[1]) % shape[1]


def inject_phase_noise(spec, rad=0.01, seed=0):
    """Defect: an independent N(0, rad) phase error on every bin of a forward spectrum (a chirp or twiddle with lost precision)."""
    rng = np.random.default_rng(seed)
    return spec * np.exp(1j * rad * rng.standard_normal(spec.shape)).astype(spec.dtype)


def inject_dropped_columns(spec, every=5):
    """Defect: one spectrum column in `every` is zero (a level that skips some columns)."""
    out = spec.copy()
    out[:, ::every] = 0
    return out


def surface32_emulated(reference_image, moving_image, defect=None):
    """The same expression on complex64 with scipy's FFT - an independent, correct float32 transform.  `defect` (CPU self-test
    only) is applied to the forward spectrum of the moving image."""
    src = sfft.fftn(np.asarray(reference_image, np.float32))
    tgt = sfft.fftn(np.asarray(moving_image, np.float32))
    assert src.dtype == np.complex64 and tgt.dtype == np.complex64
    if defect is not None:
        tgt = defect(tgt)
    prod = src * tgt.conj()
    prod /= np.maximum(np.abs(prod), np.float32(100 * np.finfo(np.float64).eps))
    cc = sfft.ifftn(prod)
    assert cc.dtype == np.complex64
    return np.abs(cc).astype(np.float64)


def margin_tolerance(cc32, cc64):
    """tol = 8 * 2 * max|surface32 - surface64| / v1: 2 delta / v1 is the first-order bound on the margin's error when every sample
    is off by at most delta; the factor 8 covers the error constants of two correct float32 FFTs (radix order, table twiddles, the
    packed inverse)."""
    return 16.0 * float(np.abs(cc32 - cc64).max()) / float(cc64.max())


# ---------------------------------------------------------------------------------------------------- scenes and crops
@functools.lru_cache(maxsize=8)
def _scene(H, W, seed):
    base, _ = synth.make_pair(H + 2 * BORDER, W + 2 * BORDER, 0.0, 0.0, seed=seed, noise_sigma=0.0)
    base.setflags(write=False)
    return base


def _crop(base, H, W, s):
    return base[BORDER - s[0]:BORDER - s[0] + H, BORDER - s[1]:BORDER - s[1] + W].astype(np.float64)


def _two_shifts(shape, rng):
    """Two different integer shifts, small against the sides, neither (0, 0)."""
    H, W = shape
    my, mx = min(30, H // 8), min(30, W // 8)
    if my == 0 and mx == 0:
        raise ValueError(f"{shape}: too small for two planted shifts")
    while True:
        s = [(int(rng.integers(-my, my + 1)), int(rng.integers(-mx, mx + 1))) for _ in range(2)]
        if s[0] != s[1] and (0, 0) not in s:
            return s


def _in_pixel_units(x, dtype):
    """Scene values (uint16 counts) on the pixel type's scale, still float64 - the casts the existing phase tests use."""
    if dtype == np.uint8:
        return x / 64.0
    if dtype == np.int16:
        return x - 9000.0
    if dtype == np.float32:
        return x * 0.25
    return x


def _cast(x, dtype):
    if dtype == np.float32:
        return x.astype(np.float32)
    info = np.iinfo(dtype)
    return np.clip(np.rint(x), info.min, info.max).astype(dtype)


class Blend:
    """a, b1, b2 and the noise plane of one case on the pixel type's scale; `b(w)` is the blended reference image."""

    def __init__(self, shape, dtype, sigma, seed):
        H, W = shape
        self.shape, self.dtype = shape, dtype
        base = _scene(H, W, 1000 + 3 * H + W + seed)
        rng = np.random.default_rng([H, W, seed])
        self.s1, self.s2 = _two_shifts(shape, rng)
        noise = rng.standard_normal(shape) * (sigma * float(base.std())) if sigma > 0 else np.zeros(shape)
        zero = (0, 0)
        self.a = _cast(_in_pixel_units(_crop(base, H, W, zero), dtype), dtype)
        self._b1 = _in_pixel_units(_crop(base, H, W, self.s1), dtype)
        self._b2 = _in_pixel_units(_crop(base, H, W, self.s2), dtype)
        self._noise = noise * (_in_pixel_units(np.float64(1.0), dtype) - _in_pixel_units(np.float64(0.0), dtype))
        self._fa = sfft.fftn(self.a.astype(np.float64)).conj()
        self.f1, self.f2 = flat_of(self.s1, shape), flat_of(self.s2, shape)

    def b(self, w):
        return _cast(w * self._b1 + (1.0 - w) * self._b2 + self._noise, self.dtype)

    def surface(self, w):
        """surface64(b(w), a) with fft(a) computed once."""
        prod = sfft.fftn(self.b(w).astype(np.float64)) * self._fa
        prod /= np.maximum(np.abs(prod), 100 * np.finfo(np.float64).eps)
        return np.abs(sfft.ifftn(prod))


class Case:
    """One committed fixture: `b` is the reference image, `a` the moving one (ops.phase_cross_correlation(b, a))."""

    def __init__(self, key, a, b, w, planted):
        self.key, self.a, self.b, self.w, self.planted = key, a, b, w, planted
        self.cc = surface64(b, a)
        self.flat, self.v1, self.v2, self.margin = top2(self.cc)
        self.shift = shift_of(self.flat, a.shape)


def case_key(shape, dtype, sigma, seed=0, tag="m"):
    return f"{tag}-{shape[0]}x{shape[1]}-{np.dtype(dtype).name}-s{sigma:g}-{seed}"


@functools.lru_cache(maxsize=None)
def pair_with_margin(shape, dtype, target, sigma, seed=0):
    """Case whose reference margin lies in `target` = (lo, hi) with the peak on the first planted shift.  The signed margin (positive
    while the peak sits on s1, negative on s2) rises with w; it is bisected towards sqrt(lo * hi).  Raises if the window is missed
    or a spurious sample outranks the planted peak."""
    lo, hi = target
    bl = Blend(shape, dtype, sigma, seed)
    goal = float(np.sqrt(lo * hi))

    def signed(w):
        i1, _, _, m = top2(bl.surface(w))
        return m if i1 == bl.f1 else -m

    wl, wh = 0.0, 1.0
    w = 0.5
    for _ in range(48):
        w = 0.5 * (wl + wh)
        m = signed(w)
        if lo * 1.15 <= m <= hi / 1.15:
            break
        if m < goal:
            wl = w
        else:
            wh = w
    case = Case(case_key(shape, dtype, sigma, seed), bl.a, bl.b(w), w, (bl.s1, bl.s2))
    if not (lo <= case.margin <= hi and case.flat == bl.f1):
        raise ValueError(f"pair_with_margin{(shape, np.dtype(dtype).name, target, sigma, seed)}: margin {case.margin:.4g} at w = {w:.6f}, "
                         f"peak at {tuple(case.shift)} (planted {bl.s1}, {bl.s2})")
    return case


@functools.lru_cache(maxsize=None)
def near_tie_pair(shape, seed=0, sigma=0.0):
    """float32 pixels (integer rounding would make the heights a step function of w): the two planted peaks are the two largest
    samples, the third largest is <= 0.9 of the first and the relative gap between the two lies in NEAR_TIE_GAP.  Raises otherwise."""
    bl = Blend(shape, np.float32, sigma, seed)

    def gap(w):
        cc = bl.surface(w).ravel()
        return (cc[bl.f1] - cc[bl.f2]) / max(cc[bl.f1], cc[bl.f2])

    wl, wh = 0.0, 1.0
    w = 0.5
    for _ in range(60):
        w = 0.5 * (wl + wh)
        g = gap(w)
        if NEAR_TIE_GAP[0] * 1.5 <= abs(g) <= NEAR_TIE_GAP[1] / 1.5:
            break
        if g < 0:
            wl = w
        else:
            wh = w
    case = Case(f"t-{shape[0]}x{shape[1]}-{seed}", bl.a, bl.b(w), w, (bl.s1, bl.s2))
    check_near_tie(case)
    return case


def check_near_tie(case):
    flat = case.cc.ravel()
    order = np.argsort(flat)[-3:][::-1]
    f1, f2 = (flat_of(s, case.a.shape) for s in case.planted)
    gap = (flat[order[0]] - flat[order[1]]) / flat[order[0]]
    if {int(order[0]), int(order[1])} != {f1, f2} or flat[order[2]] > 0.9 * flat[order[0]] or not NEAR_TIE_GAP[0] <= gap <= NEAR_TIE_GAP[1]:
        raise ValueError(f"near_tie_pair({case.key}): top three {order.tolist()} = {flat[order].tolist()}, planted {f1}, {f2}, gap {gap:.3g}")
    return gap


# ---------------------------------------------------------------------------------------------------- the committed case lists
def margin_cases(shape):
    """The eight float32-margin cases of one shape: every pixel type x sigma."""
    return [pair_with_margin(shape, dt, MARGIN_WINDOW, sg, SCENE_SEED.get(shape, 0)) for dt in DTYPES for sg in SIGMAS]


def decision_cases(shape):
    """-> [(case, expected path)]: margins under the 1 % rule (complex128 decides) and over it (float32 answers)."""
    out = []
    for dt, sg in ((np.uint16, 0.5), (np.float32, 0.0), (np.uint8, 0.5)):
        out.append((pair_with_margin(shape, dt, DECIDE_F64_WINDOW, sg, SCENE_SEED.get(shape, 0)), 2))
        out.append((pair_with_margin(shape, dt, DECIDE_F32_WINDOW, sg, SCENE_SEED.get(shape, 0)), 1))
    return out


def is_61m(n):
    """Row lengths the wave-local 61 * M form takes (k_fft.hip, factorize61)."""
    if n < 122 or n % 61:
        return False
    m = n // 61
    if m > 192 or m % 61 == 0:
        return False
    for r in (7, 5, 3, 2):
        while m % r == 0:
            m //= r
    return m == 1


def fast_forms(shape):
    """Option sets that select a different float32 kernel sequence for this shape -> [(name, {option: value})].  (Whether the
    cross-power step is fused into the first inverse pass or a kernel of its own follows from the shape: fused where H is 61 * M.)"""
    h61, w61 = is_61m(shape[0]), is_61m(shape[1])
    forms = [("default", {})]
    if h61 or w61:
        forms.append(("stockham_rows", {"fft61": 0}))
    if h61 and w61:
        forms.append(("full_plane_inverse", {"fft_herm": 0}))
    return forms


def load_tolerances():
    with np.load(GOLDEN_TOLERANCES) as z:
        return {k: float(v) for k, v in zip(z["keys"].tolist(), z["tol"].tolist())}


def compute_tolerances():
    """tol of every margin case, from the complex64 emulation and the float64 reference (never from GPU output)."""
    out = {}
    for shape in FAST_SHAPES:
        for c in margin_cases(shape):
            out[c.key] = margin_tolerance(surface32_emulated(c.b, c.a), c.cc)
    return out


if __name__ == "__main__":        # regenerates tests/golden/phase_margin_tolerances.npz
    tol = compute_tolerances()
    keys = sorted(tol)
    np.savez(GOLDEN_TOLERANCES, keys=np.array(keys), tol=np.array([tol[k] for k in keys], np.float64))
    for k in keys:
        print(f"{k:40s} {tol[k]:.3e}")
