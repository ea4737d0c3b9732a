"""CPU suite: the ZNCC search around each key point (km_zncc_search, csrc/zncc_math.hpp, csrc/k_zncc_search.hpp).

The reference has no such search; its `_zncc2` (karios/matcher/zncc_service.py:45-126) defines the value at every offset and
`ZNCCService._compute_zncc` (:186-238) the centres and the skip rule.  tests/golden/zncc_search.npz holds `_zncc2`'s own values at every
offset of a radius-4 search (tests/golden/make_golden_zncc_search.py); tests/zncc_search_restatement.py is the definition of the rest.

1. The restatement: against the golden surfaces; its exact-moment form against its two-pass form; hand-checkable known answers.
2. csrc/zncc_math.hpp and the host-build launcher of csrc/k_zncc_search.hpp - the text the kernels and the library's host side compile -
   as a stand-alone program built by g++ with -ffp-contract=off under the address and undefined-behaviour sanitizers, files in and out,
   over the shared case list (tests/zncc_search_cases.py): integer pixel types byte for byte, float32 within the stated tolerances.
3. The ABI carries the entry points; the host build of the API files links them and, as a program of its own, refuses what the header
   says it refuses and computes in its host form what the launcher computes; argument errors raise without a device; the generic path
   of `ZNCCService.search`.
"""
import os
import struct
import subprocess

import numpy as np
import pandas as pd
import pytest

import sanitizer_harness as san
import zncc_search_cases as Z
import zncc_search_restatement as R

from karios_amd import _lib, ops  # noqa: E402
from karios_amd.matcher import zncc_service  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hoststub")
GOLDEN = os.path.join(ROOT, "tests", "golden", "zncc_search.npz")


@pytest.fixture(scope="module")
def expected():
    """name -> (the case's arrays, the restatement's Result), computed once."""
    return {c.name: (Z.build(c), R.search(*Z.build(c), c.radius)) for c in Z.cases()}


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
def test_restatement_against_the_reference_values():
    """The golden surfaces are `_zncc2`'s own values.  For the float32 pair they are its values on the float64 copies of the pixels: the
    definition is float64 sums on float32 pixels.  Handed the float32 arrays themselves, numpy keeps `_zncc2`'s means, deviations and
    products in float32; that surface (`surface_f32_native`) lies 1.35e-7 from the float64 one on this content.  It is held to
    16 * 2^-24 = 9.6e-7: a value is a mean of 1849 products of magnitude <= 1 on average (Cauchy-Schwarz), each the result of at most
    5 float32 roundings after its mean and deviation (log2(1849) = 11 levels of pairwise summation each), summed pairwise again."""
    g = np.load(GOLDEN)
    radius = int(g["radius"])
    for tag in ("u16", "f32"):
        ref, mon, cols, want = g["ref_" + tag], g["mon_" + tag], g["cols_" + tag], g["surface_" + tag]
        two = R.search(ref, mon, *cols, radius, form="two_pass")
        assert np.array_equal(np.isnan(two.surface), np.isnan(want)), tag
        assert np.nanmax(np.abs(two.surface - want)) <= 1e-9, tag
        assert np.array_equal(two.status == R.SKIPPED, [R.centres(*cols[:, k], ref.shape, mon.shape) is None for k in range(cols.shape[1])])
        valued = ~np.isnan(want).all(axis=(1, 2))
        assert 20 <= valued.sum() < len(valued) and (two.status[~valued] != 0).all()
        if tag == "f32":
            native = g["surface_f32_native"]
            assert np.array_equal(np.isnan(native), np.isnan(want)) and np.nanmax(np.abs(native - two.surface)) <= 16 * 2.0 ** -24
        if tag == "u16":
            exact = R.search(ref, mon, *cols, radius, form="moments")
            assert np.array_equal(np.isnan(exact.surface), np.isnan(want))
            assert np.nanmax(np.abs(exact.surface - two.surface)) <= 1e-9
            assert np.array_equal(exact.offset, two.offset) and np.array_equal(exact.status, two.status)


def test_moment_form_equals_two_pass_form_on_the_cases(expected):
    for case in Z.cases():
        if np.dtype(case.dtype) == np.float32 or case.n == 0:
            continue
        (ref, mon, *cols), want = expected[case.name]
        two = R.search(ref, mon, *(c[:40] for c in cols), case.radius, form="two_pass")
        assert np.array_equal(np.isnan(two.surface), np.isnan(want.surface[:40])), case.name
        assert np.nanmax(np.abs(two.surface - want.surface[:40]), initial=0.0) <= 1e-9, case.name


def shifted_pair(dtype, shift, seed=5, H=110, W=120, centre=(60, 55)):
    """A textured pair with mon[y, x] = ref[y - sy, x - sx], exactly; `ref` is mirror-symmetric in x and in y about `centre`, so the
    windows at offsets +1 and -1 from the true shift hold mirrored pixels: equal moments, an exactly symmetric surface, a zero step."""
    rng = np.random.default_rng(seed)
    table = rng.integers(0, 200, (H + 40, W + 40))
    ys, xs = np.mgrid[0:H + 40, 0:W + 40]
    big = table[np.abs(ys - (centre[1] + 20)), np.abs(xs - (centre[0] + 20))].astype(dtype)
    sx, sy = shift
    return big[20:20 + H, 20:20 + W], big[20 - sy:20 - sy + H, 20 - sx:20 - sx + W]


def test_known_answers():
    f32 = np.float32
    one = [f32(60.0)], [f32(55.0)], [f32(0.0)], [f32(0.0)]
    for dtype in (np.uint8, np.uint16, np.int16, np.float32):
        ref, mon = shifted_pair(dtype, (3, -2))
        r = R.search(ref, mon, *one, 4)
        assert tuple(r.offset[0]) == (3, -2) and r.status[0] == 0
        if dtype != np.float32:
            # exact moments: cv == v1 == v2, a sub-pixel step of exactly 0; the peak is v / (sqrt(v) * sqrt(v)), 1.0 to the three roundings of that formula
            assert abs(r.peak[0] - 1.0) <= 2.0 ** -51 and tuple(r.shift[0]) == (3.0, -2.0)
        else:
            assert abs(r.peak[0] - 1.0) < 1e-12 and np.abs(r.shift[0] - (3.0, -2.0)).max() < 1e-9
        # KLT already at the shift: offset 0, the shift is the rounded displacement
        r = R.search(ref, mon, [f32(60.0)], [f32(55.0)], [f32(2.7)], [f32(-2.2)], 4)
        assert tuple(r.offset[0]) == (0, 0) and np.abs(r.shift[0] - (3.0, -2.0)).max() < 1e-9 and r.status[0] == 0
    # a shift beyond the radius: the peak lies on the rim, the rim bits are set, no sub-pixel step
    big = np.random.default_rng(6).normal(size=(150, 160))
    smooth = sum(big[i:i + 140, j:j + 150] for i in range(9) for j in range(9))            # correlation falls off over 9 pixels
    ref, mon = (np.rint(1000 + 100 * a).astype(np.uint16) for a in (smooth[10:120, 10:130], smooth[17:127, 4:124]))   # mon[y, x] = ref[y + 7, x - 6]
    r = R.search(ref, mon, *one, 4)
    assert tuple(r.offset[0]) == (4, -4) and r.status[0] == (R.RIM_X | R.RIM_Y) and tuple(r.shift[0]) == (4.0, -4.0)
    r = R.search(ref, mon, [f32(60.0)], [f32(55.0)], [f32(6.0)], [f32(0.0)], 4)           # x found, y beyond
    assert r.offset[0, 0] == 0 and r.offset[0, 1] == -4 and r.status[0] == R.RIM_Y and abs(r.shift[0, 0] - 6.0) <= 0.5 and r.shift[0, 1] == -4.0
    # a flat template: no offset has a value
    ref = ref.copy()
    ref[:] = 7
    r = R.search(ref, mon, *one, 4)
    assert r.status[0] == R.NO_VALUE and np.isnan(r.peak[0]) and np.isnan(r.shift[0]).all() and not r.offset[0].any() and np.isnan(r.surface).all()
    # a skipped row
    r = R.search(ref, mon, [f32(27.0)], [f32(55.0)], [f32(1.0)], [f32(0.0)], 4)
    assert r.status[0] == R.SKIPPED and np.isnan(r.peak[0]) and not r.offset[0].any()


def test_period_four_ties_go_to_the_first_offset_in_raster_order(expected):
    for name in ("u16_period4_r4_n5", "u8_period4_r8_n5", "i16_period4_r4_n5"):
        case = next(c for c in Z.cases() if c.name == name)
        _arrays, want = expected[name]
        for k in np.flatnonzero(want.status != R.SKIPPED):
            z, S = want.surface[k], 2 * case.radius + 1
            ones = np.argwhere(z == want.peak[k])
            assert len(ones) >= 4 and abs(want.peak[k] - 1.0) <= 2.0 ** -51                # exact ties, 4 offsets apart
            assert {tuple((a - b) % 4) for a in ones for b in ones} == {(0, 0)}
            first = min(int(iy) * S + int(ix) for iy, ix in ones)
            assert (want.offset[k, 1] + case.radius) * S + want.offset[k, 0] + case.radius == first


def test_steps_stay_within_half_a_pixel_and_float_cases_within_the_cap(expected):
    for case in Z.cases():
        (ref, mon, x0, y0, dx, dy), want = expected[case.name]
        live = (want.status & 3) == 0
        centres = np.array([R.centres(x0[k], y0[k], dx[k], dy[k], ref.shape, mon.shape) for k in np.flatnonzero(live)]).reshape(-1, 4)
        whole = np.stack([centres[:, 2] - centres[:, 0], centres[:, 3] - centres[:, 1]], axis=1) + want.offset[live]
        assert (np.abs(want.shift[live] - whole) <= 0.5).all(), case.name
        rim = np.stack([want.status[live] & R.RIM_X, want.status[live] & R.RIM_Y], axis=1) != 0
        assert (want.shift[live][rim] == whole[rim]).all(), case.name
        if np.dtype(case.dtype) == np.float32:                   # on the restatement alone: the committed float32 content stays under the cap
            assert Z.unclear_rows(want, case.radius).sum() <= Z.CAP * case.n, case.name
    assert sum(int(((w.status & 3) == 0).sum()) for _a, w in expected.values()) > 1000


def test_numpy_form_of_the_peak_step_equals_the_restatement(expected):
    for case in Z.cases():
        (ref, mon, x0, y0, dx, dy), want = expected[case.name]
        cs = [R.centres(x0[k], y0[k], dx[k], dy[k], ref.shape, mon.shape) for k in range(case.n)]
        inside = np.array([c is not None for c in cs], bool)
        centres = np.array([c if c is not None else (0, 0, 0, 0) for c in cs], np.int64).reshape(-1, 4).T
        got = zncc_service.surface_peaks(want.surface, case.radius, tuple(centres), inside)
        for field in ("offset", "peak", "shift", "status"):
            a, b = getattr(got, field), getattr(want, field)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (case.name, field)


# ---- 2. the shared header and the host-build launcher, as a sanitized program -------------------------------------------------------------
MAIN = r"""
#include "k_zncc_search.hpp"
#include <cstdio>
#include <vector>
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
// {int dtype, Href, Wref, Hmon, Wmon, n, radius, surface; long long sref, smon, off_ref, off_mon (pixels)} ref buffer (Href * sref pixels)
// mon buffer x0 y0 dx dy -> offset peak shift status [surface]; the outputs start poisoned
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    struct { int dtype, Href, Wref, Hmon, Wmon, n, radius, surface; long long sref, smon, off_ref, off_mon; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    const size_t es = h.dtype == KM_U8 ? 1 : h.dtype == KM_F32 ? 4 : 2, n = (size_t)h.n, SS = (size_t)(2 * h.radius + 1) * (2 * h.radius + 1);
    // (malloc'd to the byte: the sanitizer sees a read one pixel past a raster)
    std::vector<char> ref((size_t)h.Href * h.sref * es), mon((size_t)h.Hmon * h.smon * es);
    std::vector<float> cols[4];
    if (!rd(in, ref.data(), ref.size()) || !rd(in, mon.data(), mon.size())) return 2;
    for (auto &c : cols) { c.resize(n + 1); if (!rd(in, c.data(), 4 * n)) return 2; }
    std::vector<int32_t> offset(2 * n + 1, 0x5a5a5a5a);
    std::vector<double> peak(n + 1, -7.0), shift(2 * n + 1, -7.0), surface(h.surface ? n * SS + 1 : 1, -7.0);
    std::vector<uint8_t> status(n + 1, 0x5a);
    const kzs_args a = {ref.data() + h.off_ref * es, mon.data() + h.off_mon * es, h.dtype, h.Href, h.Wref, h.Hmon, h.Wmon, (ptrdiff_t)h.sref, (ptrdiff_t)h.smon,
                        cols[0].data(), cols[1].data(), cols[2].data(), cols[3].data(), h.n, h.radius, offset.data(), peak.data(), shift.data(), status.data(),
                        h.surface ? surface.data() : nullptr};
    if (kzs_search(nullptr, a) != KM_OK) return 3;
    if (offset[2 * n] != 0x5a5a5a5a || peak[n] != -7.0 || shift[2 * n] != -7.0 || status[n] != 0x5a || surface.back() != -7.0) return 4;   // nothing past the rows
    fclose(in);
    const bool ok = wr(out, offset.data(), 8 * n) && wr(out, peak.data(), 8 * n) && wr(out, shift.data(), 16 * n) && wr(out, status.data(), n) &&
                    (!h.surface || wr(out, surface.data(), 8 * n * SS));
    return fclose(out) || !ok ? 2 : 0;
}
"""


def payload(case, arrays, surface=True):
    """The input file of a case: the rasters travel as the wider buffers they are windows of."""
    ref, mon, x0, y0, dx, dy = arrays
    parts, meta = [], []
    for a in (ref, mon):
        base = a.base if a.base is not None else a
        assert base.flags.c_contiguous and a.strides[0] == base.strides[0]
        parts.append(base.tobytes())
        meta.append((base.shape[1], (a.ctypes.data - base.ctypes.data) // a.itemsize))
    head = struct.pack("<8i4q", _lib._DTYPES[ref.dtype], ref.shape[0], ref.shape[1], mon.shape[0], mon.shape[1], case.n, case.radius, int(surface),
                       meta[0][0], meta[1][0], meta[0][1], meta[1][1])
    return head + b"".join(parts) + b"".join(np.ascontiguousarray(c, np.float32).tobytes() for c in (x0, y0, dx, dy))


def parse(raw, n, radius, surface=True):
    S = 2 * radius + 1
    sizes = [8 * n, 8 * n, 16 * n, n] + ([8 * n * S * S] if surface else [])
    assert len(raw) == sum(sizes)
    cut = np.cumsum([0] + sizes)
    f = [raw[cut[i]:cut[i + 1]] for i in range(len(sizes))]
    return R.Result(np.frombuffer(f[0], np.int32).reshape(n, 2), np.frombuffer(f[1], np.float64), np.frombuffer(f[2], np.float64).reshape(n, 2),
                    np.frombuffer(f[3], np.uint8), np.frombuffer(f[4], np.float64).reshape(n, S, S) if surface else None)


def have_asan():
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    have_asan()
    d = tmp_path_factory.mktemp("zncc_search_main")
    src, exe = d / "zncc_search_main.cpp", d / "zncc_search_main"
    src.write_text(MAIN)
    san.build(src, exe, shared=False)

    def run(data):
        fin, fout = d / "in.bin", d / "out.bin"
        fin.write_bytes(data)
        out = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr[-4000:])
        return fout.read_bytes()
    return run


def test_host_launcher_equals_the_restatement(program, expected):
    for case in Z.cases():
        arrays, want = expected[case.name]
        got = parse(program(payload(case, arrays)), case.n, case.radius)
        Z.assert_matches(case, want, got)
        if case.n == 5:                                          # without the surface: the same rows
            got = parse(program(payload(case, arrays, surface=False)), case.n, case.radius, surface=False)
            Z.assert_matches(case, want, got, surface=False)


# ---- 3. the ABI, the host build, the arguments, the service's generic path ----------------------------------------------------------------
ENTRY_POINTS = ("km_zncc_search", "km_zncc_search_dev")

ABI_MAIN = r"""
// The host objects of the sanitizer build as a program of their own: what km_zncc_search[_dev] refuse, and the host form (upload, launcher,
// read-back) on a case file; device memory is host memory here.  Uses the public C ABI only.
#include "../../include/karios_hip.h"
#include <cstdio>
#include <vector>
static int g_failures = 0;
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); g_failures++; } } while (0)
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    km_ctx *c = nullptr;
    if (km_ctx_create(0, &c) != KM_OK) return 2;
    std::vector<uint16_t> img(100 * 100, 3);
    std::vector<float> col(4, 50.f), zero(4, 0.f);
    int32_t off[8]; double peak[4], shift[8]; uint8_t st[4];
    typedef int (*form)(km_ctx *, const void *, const void *, int, int, int, int, int, ptrdiff_t, ptrdiff_t, const float *, const float *, const float *, const float *,
                        int, int, int32_t *, double *, double *, uint8_t *, double *);
    for (form f : {(form)km_zncc_search, (form)km_zncc_search_dev}) {
        const void *p = img.data();
        const float *x = col.data();
        REQUIRE(f(c, p, p, 7, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, peak, shift, st, nullptr) == KM_E_ARG);          // dtype
        REQUIRE(f(c, p, p, KM_F64, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, peak, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 0, off, peak, shift, st, nullptr) == KM_E_ARG);     // radius
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 9, off, peak, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, -1, 4, off, peak, shift, st, nullptr) == KM_E_ARG);    // rows
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, (1 << 20) + 1, 4, off, peak, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, nullptr, x, x, 4, 4, off, peak, shift, st, nullptr) == KM_E_ARG);   // null arrays
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, nullptr, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, nullptr, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, peak, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, nullptr, nullptr, nullptr, nullptr, 0, 4, nullptr, nullptr, nullptr, nullptr, nullptr) == KM_OK);   // n = 0
        REQUIRE(km_set_image_window(c, 0, 10, 200, 100) == KM_OK);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, peak, shift, st, nullptr) == KM_E_UNSUPPORTED);
        REQUIRE(km_set_image_window(c, 0, 0, 0, 0) == KM_OK);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, zero.data(), zero.data(), 4, 4, off, peak, shift, st, nullptr) == KM_OK);
        REQUIRE(st[0] == 2 && st[3] == 2 && off[0] == 0 && peak[0] != peak[0]);          // (a flat pair: no offset has a value)
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    struct { int dtype, Href, Wref, Hmon, Wmon, n, radius, surface; long long sref, smon, off_ref, off_mon; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    const size_t es = h.dtype == KM_U8 ? 1 : h.dtype == KM_F32 ? 4 : 2, n = (size_t)h.n, SS = (size_t)(2 * h.radius + 1) * (2 * h.radius + 1);
    std::vector<char> ref((size_t)h.Href * h.sref * es), mon((size_t)h.Hmon * h.smon * es);
    std::vector<float> cols[4];
    if (!rd(in, ref.data(), ref.size()) || !rd(in, mon.data(), mon.size())) return 2;
    for (auto &v : cols) { v.resize(n + 1); if (!rd(in, v.data(), 4 * n)) return 2; }
    std::vector<int32_t> offset(2 * n + 1);
    std::vector<double> pk(n + 1), sh(2 * n + 1), surface(n * SS + 1);
    std::vector<uint8_t> status(n + 1);
    REQUIRE(km_zncc_search(c, ref.data() + h.off_ref * es, mon.data() + h.off_mon * es, h.dtype, h.Href, h.Wref, h.Hmon, h.Wmon, (ptrdiff_t)h.sref, (ptrdiff_t)h.smon,
                           cols[0].data(), cols[1].data(), cols[2].data(), cols[3].data(), h.n, h.radius, offset.data(), pk.data(), sh.data(), status.data(),
                           surface.data()) == KM_OK);
    fclose(in);
    const bool ok = wr(out, offset.data(), 8 * n) && wr(out, pk.data(), 8 * n) && wr(out, sh.data(), 16 * n) && wr(out, status.data(), n) && wr(out, surface.data(), 8 * n * SS);
    REQUIRE(ok && !fclose(out));
    REQUIRE(km_ctx_destroy(c) == KM_OK);
    if (g_failures) return 1;
    printf("ZNCC-SEARCH ABI OK\n");
    return 0;
}
"""


def test_abi_carries_the_entry_points():
    import ctypes
    header = open(os.path.join(ROOT, "include", "karios_hip.h")).read()
    api = open(os.path.join(ROOT, "karios_amd", "csrc", "api_score.hip")).read()        # a file the host build lists
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and f"int {name}(" in header and hasattr(lib, name) and f"int {name}(" in api
        assert len(_lib.SIGNATURES[name][1]) == 21
    assert "k_zncc_search.hip" in open(os.path.join(ROOT, "karios_amd", "csrc", "Makefile")).read()
    assert (ops.ZNCC_SKIPPED, ops.ZNCC_NO_VALUE, ops.ZNCC_RIM_X, ops.ZNCC_RIM_Y) == (R.SKIPPED, R.NO_VALUE, R.RIM_X, R.RIM_Y)
    assert (_lib.ZNCC_SEARCH_MAX_RADIUS, _lib.ZNCC_SEARCH_MAX_ROWS) == (R.MAX_RADIUS, R.MAX_ROWS)
    from karios_amd import resident, results
    assert callable(ops.zncc_search) and callable(resident.ResidentPair.zncc_search) and callable(zncc_service.ZNCCService.search)
    import inspect
    assert inspect.signature(results.handle_klt_results).parameters["zncc_search_radius"].default is None
    assert inspect.signature(resident.ResidentPair.score_frame).parameters["zncc_search_radius"].default is None


def test_host_build_of_the_api_files_links_refuses_and_computes(tmp_path, expected):
    have_asan()
    out = subprocess.run(["make", "-s", "-C", STUB], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-4000:]
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(STUB, "_build", "libkarios_host_asan.so")], text=True)
    assert all(f" T {name}\n" in syms for name in ENTRY_POINTS)
    # the same objects as a program of its own (no python, no preload)
    objects = sorted(os.path.join(STUB, "_build", f) for f in os.listdir(os.path.join(STUB, "_build")) if f.endswith(".o"))
    src, exe = tmp_path / "abi_main.cpp", tmp_path / "abi_main"
    src.write_text(ABI_MAIN.replace("../../include/karios_hip.h", os.path.join(ROOT, "include", "karios_hip.h")))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                           "-o", str(exe), str(src)] + objects + ["-ldl", "-lpthread"])
    for name in ("u16_96x120_r8_n300", "f32_96x120_r1_n5", "i16_period4_r4_n5"):
        case = next(c for c in Z.cases() if c.name == name)
        arrays, want = expected[name]
        (tmp_path / "in.bin").write_bytes(payload(case, arrays))
        run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0 and "ZNCC-SEARCH ABI OK" in run.stdout and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
        Z.assert_matches(case, want, parse((tmp_path / "out.bin").read_bytes(), case.n, case.radius))


def test_argument_errors_raise_without_a_device():
    img = np.zeros((100, 100), np.uint16)
    col = np.full(3, 50, np.float32)
    for radius in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="radius"):
            ops.zncc_search(img, img, col, col, col, col, radius=radius)
    with pytest.raises(ValueError, match="pixel type"):
        ops.zncc_search(img, img.astype(np.int16), col, col, col, col)
    with pytest.raises(ValueError, match="pixel type"):
        ops.zncc_search(img.astype(np.float64), img.astype(np.float64), col, col, col, col)
    with pytest.raises(ValueError, match="float32"):
        ops.zncc_search(img, img, col.astype(np.float64), col, col, col)
    with pytest.raises(ValueError, match="length"):
        ops.zncc_search(img, img, col[:2], col, col, col)
    big = np.zeros((1 << 20) + 1, np.float32)
    with pytest.raises(ValueError, match="2\\^20"):
        ops.zncc_search(img, img, big, big, big, big)
    df = pd.DataFrame({"x0": col, "y0": col, "dx": col, "dy": col})
    with pytest.raises(ValueError, match="radius"):
        zncc_service.ZNCCService().search(df, None, None, radius=0)
    # no rows: nothing is launched, the shapes are the search's
    r = ops.zncc_search(img, img, col[:0], col[:0], col[:0], col[:0], radius=2, surface=True)
    assert r.offset.shape == (0, 2) and r.peak.shape == (0,) and r.shift.shape == (0, 2) and r.status.shape == (0,) and r.surface.shape == (0, 5, 5)
    assert ops.zncc_search(img, img, col[:0], col[:0], col[:0], col[:0]).surface is None


class Raster:
    def __init__(self, array):
        self.array, self.cleared = array, 0

    def clear_cache(self):
        self.cleared += 1


def windows_by_the_restatement(img1, img2, u1, v1, u2, v2, half_size, ctx=None):
    """`ops.zncc_windows` without a device: _zncc2 by numpy, the reference's arithmetic."""
    a, b = np.asarray(img1), np.asarray(img2)
    out, outside = np.full(len(u1), np.nan), np.zeros(len(u1), bool)
    h = half_size
    for k, (r1, c1, r2, c2) in enumerate(zip(u1, v1, u2, v2)):
        if min(r1, c1, r2, c2) < h or r1 + h >= a.shape[0] or c1 + h >= a.shape[1] or r2 + h >= b.shape[0] or c2 + h >= b.shape[1]:
            outside[k] = True
            continue
        p, q = a[r1 - h:r1 + h + 1, c1 - h:c1 + h + 1].astype(np.float64), b[r2 - h:r2 + h + 1, c2 - h:c2 + h + 1].astype(np.float64)
        if p.std() != 0 and q.std() != 0:
            out[k] = np.mean((p - p.mean()) / p.std() * ((q - q.mean()) / q.std()))
    return out, outside


def test_service_takes_the_generic_path_for_float64_frames_and_mixed_types(monkeypatch):
    calls = []

    def spy(*args, **kwargs):
        calls.append(len(args[2]))
        return windows_by_the_restatement(*args, **kwargs)
    monkeypatch.setattr(ops, "zncc_windows", spy)
    monkeypatch.setattr(ops, "zncc_search", lambda *a, **k: pytest.fail("the kernel path was taken"))
    case = next(c for c in Z.cases() if c.name == "u16_96x120_r8_n300")
    ref, mon, x0, y0, dx, dy = Z.build(case)
    keep = np.r_[0:30, 150:160]                                   # the special rows and a few random ones
    radius = 2
    index = pd.Index(np.arange(len(keep)) * 3 + 7)
    # a float64 frame of values float32 holds too: the same centres, so the restatement's search is the answer
    frame = pd.DataFrame({c: v[keep].astype(np.float64) for c, v in zip(("x0", "y0", "dx", "dy"), (x0, y0, dx, dy))}, index=index)
    want = R.search(ref, mon, *(frame[c].to_numpy(np.float32) for c in ("x0", "y0", "dx", "dy")), radius, form="two_pass")
    for r_img, m_img in ((ref, mon), (ref.astype(np.int32), mon)):           # a float64 frame; a mixed-type pair on top
        rasters = Raster(m_img), Raster(r_img)
        got = zncc_service.ZNCCService().search(frame, *rasters, radius=radius)
        assert list(got.columns) == ["zncc_dx", "zncc_dy", "zncc_peak", "zncc_off_x", "zncc_off_y", "zncc_status"] and got.index.equals(frame.index)
        assert np.array_equal(got["zncc_status"].to_numpy(), want.status)
        assert np.array_equal(got[["zncc_off_x", "zncc_off_y"]].to_numpy(), want.offset)
        assert np.allclose(got[["zncc_dx", "zncc_dy"]].to_numpy(), want.shift, rtol=0, atol=1e-6, equal_nan=True)
        assert np.allclose(got["zncc_peak"].to_numpy(), want.peak, rtol=0, atol=1e-9, equal_nan=True)
        assert all(r.cleared == 1 for r in rasters)
    assert len(calls) == 2 and calls[0] == int(((want.status & R.SKIPPED) == 0).sum()) * 25      # all windows of all rows in one call
    mixed = pd.DataFrame({"x0": x0[:5], "y0": y0[:5], "dx": dx[:5], "dy": dy[:5]})                 # a float32 frame on a mixed-type pair
    got = zncc_service.ZNCCService().search(mixed, Raster(mon), Raster(ref.astype(np.int32)), radius=1)
    assert len(calls) == 3 and len(got) == 5
    empty = zncc_service.ZNCCService().search(mixed.iloc[:0], Raster(mon), Raster(ref), radius=1)
    assert len(empty) == 0 and list(empty.columns) == list(got.columns)
