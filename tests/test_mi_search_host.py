"""CPU suite: the mutual-information search around each key point (km_mi_search, csrc/mi_search_math.hpp, csrc/k_mi_search.hpp).

The reference has no such search; its `_mutual_info` (karios/matcher/mutual_info_service.py:32-63) and `_mutual_information`
(karios/matcher/zncc_service.py:129-151) define the two values at every offset.  tests/golden/mi_search.npz holds their own values at
every offset of a radius-2 search (tests/golden/make_golden_mi_search.py); tests/mi_search_restatement.py is the definition of the rest.

1. The definition: the committed table against its `decimal` build; the restatement's counts against np.histogram2d, its values against
   tests/score_restatement.py `mi_scores` and against the golden values; known answers; the numpy peak form.
2. csrc/mi_search_math.hpp and the host-build launcher of csrc/k_mi_search.hpp - the text the kernels and the library's host side compile
   - as a stand-alone program built by g++ with -ffp-contract=off under the address and undefined-behaviour sanitizers, files in and
   out, over the shared case list (tests/mi_search_cases.py): byte for byte on every case, all four pixel types.
3. The ABI carries the entry points; the host build of the API files links them and, as a program of its own, refuses what the header
   says it refuses and computes in its host form what the launcher computes; argument errors raise without a device; the generic path
   of `MutualInfoService.search`; `score_frame` / `handle_klt_results` against a recording library.
"""
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pandas as pd
import pytest

import mi_search_cases as M
import mi_search_restatement as R
import sanitizer_harness as san
import score_restatement as SR
import test_resident_calls_host as H0
import zncc_search_restatement as ZR

from karios_amd import _lib, ops, resident, results  # noqa: E402
from karios_amd.matcher import mutual_info_service, zncc_service  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hoststub")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mi_search.npz")
CASES = M.cases()


@pytest.fixture(scope="module")
def expected():
    """name -> (the case's arrays, the restatement's Result), computed once."""
    return {c.name: (M.build(c), R.search(*M.build(c), c.radius)) for c in CASES}


def case_named(name):
    return next(c for c in CASES if c.name == name)


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
def test_committed_table_equals_the_decimal_build_entry_by_entry():
    text = open(os.path.join(ROOT, "karios_amd", "csrc", "mi_clogc_q36.inc")).read()
    body = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("//"))
    got = [int(v) for v in re.findall(r"(-?\d+)LL,", body)]
    want = R.table()
    assert len(got) == len(want) == 3250 and got[0] == got[1] == 0
    assert all(a == b for a, b in zip(got, want))
    assert 2 * want[-1] < 2 ** 53 and all(b > a for a, b in zip(want[1:], want[2:]))
    # a float64 log is NOT this table: the products reach 2^51
    loose = [0, 0] + [int(np.rint(c * np.log(float(c)) * 2.0 ** 36)) for c in range(2, 3250)]
    assert sum(a != b for a, b in zip(loose, want)) > 50


def chip_pairs():
    """Random, near-constant, two-cell, two-valued and anti-correlated chip pairs of all four pixel types."""
    rng = np.random.default_rng(2300)
    out = []
    for dt in SR.TYPES:
        lo, hi = (0.0, 1.0) if dt is np.float32 else (int(np.iinfo(dt).min), int(np.iinfo(dt).max))
        span = (hi - lo) if dt is np.float32 else min(hi - lo, 40000)

        def cast(a):
            return (lo + a * span).astype(dt) if dt is np.float32 else (lo + np.rint(a * span)).astype(dt)
        for _ in range(8):
            a = rng.random((57, 57))
            out += [(cast(a), cast(rng.random((57, 57)))), (cast(a), cast(1.0 - a)), (cast(a), cast(np.clip(a + 0.05 * rng.normal(size=a.shape), 0, 1)))]
        c = np.full((57, 57), 0.5)
        one = c.copy()
        one[30, 11] = 0.75
        two = np.where(rng.random((57, 57)) > 0.5, 0.25, 0.75)
        out += [(cast(c), cast(rng.random((57, 57)))), (cast(one), cast(c)), (cast(one), cast(one)), (cast(two), cast(two)), (cast(two), cast(1.0 - two)),
                (cast(two), cast(np.where(rng.random((57, 57)) > 0.5, 0.25, 0.75)))]
    return out


def test_counts_equal_histogram2d_and_values_the_longdouble_statement():
    worst = 0.0
    pairs = chip_pairs()
    for c1, c2 in pairs:
        counts = np.bincount(R.bins(c1) * 32 + R.bins(c2), minlength=1024).reshape(32, 32)
        want, _, _ = np.histogram2d(c1.ravel(), c2.ravel(), bins=32)
        assert np.array_equal(counts, want.astype(np.int64)) and counts.sum() == 3249
        got, ref = R.values(counts), SR.mi_scores(counts)
        for a, b in zip(got, ref):
            assert np.isnan(a) == np.isnan(b)
            if not np.isnan(a):
                worst = max(worst, abs(a - b))
    print("largest difference to score_restatement.mi_scores:", worst)
    assert worst <= 1e-9 and len(pairs) >= 100
    # the two-cell extremes, exactly
    two = np.zeros((32, 32), np.int64)
    two[3, 5], two[20, 9] = 1624, 1625
    assert R.values(two) == (2.0, 1.0)                           # two cells, each alone in its row and column: H(X) = H(Y) = H(X,Y)
    two = np.zeros((32, 32), np.int64)
    two[3, 5], two[3, 9] = 1624, 1625
    assert R.values(two) == (1.0, 0.0)                           # two cells in one row: H(X) = 0, H(Y) = H(X,Y)
    one = np.zeros((32, 32), np.int64)
    one[16, 16] = 3249
    assert all(np.isnan(v) for v in R.values(one))


def test_restatement_against_the_reference_values():
    g = np.load(GOLDEN)
    radius = int(g["radius"])
    for tag in ("u16", "f32"):
        ref, mon, cols = g["ref_" + tag], g["mon_" + tag], g["cols_" + tag]
        got = R.search(ref, mon, *cols, radius)
        for mine, want in ((got.surface, g["studholme_" + tag]), (got.surface_mi, g["nmi_" + tag])):
            assert np.array_equal(np.isnan(mine), np.isnan(want)), tag
            assert np.nanmax(np.abs(mine - want)) <= 1e-9, tag
        valued = ~np.isnan(g["studholme_" + tag]).all(axis=(1, 2))
        assert valued.sum() >= 8 and np.array_equal((got.status & 3) == 0, valued)
        assert np.isnan(g["studholme_" + tag]).any(axis=(1, 2))[valued].sum() >= 3          # rim rows: NaN columns or rows
    assert np.isnan(g["studholme_f32"][8]).all() and 0 < np.isnan(g["studholme_f32"][9]).sum() < 25     # the NaN in ref: the row; the infinity in mon: some offsets


def test_known_answers(expected):
    for name in ("u16_texture_r4_n64", "u8_texture_r4_n30", "i16_texture_r4_n40", "f32_texture_r4_n40", "u16_texture_r8_n20", "f32_texture_r8_n12"):
        case = case_named(name)
        (ref, mon, x0, y0, dx, dy), want = expected[name]
        rad, S = case.radius, 2 * case.radius + 1
        assert tuple(want.offset[0]) == M.SHIFT and want.status[0] == 0 and tuple(np.rint(want.shift[0])) == M.SHIFT        # the texture and its copy
        assert abs(want.shift[0] - M.SHIFT).max() <= 0.5 and abs(want.peak_mi[0] - 2.0 * (1.0 - 1.0 / want.peak[0])) < 1e-12       # the mi_score formula: monotone in the peak
        assert want.status[1] & R.RIM_X and want.offset[1, 0] == rad                          # moved beyond R in x
        assert want.status[2] & R.RIM_Y and want.offset[2, 1] == -rad                         # ... and in y
        # 28 px from each rim of `mon`: the columns / rows beyond it hold no value, the others do
        z = want.surface
        assert np.isnan(z[3][:, :rad]).all() and not np.isnan(z[3][:, rad:]).any()
        assert np.isnan(z[4][:rad, :]).all() and not np.isnan(z[4][rad:, :]).any()
        assert np.isnan(z[5][rad + 1:, :]).all() and not np.isnan(z[5][:rad + 1, :]).any()
        assert np.isnan(z[6][:, rad + 1:]).all() and not np.isnan(z[6][:, :rad + 1]).any()
        # the extreme pixels enter and leave: the monitored chip's range differs across the surface
        ex, ey = int(M.EXTREME[0]), int(M.EXTREME[1])
        ranges = {(int(R.chip(mon, ex + ox, ey).astype(np.float64).max() * 4), int(R.chip(mon, ex + ox, ey).astype(np.float64).min() * 4)) for ox in (-1, 1, 2)}
        assert len(ranges) == 3 and want.status[7] == 0
        if case.dtype is np.uint16:
            c = R.chip(mon, ex + 1, ey)
            assert int(c.max()) - int(c.min()) == 65535
        if case.dtype is np.int16:
            assert R.chip(mon, ex + 1, ey).min() == -32768 and R.chip(ref, ex, ey).min() < 0 < R.chip(ref, ex, ey).max()
        # a constant reference chip sits in bin 16: one occupied row of the table, NMI = (0 + H(Y)) / H(Y) = 1 exactly, mi_score formula 0
        c0 = R.centres(x0[8], y0[8], dx[8], dy[8], ref.shape, mon.shape)
        assert np.ptp(R.chip(ref, c0[0], c0[1]).astype(np.float64)) == 0 and set(R.bins(R.chip(ref, c0[0], c0[1]))) == {16}
        assert want.status[8] != R.NO_VALUE and want.peak[8] == 1.0 and want.peak_mi[8] == 0.0 and (z[8][~np.isnan(z[8])] == 1.0).all()
        # both chips constant: one cell, NaN everywhere, status 2
        assert want.status[9] == R.NO_VALUE and np.isnan(z[9]).all() and np.isnan(want.peak[9]) and np.isnan(want.peak_mi[9]) and not want.offset[9].any()
        # non-finite and out-of-range coordinates, rows one pixel short of the bounds rule
        assert (want.status[10:min(21, case.n)] == R.SKIPPED).all() and np.isnan(z[10:min(21, case.n)]).all()
        if np.dtype(case.dtype) == np.float32:
            if case.n > 24:
                assert want.status[24] == R.NO_VALUE and np.isnan(z[24]).all()                # the NaN in the reference chip: the whole row
            if case.n > 25:
                assert np.isnan(z[25][rad:, :]).all() and not np.isnan(z[25][:rad, :]).any() and (want.status[25] & 3) == 0   # the infinity: some offsets
    # two-valued chips: at most four cells; every value within [1, 2]
    for name in ("u8_binary_r4_n5", "u16_binary_r8_n3", "f32_binary_r1_n5"):
        (ref, mon, *_), want = expected[name]
        assert len(np.unique(ref)) == 2 and len(np.unique(mon)) == 2
        v = want.surface[~np.isnan(want.surface)]
        assert v.size and (v >= 1.0).all() and (v <= 2.0).all()
    # the contrast-inverted copy: mutual information finds the true offset; the ZNCC search's peak on the same rows is recorded beside it
    for name in ("u16_inverted_r4_n12", "u8_inverted_r4_n5", "i16_inverted_r4_n5", "f32_inverted_r4_n5"):
        arrays, want = expected[name]
        z = ZR.search(*arrays, 4)
        print(name, "mi offset", tuple(want.offset[0]), "peak", want.peak[0], "| zncc offset", tuple(z.offset[0]), "peak", z.peak[0],
              "zncc at the true offset", z.surface[0, 4 + M.SHIFT[1], 4 + M.SHIFT[0]])
        assert tuple(want.offset[0]) == M.SHIFT and want.status[0] == 0
        assert z.surface[0, 4 + M.SHIFT[1], 4 + M.SHIFT[0]] < -0.5                            # ZNCC is strongly negative at the right place
    # the full range of the 16-bit types
    (ref, mon, *_), _ = expected["u16_fullrange_r4_n5"]
    assert int(R.chip(mon, 64, 44).max()) - int(R.chip(mon, 64, 44).min()) > 65000
    (ref, mon, *_), _ = expected["i16_fullrange_r4_n5"]
    assert R.chip(mon, 64, 44).min() < -32000 and R.chip(mon, 64, 44).max() > 32000


def test_period_four_ties_go_to_the_first_offset_in_raster_order(expected):
    for name in ("u16_period4_r4_n5", "u8_period4_r8_n3", "i16_period4_r4_n5", "f32_period4_r4_n3"):
        case = case_named(name)
        _arrays, want = expected[name]
        for k in np.flatnonzero(want.status != R.SKIPPED):
            z, S = want.surface[k], 2 * case.radius + 1
            ones = np.argwhere(z == want.peak[k])
            assert len(ones) >= (1 if np.isnan(z).any() else 4) and want.peak[k] == 2.0 and want.peak_mi[k] == 1.0     # exact ties, 4 offsets apart (fewer at the raster's rim)
            assert {tuple((a - b) % 4) for a in ones for b in ones} == {(0, 0)}
            first = min(int(iy) * S + int(ix) for iy, ix in ones)
            assert (want.offset[k, 1] + case.radius) * S + want.offset[k, 0] + case.radius == first


def test_numpy_form_of_the_peak_step_equals_the_restatement(expected):
    for case in CASES:
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
#include "k_mi_search.hpp"
#include <cstdio>
#include <vector>
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
// {int dtype, Href, Wref, Hmon, Wmon, n, radius, surface; long long sref, smon, off_ref, off_mon (pixels)} ref buffer (Href * sref pixels)
// mon buffer x0 y0 dx dy -> offset peak peak_mi shift status [surface]; the outputs start poisoned
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
    std::vector<double> peak(n + 1, -7.0), peak_mi(n + 1, -7.0), shift(2 * n + 1, -7.0), surface(h.surface ? n * SS + 1 : 1, -7.0);
    std::vector<uint8_t> status(n + 1, 0x5a);
    const kms_args a = {ref.data() + h.off_ref * es, mon.data() + h.off_mon * es, h.dtype, h.Href, h.Wref, h.Hmon, h.Wmon, (ptrdiff_t)h.sref, (ptrdiff_t)h.smon,
                        cols[0].data(), cols[1].data(), cols[2].data(), cols[3].data(), h.n, h.radius, offset.data(), peak.data(), peak_mi.data(), shift.data(),
                        status.data(), h.surface ? surface.data() : nullptr};
    if (kms_search(nullptr, a) != KM_OK) return 3;
    if (offset[2 * n] != 0x5a5a5a5a || peak[n] != -7.0 || peak_mi[n] != -7.0 || shift[2 * n] != -7.0 || status[n] != 0x5a || surface.back() != -7.0) return 4;   // nothing past the rows
    fclose(in);
    const bool ok = wr(out, offset.data(), 8 * n) && wr(out, peak.data(), 8 * n) && wr(out, peak_mi.data(), 8 * n) && wr(out, shift.data(), 16 * n) &&
                    wr(out, status.data(), n) && (!h.surface || wr(out, surface.data(), 8 * n * SS));
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
    sizes = [8 * n, 8 * n, 8 * n, 16 * n, n] + ([8 * n * S * S] if surface else [])
    assert len(raw) == sum(sizes)
    cut = np.cumsum([0] + sizes)
    f = [raw[cut[i]:cut[i + 1]] for i in range(len(sizes))]
    return R.Result(np.frombuffer(f[0], np.int32).reshape(n, 2), np.frombuffer(f[1], np.float64), np.frombuffer(f[2], np.float64),
                    np.frombuffer(f[3], np.float64).reshape(n, 2), np.frombuffer(f[4], np.uint8),
                    np.frombuffer(f[5], np.float64).reshape(n, S, S) if surface else None, None)


def have_asan():
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    have_asan()
    d = tmp_path_factory.mktemp("mi_search_main")
    src, exe = d / "mi_search_main.cpp", d / "mi_search_main"
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
    for case in CASES:
        arrays, want = expected[case.name]
        got = parse(program(payload(case, arrays)), case.n, case.radius)
        M.assert_matches(case, want, got)
        if case.n == 5:                                          # without the surface: the same rows
            got = parse(program(payload(case, arrays, surface=False)), case.n, case.radius, surface=False)
            M.assert_matches(case, want, got, surface=False)


# ---- 3. the ABI, the host build, the arguments, the service's generic path, the frame columns ---------------------------------------------
ENTRY_POINTS = ("km_mi_search", "km_mi_search_dev")

ABI_MAIN = r"""
// The host objects of the sanitizer build as a program of their own: what km_mi_search[_dev] refuse, and the host form (upload, launcher,
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
    int32_t off[8]; double peak[4], pmi[4], shift[8]; uint8_t st[4];
    typedef int (*form)(km_ctx *, const void *, const void *, int, int, int, int, int, ptrdiff_t, ptrdiff_t, const float *, const float *, const float *, const float *,
                        int, int, int32_t *, double *, double *, double *, uint8_t *, double *);
    for (form f : {(form)km_mi_search, (form)km_mi_search_dev}) {
        const void *p = img.data();
        const float *x = col.data();
        REQUIRE(f(c, p, p, 7, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, peak, pmi, shift, st, nullptr) == KM_E_ARG);          // dtype
        REQUIRE(f(c, p, p, KM_F64, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, peak, pmi, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, p, p, KM_I32, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, peak, pmi, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, p, p, KM_U32, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, peak, pmi, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 0, off, peak, pmi, shift, st, nullptr) == KM_E_ARG);     // radius
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 9, off, peak, pmi, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, -1, 4, off, peak, pmi, shift, st, nullptr) == KM_E_ARG);    // rows
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, (1 << 20) + 1, 4, off, peak, pmi, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, nullptr, x, x, 4, 4, off, peak, pmi, shift, st, nullptr) == KM_E_ARG);   // null arrays
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, nullptr, pmi, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, peak, nullptr, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, nullptr, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, peak, pmi, shift, st, nullptr) == KM_E_ARG);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, nullptr, nullptr, nullptr, nullptr, 0, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == KM_OK);   // n = 0
        REQUIRE(km_set_image_window(c, 0, 10, 200, 100) == KM_OK);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, x, x, 4, 4, off, peak, pmi, shift, st, nullptr) == KM_E_UNSUPPORTED);
        REQUIRE(km_set_image_window(c, 0, 0, 0, 0) == KM_OK);
        REQUIRE(f(c, p, p, KM_U16, 100, 100, 100, 100, 100, 100, x, x, zero.data(), zero.data(), 4, 4, off, peak, pmi, shift, st, nullptr) == KM_OK);
        REQUIRE(st[0] == 2 && st[3] == 2 && off[0] == 0 && peak[0] != peak[0] && pmi[3] != pmi[3]);          // (a flat pair: one cell at every offset)
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
    std::vector<double> pk(n + 1), pm(n + 1), sh(2 * n + 1), surface(n * SS + 1);
    std::vector<uint8_t> status(n + 1);
    REQUIRE(km_mi_search(c, ref.data() + h.off_ref * es, mon.data() + h.off_mon * es, h.dtype, h.Href, h.Wref, h.Hmon, h.Wmon, (ptrdiff_t)h.sref, (ptrdiff_t)h.smon,
                         cols[0].data(), cols[1].data(), cols[2].data(), cols[3].data(), h.n, h.radius, offset.data(), pk.data(), pm.data(), sh.data(), status.data(),
                         surface.data()) == KM_OK);
    fclose(in);
    const bool ok = wr(out, offset.data(), 8 * n) && wr(out, pk.data(), 8 * n) && wr(out, pm.data(), 8 * n) && wr(out, sh.data(), 16 * n) && wr(out, status.data(), n) &&
                    wr(out, surface.data(), 8 * n * SS);
    REQUIRE(ok && !fclose(out));
    REQUIRE(km_ctx_destroy(c) == KM_OK);
    if (g_failures) return 1;
    printf("MI-SEARCH ABI OK\n");
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
        assert len(_lib.SIGNATURES[name][1]) == 22
    assert "k_mi_search.hip" in open(os.path.join(ROOT, "karios_amd", "csrc", "Makefile")).read()
    assert ops.MiSearch._fields == ("offset", "peak", "peak_mi", "shift", "status", "surface")
    assert callable(ops.mi_search) and callable(resident.ResidentPair.mi_search) and callable(mutual_info_service.MutualInfoService.search)
    assert resident.MI_SEARCH_COLUMNS == ["mi_dx", "mi_dy", "mi_peak", "mi_peak_mi", "mi_off_x", "mi_off_y", "mi_status"]
    assert inspect.signature(results.handle_klt_results).parameters["mi_search_radius"].default is None
    assert inspect.signature(resident.ResidentPair.score_frame).parameters["mi_search_radius"].default is None


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
    for name in ("u16_texture_r8_n20", "f32_texture_r1_n64", "i16_period4_r4_n5", "u8_texture_r4_n30"):
        case = case_named(name)
        arrays, want = expected[name]
        (tmp_path / "in.bin").write_bytes(payload(case, arrays))
        run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0 and "MI-SEARCH ABI OK" in run.stdout and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
        M.assert_matches(case, want, parse((tmp_path / "out.bin").read_bytes(), case.n, case.radius))


def test_argument_errors_raise_without_a_device():
    img = np.zeros((100, 100), np.uint16)
    col = np.full(3, 50, np.float32)
    for radius in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="radius"):
            ops.mi_search(img, img, col, col, col, col, radius=radius)
    with pytest.raises(ValueError, match="pixel type"):
        ops.mi_search(img, img.astype(np.int16), col, col, col, col)
    for other in (np.float64, np.int32, np.uint32):
        with pytest.raises(ValueError, match="pixel type"):
            ops.mi_search(img.astype(other), img.astype(other), col, col, col, col)
    with pytest.raises(ValueError, match="float32"):
        ops.mi_search(img, img, col.astype(np.float64), col, col, col)
    with pytest.raises(ValueError, match="length"):
        ops.mi_search(img, img, col[:2], col, col, col)
    big = np.zeros((1 << 20) + 1, np.float32)
    with pytest.raises(ValueError, match="2\\^20"):
        ops.mi_search(img, img, big, big, big, big)
    df = pd.DataFrame({"x0": col, "y0": col, "dx": col, "dy": col})
    with pytest.raises(ValueError, match="radius"):
        mutual_info_service.MutualInfoService().search(df, None, None, radius=0)
    # no rows: nothing is launched, the shapes are the search's
    r = ops.mi_search(img, img, col[:0], col[:0], col[:0], col[:0], radius=2, surface=True)
    assert r.offset.shape == (0, 2) and r.peak.shape == r.peak_mi.shape == (0,) and r.shift.shape == (0, 2) and r.status.shape == (0,) and r.surface.shape == (0, 5, 5)
    assert ops.mi_search(img, img, col[:0], col[:0], col[:0], col[:0]).surface is None


class Raster:
    def __init__(self, array):
        self.array, self.cleared = array, 0

    def clear_cache(self):
        self.cleared += 1


def mi_batch_by_the_restatement(ref, mon, x0, y0, dx, dy, ctx=None):
    """`ops.mi_batch` without a device: both scores of every row by tests/score_restatement.py (longdouble sums)."""
    _z, st, nmi = SR.scores(np.asarray(ref), np.asarray(mon), x0, y0, dx, dy)
    return st, nmi


def test_service_takes_the_generic_path_for_float64_frames_and_mixed_types(monkeypatch):
    calls = []

    def spy(*args, **kwargs):
        calls.append(len(args[2]))
        return mi_batch_by_the_restatement(*args, **kwargs)
    monkeypatch.setattr(ops, "mi_batch", spy)
    monkeypatch.setattr(ops, "mi_search", lambda *a, **k: pytest.fail("the kernel path was taken"))
    case = case_named("u16_texture_r4_n64")
    ref, mon, x0, y0, dx, dy = M.build(case)
    keep = np.r_[0:12, 30:34]                                     # the special rows and a few random ones
    radius = 1
    index = pd.Index(np.arange(len(keep)) * 3 + 7)
    # a float64 frame of values float32 holds too: the same centres, so the restatement's search is the answer
    frame = pd.DataFrame({c: v[keep].astype(np.float64) for c, v in zip(("x0", "y0", "dx", "dy"), (x0, y0, dx, dy))}, index=index)
    want = R.search(ref, mon, *(frame[c].to_numpy(np.float32) for c in ("x0", "y0", "dx", "dy")), radius)
    for r_img, m_img in ((ref, mon), (ref.astype(np.int32), mon)):           # a float64 frame; a mixed-type pair on top
        rasters = Raster(m_img), Raster(r_img)
        got = mutual_info_service.MutualInfoService().search(frame, *rasters, radius=radius)
        assert list(got.columns) == resident.MI_SEARCH_COLUMNS and got.index.equals(frame.index)
        assert np.array_equal(got["mi_status"].to_numpy(), want.status)
        assert np.array_equal(got[["mi_off_x", "mi_off_y"]].to_numpy(), want.offset)
        assert np.allclose(got[["mi_dx", "mi_dy"]].to_numpy(), want.shift, rtol=0, atol=1e-5, equal_nan=True)
        assert np.allclose(got["mi_peak"].to_numpy(), want.peak, rtol=0, atol=1e-9, equal_nan=True)
        assert np.allclose(got["mi_peak_mi"].to_numpy(), want.peak_mi, rtol=0, atol=1e-9, equal_nan=True)
        assert all(r.cleared == 1 for r in rasters)
    assert len(calls) == 2 and calls[0] == int(((want.status & R.SKIPPED) == 0).sum()) * 9       # all offsets of all rows in one call
    empty = mutual_info_service.MutualInfoService().search(frame.iloc[:0], Raster(mon), Raster(ref), radius=1)
    assert len(empty) == 0 and list(empty.columns) == resident.MI_SEARCH_COLUMNS


def _frame(n=3):
    cols = {c: np.linspace(30.0, 40.0, n).astype(np.float32) for c in ("x0", "y0")}
    cols.update({"dx": np.full(n, 0.5, np.float32), "dy": np.full(n, -0.25, np.float32), "score": np.array([0.9, 0.1, 0.8][:n], np.float32)})
    return pd.DataFrame(cols)


def test_frame_columns_against_a_recording_library_the_default_changes_nothing(tmp_path):
    def run(name, **kw):
        ctx = H0.make_ctx()
        pair = H0.make_pair(ctx, False)
        csv = tmp_path / name
        frame = results.handle_klt_results(iter([_frame()]), csv, pair, 0.4, **kw)
        return frame, csv.read_bytes(), [c for c in ctx.lib.take() if c[0] != "km_host_alloc"]

    plain, plain_csv, plain_calls = run("plain.csv")
    again, again_csv, again_calls = run("again.csv", mi_search_radius=None)
    assert list(plain.columns) == results.CSV_COLUMNS and list(again.columns) == results.CSV_COLUMNS and plain_csv == again_csv
    assert [c[0] for c in plain_calls] == [c[0] for c in again_calls] and not any("search" in c[0] for c in plain_calls)
    assert [c[1][2:9] + c[1][13:14] for c in plain_calls if c[1]] == [c[1][2:9] + c[1][13:14] for c in again_calls if c[1]]     # pixel type, sizes, strides, rows
    mi, mi_csv, mi_calls = run("mi.csv", mi_search_radius=3)
    assert list(mi.columns) == results.CSV_COLUMNS + resident.MI_SEARCH_COLUMNS
    assert mi_csv.splitlines()[0].decode().split(";") == list(mi.columns)
    assert [c[0] for c in mi_calls] == [c[0] for c in plain_calls] + ["km_mi_search_dev", "km_ctx_sync"]
    name, args = mi_calls[-2]
    assert args[13:15] == (2, 3) and args[20] is None                        # the two confident rows, radius 3, no surface
    assert mi.loc[1, resident.MI_SEARCH_COLUMNS].isna().all() and mi.loc[[0, 2], "mi_status"].notna().all()
    both, _csv, both_calls = run("both.csv", zncc_search_radius=2, mi_search_radius=1)
    assert list(both.columns) == results.CSV_COLUMNS + resident.ZNCC_SEARCH_COLUMNS + resident.MI_SEARCH_COLUMNS
    names = [c[0] for c in both_calls]
    assert names.index("km_zncc_search_dev") < names.index("km_mi_search_dev")
    # ResidentPair.mi_search lays its outputs out as the entry point reads them
    ctx = H0.make_ctx()
    pair = H0.make_pair(ctx, False)
    found = pair.mi_search(*(np.full(3, 30.0, np.float32),) * 4, radius=2, surface=True)
    assert found.offset.shape == (3, 2) and found.peak.shape == found.peak_mi.shape == (3,) and found.shift.shape == (3, 2) and found.surface.shape == (3, 5, 5)
    (name, args), = [c for c in ctx.lib.take() if c[0] == "km_mi_search_dev"]
    o = ctx.__dict__["_kp_staging"].ctypes.data
    assert args[13:] == (3, 2, o + 32 * 3, o, o + 8 * 3, o + 16 * 3, o + 40 * 3, o + 48 * 3)
    windowed = H0.make_pair(H0.make_ctx(), True)
    with pytest.raises(resident.KariosHipError, match="window"):
        windowed.mi_search(*(np.full(3, 30.0, np.float32),) * 4)
