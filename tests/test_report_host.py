"""CPU suite: the report's numbers - the display range of OverviewPlot._plot_image (karios/report/overview_plot.py:134-194) and
mean_profile (karios/report/commons.py:49-71).

1. tests/report_restatement.py - the definition - against the recorded results of the reference (tests/golden/report_numbers.npz)
   and against numpy's and the installed pandas' own evaluation on fresh inputs.
2. csrc/report_math.hpp and the host-build launchers of csrc/k_report.hpp - the text the kernels and the library's host side
   compile - as a stand-alone program built by g++ with -ffp-contract=off under the address and undefined-behaviour sanitizers, files
   in and out, against the restatement by bits.
3. The ABI carries the entry points; the host build of the API files links them; argument errors raise without a device.

Comparisons are by bits; two NaN count as equal whatever their sign and payload (numpy's and the device's default NaN differ).
"""
import os
import struct
import subprocess
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

import report_restatement as R
import sanitizer_harness as san

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_report as G  # noqa: E402

from karios_amd import _lib, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "report_numbers.npz"))
f32 = np.float32


def same(a, b):
    """Same dtype, shape and bits; NaN equals NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        nan = np.isnan(a)
        return bool(np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes())
    return a.tobytes() == b.tobytes()


def same_profile(got, want):
    return all(same(getattr(got, k), getattr(want, k)) for k in ("key", "position", "count", "mean", "std"))


@pytest.fixture(scope="module")
def range_cases():
    cases = G.range_cases()
    for name, a, mask, _nv, _nd in cases:
        assert G.crc(a, *([] if mask is None else [mask])) == int(GOLD[f"crc_{name}"][0]), "the rebuilt rasters are not the recorded ones"
    return cases


@pytest.fixture(scope="module")
def profile_cases():
    cases = G.profile_cases()
    for name, v, p, _b in cases:
        assert G.crc(v, p) == int(GOLD[f"crc_{name}"][0]), "the rebuilt columns are not the recorded ones"
    return cases


def restated_range(a, mask, no_values, nodata, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return R.display_range(a, mask, no_values, nodata, **kw)


# ---- 1. the definition -----------------------------------------------------------------------------------------------------------------
def test_range_restatement_equals_the_reference(range_cases):
    fallbacks = 0
    for name, a, mask, no_values, nodata in range_cases:
        r = restated_range(a, mask, no_values, nodata)
        assert r.n_invalid == int(GOLD[f"invalid_{name}"][0]), name
        vmin, vmax = GOLD[f"vmin_{name}"], GOLD[f"vmax_{name}"]
        if r.n_valid == 0 and vmin == 0:          # numpy's sign of a zero extreme depends on the element order; the definition gives +0.0
            vmin = np.abs(vmin)
        if r.n_valid == 0 and vmax == 0:
            vmax = np.abs(vmax)
        assert same(r.v_min, vmin) and same(r.v_max, vmax), (name, r.v_min, vmin, r.v_max, vmax)
        fallbacks += r.n_valid == 0
    assert fallbacks >= 5
    names = [c[0] for c in range_cases]
    assert np.isnan(GOLD["vmin_all_nan_float32"]) and {"valid1_int16", "valid2_float32", "list16_uint16"} <= set(names)


def test_profile_restatement_equals_the_reference(profile_cases):
    for name, v, p, b in profile_cases:
        r = R.mean_profile(v, p, b)
        want = R.Profile(key=GOLD[f"key_{name}"].astype(f32) + f32(0), position=GOLD[f"pos_{name}"], count=GOLD[f"count_{name}"], mean=GOLD[f"mean_{name}"],
                         std=GOLD[f"std_{name}"])
        assert same_profile(r, want) and r.out_of_range == 0, name
    assert GOLD["key_empty"].size == 0 and GOLD["key_one_group"].size == 1 and GOLD["count_single_rows"].max() == 1


def numpy_range(a, mask, no_values, nodata):
    """The reference's two functions, written out (overview_plot.py:142-151, 168-178)."""
    invalid = None
    if mask is not None:
        invalid = mask == 0
    if no_values:
        nv = np.isin(a, no_values)
        invalid = nv if invalid is None else (invalid | nv)
    if nodata is not None:
        nd = a == nodata
        invalid = nd if invalid is None else (invalid | nd)
    n_invalid = 0 if invalid is None else int(invalid.sum())
    invalid = invalid if invalid is not None and invalid.any() else None
    valid = a[np.isfinite(a) & (a != 0) & ~invalid] if invalid is not None else a[np.isfinite(a) & (a != 0)]
    if len(valid) > 0:
        return np.percentile(valid, 0.5), np.percentile(valid, 99.5), len(valid), n_invalid
    return np.nanmin(a), np.nanmax(a), 0, n_invalid


def fresh_raster(rng, dt, shape):
    if dt == "float32":
        a = (rng.standard_normal(shape) * 100).astype(f32)
        a[rng.random(shape) < 0.05] = 0
        a[rng.random(shape) < 0.03] = f32(-0.0)
        a[rng.random(shape) < 0.03] = np.nan
        a[rng.random(shape) < 0.02] = np.inf
        a[rng.random(shape) < 0.02] = -np.inf
        return a
    info = np.iinfo(dt)
    a = rng.integers(max(info.min, -500), min(info.max, 4000) + 1, shape).astype(dt)
    a[rng.random(shape) < 0.05] = 0
    return a


@pytest.mark.parametrize("dt", G.DTYPES)
def test_range_restatement_equals_numpy_on_fresh_rasters(dt):
    rng = np.random.default_rng(len(dt) * 7 + 1)
    shapes = ((1, 1), (3, 257), (37, 53), (64, 211))
    for shape in shapes:
        a = fresh_raster(rng, dt, shape)
        present = [a[rng.integers(shape[0]), rng.integers(shape[1])].item() for _ in range(16)]
        lists = (None, [], [present[0]], present, [present[1], -1, 70000, 0.5, float("nan"), 0])
        nodatas = (None, 0, 0.0, float("nan"), present[2], np.float64(present[3]), 0.1, -1, 1e40)
        for mask in (None, (rng.random(shape) < 0.7).astype(np.uint8)):
            for no_values in lists:
                for nodata in nodatas:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        want = numpy_range(a, mask, no_values, nodata)
                    got = restated_range(a, mask, no_values, nodata)
                    wmin, wmax = want[0], want[1]
                    if want[2] == 0:
                        wmin, wmax = (np.abs(v) if v == 0 else v for v in (wmin, wmax))
                    assert same(got.v_min, wmin) and same(got.v_max, wmax) and (got.n_valid, got.n_invalid) == want[2:], (shape, no_values, nodata)
                    # the rules the library's argument handling rests on: a value as the pixel type holds it, or no match at all
                    for v in (no_values or []):
                        c = R.representable(v, a.dtype)
                        assert np.array_equal(np.isin(a, [v]), a == c if c is not None else np.zeros(shape, bool)), (dt, v)
                    nd = R.nodata_as_compared(a.dtype, nodata)
                    if nd is not None:
                        c = R.representable(nd, a.dtype)
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore")
                            assert np.array_equal(a == nodata, a == c if c is not None else np.zeros(shape, bool)), (dt, nodata)


def test_range_restatement_edge_counts():
    for n_valid in (0, 1, 2):
        a = np.zeros((4, 7), np.uint16)
        a.ravel()[:n_valid] = (300, 9)[:n_valid]
        r = restated_range(a, None, None, None)
        assert r.n_valid == n_valid and same(r.v_min, numpy_range(a, None, None, None)[0])
    r = restated_range(np.full((3, 3), np.nan, f32), None, None, None)
    assert r.n_valid == 0 and np.isnan(r.v_min) and np.isnan(r.v_max) and np.isnan(r.raster_min)
    r = restated_range(np.array([[-0.0, np.nan], [np.inf, -np.inf]], f32), None, [0], None)
    assert (r.n_valid, r.n_invalid) == (0, 1) and r.v_min == -np.inf and r.v_max == np.inf


def pandas_profile(v, p, b):
    """The reference's mean_profile, written out (commons.py:62-69)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        values, positions = pd.Series(v), pd.Series(p)
        group = pd.DataFrame.from_dict({"val": values, "po": np.floor_divide(positions, b)}).groupby("po")
        pos = (group["po"].first() * b + b // 2).astype(np.int32)
        # (pandas labels the zero group with the sign of its first row; the definition's label is +0.0)
        return R.Profile(key=pos.index.to_numpy().astype(f32) + f32(0), position=pos.to_numpy(), count=group["val"].count().to_numpy(),
                         mean=group["val"].mean().to_numpy(), std=group["val"].std().to_numpy())


def fresh_columns(rng, n, kind):
    v = (rng.standard_normal(n) * 10.0 ** rng.integers(-2, 4)).astype(f32)
    p = (rng.random(n) * 2000 - (600 if kind != "positive" else 0)).astype(f32)
    if kind == "odd" and n:
        v[rng.random(n) < 0.1] = np.nan
        v[rng.random(n) < 0.02] = np.inf
        v[rng.random(n) < 0.02] = -np.inf
        p[rng.random(n) < 0.05] = np.nan
        p[rng.random(n) < 0.03] = np.inf
        p[rng.random(n) < 0.03] = -np.inf
        p[rng.random(n) < 0.03] = f32(-0.0)
        p[rng.random(n) < 0.03] = f32(-0.5)
    if kind == "integer":
        p = np.floor(p)
    return v, p


@pytest.mark.parametrize("b", [1, 7, 20, 100])
def test_profile_restatement_equals_pandas_on_fresh_frames(b):
    rng = np.random.default_rng(b)
    for n in (0, 1, 2, 5, 64, 1000, 5000):
        for kind in ("positive", "integer", "negative", "odd"):
            v, p = fresh_columns(rng, n, kind)
            assert same_profile(R.mean_profile(v, p, b), pandas_profile(v, p, b)), (n, kind)
    v = np.arange(50, dtype=f32)
    assert same_profile(R.mean_profile(v, v * f32(b), b), pandas_profile(v, v * f32(b), b))          # single-row groups
    for x in np.concatenate([fresh_columns(rng, 400, "odd")[1], np.array([-0.0, 0.0, -1e-30, 1e30, -3.0 * b, 16777216.0], f32)]):
        with np.errstate(all="ignore"):
            assert same(R.floor_divide_f32(x, b), np.floor_divide(f32(x), f32(b))), (x, b)


def test_profile_position_outside_int32_is_counted():
    r = R.mean_profile(np.ones(3, f32), np.array([1e12, -1e12, 5], f32), 20)
    assert r.out_of_range == 2 and list(r.position) == [0, 10, 0]
    assert R.group_position(f32(2 ** 31 / 20), 20)[1] is False and R.group_position(f32(-2 ** 31 / 20), 20)[1] is True


# ---- 2. the shared header and the host-build launchers, as a sanitized program -----------------------------------------------------------
MAIN = r"""
#include "k_report.hpp"
#include <cstdio>
#include <vector>
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
// range: {int dtype, H, W, n_values, has_nodata, n_q; long long ss, ms (0: no mask); double nodata} values q raster mask -> kr_range_result
static int range(FILE *in, FILE *out)
{
    struct { int dtype, H, W, n_values, has_nodata, n_q; long long ss, ms; double nodata; } h;
    if (!rd(in, &h, sizeof h) || h.n_values > rp::MAX_NO_VALUES || h.n_q > KR_MAX_Q) return 2;
    const size_t es = h.dtype == KM_U8 ? 1 : h.dtype == KM_F32 ? 4 : 2;
    std::vector<double> values((size_t)h.n_values + 1), q((size_t)h.n_q + 1);
    std::vector<unsigned char> img((size_t)h.H * h.ss * es), mask((size_t)h.H * h.ms);
    if (!rd(in, values.data(), 8 * (size_t)h.n_values) || !rd(in, q.data(), 8 * (size_t)h.n_q) || !rd(in, img.data(), img.size()) ||
        !rd(in, mask.data(), mask.size()))
        return 2;
    rp::tests t = kr_no_tests();
    for (int k = 0; k < h.n_values; k++) kr_add_test(t, h.dtype, values[(size_t)k]);
    if (h.has_nodata) kr_add_test(t, h.dtype, h.nodata);
    kr_range_result res;
    for (int j = 0; j < KR_MAX_Q; j++) res.vi[j] = res.v0[j] = res.v1[j] = -1.0;
    if (kr_display_range(nullptr, img.data(), h.dtype, h.H, h.W, (ptrdiff_t)h.ss, h.ms ? mask.data() : nullptr, (ptrdiff_t)h.ms, t, h.n_q, q.data(), nullptr, &res))
        return 3;
    return wr(out, &res, sizeof res) ? 0 : 2;
}
// profile: {int n, bin} values positions -> counts[KR_COUNTS], then key position count mean std of every group
static int profile(FILE *in, FILE *out)
{
    struct { int n, bin; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    const size_t n = (size_t)h.n, cap = n ? n : 1;
    std::vector<float> v(cap), p(cap), key(cap), mean(cap), sd(cap);
    std::vector<int32_t> pos(cap), cnt(cap);
    std::vector<unsigned long long> ka(cap), kb(cap);
    std::vector<unsigned> flags(cap);
    if (!rd(in, v.data(), 4 * n) || !rd(in, p.data(), 4 * n)) return 2;
    const kr_profile pr = {v.data(), p.data(), h.bin, key.data(), pos.data(), cnt.data(), mean.data(), sd.data()};
    const kr_profile_ws ws = {ka.data(), kb.data(), flags.data()};
    int32_t counts[KR_COUNTS];
    if (kr_mean_profile(nullptr, pr, h.n, ws, counts)) return 3;
    const size_t g = 4 * (size_t)counts[KR_GROUPS];
    return wr(out, counts, sizeof counts) && wr(out, key.data(), g) && wr(out, pos.data(), g) && wr(out, cnt.data(), g) && wr(out, mean.data(), g) &&
           wr(out, sd.data(), g) ? 0 : 2;
}
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const int rc = argv[1][0] == 'r' ? range(in, out) : profile(in, out);
    fclose(in);
    return fclose(out) ? 2 : rc;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")
    d = tmp_path_factory.mktemp("report_main")
    src, exe = d / "report_main.cpp", d / "report_main"
    src.write_text(MAIN)
    san.build(src, exe, shared=False)

    def run(mode, payload):
        fin, fout = d / "in.bin", d / "out.bin"
        fin.write_bytes(payload)
        out = subprocess.run([str(exe), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
        return fout.read_bytes()
    return run


def run_range(program, a, mask, no_values, nodata, percents=(0.5, 99.5), pad=0):
    """-> ops.DisplayRange through the host launcher; `pad` > 0 puts raster and mask into wider, poisoned buffers."""
    buf = np.full((a.shape[0], a.shape[1] + pad), 77, a.dtype)
    buf[:, :a.shape[1]] = a
    mbuf = b""
    ms = 0
    if mask is not None:
        ms = a.shape[1] + (pad + 3 if pad else 0)
        m = np.zeros((a.shape[0], ms), np.uint8)
        m[:, :a.shape[1]] = mask
        mbuf = m.tobytes()
    values = [float(v) for v in (no_values or [])]
    nd = R.nodata_as_compared(a.dtype, nodata)
    q = [float(np.true_divide(p, f32(100) if a.dtype == f32 else 100)) for p in percents]
    head = struct.pack("<6i2qd", _lib._DTYPES[a.dtype], *a.shape, len(values), nd is not None, len(q), buf.shape[1], ms, 0.0 if nd is None else nd)
    raw = program("range", head + np.array(values, np.float64).tobytes() + np.array(q, np.float64).tobytes() + buf.tobytes() + mbuf)
    n_valid, n_invalid = struct.unpack("<2q", raw[:16])
    d = np.frombuffer(raw[16:], np.float64)
    vi, v0, v1, rmin, rmax = d[0:4], d[4:8], d[8:12], a.dtype.type(d[12]), a.dtype.type(d[13])
    k = len(q)
    vals = ops.lerp_as_numpy(v0[:k], v1[:k], vi[:k], n_valid, a.dtype) if n_valid else [rmin, rmax]
    return ops.DisplayRange(vals, n_valid, n_invalid, rmin, rmax)


def same_range(got, want):
    return (same(got.v_min, want.v_min) and same(got.v_max, want.v_max) and (got.n_valid, got.n_invalid) == (want.n_valid, want.n_invalid) and
            same(got.raster_min, want.raster_min) and same(got.raster_max, want.raster_max))


def test_host_range_equals_the_restatement(program, range_cases):
    for name, a, mask, no_values, nodata in range_cases:
        assert same_range(run_range(program, a, mask, no_values, nodata), restated_range(a, mask, no_values, nodata)), name
    rng = np.random.default_rng(5)
    for dt in G.DTYPES:
        a = fresh_raster(rng, dt, (61, 200))
        mask = (rng.random(a.shape) < 0.6).astype(np.uint8)
        nv = [a[3, 3].item(), 0, -1, 0.5, float("nan"), 70000]
        for args in ((None, None, None), (mask, None, None), (None, nv, None), (None, None, a[9, 9].item()), (mask, nv, a[9, 9].item())):
            assert same_range(run_range(program, a, *args, pad=11), restated_range(a, *args)), (dt, args[1:])
        got = run_range(program, a, mask, nv, None, percents=(0, 33.3, 50, 100))
        want = restated_range(a, mask, nv, None, percents=(0, 33.3, 50, 100))
        assert all(same(g, w) for g, w in zip(got.values, want.values)), dt


def run_profile(program, v, p, b):
    raw = program("profile", struct.pack("<2i", v.size, b) + v.tobytes() + p.tobytes())
    counts = np.frombuffer(raw[:16], np.int32)
    g = int(counts[0])
    cols = [np.frombuffer(raw[16 + 4 * g * i:16 + 4 * g * (i + 1)], t) for i, t in enumerate((f32, np.int32, np.int32, f32, f32))]
    assert len(raw) == 16 + 20 * g
    return R.Profile(key=cols[0], position=cols[1], count=cols[2].astype(np.int64), mean=cols[3], std=cols[4], out_of_range=int(counts[1]))


def test_host_profiles_equal_the_restatement(program, profile_cases):
    for name, v, p, b in profile_cases:
        got, want = run_profile(program, v, p, b), R.mean_profile(v, p, b)
        assert same_profile(got, want) and got.out_of_range == 0, name
    rng = np.random.default_rng(8)
    for n in (0, 1, 2, 63, 64, 65, 2049):
        for b in (1, 7, 20, 100, 1 << 24):
            v, p = fresh_columns(rng, n, "odd")
            assert same_profile(run_profile(program, v, p, b), R.mean_profile(v, p, b)), (n, b)
    got = run_profile(program, np.ones(3, f32), np.array([1e12, -1e12, 5], f32), 20)
    want = R.mean_profile(np.ones(3, f32), np.array([1e12, -1e12, 5], f32), 20)
    assert same_profile(got, want) and got.out_of_range == want.out_of_range == 2


# ---- 3. the ABI, the host build, the arguments ----------------------------------------------------------------------------------------------
ENTRY_POINTS = {"km_display_range": "api_prep.hip", "km_display_range_dev": "api_prep.hip", "km_mean_profiles": "api_report.hip",
                "km_mean_profiles_dev": "api_report.hip"}


def test_abi_carries_the_entry_points():
    import ctypes
    header = open(os.path.join(ROOT, "include", "karios_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, home in ENTRY_POINTS.items():
        assert name in _lib.SIGNATURES and f"int {name}(" in header and hasattr(lib, name)
        assert f"int {name}(" in open(os.path.join(ROOT, "karios_amd", "csrc", home)).read()      # a file the host build already lists
    assert ctypes.sizeof(_lib.DisplayRangeResult) == 32 and ctypes.sizeof(_lib.Profile) == 8 * ctypes.sizeof(ctypes.c_void_p)
    for name, value in (("KM_DISPLAY_MAX_NO_VALUES", _lib.DISPLAY_MAX_NO_VALUES), ("KM_PROFILE_MAX", _lib.PROFILE_MAX)):
        assert f"#define {name} {value}" in header
    assert R.MAX_NO_VALUES == _lib.DISPLAY_MAX_NO_VALUES and R.MAX_PROFILE_ROWS == _lib.PROFILE_MAX_ROWS and R.MAX_BIN_SIZE == _lib.PROFILE_MAX_BIN
    assert "k_report.hip" in open(os.path.join(ROOT, "karios_amd", "csrc", "Makefile")).read()


def test_host_build_of_the_api_files_still_links():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "hoststub")], capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-4000:]
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "tests", "hoststub", "_build", "libkarios_host_asan.so")], text=True)
    assert all(f" T {name}\n" in syms for name in ENTRY_POINTS)


def test_argument_errors_raise_without_a_device():
    a = np.ones((4, 4), np.uint16)
    with pytest.raises(ValueError, match="at most 16"):
        ops.display_range(a, no_values=list(range(17)))
    with pytest.raises(_lib.KariosHipError, match="unsupported pixel type"):
        ops.display_range(a.astype(np.float64))
    with pytest.raises(ValueError, match="range"):
        ops.display_range(a, percents=(0.5, 101))
    v = np.zeros(4, f32)
    for n_prof in (0, 9):
        with pytest.raises(ValueError, match="profiles"):
            ops.mean_profiles([(v, v, 20)] * n_prof)
    for b in (0, (1 << 24) + 1, 2.5):
        with pytest.raises(ValueError, match="bin size"):
            ops.mean_profiles([(v, v, b)])
    big = np.zeros((1 << 20) + 1, f32)
    with pytest.raises(ValueError, match="rows"):
        ops.mean_profiles([(big, big, 20)])
    with pytest.raises(ValueError, match="float32"):
        ops.mean_profiles([(v.astype(np.float64), v, 20)])
    with pytest.raises(ValueError, match="length"):
        ops.mean_profiles([(v, v[:3], 20)])


def test_non_float32_columns_take_the_pandas_expression():
    from karios_amd.report import commons
    rng = np.random.default_rng(2)
    v, p = rng.standard_normal(300) * 10.0, np.floor(rng.random(300) * 900).astype(f32)          # dx times a float64 resolution
    got, want = commons.mean_profile(pd.Series(v), pd.Series(p), 20), pandas_profile(v, p, 20)
    assert same(got.mean_values.to_numpy(), want.mean) and same(got.values_std.to_numpy(), want.std) and same(got.nb_pos.to_numpy(), want.count)
    assert same(got.groups_positions.to_numpy(), want.position) and got.grouped_values.ngroups == want.key.size
    lo, hi = got.compute_std_min_max()
    assert len(lo) == len(hi) == want.key.size
