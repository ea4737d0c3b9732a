"""CPU suite: the report's products and the altitude figure's numbers - the key-point rasters of ProductGenerator
(karios/report/product_generator.py:138-218), the altitude column (karios/api/core.py:1049-1053) and the box statistics of
MeanShiftByAltitudeGroupPlot._plot_alt (karios/report/shift_by_alt_plot.py:127-171).

1. tests/products_restatement.py - the definition - against the recorded results of the reference (tests/golden/products.npz) and
   against numpy's fancy indexing, the installed pandas and matplotlib.cbook.boxplot_stats on fresh inputs.
2. csrc/products_math.hpp and the host-build launchers of csrc/k_products.hpp - the text the kernels and the library's host side
   compile - as a stand-alone program built by g++ with -ffp-contract=off under the address and undefined-behaviour sanitizers, files
   in and out, against the restatement by bits.
3. The ABI carries the entry points; the host build of the API files links them; argument errors raise without a device.

Comparisons are by bits; two NaN count as equal.  The sign of a zero is folded for the order statistics and whisker ends only.
"""
import os
import struct
import subprocess
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

import products_restatement as P
import sanitizer_harness as san

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_products as G  # noqa: E402

from karios_amd import _lib, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "products.npz"))
f32 = np.float32
f64 = np.float64


def same(a, b):
    """Same dtype, shape and bits; NaN equals NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        nan = np.isnan(a)
        return bool(np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes())
    return a.tobytes() == b.tobytes()


def folded(a):
    a = np.array(a, copy=True)
    a[a == 0] = 0
    return a


def same_stat(name, got, want):
    return same(folded(got), folded(want)) if name in P.ZERO_FOLDED else same(got, want)


def same_box(got, want):
    return (all(same(getattr(got, k), getattr(want, k)) for k in ("key", "count", "mean", "cls")) and
            all(same_stat(k, getattr(got, k), getattr(want, k)) for k in P.STAT_NAMES))


@pytest.fixture(scope="module")
def raster_cases():
    cases = G.raster_cases()
    for name, x, y, dx, dy, _h, _w in cases:
        assert G.crc(x, y, dx, dy) == int(GOLD[f"crc_{name}"][0]), "the rebuilt frames are not the recorded ones"
    return cases


@pytest.fixture(scope="module")
def altitude_cases():
    cases = G.altitude_cases()
    for name, v, alt, _r, _b in cases:
        assert G.crc(v, alt) == int(GOLD[f"crc_{name}"][0]), "the rebuilt columns are not the recorded ones"
    return cases


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
def test_numpy_facts_the_definition_rests_on():
    row = np.zeros(4, f32)
    row[1] = float(f32(np.nan))
    assert row.view(np.uint32)[1] == P.NAN_FILL_BITS                       # the fill's bits
    r = np.zeros(5)
    r[[2, 2, 2]] = [1, 2, 3]
    assert r[2] == 3                                                       # the last of several assignments to one element wins
    assert list(np.array([-0.9, 0.9, -1.0, 1.99], f32).astype(int)) == [0, 0, -1, 1]
    x = np.random.default_rng(1).standard_normal(778).astype(f32)          # (fractional virtual indices for all three)
    a, b = np.percentile(x, [25, 50, 75]), [np.percentile(x, q) for q in (25, 50, 75)]
    assert a.dtype == f64 and all(type(v) is f32 for v in b) and any(f64(v) != w for v, w in zip(b, a))      # list of percents: float64
    assert same(np.array([32767], np.int16) // 20 * 20 + 10, np.array([-32766], np.int16))
    s = pd.Series(np.ones(3, f32)) * 10
    assert s.dtype == f32 and (np.ones(3, f32) * f64(10)).dtype == f64 and (pd.Series(np.ones(3, f32)) * f64(0.1)).dtype == f32
    assert same((pd.Series(np.full(3, f32(3))) * 0.1).to_numpy(), np.full(3, f32(3)) * f32(0.1))       # a Python number: a float32 product


def test_rasters_restatement_equals_the_reference(raster_cases):
    for name, x, y, dx, dy, h, w in raster_cases:
        mask, delta, bad = P.point_rasters(x, y, dx, dy, h, w)
        assert bad == 0 and same(mask, GOLD[f"mask_{name}"]) and same(delta.view(np.uint32), GOLD[f"delta_{name}"]), name
        only, none, _ = P.point_rasters(x, y, None, None, h, w)
        assert none is None and same(only, mask)


def numpy_rasters(x0, y0, dx, dy, h, w):
    """The reference's two loops without GDAL, on rows it accepts."""
    xi, yi = x0.astype(int), y0.astype(int)
    order = np.argsort(yi, kind="stable")
    mask, delta = np.zeros((h, w), np.uint8), np.full((2, h, w), float(f32(np.nan)), f32)
    for row in np.unique(yi):
        sel = order[yi[order] == row]
        mask[row][xi[sel]] = 1
        delta[0, row][xi[sel]] = dx[sel]
        delta[1, row][xi[sel]] = dy[sel]
    return mask, delta


def test_rasters_restatement_equals_numpy_on_fresh_frames():
    rng = np.random.default_rng(3)
    for h, w, n in ((37, 53, 500), (5, 9, 200), (1, 1, 3), (64, 100, 0), (3, 7, 1)):
        x = (rng.random(n) * 2 * w - w).astype(f32)                        # both halves of the wrap
        y = (rng.random(n) * h).astype(f32)
        x, y = np.clip(x, -w, f32(w) - f32(0.5)), np.minimum(y, f32(h) - f32(0.5))
        dx, dy = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
        mask, delta, bad = P.point_rasters(x, y, dx, dy, h, w)
        want_mask, want_delta = numpy_rasters(x, y, dx, dy, h, w)
        assert bad == 0 and same(mask, want_mask) and same(delta.view(np.uint32), want_delta.view(np.uint32)), (h, w, n)


OUT_OF_RANGE = ((np.nan, 1), (np.inf, 1), (1, -np.inf), (1, -1), (1, 37), (53, 1), (-54, 1), (1e30, 1))


def test_rows_out_of_range_are_counted():
    for k, (x, y) in enumerate(OUT_OF_RANGE):
        xs, ys = np.array([2, x, 3], f32), np.array([2, y, 3], f32)
        mask, delta, bad = P.point_rasters(xs, ys, np.ones(3, f32), np.ones(3, f32), 37, 53)
        assert bad == 1 and mask.sum() == 2 and np.isfinite(delta).sum() == 4, (x, y)
    xs, ys = np.array([p[0] for p in OUT_OF_RANGE], f32), np.array([p[1] for p in OUT_OF_RANGE], f32)
    assert P.point_rasters(xs, ys, None, None, 37, 53)[2] == len(OUT_OF_RANGE)
    raster = np.arange(37 * 53, dtype=np.uint16).reshape(37, 53)
    for x, y in ((np.nan, 1), (1, np.inf), (1, 37), (1, -38), (53, 1), (-54, 1)):
        out, bad = P.sample_points(raster, np.array([x], f32), np.array([y], f32))
        assert bad == 1 and out[0] == 0
        if np.isfinite(x) and np.isfinite(y):
            with pytest.raises(IndexError):
                raster[np.array([y], f32).astype(int), np.array([x], f32).astype(int)]


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16", "float32"])
def test_sampling_restatement_equals_numpy(dtype):
    rng = np.random.default_rng(4)
    raster = (rng.random((37, 53)) * 250).astype(dtype)
    x = (rng.random(400) * 106 - 53).astype(f32)
    y = (rng.random(400) * 74 - 37).astype(f32)
    x, y = np.clip(x, -53, f32(52.5)), np.clip(y, -37, f32(36.5))
    out, bad = P.sample_points(raster, x, y)
    assert bad == 0 and same(out, raster[y.astype(int), x.astype(int)])


def test_box_restatement_equals_the_reference(altitude_cases):
    for name, v, alt, x_res, b in altitude_cases:
        values = v * f32(x_res)
        assert same(values, (pd.Series(v) * x_res).to_numpy())
        got = P.box_stats(values, alt.astype(f32), b)
        if alt.dtype.kind in "ui":
            key, pos = P.integer_labels(got.key, alt.dtype, b)
        else:
            key, pos = got.key, np.array([P_report.group_position(k, b)[0] for k in got.key], np.int32)
        assert same(key, GOLD[f"key_{name}"]) and same(pos, GOLD[f"pos_{name}"]) and same(got.count, GOLD[f"count_{name}"]), name
        assert same(got.mean, GOLD[f"mean_{name}"]), name
        for k in P.STAT_NAMES:
            assert same_stat(k, getattr(got, k), GOLD[f"{k}_{name}"]), (name, k)
        fl = [P.fliers(values[g], got.cls[g]) for g in P.groups_of(values, alt.astype(f32), b)]
        assert same(np.concatenate(fl) if fl else np.zeros(0, f32), GOLD[f"fliers_{name}"]), name
        assert same(np.array([a.size for a in fl], np.int32), GOLD[f"nfliers_{name}"]), name
    assert same(P.integer_labels(np.array([1638], f32), np.int16, 20)[1], np.array([-32766], np.int32))
    assert same(P.integer_labels(np.array([85], f32), np.uint8, 3)[1], np.array([0], np.int32))
    with pytest.raises(OverflowError):
        P.integer_labels(np.array([1], f32), np.int16, 40000)


import report_restatement as P_report  # noqa: E402


def box_cases():
    """-> list of (name, values, positions, bin): the shapes the percentile's interpolation and the pairwise tree turn on."""
    rng = np.random.default_rng(6)
    out = []
    sizes = (1, 2, 3, 4, 5, 127, 128, 129, 8193)
    pos = np.concatenate([np.full(s, 20 * i + 3, f32) for i, s in enumerate(sizes)])
    perm = rng.permutation(pos.size)
    out.append(("sizes", ((rng.standard_normal(pos.size) * 3).astype(f32))[perm], pos[perm], 20))
    out.append(("own_groups", rng.standard_normal(300).astype(f32), (np.arange(300) * 7).astype(f32)[rng.permutation(300)], 7))
    v = rng.standard_normal(200).astype(f32)
    v[17] = np.nan
    out.append(("nan_value", v, np.repeat(np.arange(4, dtype=f32) * 20, 50), 20))
    out.append(("equal", np.full(64, f32(2.5)), np.repeat(np.arange(2, dtype=f32) * 20, 32), 20))
    # q1 = 1, q3 = 3, iqr = 2: the fences are -2 and 6; -2 and 6 lie ON them (inside), -2.5 and 6.5 beyond
    out.append(("fences", np.array([1, 1, 2, 3, 3, -2, 6, -2.5, 6.5, 1, 3, 2, 2], f32), np.zeros(13, f32), 20))
    p = np.array([-0.0, 0.0, -0.25, 0.25, np.nan, np.inf, -np.inf, 19.9, -19.9, 20.0] * 6, f32)
    out.append(("odd_positions", rng.standard_normal(p.size).astype(f32), p, 20))
    out.append(("infinite_values", np.array([1, 2, np.inf, np.inf, np.inf, -np.inf, 1, 2, 3, 4, np.inf, 5], f32), np.repeat(np.array([0, 20, 40], f32), [5, 6, 1]), 20))
    out.append(("zeros", np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], f32), np.zeros(6, f32), 20))
    out.append(("empty", np.zeros(0, f32), np.zeros(0, f32), 20))
    return out


def matplotlib_box(values, positions, b):
    cbook = pytest.importorskip("matplotlib.cbook")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        group = pd.DataFrame({"val": values, "po": np.floor_divide(positions, b)}).groupby("po")["val"]
        arr = [g[1].to_numpy() for g in group]
        stats = cbook.boxplot_stats(arr, whis=1.5, bootstrap=None, autorange=False) if arr else []
    return arr, stats


def check_against_matplotlib(values, positions, b, tag):
    got = P.box_stats(values, positions, b)
    arr, stats = matplotlib_box(values, positions, b)
    groups = P.groups_of(values, positions, b)
    assert len(arr) == got.key.size == len(groups), tag
    for g, (x, st) in enumerate(zip(arr, stats)):
        assert same(x, values[groups[g]]) and got.count[g] == len(x), (tag, g)
        assert same(got.mean[g], st["mean"]), (tag, g)
        for k in P.STAT_NAMES:
            assert same_stat(k, getattr(got, k)[g], f64(st[k])), (tag, g, k)
        assert same(P.fliers(x, got.cls[groups[g]]), st["fliers"]), (tag, g)
    dropped = np.setdiff1d(np.arange(values.size), np.concatenate(groups) if groups else np.zeros(0, int))
    assert (got.cls[dropped] == -1).all()


def test_box_restatement_equals_matplotlib_on_fresh_frames():
    for name, v, p, b in box_cases():
        check_against_matplotlib(v, p, b, name)
    rng = np.random.default_rng(7)
    for n in (1, 2, 5, 64, 1000, 5000):
        for b in (1, 7, 20, 100):
            v = (rng.standard_normal(n) * rng.choice([1, 1, 1, 8], n)).astype(f32)
            check_against_matplotlib(v, (rng.random(n) * 400 - 100).astype(f32), b, (n, b))
    v = (rng.standard_normal(70001) * 5).astype(f32)
    check_against_matplotlib(v, (rng.random(v.size) * 19).astype(f32), 20, "one_group")


# ---- 2. the shared header and the host-build launchers, as a sanitized program -----------------------------------------------------------
MAIN = r"""
#include "k_products.hpp"
#include <cstdio>
#include <vector>
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
// rasters: {int n, H, W, has_mask, has_delta; long long ms, rs, bs} x0 y0 dx dy -> count, the mask buffer (H * ms), the delta buffer (2 * bs);
// both buffers start poisoned: what the launcher leaves alone shows
static int rasters(FILE *in, FILE *out)
{
    struct { int n, H, W, has_mask, has_delta; long long ms, rs, bs; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    const size_t n = (size_t)h.n, cap = n ? n : 1;
    std::vector<float> c(4 * cap);
    if (!rd(in, c.data(), 4 * n) || !rd(in, c.data() + cap, 4 * n) || !rd(in, c.data() + 2 * cap, 4 * n) || !rd(in, c.data() + 3 * cap, 4 * n)) return 2;
    std::vector<uint8_t> mask((size_t)h.H * h.ms, 0xAB);
    std::vector<float> delta((size_t)2 * h.bs, -7.0f);
    const kpd_rasters r = {c.data(), c.data() + cap, c.data() + 2 * cap, c.data() + 3 * cap, h.n, h.H, h.W, h.has_mask ? mask.data() : nullptr, (ptrdiff_t)h.ms,
                           h.has_delta ? delta.data() : nullptr, (ptrdiff_t)h.bs, (ptrdiff_t)h.rs};
    const kpd_rasters_ws ws = {nullptr, nullptr};
    int32_t bad = -1;
    if (kpd_point_rasters(nullptr, r, ws, &bad)) return 3;
    return wr(out, &bad, 4) && wr(out, mask.data(), mask.size()) && wr(out, delta.data(), 4 * delta.size()) ? 0 : 2;
}
// sample: {int dtype, H, W, n; long long stride} raster x0 y0 -> count, out
static int sample(FILE *in, FILE *out)
{
    struct { int dtype, H, W, n; long long stride; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    const size_t es = h.dtype == KM_U8 ? 1 : h.dtype == KM_F32 ? 4 : 2, n = (size_t)h.n, cap = n ? n : 1;
    std::vector<unsigned char> img((size_t)h.H * h.stride * es), res(cap * es);
    std::vector<float> x(cap), y(cap);
    if (!rd(in, img.data(), img.size()) || !rd(in, x.data(), 4 * n) || !rd(in, y.data(), 4 * n)) return 2;
    int32_t bad = -1;
    if (kpd_sample_points(nullptr, img.data(), h.dtype, h.H, h.W, (ptrdiff_t)h.stride, h.n, x.data(), y.data(), res.data(), &bad)) return 3;
    return wr(out, &bad, 4) && wr(out, res.data(), n * es) ? 0 : 2;
}
// box: {int n, bin} values positions -> counts[KPD_COUNTS], key count mean of every group, the stats columns (groups each), cls (n)
static int box(FILE *in, FILE *out)
{
    struct { int n, bin; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    const size_t n = (size_t)h.n, cap = n ? n : 1;
    std::vector<float> v(cap), p(cap), key(cap), mean(cap);
    std::vector<int32_t> cnt(cap);
    std::vector<double> stats(pm::N_STATS * cap);
    std::vector<int8_t> cls(cap);
    std::vector<unsigned long long> ka(cap), kb(cap);
    std::vector<unsigned> flags(cap);
    std::vector<uint32_t> misc(KPD_BOX_MISC_WORDS(cap));
    if (!rd(in, v.data(), 4 * n) || !rd(in, p.data(), 4 * n)) return 2;
    const kpd_box b = {v.data(), p.data(), h.bin, key.data(), cnt.data(), mean.data(), stats.data(), cls.data()};
    const kpd_box_ws ws = {ka.data(), kb.data(), flags.data(), misc.data()};
    int32_t counts[KPD_COUNTS];
    if (kpd_box_stats(nullptr, b, h.n, ws, counts)) return 3;
    const size_t g = (size_t)counts[KPD_GROUPS];
    bool ok = wr(out, counts, sizeof counts) && wr(out, key.data(), 4 * g) && wr(out, cnt.data(), 4 * g) && wr(out, mean.data(), 4 * g);
    for (int s = 0; s < pm::N_STATS && ok; s++) ok = wr(out, stats.data() + (size_t)s * n, 8 * g);
    return ok && wr(out, cls.data(), n) ? 0 : 2;
}
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const int rc = argv[1][0] == 'r' ? rasters(in, out) : argv[1][0] == 's' ? sample(in, out) : box(in, out);
    fclose(in);
    return fclose(out) ? 2 : rc;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")
    d = tmp_path_factory.mktemp("products_main")
    src, exe = d / "products_main.cpp", d / "products_main"
    src.write_text(MAIN)
    san.build(src, exe, shared=False)

    def run(mode, payload):
        fin, fout = d / "in.bin", d / "out.bin"
        fin.write_bytes(payload)
        out = subprocess.run([str(exe), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
        return fout.read_bytes()
    return run


def run_rasters(program, x, y, dx, dy, h, w, mask=True, delta=True, pad=0):
    """-> (mask buffer h x (w + pad), delta buffer 2 x (h + 1) x (w + pad) [one spare row per band], count)."""
    ms = rs = w + pad
    bs = (h + 1) * rs
    zero = np.zeros(x.size, f32)
    head = struct.pack("<5i4x3q", x.size, h, w, mask, delta, ms, rs, bs)
    raw = program("rasters", head + x.tobytes() + y.tobytes() + (zero if dx is None else dx).tobytes() + (zero if dy is None else dy).tobytes())
    bad = struct.unpack("<i", raw[:4])[0]
    m = np.frombuffer(raw[4:4 + h * ms], np.uint8).reshape(h, ms)
    d = np.frombuffer(raw[4 + h * ms:], f32).reshape(2, h + 1, rs)
    return m, d, bad


def check_rasters_program(program, x, y, dx, dy, h, w, tag):
    want_mask, want_delta, want_bad = P.point_rasters(x, y, dx, dy, h, w)
    for pad in (0, 5):
        m, d, bad = run_rasters(program, x, y, dx, dy, h, w, pad=pad)
        assert bad == want_bad and same(m[:, :w], want_mask) and same(d[:, :h, :w].view(np.uint32), want_delta.view(np.uint32)), (tag, pad)
        assert (m[:, w:] == 0xAB).all() and (d[:, h:, :] == -7).all() and (d[:, :, w:] == -7).all(), (tag, pad)   # nothing outside the windows
    m, d, _ = run_rasters(program, x, y, dx, dy, h, w, delta=False)
    assert same(m, want_mask) and (d == -7).all(), tag
    m, d, _ = run_rasters(program, x, y, dx, dy, h, w, mask=False)
    assert (m == 0xAB).all() and same(d[:, :h].view(np.uint32), want_delta.view(np.uint32)), tag


def test_host_rasters_equal_the_restatement(program, raster_cases):
    for name, x, y, dx, dy, h, w in raster_cases:
        check_rasters_program(program, x, y, dx, dy, h, w, name)
    xs, ys = np.array([p[0] for p in OUT_OF_RANGE] + [3], f32), np.array([p[1] for p in OUT_OF_RANGE] + [4], f32)
    check_rasters_program(program, xs, ys, np.arange(xs.size, dtype=f32), -np.arange(xs.size, dtype=f32), 37, 53, "out_of_range")


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16", "float32"])
def test_host_sampling_equals_the_restatement(program, dtype):
    rng = np.random.default_rng(9)
    raster = (rng.random((37, 53)) * 250 - (100 if dtype in ("int16", "float32") else 0)).astype(dtype)
    buf = np.full((37, 60), 77, dtype)
    buf[:, :53] = raster
    x = np.concatenate([(rng.random(300) * 106 - 53).astype(f32), np.array([p[0] for p in OUT_OF_RANGE], f32), np.array([-53, 52.9, -0.9], f32)])
    y = np.concatenate([(rng.random(300) * 74 - 37).astype(f32), np.array([p[1] for p in OUT_OF_RANGE], f32), np.array([-37, 36.9, -0.9], f32)])
    x[:300], y[:300] = np.clip(x[:300], -53, f32(52.5)), np.clip(y[:300], -37, f32(36.5))
    raw = program("sample", struct.pack("<4iq", _lib._DTYPES[np.dtype(dtype)], 37, 53, x.size, 60) + buf.tobytes() + x.tobytes() + y.tobytes())
    want, want_bad = P.sample_points(raster, x, y)
    assert struct.unpack("<i", raw[:4])[0] == want_bad and same(np.frombuffer(raw[4:], dtype), want)


def run_box(program, v, p, b):
    raw = program("box", struct.pack("<2i", v.size, b) + v.tobytes() + p.tobytes())
    counts = np.frombuffer(raw[:16], np.int32)
    g, n, at = int(counts[0]), v.size, 16
    cols = {}
    for name, t in (("key", f32), ("count", np.int32), ("mean", f32)) + tuple((k, f64) for k in P.STAT_NAMES):
        size = g * np.dtype(t).itemsize
        cols[name] = np.frombuffer(raw[at:at + size], t)
        at += size
    assert len(raw) == at + n
    return P.BoxStats(cls=np.frombuffer(raw[at:], np.int8), **cols)


def test_host_box_stats_equal_the_restatement(program, altitude_cases):
    for name, v, p, b in box_cases():
        assert same_box(run_box(program, v, p, b), P.box_stats(v, p, b)), name
    for name, v, alt, x_res, b in altitude_cases:
        values = v * f32(x_res)
        assert same_box(run_box(program, values, alt.astype(f32), b), P.box_stats(values, alt.astype(f32), b)), name
    rng = np.random.default_rng(10)
    for n in (1, 2, 63, 64, 65, 2049):
        for b in (1, 7, 20, 1 << 24):
            v, p = (rng.standard_normal(n) * 4).astype(f32), (rng.random(n) * 300 - 80).astype(f32)
            assert same_box(run_box(program, v, p, b), P.box_stats(v, p, b)), (n, b)
    v = (rng.standard_normal(70001) * 5).astype(f32)
    p = (rng.random(v.size) * 19).astype(f32)
    assert same_box(run_box(program, v, p, 20), P.box_stats(v, p, 20))


# ---- 3. the ABI, the host build, the arguments ----------------------------------------------------------------------------------------------
ENTRY_POINTS = ("km_point_rasters", "km_point_rasters_dev", "km_sample_points", "km_sample_points_dev", "km_box_stats", "km_box_stats_dev")


def test_abi_carries_the_entry_points():
    import ctypes
    header = open(os.path.join(ROOT, "include", "karios_hip.h")).read()
    api = open(os.path.join(ROOT, "karios_amd", "csrc", "api_report.hip")).read()     # a file the host build lists
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and f"int {name}(" in header and hasattr(lib, name) and f"int {name}(" in api
    assert f"#define KM_BOX_STATS {_lib.BOX_STATS}" in header and len(ops.BOX_STAT_NAMES) == _lib.BOX_STATS == len(P.STAT_NAMES)
    assert ops.BOX_STAT_NAMES == P.STAT_NAMES and P.MAX_ROWS == _lib.PROFILE_MAX_ROWS
    assert "k_products.hip" in open(os.path.join(ROOT, "karios_amd", "csrc", "Makefile")).read()


def test_host_build_of_the_api_files_still_links():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "hoststub")], capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-4000:]
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "tests", "hoststub", "_build", "libkarios_host_asan.so")], text=True)
    assert all(f" T {name}\n" in syms for name in ENTRY_POINTS)


def test_argument_errors_raise_without_a_device():
    v = np.zeros(4, f32)
    big = np.zeros((1 << 20) + 1, f32)
    with pytest.raises(ValueError, match="shape"):
        ops.point_rasters(v, v)
    with pytest.raises(ValueError, match="raster of"):
        ops.point_rasters(v, v, shape=(0, 5))
    with pytest.raises(ValueError, match="raster of"):
        ops.point_rasters(v, v, shape=(1 << 16, 1 << 16))
    with pytest.raises(ValueError, match="come together"):
        ops.point_rasters(v, v, v, None, shape=(4, 4))
    with pytest.raises(ValueError, match="float32"):
        ops.point_rasters(v.astype(np.float64), v, shape=(4, 4))
    with pytest.raises(ValueError, match="length"):
        ops.point_rasters(v, v[:3], shape=(4, 4))
    with pytest.raises(ValueError, match="rows"):
        ops.point_rasters(big, big, shape=(4, 4))
    with pytest.raises(ValueError, match="output"):
        ops.point_rasters(v, v, shape=(4, 4), out_mask=np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError, match="output"):
        ops.point_rasters(v, v, v, v, shape=(4, 4), out_delta=np.zeros((2, 4, 4), np.float64))
    with pytest.raises(_lib.KariosHipError, match="unsupported pixel type"):
        ops.sample_points(np.zeros((4, 4), np.float64), v, v)
    with pytest.raises(_lib.KariosHipError, match="2-D"):
        ops.sample_points(np.zeros(4, np.uint8), v, v)
    with pytest.raises(ValueError, match="rows"):
        ops.sample_points(np.zeros((4, 4), np.uint8), big, big)
    for b in (0, (1 << 24) + 1, 2.5):
        with pytest.raises(ValueError, match="bin size"):
            ops.box_stats(v, v, b)
    with pytest.raises(ValueError, match="rows"):
        ops.box_stats(big, big, 20)
    with pytest.raises(ValueError, match="float32"):
        ops.box_stats(v.astype(np.float64), v, 20)
    from karios_amd.report import product_generator, shift_by_alt
    with pytest.raises(ValueError, match="Missing required columns"):
        product_generator.kp_delta(pd.DataFrame({"x0": v, "y0": v}), (4, 4))
    with pytest.raises(OverflowError):
        shift_by_alt.altitude_profile(pd.DataFrame({"x0": v, "y0": v, "dx": v}), np.zeros((4, 4), np.int16), "dx", 10, 40000)
