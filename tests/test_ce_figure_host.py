"""CPU suite: the numbers of the circular-error figure (karios/report/circular_error_plot.py).

1. tests/ce_figure_restatement.py - the definition - against the recorded results of the reference (tests/golden/ce_figure.npz)
   and against the installed numpy's and scipy's own evaluation of the reference's expressions on fresh inputs.
2. csrc/ce_math.hpp and the host-build launchers of csrc/k_ce.hpp - the text the kernels and the library's host side compile - as
   a stand-alone program built by g++ with -ffp-contract=off under the address and undefined-behaviour sanitizers, files in and
   out, against the restatement by bits.
3. The ABI carries the entry points; the host build of the API files links them; argument errors raise without a device; what
   the device form does not define goes through numpy / scipy.

Comparisons are by bits; two NaN count as equal whatever their sign and payload.
"""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import accuracy_restatement as A
import ce_figure_cases as K
import ce_figure_restatement as R
import sanitizer_harness as san

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_ce_figure as G  # noqa: E402

from karios_amd import _lib, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "ce_figure.npz"))
f32 = np.float32
same = K.same


@pytest.fixture(scope="module")
def golden_cases():
    cases = G.cases()
    for name, dx, dy, score, _res, _carto in cases:
        assert G.crc(dx, dy, score) == int(GOLD[f"crc_{name}"][0]), "the rebuilt columns are not the recorded ones"
    return cases


@pytest.fixture(scope="module")
def restated(golden_cases):
    return {name: R.figure(dx, dy, score, G.THRESHOLD, res, carto) for name, dx, dy, score, res, carto in golden_cases}


def rows_in_order(x, y, z):
    """The (x, y, z) rows as a set: sorted by their bits."""
    rows = np.stack([np.asarray(a, f32) + f32(0) for a in (x, y, np.nan_to_num(z, nan=3e38))], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


# ---- 1. the definition -----------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference(golden_cases, restated):
    outside = 0
    for name, *_ in golden_cases:
        r = restated[name]
        for axis in "xy":
            hist, bins = getattr(r, f"hist_{axis}"), getattr(r, f"bins_{axis}")
            assert same(hist, GOLD[f"hist_{axis}_{name}"]) and same(bins, GOLD[f"bins_{axis}_{name}"]), (name, axis)
            mu, sigma = getattr(r, f"mu_{axis}"), getattr(r, f"sigma_{axis}")
            with np.errstate(all="ignore"):                                   # the overlay: the reference's expression on the restated numbers
                n = 1 / (sigma * np.sqrt(2 * np.pi)) * np.exp(-((bins - mu) ** 2) / (2 * sigma**2))
                curve = n / (np.sum(n)) * np.sum(hist)
            assert same(curve, GOLD[f"curve_{axis}_{name}"]), (name, axis)
        # numpy's own argsort is not stable: the densities in drawing order are the same, the rows as a set
        assert same(r.scatter_z, GOLD[f"scatter_z_{name}"]), name
        assert same(rows_in_order(r.scatter_x, r.scatter_y, r.scatter_z),
                    rows_in_order(GOLD[f"scatter_x_{name}"], GOLD[f"scatter_y_{name}"], GOLD[f"scatter_z_{name}"])), name
        assert same(r.radial, GOLD[f"radial_{name}"]) and same(np.array([r.ce90, r.ce95]), GOLD[f"ce_{name}"]), name
        outside += int(np.isnan(r.scatter_z).sum())
        assert np.isnan(r.scatter_z[r.sample - int(np.isnan(r.scatter_z).sum()):]).all()                  # NaN last
    assert outside > 50
    assert restated["far_500"].bins_x.size - 1 > R.LDS_BINS and restated["equal_40"].bins_x.size == 2 and restated["zeros_12"].bins_x[0] == -0.5
    assert restated["sample_1"].sample == 1 and restated["quantised_900"].sample > 600


def test_string_block_equals_the_reference(golden_cases):
    from karios_amd.accuracy_analysis import GeometricStat
    for name, dx, dy, score, res, carto in golden_cases:
        x, y, _c = A.sample(dx, dy, score, G.THRESHOLD, carto)
        s = GeometricStat.__new__(GeometricStat)
        s.confidence = G.THRESHOLD
        s.percentage_of_pixel = 100 * np.double(x.size) / np.double(G.VALID_PIXELS)
        for axis, v in (("x", x), ("y", y)):                  # (numpy's own: the sign of a zero median is not pinned by the definition)
            for key, fn in (("min", np.min), ("max", np.max), ("median", np.median), ("mean", np.mean), ("std", np.std)):
                setattr(s, f"{key}_{axis}", fn(v))
        for axis in "xy":
            assert s.get_string_block(res, direction=axis) == str(GOLD[f"text_{axis}_{name}"]), (name, axis)


@pytest.mark.parametrize("res", [1.0, 0.1, 10.0, 30.0])
def test_restatement_equals_numpy_and_scipy_on_fresh_frames(res):
    bins = []
    for kind in K.KINDS:
        for n in (1, 2, 3, 65, 4999):
            dx, dy, score, carto = K.fresh(kind, n, seed=int(res * 10))
            got, want = R.figure(dx, dy, score, K.THRESHOLD, res, carto), K.numpy_figure(dx, dy, score, K.THRESHOLD, res, carto)
            assert got.sample == n and not K.differing(got, want), (kind, n, K.differing(got, want))
            bins.append((kind, n, got.bins_x.size - 1))
    assert max(b for k, n, b in bins if k == "far") > R.LDS_BINS and all(b == 1 for k, n, b in bins if k == "equal")


def test_restatement_of_a_sample_beyond_the_cap_and_of_an_empty_one():
    dx, dy, score, carto = K.beyond_the_cap()
    got = R.figure(dx, dy, score, K.THRESHOLD, 1.0, carto)
    assert got.bins_x.size - 1 > R.MAX_BINS >= got.bins_y.size - 1 and not K.differing(got, K.numpy_figure(dx, dy, score, K.THRESHOLD, 1.0, carto))
    with pytest.raises(ValueError, match="zero-size"):
        R.figure(dx, dy, np.zeros_like(score), K.THRESHOLD, 1.0)


# ---- 2. the shared header and the host-build launchers, as a sanitized program -----------------------------------------------------------
MAIN = r"""
#include "k_ce.hpp"
#include <cstdio>
#include <vector>
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
// {int n, carto, bins_x, bins_y, pad; double thr, res} dx dy score (pad + n + pad floats each, the column in the middle) edges_x edges_y
// grid[22] spline -> block hist_x hist_y counts[100] tail scatter_x scatter_y scatter_z radial (sample each)
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    struct { int n, carto, bins_x, bins_y, pad, unused; double thr, res; } h;
    if (!rd(in, &h, sizeof h) || h.n < 1) return 2;
    const size_t n = (size_t)h.n, len = n + 2 * (size_t)h.pad;
    std::vector<float> dx(len), dy(len), score(len), ex((size_t)h.bins_x + 1), ey((size_t)h.bins_y + 1), grid(2 * (ce::GRID + 1));
    kce_spline sp;
    if (!rd(in, dx.data(), 4 * len) || !rd(in, dy.data(), 4 * len) || !rd(in, score.data(), 4 * len) || !rd(in, ex.data(), 4 * ex.size()) ||
        !rd(in, ey.data(), 4 * ey.size()) || !rd(in, grid.data(), 4 * grid.size()) || !rd(in, &sp, sizeof sp))
        return 2;
    std::vector<float> cols(3 * n), scaled(4 * n), bsum(3 * (size_t)ka_nblocks(h.n)), o(4 * n);
    std::vector<unsigned> hx((size_t)h.bins_x), hy((size_t)h.bins_y), cg(ce::GRID * ce::GRID);
    std::vector<unsigned long long> k0(2 * n), k1(2 * n);
    kce_state s = kce_state();
    if (ka_compact(nullptr, dx.data() + h.pad, dy.data() + h.pad, score.data() + h.pad, h.n, h.thr, h.carto, cols.data(), &s.st) ||
        kce_scale(nullptr, cols.data(), h.n, (float)h.res, scaled.data(), &s) || ka_block_sums(nullptr, scaled.data(), h.n, &s.scaled, 0, bsum.data()) ||
        ka_finish(nullptr, bsum.data(), h.n, &s.scaled, 0) || ka_block_sums(nullptr, scaled.data(), h.n, &s.scaled, 1, bsum.data()) ||
        ka_finish(nullptr, bsum.data(), h.n, &s.scaled, 1) || kce_block(nullptr, &s))
        return 3;
    const kce_axis ax = {ex.data(), hx.data(), h.bins_x}, ay = {ey.data(), hy.data(), h.bins_y};
    if (kce_axis_hist(nullptr, scaled.data(), h.n, &s, ax, ay) || kce_grid_hist(nullptr, scaled.data(), h.n, &s, grid.data(), cg.data()) ||
        kce_density_keys(nullptr, scaled.data(), h.n, &s, &sp, scaled.data() + 3 * n, k0.data()) ||
        kce_sort_gather(nullptr, scaled.data(), scaled.data() + 3 * n, k0.data(), k1.data(), h.n, &s, o.data(), o.data() + n, o.data() + 2 * n, o.data() + 3 * n))
        return 3;
    const size_t got = 4 * (size_t)s.st.n;
    const bool ok = wr(out, &s.block, sizeof s.block) && wr(out, hx.data(), 4 * hx.size()) && wr(out, hy.data(), 4 * hy.size()) && wr(out, cg.data(), 4 * cg.size()) &&
                    wr(out, &s.tail, sizeof s.tail) && wr(out, o.data(), got) && wr(out, o.data() + n, got) && wr(out, o.data() + 2 * n, got) &&
                    wr(out, o.data() + 3 * n, got);
    fclose(in);
    return fclose(out) || !ok ? 2 : 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")
    d = tmp_path_factory.mktemp("ce_main")
    src, exe = d / "ce_main.cpp", d / "ce_main"
    src.write_text(MAIN)
    san.build(src, exe, shared=False)

    def run(payload):
        fin, fout = d / "in.bin", d / "out.bin"
        fin.write_bytes(payload)
        out = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
        return fout.read_bytes()
    return run


def run_figure(program, dx, dy, score, t, res, carto, want, pad=0):
    """The whole figure through the host launchers.  Edges and spline are the restatement's (numpy's linspace, scipy's fit): the
    program's own block is compared with the numbers they were built from."""
    cx, cy = R.centres(want.x_edges), R.centres(want.y_edges)
    tx, ty, c = R.fit(cx, cy, want.counts2d)
    bx, by = want.bins_x.size - 1, want.bins_y.size - 1

    def padded(a):
        return np.concatenate([np.full(pad, 7e30, f32), a, np.full(pad, np.nan, f32)]).tobytes()
    head = struct.pack("<6i2d", dx.size, int(carto), bx, by, pad, 0, A.threshold_as_double(t), float(f32(res)))
    spline = tx.tobytes() + ty.tobytes() + c.tobytes() + np.array([cx[0], cx[-1], cy[0], cy[-1]], f32).tobytes()
    raw = program(head + padded(dx) + padded(dy) + padded(score) + want.bins_x.tobytes() + want.bins_y.tobytes() + want.x_edges.tobytes() +
                  want.y_edges.tobytes() + spline)
    blk = _lib.CeBlock.from_buffer_copy(raw[:64])
    at = 64
    r = R.Figure()
    r.sample = int(blk.sample)
    r.hist_x, at = np.frombuffer(raw, np.uint32, bx, at).astype(np.int64), at + 4 * bx
    r.hist_y, at = np.frombuffer(raw, np.uint32, by, at).astype(np.int64), at + 4 * by
    r.counts2d, at = np.frombuffer(raw, np.uint32, 100, at).astype(np.float64).reshape(10, 10), at + 400
    tail, at = _lib.CeTail.from_buffer_copy(raw[at:at + 32]), at + 32
    cols = np.frombuffer(raw, f32, 4 * r.sample, at).reshape(4, r.sample)
    assert len(raw) == at + 16 * r.sample
    r.scatter_x, r.scatter_y, r.scatter_z, r.radial = cols
    r.mu_x, r.sigma_x, r.mu_y, r.sigma_y = (f32(v) for v in (blk.mu_x, blk.sigma_x, blk.mu_y, blk.sigma_y))
    ext = np.array(blk.ext, f32)
    r.bins_x, r.bins_y = (ops.ce_axis_edges(ext[2 * k], ext[2 * k + 1], ext[4 + 2 * k], ext[5 + 2 * k], r.sample, f32(res)) for k in (0, 1))
    r.x_edges, r.y_edges = ops.ce_grid_edges(ext[4], ext[5]), ops.ce_grid_edges(ext[6], ext[7])
    r.plot_limit = np.max(np.abs(ext[4:8]))
    order = np.array(tail.order, f32)
    r.ce90, r.ce95 = (order[2 * k] + (order[2 * k + 1] - order[2 * k]) * ops.ce_ranks(p, r.sample)[2] for k, p in enumerate((0.9, 0.95)))
    assert tail.n_outside == int(np.isnan(r.scatter_z).sum()) and blk.n_nan == 0
    return r


def test_host_figure_equals_the_restatement_on_the_golden_cases(program, golden_cases, restated):
    for name, dx, dy, score, res, carto in golden_cases:
        got = run_figure(program, dx, dy, score, G.THRESHOLD, res, carto, restated[name])
        assert not K.differing(got, restated[name]), (name, K.differing(got, restated[name]))


def test_host_figure_equals_the_restatement_on_fresh_frames(program):
    for kind, n, res in (("normal", 8193, 10.0), ("quantised", 2049, 1.0), ("far", 700, 0.1), ("equal", 64, 30.0), ("carto", 4999, 30.0)):
        dx, dy, score, carto = K.fresh(kind, n, seed=3)
        want = R.figure(dx, dy, score, K.THRESHOLD, res, carto)
        got = run_figure(program, dx, dy, score, K.THRESHOLD, res, carto, want, pad=5)
        assert not K.differing(got, want), (kind, K.differing(got, want))


# ---- 3. the ABI, the host build, the arguments ----------------------------------------------------------------------------------------------
ENTRY_POINTS = ("km_ce_figure", "km_ce_figure_dev")


def test_abi_carries_the_entry_points():
    import ctypes
    header = open(os.path.join(ROOT, "include", "karios_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    home = open(os.path.join(ROOT, "karios_amd", "csrc", "api_report.hip")).read()          # a file the host build already lists
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and f"int {name}(" in header and hasattr(lib, name) and f"int {name}(" in home
    assert ctypes.sizeof(_lib.CeBlock) == 64 and ctypes.sizeof(_lib.CeTail) == 32 and ctypes.sizeof(_lib.CeJob) == 40 + 19 * ctypes.sizeof(ctypes.c_void_p)
    assert f"#define KM_CE_MAX_BINS {_lib.CE_MAX_BINS}" in header and _lib.CE_MAX_BINS == R.MAX_BINS >= 65536
    math = open(os.path.join(ROOT, "karios_amd", "csrc", "ce_math.hpp")).read()
    assert f"MAX_BINS = {R.MAX_BINS}" in math and f"LDS_BINS = {R.LDS_BINS}" in math
    for k, name in enumerate(("KM_CE_SAMPLE", "KM_CE_COUNTS", "KM_CE_CURVES")):
        assert f"#define {name} {k}" in header
    assert "k_ce.hip" in open(os.path.join(ROOT, "karios_amd", "csrc", "Makefile")).read()


def test_host_build_of_the_api_files_still_links():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "hoststub")], capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-4000:]
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "tests", "hoststub", "_build", "libkarios_host_asan.so")], text=True)
    assert all(f" T {name}\n" in syms for name in ENTRY_POINTS)


def test_argument_errors_raise_without_a_device():
    v = np.zeros(4, f32)
    with pytest.raises(ValueError, match="one length"):
        ops.ce_figure(v, v[:3], v, 0.4, 1.0)
    with pytest.raises(ValueError, match="1-D"):
        ops.ce_figure(v.reshape(2, 2), v.reshape(2, 2), v.reshape(2, 2), 0.4, 1.0)
    with pytest.raises(ValueError, match="not a number"):
        ops.ce_figure(v, v, v, 0.4, "10")
    with pytest.raises(ValueError, match="zero-size"):
        ops.ce_figure(v[:0], v[:0], v[:0], 0.4, 1.0)
    with pytest.raises(ValueError):                                       # numpy's own, through the host expressions
        ops.ce_figure(v.astype(np.float64), v.astype(np.float64), v.astype(np.float64), 0.4, 1.0)


def test_what_the_device_form_does_not_define_goes_through_numpy_and_scipy():
    dx, dy, score, _ = K.fresh("normal", 700, seed=9)
    for cols, res in (((dx.astype(np.float64), dy.astype(np.float64), score), 10.0), ((dx, dy, score), np.float64(10.0))):
        got = ops.ce_figure(*cols, K.THRESHOLD, res, carto=True)
        assert got.path == "host" and not K.differing(got, K.numpy_figure(*cols, K.THRESHOLD, res, True))
        assert got.n_outside == int(np.isnan(got.scatter_z).sum()) > 0


def test_report_module_hands_matplotlib_the_reference_numbers(golden_cases):
    """CircularErrorNumbers on a host-path frame (float64 columns): the arguments of axes.hist / scatter / plot and the text."""
    from karios_amd.report.circular_error import CircularErrorNumbers, rmse
    name, dx, dy, score, res, carto = golden_cases[0]
    want = K.numpy_figure(dx.astype(np.float64), dy.astype(np.float64), score, G.THRESHOLD, res, carto)

    class Stats:
        columns = (dx.astype(np.float64), dy.astype(np.float64), score, G.THRESHOLD, carto)
        sample_pixel, confidence, percentage_of_pixel = want.sample, G.THRESHOLD, 12.3456
        min_x, max_x, mean_x, std_x, min_y, max_y, mean_y, std_y = (f32(v) for v in (-1, 2, 0.25, 0.5, -3, 4, 0.75, 1.5))
    num = CircularErrorNumbers(Stats(), res)
    hist, bins = num.compute_histogram("y")
    assert same(hist, want.hist_y) and same(bins, want.bins_y)
    x, y, z, limit, ce90 = num.ce_scatter()
    assert same(x, want.scatter_x) and same(y, want.scatter_y) and same(z, want.scatter_z) and same(limit, want.plot_limit) and same(ce90, want.ce90)
    pct, v, ce90, ce95 = num.radial_error()
    assert same(v, want.radial) and same(pct, np.linspace(0, 100, want.sample)) and same(ce95, want.ce95)
    b, curve, mu, sigma = num.gaussian("x")
    assert same(mu, want.mu_x) and same(sigma, want.sigma_x) and curve.shape == b.shape == want.bins_x.shape and np.isclose(curve.sum(), want.hist_x.sum())
    lines = num.text_lines(pixel_size_line="Pixel size : 10.0 m")
    assert lines[0] == f"Total Number of Key Point : {want.sample}" and lines[3] == "Pixel size : 10.0 m" and lines[2] == "Percentage of Confident Pixels : 12.35%"
    assert lines[5] == "Easting displacement (meter):" and lines[6] == "\tMin : -10.00 m" and lines[10] == f"\tRMSE : {rmse(f32(0.25), f32(0.5), res):.2f} m"
    assert lines[-2] == f"CE @90 the percentile : {want.ce90:.2f} m" and len(lines) == 22
    assert CircularErrorNumbers(Stats(), None).short_unit == "px"
