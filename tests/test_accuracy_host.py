"""CPU suite: KariosAPI.analyze_accuracy (karios/api/core.py:268-328) - the valid-pixel count and GeometricStat.

1. tests/accuracy_restatement.py - the definition - against the recorded results of the reference (tests/golden/accuracy.npz) and
   against the installed numpy / pandas, by bits; the inputs are such that a plain left-to-right sum answers differently.
2. csrc/accuracy_math.hpp and the host-build launchers of csrc/k_accuracy.hpp - the text the kernels and the library's host side
   compile - as a stand-alone program built by g++ with -ffp-contract=off under the address and undefined-behaviour sanitizers,
   files in and out, against the restatement by bits.
3. The GeometricStat mirror's arguments and its line of correl_res.txt; the ABI carries the entry points.
"""
import os
import struct
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import accuracy_restatement as A
import sanitizer_harness as san

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_accuracy as G  # noqa: E402

from karios_amd import _lib, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "accuracy.npz"))
f32 = np.float32
RESULT_BYTES = 144            # sizeof(km_accuracy_result)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)


def same_stats(got, want):
    """15 statistics: min / max / median by value (the sign of a zero is not pinned), the rest by bits."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    by_value = list(A.BY_VALUE)
    rest = [i for i in range(15) if i not in by_value]
    return np.array_equal(got[by_value], want[by_value]) and np.array_equal(bits(got[rest]), bits(want[rest]))


def golden_frame(i, n):
    dx, dy, score = G.frame(n, i)
    assert [G.crc(dx), G.crc(dy), G.crc(score)] == list(GOLD[f"crc_{n}"]), "the rebuilt columns are not the recorded ones"
    assert np.array_equal(bits(score), bits(GOLD[f"score_{n}"]))
    if n <= G.STORE_COLUMNS_UP_TO:
        assert np.array_equal(bits(dx), bits(GOLD[f"dx_{n}"])) and np.array_equal(bits(dy), bits(GOLD[f"dy_{n}"]))
    return dx, dy, score


def columns(kind, n, rng):
    if kind == "noise":
        return (3 * rng.standard_normal(n)).astype(f32)
    if kind == "offset":
        return (1000 + 0.01 * rng.standard_normal(n)).astype(f32)
    if kind == "zero":
        return np.zeros(n, f32)
    return np.full(n, -0.0, f32)


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,n", list(enumerate(G.SIZES)))
def test_restatement_equals_the_reference_results(i, n):
    dx, dy, score = golden_frame(i, n)
    for tag, thr in (("py", G.THRESHOLD), ("f64", np.float64(G.THRESHOLD))):
        for carto in (False, True):
            key = f"{n}_{tag}_{int(carto)}"
            sample, stats = A.statistics(dx, dy, score, thr, carto)
            assert sample == int(GOLD[f"sample_{key}"]) == n + (tag == "f64")
            assert same_stats(stats, GOLD[f"stats_{key}"]), key
            x, y, _c = A.sample(dx, dy, score, thr, carto)
            ce = [A.ce(x, y, p, f) for f in G.FACTORS for p in G.PERCENTS]
            assert np.array_equal(bits(ce), bits(GOLD[f"ce_{key}"])), key


def test_the_threshold_kinds_part_at_the_ulp_rows():
    s = np.array(G.ULP_ROWS + (f32(0.5),), f32)
    ser = pd.Series(s)
    for t, want in ((0.4, [False, True, False, True]), (np.float64(0.4), [True, True, False, True]), (f32(0.4), [False, True, False, True])):
        assert list(ser.gt(t)) == want
        assert list(s.astype(np.float64) > A.threshold_as_double(t)) == want


@pytest.mark.parametrize("kind", ["noise", "offset", "zero", "negzero"])
def test_restatement_equals_numpy_on_every_small_size(kind):
    rng = np.random.default_rng(7)
    order_seen = False
    for n in list(range(0, 301)) + [1000, 8191, 8192, 8193, 16389, 20000]:
        a = columns(kind, n, rng)
        assert bits(A.sum_f32(a)) == bits(np.add.reduce(a)), (kind, n)
        if n == 0:
            continue
        got = A.column_stats(a)
        want = [np.min(a), np.max(a), np.median(a), np.mean(a), np.std(a)]
        assert got[:3] == want[:3] and np.array_equal(bits(got[3:]), bits(want[3:])), (kind, n)
        order_seen |= bits(A.sum_left_to_right(a)) != bits(A.sum_f32(a))
    # the order is under test only where a plain loop answers differently
    assert order_seen == (kind in ("noise", "offset"))


def test_restatement_ce_equals_numpy():
    rng = np.random.default_rng(8)
    for n in list(range(1, 301)) + [8193, 20000]:
        x, y = columns("noise", n, rng), columns("offset", n, rng)
        for factor in (1.0, 10.0, 0.3, f32(0.3)):
            xs, ys = x * factor, y * factor
            v_s = np.sort(np.sqrt(xs * xs + ys * ys))
            assert np.array_equal(bits(v_s), bits(np.sort(A.radial(x, y, factor))))
            for percent in (0.9, 0.95, 0.5):
                p = percent * n
                k = int(p)
                want = v_s[k - 1] + (v_s[k] - v_s[k - 1]) * (p - k)
                assert type(want) is f32 and bits(want) == bits(A.ce(x, y, percent, factor)), (n, factor, percent)
    with pytest.raises(IndexError):
        A.ce(np.zeros(0, f32), np.zeros(0, f32), 0.9, 1.0)
    with pytest.raises(IndexError):
        A.ce(np.ones(4, f32), np.ones(4, f32), 1.0, 1.0)


def test_nan_poisons_like_numpy():
    a = np.array([1, np.nan, 3, -2], f32)
    got, want = A.column_stats(a), [np.min(a), np.max(a), np.median(a), np.mean(a), np.std(a)]
    assert all(np.isnan(g) and np.isnan(w) for g, w in zip(got, want))


@pytest.mark.parametrize("dt", G.DTYPES)
def test_count_restatement_equals_the_reference_expression(dt):
    a, mask = G.raster(dt)
    assert np.array_equal(a.view(np.uint8), GOLD[f"raster_{dt}"].view(np.uint8)) and np.array_equal(mask, GOLD[f"mask_{dt}"])
    assert [A.count_valid_pixels(a), A.count_valid_pixels(a, mask)] == list(GOLD[f"count_{dt}"])
    masked = a.copy()
    masked[mask == 0] = 0
    assert A.count_valid_pixels(a, mask) == np.count_nonzero(masked) and 0 < np.count_nonzero(masked) < np.count_nonzero(a) < a.size


# ---- 2. the shared header and the host-build launchers, as a sanitized program ---------------------------------------------------------
MAIN = r"""
#include "k_accuracy.hpp"
#include <cstdio>
#include <vector>
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
// stats: {int n, carto, n_percent, pad; double thr, factor, percents[8]} dx dy score -> result, 3 sums, 3 header sums, radial of the sample
static int stats(FILE *in, FILE *out)
{
    struct { int n, carto, n_percent, pad; double thr, factor, q[KM_ACC_MAX_PERCENTS]; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    const size_t n = (size_t)h.n, cap = n ? n : 1;
    std::vector<float> dx(cap), dy(cap), sc(cap), cols(3 * cap), bsum(3 * (size_t)ka_nblocks((int)cap));
    if (!rd(in, dx.data(), 4 * n) || !rd(in, dy.data(), 4 * n) || !rd(in, sc.data(), 4 * n)) return 2;
    ka_state st;
    km_accuracy_result res;
    ka_percents pc;
    pc.n = h.n_percent;
    for (int k = 0; k < KM_ACC_MAX_PERCENTS; k++) pc.q[k] = h.q[k];
    if (ka_compact(nullptr, dx.data(), dy.data(), sc.data(), h.n, h.thr, h.carto, cols.data(), &st)) return 3;
    if (ka_block_sums(nullptr, cols.data(), h.n, &st, 0, bsum.data()) || ka_finish(nullptr, bsum.data(), h.n, &st, 0)) return 3;
    float sums[3] = {st.sum[0], st.sum[1], st.sum[2]};
    if (ka_block_sums(nullptr, cols.data(), h.n, &st, 1, bsum.data()) || ka_finish(nullptr, bsum.data(), h.n, &st, 1)) return 3;
    if (ka_order(nullptr, cols.data(), h.n, (float)h.factor, pc, &st, &res)) return 3;
    // the header alone, without the launchers: the sum of each column
    float direct[3];
    for (int col = 0; col < 3; col++) {
        float acc = 0.0f;
        for (int b = 0; b < st.n; b += ac::BLOCK) acc += ac::block_sum(cols.data() + col * (size_t)h.n + b, st.n - b < ac::BLOCK ? st.n - b : ac::BLOCK);
        direct[col] = acc;
    }
    std::vector<float> rad((size_t)(st.n ? st.n : 1));
    for (int i = 0; i < st.n; i++) rad[i] = ac::radial(cols[i], cols[(size_t)h.n + i], (float)h.factor);
    return wr(out, &res, sizeof res) && wr(out, sums, sizeof sums) && wr(out, direct, sizeof direct) && wr(out, rad.data(), 4 * (size_t)st.n) ? 0 : 2;
}
// count: {int dtype, H, W, has_mask; long stride, mstride} raster mask -> count
static int count(FILE *in, FILE *out)
{
    struct { int dtype, H, W, has_mask; long long stride, mstride; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    const size_t es = h.dtype == KM_U8 ? 1 : h.dtype == KM_F32 ? 4 : 2;
    std::vector<unsigned char> img((size_t)h.H * h.stride * es), mask((size_t)h.H * h.mstride + 1);
    if (!rd(in, img.data(), img.size()) || (h.has_mask && !rd(in, mask.data(), mask.size() - 1))) return 2;
    unsigned long long n = 0;
    if (ka_count_valid(nullptr, img.data(), h.dtype, h.H, h.W, (ptrdiff_t)h.stride, h.has_mask ? mask.data() : nullptr, (ptrdiff_t)h.mstride, &n)) return 3;
    return wr(out, &n, sizeof n) ? 0 : 2;
}
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const int rc = argv[1][0] == 's' ? stats(in, out) : count(in, out);
    fclose(in);
    return fclose(out) ? 2 : rc;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")
    d = tmp_path_factory.mktemp("accuracy_main")
    src, exe = d / "accuracy_main.cpp", d / "accuracy_main"
    src.write_text(MAIN)
    san.build(src, exe, shared=False)

    def run(mode, payload):
        fin, fout = d / "in.bin", d / "out.bin"
        fin.write_bytes(payload)
        out = subprocess.run([str(exe), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
        return fout.read_bytes()
    return run


def run_stats(program, dx, dy, score, thr, carto, factor, percents):
    q = list(percents) + [0.0] * (_lib.ACC_MAX_PERCENTS - len(percents))
    head = struct.pack("<4i10d", len(dx), int(carto), len(percents), 0, thr, float(factor), *q)
    raw = program("stats", head + dx.tobytes() + dy.tobytes() + score.tobytes())
    res = _lib.AccuracyResult.from_buffer_copy(raw[:RESULT_BYTES])
    tail = np.frombuffer(raw[RESULT_BYTES:], f32)
    return res, tail[:3], tail[3:6], tail[6:]


def check_against_restatement(program, dx, dy, score, t, carto, factor):
    res, sums, direct, rad = run_stats(program, dx, dy, score, A.threshold_as_double(t), carto, factor, G.PERCENTS)
    x, y, c = A.sample(dx, dy, score, t, carto)
    n, stats = A.statistics(dx, dy, score, t, carto)
    assert res.sample == n and res.n_nan == 0
    order = np.array(res.order, f32)
    if n == 0:
        assert np.isnan(np.array(res.stats, f32)).all() and np.isnan(order).all()
        return
    want_sums = [A.sum_f32(v) for v in (x, y, c)]
    assert np.array_equal(bits(sums), bits(want_sums)) and np.array_equal(bits(direct), bits(want_sums))
    assert same_stats(np.array(res.stats, f32), stats)
    r = A.radial(x, y, factor)
    assert np.array_equal(bits(rad), bits(r))
    s = np.sort(r)
    for k, percent in enumerate(G.PERCENTS):
        lo, hi, _frac = A.ce_ranks(percent, n)
        assert order[2 * k] == s[lo] and order[2 * k + 1] == s[hi]


def test_header_and_host_launchers_equal_the_restatement(program):
    for i, n in enumerate(G.SIZES):
        dx, dy, score = golden_frame(i, n)
        for t, carto, factor in ((0.4, False, 1.0), (np.float64(0.4), True, 0.3), (0.4, True, 10.0)):
            check_against_restatement(program, dx, dy, score, t, carto, factor)
    rng = np.random.default_rng(9)
    for n in list(range(0, 301)) + [70001]:
        for kind in ("noise", "offset") if n < 100 else ("noise",):
            dx, dy = columns(kind, n, rng), columns("offset", n, rng)
            score = rng.random(n).astype(f32)
            check_against_restatement(program, dx, dy, score, 0.25, bool(n & 1), 0.3)
    for kind in ("zero", "negzero"):
        a = columns(kind, 8200, rng)
        res, sums, direct, _rad = run_stats(program, a, a, np.ones(8200, f32), 0.4, False, 1.0, ())
        assert res.sample == 8200 and not bits(sums[:2]).any() and not bits(direct[:2]).any()      # +0, as numpy gives
        assert np.array(res.stats, f32)[3] == 0 and bits(np.array(res.stats, f32)[3:5]).tolist() == [0, 0]
    # nothing above the threshold; a NaN in the sample is counted
    check_against_restatement(program, np.ones(9, f32), np.ones(9, f32), np.zeros(9, f32), 0.4, False, 1.0)
    dx = np.array([1, np.nan, 2, np.nan], f32)
    res, *_ = run_stats(program, dx, np.ones(4, f32), np.array([1, 1, 1, 0], f32), 0.4, False, 1.0, ())
    assert res.sample == 3 and res.n_nan == 1


def run_count(program, a, mask, stride=None, mstride=None):
    H, W = a.shape
    stride, mstride = stride or W, mstride or W
    img = np.full((H, stride), 1, a.dtype)
    if a.dtype == np.float32:
        img.view(np.uint32)[:] = 0x7FC00000          # poison the padding with non-zero pixels
    img[:, :W] = a
    m = np.full((H, mstride), 255, np.uint8)
    if mask is not None:
        m[:, :W] = mask
    head = struct.pack("<4i2q", _lib._DTYPES[a.dtype], H, W, int(mask is not None), stride, mstride)
    raw = program("count", head + img.tobytes() + (m.tobytes() if mask is not None else b""))
    return int(np.frombuffer(raw, np.uint64)[0])


@pytest.mark.parametrize("dt", G.DTYPES)
def test_host_count_equals_the_restatement(program, dt):
    a, mask = G.raster(dt)
    assert run_count(program, a, None) == A.count_valid_pixels(a)
    assert run_count(program, a, mask) == A.count_valid_pixels(a, mask)
    assert run_count(program, a, mask, stride=23, mstride=19) == A.count_valid_pixels(a, mask)
    assert run_count(program, a, np.zeros_like(mask)) == 0


def test_nonzero_test_on_float_bit_patterns(program):
    pat = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7FC00000, 0xFFC00001, 0x7F800000, 0x3F800000], np.uint32)
    a = pat.view(f32).reshape(1, -1)
    assert run_count(program, a, None) == 6 == A.count_valid_pixels(a)
    for j in range(pat.size):
        assert run_count(program, a[:, j:j + 1], None) == int(j >= 2)


# ---- 3. the mirror ------------------------------------------------------------------------------------------------------------------------
def test_geometric_stat_line_equals_the_recorded_one(monkeypatch, tmp_path):
    """The mirror's text of correl_res.txt from the recorded statistics: the device call is replaced by the recorded numbers."""
    from karios_amd.accuracy_analysis import GeometricStat
    from karios_amd.core.configuration import AccuracyAnalysisConfiguration
    for i, n in enumerate(G.SIZES):
        dx, dy, score = golden_frame(i, n)
        stats = dict(zip(ops.ACCURACY_STAT_NAMES, GOLD[f"stats_{n}_py_0"]))
        monkeypatch.setattr(ops, "accuracy_statistics", lambda *a, **k: ops.AccuracyStatistics(n, 0, stats, (), "device"))
        st = GeometricStat(AccuracyAnalysisConfiguration(confidence_threshold=0.4), pd.DataFrame({"dx": dx, "dy": dy, "score": score}))
        st.compute_stats(1000 + n)
        assert st.valid and type(st.mean_x) is f32 and st.sample_pixel == n
        path = tmp_path / f"correl_{n}.txt"
        st.update_statistic_file("ref.tif", "mon.tif", str(path))
        st.update_statistic_file("ref.tif", "mon.tif", str(path))
        assert path.read_text(encoding="utf-8") == str(GOLD["correl_res"][i])
        assert np.array_equal(st.v_x_th, dx[score > f32(0.4)]) and st.v_c_th.size == n
    with pytest.raises(ValueError, match="Missing required columns"):
        GeometricStat(AccuracyAnalysisConfiguration(), pd.DataFrame({"dx": dx, "dy": dy}))


def test_host_path_of_the_wrapper_is_numpy():
    """Columns that are not float32, an np.float64 factor: numpy's own expressions, no device."""
    rng = np.random.default_rng(10)
    dx, dy, score = rng.standard_normal(500), rng.standard_normal(500), rng.random(500)
    res = ops.accuracy_statistics(dx, dy, score, 0.4, carto=True)
    keep = score > 0.4
    assert res.path == "host" and res.sample == keep.sum() and res.stats["mean_y"] == np.mean(-dy[keep]) and res.stats["std_x"] == np.std(dx[keep])
    v_s = np.sort(np.sqrt(dx[keep] ** 2 + dy[keep] ** 2))
    p = 0.9 * keep.sum()
    assert res.ce[0] == v_s[int(p) - 1] + (v_s[int(p)] - v_s[int(p) - 1]) * (p - int(p))
    d32 = [a.astype(f32) for a in (dx, dy, score)]
    res = ops.accuracy_statistics(*d32, 0.4, factor=np.float64(0.3))
    assert res.path == "host" and type(res.ce[0]) is np.float64
    res = ops.accuracy_statistics(dx, dy, score, 2.0)
    assert res.sample == 0 and res.stats is None and res.ce == (None, None)
    with pytest.raises(ValueError):
        ops.accuracy_statistics(d32[0], d32[1][:5], d32[2], 0.4)


def test_abi_carries_the_entry_points():
    import ctypes
    assert ctypes.sizeof(_lib.AccuracyResult) == RESULT_BYTES
    header = open(os.path.join(ROOT, "include", "karios_hip.h")).read()
    for name in ("km_count_valid_pixels", "km_count_valid_pixels_dev", "km_accuracy_stats", "km_accuracy_stats_dev"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header
    assert f"#define KM_ACC_MAX_PERCENTS {_lib.ACC_MAX_PERCENTS}" in header
