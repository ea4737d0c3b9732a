"""CPU suite: the tracker's iterative outlier clip (karios/matcher/klt.py:52-71) as the library computes it.

1. tests/clip_restatement.py - the definition - against its two sources: `karios_amd.frames.sigma_clip` on the installed numpy, by
   index, and the reference's recorded result (tests/golden/outliers.npz); fixtures whose survivors change when the sums run left to
   right show that the summation order is under test.
2. csrc/clip_math.hpp and the host-build launcher of csrc/k_clip.hpp - the text the kernel and the library's host side compile - as a
   stand-alone program built by g++ with -ffp-contract=off under the address and undefined-behaviour sanitizers, files in and out,
   against the restatement by bits: survivors, round counts, whole clipped frame blocks; the leaf table and the combine against
   ac::block_sum for every length 1 .. 8192.
3. The ABI carries the entry point and the option.
"""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import clip_restatement as R
import sanitizer_harness as san

from karios_amd import _lib, frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def fixtures():
    return {name: (dx, dy) for name, dx, dy in R.fixtures()}


@functools.lru_cache(maxsize=None)
def restated(name):
    dx, dy = fixtures()[name]
    return R.sigma_clip(dx, dy)


NAMES = [name for name, _dx, _dy in R.fixtures()]


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference_result():
    g = np.load(os.path.join(ROOT, "tests", "golden", "outliers.npz"))
    keep, rounds = R.sigma_clip(g["x1"] - g["x0"], g["y1"] - g["y0"])
    assert len(g["x0"]) == 400 and len(keep) == 376 and rounds >= 2
    for i, name in enumerate(("x0", "y0", "x1", "y1", "score")):
        assert np.array_equal(bits(g[name][keep]), bits(g[f"out_{i}"]))


@pytest.mark.parametrize("kind", R.KINDS + ("order", "special"))
def test_restatement_equals_numpy_by_index(kind):
    names = [n for n in NAMES if n.startswith(kind + "_")] if kind != "special" else list(R.special_cases())
    assert names
    several_rounds = 0
    for name in names:
        dx, dy = fixtures()[name]
        keep, rounds = restated(name)
        with np.errstate(all="ignore"):
            want = frames.sigma_clip(dx, dy)
        assert np.array_equal(keep, want), name
        assert rounds <= len(dx) + 1 and (rounds == 0) == (len(dx) == 0)
        several_rounds += rounds >= 2
    assert several_rounds >= (1 if kind == "special" else 3)


def test_cases_that_end_empty_and_the_strict_limit():
    sp = R.special_cases()
    for name in ("constant_dx", "constant_dy", "nan_dx", "nan_dy", "single"):
        keep, rounds = restated(name)
        assert len(keep) == 0 and rounds >= 1, name
    assert restated("empty")[1] == 0 and len(restated("empty")[0]) == 0
    dx, _dy = sp["exactly_20"]
    keep, rounds = restated("exactly_20")
    assert rounds == 2 and np.array_equal(keep, np.flatnonzero(np.abs(dx) < 20))      # a `<=` would keep all sixteen in one round
    assert len(keep) == 8


@pytest.mark.parametrize("n,seed", R.ORDER_SENSITIVE)
def test_order_sensitive_fixtures_discriminate(n, seed):
    """The fixture's survivors depend on the summation order: a clip on left-to-right sums keeps another set."""
    dx, dy = R.order_sensitive(n, seed)
    keep, _ = restated(f"order_{n}_{seed}")
    other, _ = R.sigma_clip_left_to_right(dx, dy)
    assert not np.array_equal(keep, other)


def test_there_are_enough_order_sensitive_fixtures():
    assert len(R.ORDER_SENSITIVE) >= 4 and len(set(R.ORDER_SENSITIVE)) == len(R.ORDER_SENSITIVE)


# ---- 2. the shared header and the host-build launcher, as a sanitized program ----------------------------------------------------------
MAIN = r"""
#include "k_clip.hpp"
#include <cstdio>
#include <vector>
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
struct work {
    std::vector<float> u, v;
    std::vector<int32_t> idx, lab;
    explicit work(int rows) : u(kc_ws_rows(rows)), v(kc_ws_rows(rows)), idx(kc_ws_rows(rows)), lab(kc_ws_rows(rows)) {}
    void bind(kc_unit &q) { q.u = u.data(); q.v = v.data(); q.idx = idx.data(); q.lab = lab.data(); }
};
// columns: {int units} then per unit {int n} dx dy -> per unit {count, rounds} and `count` indices.  All units in ONE launcher call
static int columns(FILE *in, FILE *out)
{
    int units;
    if (!rd(in, &units, sizeof units) || units < 1 || units > KC_UNITS_MAX) return 2;
    std::vector<std::vector<float>> dx(units), dy(units);
    std::vector<std::vector<int32_t>> keep(units);
    std::vector<work> w;
    std::vector<km_clip_result> rec(units);
    kc_units A;
    for (int k = 0; k < units; k++) {
        int n;
        if (!rd(in, &n, sizeof n) || n < 0 || n > cl::MAX_ROWS) return 2;
        dx[k].resize(n); dy[k].resize(n); keep[k].assign(n, -1);
        if (!rd(in, dx[k].data(), 4 * (size_t)n) || !rd(in, dy[k].data(), 4 * (size_t)n)) return 2;
        w.emplace_back(n);
    }
    for (int k = 0; k < units; k++) {
        kc_unit &q = A.u[k];
        q = kc_unit();
        q.dx = dx[k].data(); q.dy = dy[k].data(); q.n = (int)dx[k].size(); q.keep_index = keep[k].data(); q.rec = &rec[k];
        w[k].bind(q);
    }
    if (kc_clip_units(nullptr, A, units)) return 3;
    for (int k = 0; k < units; k++)
        if (!wr(out, &rec[k], sizeof rec[k]) || !wr(out, keep[k].data(), 4 * (size_t)rec[k].count)) return 2;
    return 0;
}
// block: {int cap, words} block -> {count, rounds} block
static int block(FILE *in, FILE *out)
{
    int h[2];
    if (!rd(in, h, sizeof h) || h[0] < 1 || h[0] > cl::MAX_ROWS || h[1] < 4 + 6 * h[0]) return 2;
    std::vector<float> b((size_t)h[1]);
    if (!rd(in, b.data(), 4 * b.size())) return 2;
    work w(h[0]);
    km_clip_result rec;
    kc_units A;
    kc_unit &q = A.u[0];
    q = kc_unit();
    q.frame = (char *)b.data(); q.cap = h[0]; q.rec = &rec;
    w.bind(q);
    if (kc_clip_units(nullptr, A, 1)) return 3;
    return wr(out, &rec, sizeof rec) && wr(out, b.data(), 4 * b.size()) ? 0 : 2;
}
// tree: 8192 floats -> {lengths whose leaf table + combine differ from ac::block_sum or whose leaves do not tile [0, n), most leaves}
static int tree(FILE *in, FILE *out)
{
    std::vector<float> a(ac::BLOCK);
    if (!rd(in, a.data(), 4 * a.size())) return 2;
    int res[2] = {0, 0};
    for (int n = 1; n <= ac::BLOCK; n++) {
        unsigned short off[cl::LEAVES_MAX], len[cl::LEAVES_MAX];
        float leaf[cl::LEAVES_MAX];
        const int nl = cl::leaf_table(n, off, len);
        if (nl > cl::LEAVES_MAX) return 4;
        bool ok = true;
        int at = 0;
        for (int k = 0; k < nl; k++) {
            ok = ok && off[k] == at && len[k] >= 1 && len[k] <= ac::LEAF;
            at += len[k];
            leaf[k] = ac::leaf_sum(a.data() + off[k], len[k]);
            ok = ok && ac::f32_bits(leaf[k]) == ac::f32_bits(cl::leaf_sum<false>(a.data() + off[k], len[k], 0.0f));
        }
        ok = ok && at == n && ac::f32_bits(cl::combine(leaf, n)) == ac::f32_bits(ac::block_sum(a.data(), n));
        ok = ok && ac::f32_bits(cl::sum_f32<false>(a.data(), n, 0.0f)) == ac::f32_bits(0.0f + ac::block_sum(a.data(), n));
        res[0] += ok ? 0 : 1;
        res[1] = nl > res[1] ? nl : res[1];
    }
    return wr(out, res, sizeof res) ? 0 : 2;
}
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const int rc = argv[1][0] == 'c' ? columns(in, out) : argv[1][0] == 'b' ? block(in, out) : tree(in, out);
    fclose(in);
    return fclose(out) ? 2 : rc;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")
    d = tmp_path_factory.mktemp("clip_main")
    src, exe = d / "clip_main.cpp", d / "clip_main"
    src.write_text(MAIN)
    san.build(src, exe, shared=False)

    def run(mode, payload):
        fin, fout = d / "in.bin", d / "out.bin"
        fin.write_bytes(payload)
        out = subprocess.run([str(exe), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
        return fout.read_bytes()
    return run


def run_columns(program, units):
    """[(dx, dy), ...] through ONE call of the host launcher -> [(indices, rounds), ...]."""
    payload = struct.pack("<i", len(units))
    for dx, dy in units:
        payload += struct.pack("<i", len(dx)) + np.ascontiguousarray(dx, f32).tobytes() + np.ascontiguousarray(dy, f32).tobytes()
    raw = np.frombuffer(program("columns", payload), np.int32)
    out, at = [], 0
    for _ in units:
        count, rounds = int(raw[at]), int(raw[at + 1])
        out.append((raw[at + 2:at + 2 + count].astype(np.int64), rounds))
        at += 2 + count
    assert at == raw.size
    return out


def test_host_launcher_equals_the_restatement(program):
    for start in range(0, len(NAMES), 16):
        names = NAMES[start:start + 16]
        got = run_columns(program, [fixtures()[n] for n in names])
        for name, (keep, rounds) in zip(names, got):
            want, want_rounds = restated(name)
            assert np.array_equal(keep, want) and rounds == want_rounds, name


def make_block(dx, dy, cap, rng, score_words=0):
    """A frame block whose kept list in corner order is (dx, dy): rows in a random (x0, y0) order, column 5 = the corner position."""
    n = len(dx)
    label = rng.permutation(n).astype(np.int32)
    block = rng.random(4 + 6 * cap + score_words).astype(f32)          # (rows behind the count and the score columns: anything)
    block[:4].view(np.int32)[:] = (n, n + 11, 0, 12345)
    body = block[4:4 + 6 * cap].reshape(6, cap)
    body[0, :n], body[1, :n] = np.arange(n, dtype=f32), (7 * np.arange(n) % 13).astype(f32)
    body[2, :n], body[3, :n] = dx[label], dy[label]
    body[4, :n] = rng.random(n).astype(f32)
    body[5, :n] = label.view(f32)
    return block


@pytest.mark.parametrize("name", ["tails_1", "tails_257", "far_1000", "offset_8193", "order_8969_2", "order_12000_5", "tails_20000", "far_32768",
                                  "nan_dx", "constant_dy", "exactly_20"])
def test_host_launcher_clips_whole_frame_blocks(program, name):
    dx, dy = fixtures()[name]
    rng = np.random.default_rng(len(dx))
    cap = min(len(dx) + 3, R.MAX_ROWS)
    block = make_block(dx, dy, cap, rng, score_words=2 * cap)
    raw = program("block", struct.pack("<2i", cap, block.size) + block.tobytes())
    count, rounds = (int(v) for v in np.frombuffer(raw[:8], np.int32))
    got = np.frombuffer(raw[8:], f32)
    want, want_rounds = R.clip_block(block, cap)
    keep, _ = restated(name)
    assert count == len(keep) and rounds == want_rounds == restated(name)[1]
    assert np.array_equal(got[:4].view(np.int32), want[:4].view(np.int32)) and got[:1].view(np.int32)[0] == count
    g, w = got[4:4 + 6 * cap].reshape(6, cap)[:, :count], want[4:4 + 6 * cap].reshape(6, cap)[:, :count]
    assert np.array_equal(bits(g), bits(w))
    assert np.array_equal(bits(got[4 + 6 * cap:]), bits(block[4 + 6 * cap:]))          # the score columns are not the clip's
    # the labels are the positions among the survivors, the rows are still in frame order
    assert np.array_equal(np.sort(g[5].view(np.int32)), np.arange(count)) and np.all(np.diff(g[0]) > 0)


def test_leaf_table_and_combine_equal_block_sum_for_every_length(program):
    rng = np.random.default_rng(11)
    a = (1000 + 3 * rng.standard_normal(8192)).astype(f32)
    bad, most = np.frombuffer(program("tree", a.tobytes()), np.int32)
    assert bad == 0 and 64 <= most <= 127


# ---- 3. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_carries_the_entry_point_and_the_option():
    header = open(os.path.join(ROOT, "include", "karios_hip.h")).read()
    assert "km_sigma_clip_dev" in _lib.SIGNATURES and "int km_sigma_clip_dev(" in header
    assert '"frame_clip"' in header and "not applied here" not in header
    import ctypes
    assert ctypes.sizeof(_lib.ClipResult) == 8
