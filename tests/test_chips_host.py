"""CPU suite: ChipService.generate_chips (karios/report/chip_service.py) - the key-point selection, the chip windows, the uint8 and
Laplacian chips.

1. tests/chips_restatement.py - the definition - against the recorded results of the reference (tests/golden/chips.npz): selected
   rows, written rows, names, uint8 and Laplacian chips by bytes, the text of chips.csv; and against the installed pandas' evaluation
   of the selection rule on fresh frames.
2. csrc/chips_math.hpp and the host-build launchers of csrc/k_chips.hpp - the text the kernels and the library's host side compile -
   as a stand-alone program built by g++ with -ffp-contract=off under the address and undefined-behaviour sanitizers, files in and
   out, against the restatement by bits.
3. The ABI carries the entry points; the mirror's argument handling where no device is needed.
"""
import logging
import os
import struct
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import chips_restatement as R
import sanitizer_harness as san

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_chips as G  # noqa: E402

from karios_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "chips.npz"))
f32 = np.float32
IMAGE_KEYS = ("ref_u8", "mon_u8", "ref_lap", "mon_lap")


@pytest.fixture(scope="module")
def selections():
    cases = G.selection_cases()
    for name, x0, y0, score, _w, _h in cases:
        assert G.crc(x0, y0, score) == int(GOLD[f"crc_{name}"][0]), "the rebuilt columns are not the recorded ones"
    return cases


@pytest.fixture(scope="module")
def chip_cases():
    cases = G.chip_cases()
    for name, ref, mon, x0, y0, dx, dy, _ks in cases:
        assert G.crc(ref, mon, x0, y0, dx, dy) == int(GOLD[f"crc_{name}"][0]), "the rebuilt rasters are not the recorded ones"
    return cases


def check_chips_against_golden(got, tag):
    """got: dict with written, names, ref_u8 ... of every row -> equal to the recorded rows of `tag`."""
    written = GOLD[f"written_{tag}"]
    assert np.array_equal(np.asarray(got["written"], bool), written), tag
    assert [" ".join(n) for n in got["names"]] == list(GOLD[f"names_{tag}"]), tag
    for key in IMAGE_KEYS:
        if f"{key}_{tag}" in GOLD.files:
            assert np.asarray(got[key])[written].tobytes() == GOLD[f"{key}_{tag}"].tobytes(), (tag, key)
        else:
            assert got[key] is None or not written.any(), (tag, key)
        if got[key] is not None:
            assert not np.asarray(got[key])[~written].any(), (tag, key)


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
def test_select_restatement_equals_the_reference(selections):
    for name, x0, y0, score, width, height in selections:
        for tag, thr in G.THRESHOLDS:
            assert np.array_equal(R.select(x0, y0, score, width, height, thr), GOLD[f"sel_{name}_{tag}"]), (name, tag)
    # the two kinds of threshold part at the row that sits AT float32(0.4)
    assert 0 in GOLD["sel_ulp_py_hi"] and 0 not in GOLD["sel_ulp_f64_hi"]


def test_chips_csv_text_equals_the_reference(selections):
    name, x0, y0, score, width, height = next(c for c in selections if c[0] == G.CSV_CASE)
    frame = G.points_frame(x0, y0, score)
    sel = frame.iloc[R.select(x0, y0, score, width, height, G.THRESHOLD)].astype(np.float64).reset_index(drop=True)
    assert sel.to_csv(sep=";", index=False) == str(GOLD["csv_text"])


def test_chip_restatement_equals_the_reference(chip_cases):
    for name, ref, mon, x0, y0, dx, dy, ksizes in chip_cases:
        for ks in ksizes:
            check_chips_against_golden(R.chips(ref, mon, x0, y0, dx, dy, ks), f"{name}_{G.ktag(ks)}")


def test_window_rule_rounds_the_float64_sum():
    x0, dx = np.array([1001, 1001, 60, 61, 60, 61], f32), np.array([0.49999, 0.5, 0.5, 0.5, -0.5, -0.5], f32)
    _X0, _Y0, X1, _Y1, ok = R.windows(x0, np.full(6, 100, f32), dx, np.zeros(6, f32), (4000, 4000), (4000, 4000))
    assert list(X1) == [1001, 1002, 60, 62, 60, 60] and ok.all()
    assert round(float(x0[0] + dx[0])) == 1002                   # ... where the float32 sum of the ZNCC windows rounds up
    bad = R.windows(np.array([np.nan, 100, 3e9], f32), np.full(3, 100, f32), np.array([0, np.inf, 0], f32), np.zeros(3, f32), (400, 400), (400, 400))
    assert not bad[4].any() and list(bad[0]) == [0, 100, 0] and list(bad[2]) == [0, 0, 0]


def pandas_select(df, width, height, rows=5, cols=5):
    """The selection rule evaluated by pandas on the float32 frame (Series arithmetic with Python floats, Series.median, idxmax)."""
    cw, ch = width / cols, height / rows
    cell = (np.clip(np.floor(df["y0"] / ch).astype(int), 0, rows - 1) * cols + np.clip(np.floor(df["x0"] / cw).astype(int), 0, cols - 1))
    out = []

    def best(part, key):
        cand = part[part[key] == part[key].min()]
        return cand["score"].idxmax() if len(cand) > 1 else cand.index[0]

    for cid in range(rows * cols):
        part = df[cell == cid].copy()
        if part.empty:
            continue
        xs, xe, ys, ye, cx, cy = R.cell_bounds(cid, width, height, rows, cols)
        part["d"] = np.sqrt((part["x0"] - cx) ** 2 + (part["y0"] - cy) ** 2)
        centre = best(part, "d")
        out.append(centre)
        part = part[part.index != centre]
        xm, ym = xs + (xe - xs) / 2, ys + (ye - ys) / 2
        for q, (xl, xh, yl, yh) in enumerate(((xs, xm, ys, ym), (xm, xe, ys, ym), (xs, xm, ym, ye), (xm, xe, ym, ye))):
            m = (part["x0"] >= xl) & (part["x0"] < xh) & (part["y0"] >= yl) & (part["y0"] < yh)
            if q in (1, 3):
                m |= part["x0"] == xh
            if q in (2, 3):
                m |= part["y0"] == yh
            quarter = part[m].copy()
            if quarter.empty:
                continue
            quarter["dev"] = np.abs(quarter["d"] - quarter["d"].median())
            out.append(best(quarter, "dev"))
    return np.array(out, np.int64)


@pytest.mark.parametrize("width,height", [(640, 403), (10980, 10980), (64, 64)])
def test_select_restatement_equals_pandas_on_fresh_frames(width, height):
    rng = np.random.default_rng(width)
    for n in (1, 2, 3, 17, 200, 3000):
        step = 4 if width == 64 else 1                           # few positions: ties in distance, ties in distance and score
        x0 = (np.floor(rng.random(n) * width / step) * step).astype(f32)
        y0 = (np.floor(rng.random(n) * height / step) * step).astype(f32)
        if n >= 17:
            x0[::5], y0[::7] = f32(width), f32(height)           # rows on x_end / y_end of the last column / row
            x0[1::9] += f32(0.37)
        score = (rng.integers(16, 65, n) / 64).astype(f32)
        df = pd.DataFrame({"x0": x0, "y0": y0, "score": score})
        for thr in (0.4, np.float64(0.4), 0.75):
            keep = df[df["score"] >= thr]
            assert np.array_equal(R.select(x0, y0, score, width, height, thr), pandas_select(keep, width, height)), (n, thr)
    df = pd.DataFrame({"x0": x0, "y0": y0, "score": score})
    assert np.array_equal(R.select(x0, y0, score, width, height, 0.4, (3, 7)), pandas_select(df[df["score"] >= 0.4], width, height, 3, 7))


def test_images_restatement_equals_the_oracle():
    from oracle import oracle as O
    rng = np.random.default_rng(3)
    for dt in G.DTYPES:
        chip = (rng.random((57, 57)) * 200 - 50).astype(dt)
        if dt == "float32":
            chip[5, 7] = np.nan
        assert np.array_equal(R.to_uint8(chip), O.to_uint8(chip)), dt
        for k in (1, 3, 5, 7, 9, 11):
            u8, lap = R.images(chip, k)
            assert np.array_equal(lap, O.laplacian_u8(u8, k)) and 0 < lap.mean() < 255, (dt, k)
    assert not R.to_uint8(np.full((57, 57), np.nan, f32)).any() and not R.to_uint8(np.full((57, 57), 7, np.int16)).any()


# ---- 2. the shared header and the host-build launchers, as a sanitized program ---------------------------------------------------------
MAIN = r"""
#include "k_chips.hpp"
#include <cstdio>
#include <vector>
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
// select: {int n, rows, cols, f64; double width, height, thr} x0 y0 score -> count, indices; the distances to the centre of cell 0
static int select(FILE *in, FILE *out)
{
    struct { int n, rows, cols, f64; double width, height, thr; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    const size_t n = (size_t)h.n, cap = n ? n : 1;
    std::vector<float> x(cap), y(cap), s(cap), d(cap);
    if (!rd(in, x.data(), 4 * n) || !rd(in, y.data(), 4 * n) || !rd(in, s.data(), 4 * n)) return 2;
    ch::grid g;
    g.rows = h.rows; g.cols = h.cols; g.width = h.width; g.height = h.height;
    g.thr = h.f64 ? h.thr : (double)(float)h.thr;
    std::vector<int32_t> slots(kch_slots(g)), index(kch_slots(g));
    int32_t count = -1;
    if (kch_select(nullptr, x.data(), y.data(), s.data(), h.n, g, slots.data(), index.data(), &count)) return 3;
    const ch::cell_box b = ch::make_box(g, 0);
    for (size_t i = 0; i < n; i++) d[i] = ch::dist(x[i], y[i], b);
    return wr(out, &count, sizeof count) && wr(out, index.data(), 4 * (size_t)count) && wr(out, d.data(), 4 * n) ? 0 : 2;
}
// chips: {int dtype, Href, Wref, Hmon, Wmon, n, kref, kmon; long sref, smon} ref mon x0 y0 dx dy
//        -> ok windows ref_raw mon_raw ref_u8 mon_u8 [ref_lap] [mon_lap]
static int chips(FILE *in, FILE *out)
{
    struct { int dtype, Href, Wref, Hmon, Wmon, n, kref, kmon; long long sref, smon; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    const size_t es = h.dtype == KM_U8 ? 1 : h.dtype == KM_F32 ? 4 : 2, n = (size_t)h.n, px = n * ch::PIXELS;
    std::vector<unsigned char> ref((size_t)h.Href * h.sref * es), mon((size_t)h.Hmon * h.smon * es);
    std::vector<float> col(4 * n + 1);
    if (!rd(in, ref.data(), ref.size()) || !rd(in, mon.data(), mon.size()) || !rd(in, col.data(), 16 * n)) return 2;
    std::vector<unsigned char> raw(2 * px * es + 1), u8(2 * px + 1), lap(2 * px + 1), ok(n + 1);
    std::vector<int32_t> win(4 * n + 1);
    km_chip_outputs o;
    o.ref_raw = raw.data(); o.mon_raw = raw.data() + px * es;
    o.ref_u8 = u8.data(); o.mon_u8 = u8.data() + px;
    o.ref_lap = h.kref ? lap.data() : nullptr; o.mon_lap = h.kmon ? lap.data() + px : nullptr;
    o.ok = ok.data(); o.windows = win.data();
    const kch_images I = {ref.data(), mon.data(), h.dtype, h.Href, h.Wref, h.Hmon, h.Wmon, (ptrdiff_t)h.sref, (ptrdiff_t)h.smon};
    const kch_rows R = {col.data(), col.data() + n, col.data() + 2 * n, col.data() + 3 * n, h.n};
    if (kch_chips(nullptr, I, R, h.kref, h.kmon, o)) return 3;
    bool good = wr(out, ok.data(), n) && wr(out, win.data(), 16 * n) && wr(out, raw.data(), 2 * px * es) && wr(out, u8.data(), 2 * px);
    if (h.kref) good = good && wr(out, lap.data(), px);
    if (h.kmon) good = good && wr(out, lap.data() + px, px);
    return good ? 0 : 2;
}
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const int rc = argv[1][0] == 's' ? select(in, out) : chips(in, out);
    fclose(in);
    return fclose(out) ? 2 : rc;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")
    d = tmp_path_factory.mktemp("chips_main")
    src, exe = d / "chips_main.cpp", d / "chips_main"
    src.write_text(MAIN)
    san.build(src, exe, shared=False)

    def run(mode, payload):
        fin, fout = d / "in.bin", d / "out.bin"
        fin.write_bytes(payload)
        out = subprocess.run([str(exe), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
        return fout.read_bytes()
    return run


def run_select(program, x0, y0, score, width, height, thr, grid=(5, 5)):
    head = struct.pack("<4i3d", x0.size, grid[0], grid[1], int(isinstance(thr, np.float64)), width, height, float(thr))
    raw = program("select", head + x0.tobytes() + y0.tobytes() + score.tobytes())
    count = int(np.frombuffer(raw[:4], np.int32)[0])
    return np.frombuffer(raw[4:4 + 4 * count], np.int32), np.frombuffer(raw[4 + 4 * count:], f32)


def run_chips(program, ref, mon, x0, y0, dx, dy, ks, pad=0):
    """-> dict like chips_restatement.chips; `pad` > 0 puts the rasters into wider, poisoned buffers."""
    kr, km = R.kernel_sizes(ks)
    n, es = x0.size, ref.dtype.itemsize
    bufs = []
    for a in (ref, mon):
        b = np.full((a.shape[0], a.shape[1] + pad), 201, a.dtype)
        if a.dtype == np.float32:
            b[:] = np.nan
        b[:, :a.shape[1]] = a
        bufs.append(b)
    head = struct.pack("<8i2q", _lib._DTYPES[ref.dtype], *ref.shape, *mon.shape, n, kr, km, bufs[0].shape[1], bufs[1].shape[1])
    raw = program("chips", head + bufs[0].tobytes() + bufs[1].tobytes() + b"".join(c.tobytes() for c in (x0, y0, dx, dy)))
    px, at = n * R.CHIP * R.CHIP, 0

    def take(size, dtype, shape):
        nonlocal at
        at += size
        return np.frombuffer(raw[at - size:at], dtype).reshape(shape)
    shape = (n, R.CHIP, R.CHIP)
    out = {"written": take(n, np.uint8, (n,)) != 0, "windows": take(16 * n, np.int32, (n, 4))}
    out["ref_raw"], out["mon_raw"] = take(px * es, ref.dtype, shape), take(px * es, ref.dtype, shape)
    out["ref_u8"], out["mon_u8"] = take(px, np.uint8, shape), take(px, np.uint8, shape)
    out["ref_lap"] = take(px, np.uint8, shape) if kr else None
    out["mon_lap"] = take(px, np.uint8, shape) if km else None
    assert at == len(raw)
    out["names"] = [(f"REF_{w[0]}_{w[1]}", f"MON_{w[0]}_{w[1]}") for w in out["windows"]]
    return out


def same_chips(got, want):
    assert np.array_equal(got["written"], want["written"]) and np.array_equal(got["windows"], want["windows"])
    for key in ("ref_raw", "mon_raw") + IMAGE_KEYS:
        assert (got[key] is None) == (want[key] is None), key
        if got[key] is not None:
            assert got[key].tobytes() == want[key].tobytes(), key


def test_host_selection_equals_the_restatement(program, selections):
    for name, x0, y0, score, width, height in selections:
        for tag, thr in G.THRESHOLDS:
            got, dist = run_select(program, x0, y0, score, width, height, thr)
            assert np.array_equal(got, GOLD[f"sel_{name}_{tag}"]), (name, tag)
        b = R.cell_bounds(0, width, height, 5, 5)
        assert dist.tobytes() == R.distance(x0, y0, b[4], b[5]).tobytes(), name
    rng = np.random.default_rng(12)
    for n in (0, 1, 2, 63, 64, 65, 1000, 70001):
        x0, y0 = (rng.random(n) * 640).astype(f32), np.floor(rng.random(n) * 403).astype(f32)
        score = (rng.integers(0, 65, n) / 64).astype(f32)
        for grid in ((1, 1), (5, 5), (3, 7)):
            got, _ = run_select(program, x0, y0, score, 640, 403, 0.4, grid)
            assert np.array_equal(got, R.select(x0, y0, score, 640, 403, 0.4, grid)), (n, grid)


def test_host_chips_equal_the_reference_and_the_restatement(program, chip_cases):
    for name, ref, mon, x0, y0, dx, dy, ksizes in chip_cases:
        for ks in ksizes:
            got = run_chips(program, ref, mon, x0, y0, dx, dy, ks)
            check_chips_against_golden(got, f"{name}_{G.ktag(ks)}")
            same_chips(got, R.chips(ref, mon, x0, y0, dx, dy, ks))
    # windows of wider, poisoned buffers; no rows; rows that are not finite
    name, ref, mon, x0, y0, dx, dy, ksizes = next(c for c in chip_cases if c[0] == "types_float32")      # NaN inside the chips
    same_chips(run_chips(program, ref, mon, x0, y0, dx, dy, {"ref": 9, "mon": 1}, pad=19), R.chips(ref, mon, x0, y0, dx, dy, {"ref": 9, "mon": 1}))
    empty = np.zeros(0, f32)
    assert run_chips(program, ref, mon, empty, empty, empty, empty, 3)["written"].size == 0
    odd = [np.array(c, f32) for c in zip((np.nan, 48, 0, 0), (65, 48, np.inf, 0), (3e9, 48, 0, 0), (65, 48, 0, -np.inf), (65, 48, 0, 0))]
    got = run_chips(program, ref, mon, *odd, 3)
    same_chips(got, R.chips(ref, mon, *odd, 3))
    assert list(got["written"]) == [False, False, False, False, True]


# ---- 3. the ABI and the mirror -------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ("km_chip_select", "km_chip_select_dev", "km_chips", "km_chips_dev")


def test_abi_carries_the_entry_points():
    import ctypes
    header = open(os.path.join(ROOT, "include", "karios_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and f"int {name}(" in header and hasattr(lib, name)
    assert ctypes.sizeof(_lib.ChipOutputs) == 8 * ctypes.sizeof(ctypes.c_void_p)
    for name, value in (("KM_CHIP_SIZE", _lib.CHIP_SIZE), ("KM_CHIP_MAX_GRID", _lib.CHIP_MAX_GRID), ("KM_CHIP_PICKS", _lib.CHIP_PICKS)):
        assert f"#define {name} {value}" in header
    # the entry points live in a file the host build already lists
    assert all(f"int {name}(" in open(os.path.join(ROOT, "karios_amd", "csrc", "api_chips.hip")).read() for name in ENTRY_POINTS)


def test_host_build_of_the_api_files_still_links():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "hoststub")], capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-4000:]
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "tests", "hoststub", "_build", "libkarios_host_asan.so")], text=True)
    assert all(f" T {name}\n" in syms for name in ENTRY_POINTS)


def test_kernel_size_lookup():
    from karios_amd.report import chip_service as cs
    assert cs.kernel_sizes(None) == (None, None) and cs.kernel_sizes(5) == (5, 5)
    assert cs.kernel_sizes({"mon": 5}) == (5, 5) and cs.kernel_sizes({"ref": 7}) == (7, 7) and cs.kernel_sizes({}) == (1, 1)
    assert cs.kernel_sizes({"mon": 7, "ref": 11}) == (11, 7) == R.kernel_sizes({"mon": 7, "ref": 11})
    from karios_amd import ops
    assert ops.chip_ksize(None) == 0 and [ops.chip_ksize(k) for k in ops.CHIP_KSIZES] == list(ops.CHIP_KSIZES)
    for bad in (0, 2, 4, 13, -1, 3.5):
        with pytest.raises(ValueError):
            ops.chip_ksize(bad)


def test_mirror_arguments_without_a_device(caplog, tmp_path):
    from karios_amd.core import NumpyRasterImage
    from karios_amd.report import CenterAndQuarterCellPointSelector, ChipService
    img = NumpyRasterImage(np.zeros((64, 64), np.uint16))
    sel = CenterAndQuarterCellPointSelector(640, 403)
    empty = sel.select_points(pd.DataFrame({"x0": [], "y0": [], "score": []}))
    assert isinstance(empty, pd.DataFrame) and empty.empty
    with pytest.raises(ValueError, match="Missing required columns"):
        sel.select_points(pd.DataFrame({"x0": [1.0], "y0": [2.0]}))
    points = pd.DataFrame({"x0": [30.0], "y0": [30.0], "dx": [0.0], "dy": [0.0], "score": [0.2]}, dtype=f32)
    with pytest.raises(ValueError, match="Missing required columns"):
        ChipService().generate_chips(img, img, points.drop(columns="dy"), 0.4)
    with pytest.raises(ValueError, match="kernel size"):
        ChipService().generate_chips(img, img, points, 0.4, laplacian_ksize={"mon": 4})
    with caplog.at_level(logging.WARNING):
        assert ChipService().generate_chips(img, img, points, 0.4, output_dir=tmp_path) is None
        assert ChipService().generate_chips(img, img, points.iloc[:0], 0.4) is None
    assert "No KP found having score gte to confident threshold 0.4" in caplog.text and not os.path.exists(tmp_path / "chips")
