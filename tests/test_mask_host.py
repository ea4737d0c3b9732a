"""CPU suite: vector masks - the polygon burn of rasterize_vector_mask (karios/core/image.py:104-191,
gdal.RasterizeLayer(..., options=['BURN=1', 'ALL_TOUCHED=TRUE'])) and the AND of _load_mask (karios/api/core.py:593-612).

No recorded GDAL results exist: GDAL is installed nowhere this project is built or tested, so tests/rasterize_restatement.py - written
from knowledge of GDAL 3.x - is the definition, and what it is checked against here is exact geometry.  A live cross-check runs where
`import osgeo` works (it is skipped elsewhere).

1. The restatement: its known answers; its fill against the even-odd rule at pixel centres and its line pass against the set of
   pixels whose closed square meets a segment, both in exact rational arithmetic; its two forms of the fill against each other.
2. csrc/mask_math.hpp and the host-build launchers of csrc/k_mask.hpp - the text the kernels and the library's host side compile - as a
   stand-alone program built by g++ with -ffp-contract=off under the address and undefined-behaviour sanitizers, files in and out,
   against the restatement by bytes on the shared case list (tests/mask_cases.py).
3. The ABI carries the entry points; the host build of the API files links them; argument errors raise without a device; GeoJSON
   parsing and the world-to-pixel transform against hand-computed values.
"""
import json
import math
import os
import random
import struct
import subprocess
from fractions import Fraction as Fr

import numpy as np
import pytest

import mask_cases as M
import rasterize_restatement as R
import sanitizer_harness as san

from karios_amd import _lib, ops  # noqa: E402
from karios_amd.ops import mask as ops_mask  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def expected():
    """name -> (fill, lines, stats) of every shared case, computed once."""
    out = {}
    for name, features, H, W, _options in M.cases():
        stats = R.Stats()
        fill, lines = R.rasterize_parts(features, H, W, stats=stats)
        out[name] = (fill, lines, stats)
    return out


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
def test_known_answers(expected):
    ring = R.geo_to_pixel([[10, 90], [50, 90], [50, 50], [10, 50], [10, 90]], [0, 1, 0, 100, 0, -1])     # the reference's own test input
    assert ring == [(10.0, 10.0), (50.0, 10.0), (50.0, 50.0), (10.0, 50.0), (10.0, 10.0)]
    fill, lines = R.rasterize_parts([[ring]], 100, 100)
    want = np.zeros((100, 100), np.uint8)
    want[10:51, 10:51] = 1
    assert np.array_equal(fill | lines, want) and int((fill | lines).sum()) == 1681
    want[:] = 0
    want[10:50, 10:50] = 1
    assert np.array_equal(fill, want) and int(fill.sum()) == 1600
    assert np.array_equal(expected["reference_input"][0], fill)

    fill, lines, _ = expected["half_open_rules"]                # top row in, left column out
    want = np.zeros((10, 10), np.uint8)
    want[2:7, 3:8] = 1
    assert np.array_equal(fill, want)
    frame = np.zeros((10, 10), np.uint8)
    frame[2, 2:8] = frame[6, 2:8] = 1
    frame[2:7, 2] = frame[2:7, 7] = 1
    assert np.array_equal(lines, frame)


def exact_fill(rings, H, W):
    """Even-odd at pixel centres: a centre is inside iff an odd number of edges cross its row's centre line strictly left of it; an
    edge owns its upper end (min y <= centre < max y)."""
    out = np.zeros((H, W), np.uint8)
    edges = [(Fr(a[0]), Fr(a[1]), Fr(b[0]), Fr(b[1])) for ring in rings for a, b in zip(ring[:-1], ring[1:])]
    for y in range(H):
        cy = Fr(2 * y + 1, 2)
        xs = [x1 + (cy - y1) * (x2 - x1) / (y2 - y1) for x1, y1, x2, y2 in edges if y1 != y2 and min(y1, y2) <= cy < max(y1, y2)]
        for x in range(W):
            out[y, x] = sum(1 for v in xs if v < Fr(2 * x + 1, 2)) & 1
    return out


def segment_meets_square(x0, y0, x1, y1, ix, iy):
    """Exact: the closed segment meets the closed square [ix, ix + 1] x [iy, iy + 1] (Liang-Barsky on rationals)."""
    t0, t1, dx, dy = Fr(0), Fr(1), x1 - x0, y1 - y0
    for p, q in ((-dx, x0 - ix), (dx, ix + 1 - x0), (-dy, y0 - iy), (dy, iy + 1 - y0)):
        if p == 0:
            if q < 0:
                return False
            continue
        r = q / p
        if p < 0:
            t0 = max(t0, r)
        else:
            t1 = min(t1, r)
        if t0 > t1:
            return False
    return True


def exact_touched(rings, H, W):
    out = np.zeros((H, W), np.uint8)
    for ring in rings:
        for a, b in zip(ring[:-1], ring[1:]):
            x0, y0, x1, y1 = Fr(a[0]), Fr(a[1]), Fr(b[0]), Fr(b[1])
            for ix in range(max(math.floor(min(a[0], b[0])) - 1, 0), min(math.floor(max(a[0], b[0])) + 1, W - 1) + 1):
                if a[0] == b[0]:
                    lo, hi = min(a[1], b[1]), max(a[1], b[1])
                else:                                   # (float: only picks the rows worth the exact test, with a margin of one)
                    ya, yb = (a[1] + (c - a[0]) * (b[1] - a[1]) / (b[0] - a[0]) for c in (ix - 1.0, ix + 2.0))
                    lo, hi = max(min(ya, yb), min(a[1], b[1])), min(max(ya, yb), max(a[1], b[1]))
                for iy in range(max(math.floor(lo) - 1, 0), min(math.floor(hi) + 1, H - 1) + 1):
                    if not out[iy, ix] and segment_meets_square(x0, y0, x1, y1, ix, iy):
                        out[iy, ix] = 1
    return out


def corner_within(rings, ix, iy, eps):
    """Some corner of the pixel lies within eps of some segment (float: the distance only has to be told from 1e-6)."""
    for ring in rings:
        for (ax, ay), (bx, by) in zip(ring[:-1], ring[1:]):
            dx, dy = bx - ax, by - ay
            for cx, cy in ((ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1)):
                t = 0.0 if dx == dy == 0 else min(1.0, max(0.0, ((cx - ax) * dx + (cy - ay) * dy) / (dx * dx + dy * dy)))
                if math.hypot(ax + t * dx - cx, ay + t * dy - cy) < eps:
                    return True
    return False


def test_restatement_equals_exact_geometry():
    """Seeded random polygons, 1 - 2 rings of 3 - 8 vertices, uniform in [-6, W + 6] x [-6, H + 6] on a 24 x 40 grid: equality is the
    condition, not a tolerance.  A polygon with an edge whose |dx| or |dy| is below .01 is drawn again: there the line pass takes GDAL's
    axis-parallel shortcut (one column, or one row), which is not exact geometry on purpose.  A mismatching pixel with a corner
    within 1e-6 of a segment would be excluded by name, at most 0.1 % of the touched pixels: none has occurred."""
    H, W = 24, 40
    rng = random.Random(5)
    touched = excluded = polygons = 0
    stats = R.Stats()
    while polygons < 60:
        rings = M.random_polygon(rng, H, W)
        if any(abs(a[0] - b[0]) < .01 or abs(a[1] - b[1]) < .01 for ring in rings for a, b in zip(ring[:-1], ring[1:])):
            continue
        polygons += 1
        fill, lines = R.rasterize_parts([rings], H, W, stats=stats)
        assert np.array_equal(fill, exact_fill(rings, H, W)), polygons
        want = exact_touched(rings, H, W)
        touched += int(want.sum())
        for iy, ix in np.argwhere(lines != want):
            assert corner_within(rings, int(ix), int(iy), 1e-6), (polygons, int(iy), int(ix), int(lines[iy, ix]), int(want[iy, ix]))
            excluded += 1
    assert touched > 5000 and excluded <= touched // 1000, (touched, excluded)
    assert stats.refused_columns == 0 and stats.max_cap_fraction < 0.5


def test_fill_forms_agree_and_counts_are_even(expected):
    """The pairs rule and the prefix-parity form the device uses give the same bytes; every row of every feature collects an even
    number of crossings, which the equivalence rests on."""
    rng = random.Random(7)
    extra = [(f"random_{k}", [M.random_polygon(rng, 24, 40) for _ in range(2)], 24, 40, {}) for k in range(40)]
    for name, features, H, W, _options in M.cases() + extra:
        if name == "star_5000":
            continue                                    # (its crossings are counted below on a coarser copy: the pure-Python pass is slow)
        rows_a, rows_b, counts = [bytearray(W) for _ in range(H)], [bytearray(W) for _ in range(H)], []
        for rings in R.normalize(features, H, W):
            R.fill_feature(rings, H, W, rows_a, counts=counts)
            R.fill_feature(rings, H, W, rows_b, parity=True)
        assert rows_a == rows_b, name
        assert all(c % 2 == 0 for c in counts), name
        if name in expected:
            assert b"".join(bytes(r) for r in rows_a) == expected[name][0].tobytes(), name
    counts = []
    R.fill_feature(R.normalize([[M.star(31.7, 32.2, 40.0, 11.0, 500)]], 64, 64)[0], 64, 64, [bytearray(64) for _ in range(64)], counts=counts)
    assert counts and all(c % 2 == 0 for c in counts) and max(counts) > 2


def test_no_walk_comes_near_its_cap(expected):
    for name, (_fill, _lines, stats) in expected.items():
        assert stats.refused_columns == 0 and stats.max_cap_fraction < 0.5, (name, stats.max_steps)
    assert any(stats.walks > 0 for _f, _l, stats in expected.values())
    rng = random.Random(9)
    stats = R.Stats()
    for _ in range(300):                                # single segments, far outside the raster too
        H, W = rng.choice(((1, 1), (3, 50), (50, 3), (24, 40)))
        seg = [(rng.uniform(-3 * W - 5, 4 * W + 5), rng.uniform(-3 * H - 5, 4 * H + 5)) for _ in range(2)]
        R.rasterize_parts([[seg]], H, W, stats=stats)
    assert stats.refused_columns == 0 and stats.max_cap_fraction < 0.5 and stats.walks > 100


def test_domain_errors_of_the_restatement():
    for bad in (float("nan"), float("inf"), 2.0 ** 30 + 1024.0, -2.0 ** 31):
        with pytest.raises(ValueError):
            R.rasterize([[[(1.0, 1.0), (bad, 2.0), (3.0, 3.0)]]], 8, 8)
    with pytest.raises(ValueError):
        R.rasterize([], 0, 8)
    with pytest.raises(ValueError):
        R.rasterize([], 1 << 16, 1 << 16)
    assert R.rasterize([[[(2.0 ** 30, -2.0 ** 30), (1.0, 1.0), (3.0, 5.0)]]], 8, 8).shape == (8, 8)


def test_live_gdal_where_it_is_installed(expected):
    """Parity with GDAL itself is unpinned: this runs only where osgeo can be imported, which is nowhere this project is tested."""
    osgeo = pytest.importorskip("osgeo")
    from osgeo import gdal, ogr
    for name, features, H, W, _options in M.cases():
        features = [f for f in R.normalize(features, H, W) if f]
        if not features or name.startswith("far_"):
            continue
        ds = gdal.GetDriverByName("MEM").Create("", W, H, 1, gdal.GDT_Byte)
        ds.SetGeoTransform([0, 1, 0, 0, 0, 1])
        src = ogr.GetDriverByName("Memory").CreateDataSource("m")
        layer = src.CreateLayer("l", geom_type=ogr.wkbMultiPolygon)
        for rings in features:
            geom = ogr.Geometry(ogr.wkbPolygon)         # (all rings in one polygon: the same ring list reaches the burn)
            for ring in rings:
                lr = ogr.Geometry(ogr.wkbLinearRing)
                for x, y in ring:
                    lr.AddPoint_2D(x, y)
                geom.AddGeometry(lr)
            feat = ogr.Feature(layer.GetLayerDefn())
            feat.SetGeometry(geom)
            layer.CreateFeature(feat)
        gdal.RasterizeLayer(ds, [1], layer, options=["BURN=1", "ALL_TOUCHED=TRUE"])
        assert np.array_equal(ds.GetRasterBand(1).ReadAsArray(), expected[name][0] | expected[name][1]), (name, osgeo.__version__)


# ---- 2. the shared header and the host-build launchers, as a sanitized program -----------------------------------------------------------
MAIN = r"""
#include "k_mask.hpp"
#include <cstdio>
#include <vector>
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
// polygons: {int H, W, nv, nr, nf, pad; long long stride} xy ring_sizes feature_rings -> {int refused, flag}, the buffer (H * stride),
// which starts poisoned: what the launchers leave alone shows
static int polygons(FILE *in, FILE *out)
{
    struct { int H, W, nv, nr, nf, pad; long long stride; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    std::vector<double> xy(2 * (size_t)h.nv + 1);
    std::vector<int32_t> rs((size_t)h.nr + 1), fr((size_t)h.nf + 1);
    if (!rd(in, xy.data(), 16 * (size_t)h.nv) || !rd(in, rs.data(), 4 * (size_t)h.nr) || !rd(in, fr.data(), 4 * (size_t)h.nf)) return 2;
    std::vector<mk::edge> edges;
    std::vector<kmk_feature> features;
    std::vector<uint8_t> buf((size_t)h.H * h.stride, 0xAB);
    int32_t res[2] = {0, 0};
    if (kmk_tables(xy.data(), h.nv, rs.data(), h.nr, fr.data(), h.nf, h.H, edges, features)) res[0] = 1;
    else {
        const kmk_polygons p = {edges.data(), (int)edges.size(), features.data(), (int)features.size(), h.H, h.W, buf.data(), (ptrdiff_t)h.stride};
        if (kmk_fill(nullptr, p, 0) || kmk_lines(nullptr, p, &res[1])) return 3;
    }
    return wr(out, res, sizeof res) && wr(out, buf.data(), buf.size()) ? 0 : 2;
}
// and: {int H, W; long long sa, sb, so} a (H * sa) b (H * sb) -> counts[3], the buffer (H * so), poisoned
static int mask_and(FILE *in, FILE *out)
{
    struct { int H, W; long long sa, sb, so; } h;
    if (!rd(in, &h, sizeof h)) return 2;
    std::vector<uint8_t> a((size_t)h.H * h.sa), b((size_t)h.H * h.sb), o((size_t)h.H * h.so, 0xAB);
    if (!rd(in, a.data(), a.size()) || !rd(in, b.data(), b.size())) return 2;
    unsigned long long counts[3];
    if (kmk_mask_and(nullptr, a.data(), (ptrdiff_t)h.sa, b.data(), (ptrdiff_t)h.sb, h.H, h.W, o.data(), (ptrdiff_t)h.so, counts)) return 3;
    return wr(out, counts, sizeof counts) && wr(out, o.data(), o.size()) ? 0 : 2;
}
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const int rc = argv[1][0] == 'p' ? polygons(in, out) : mask_and(in, out);
    fclose(in);
    return fclose(out) ? 2 : rc;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")
    d = tmp_path_factory.mktemp("mask_main")
    src, exe = d / "mask_main.cpp", d / "mask_main"
    src.write_text(MAIN)
    san.build(src, exe, shared=False)

    def run(mode, payload):
        fin, fout = d / "in.bin", d / "out.bin"
        fin.write_bytes(payload)
        out = subprocess.run([str(exe), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
        return fout.read_bytes()
    return run


def run_polygons(program, xy, ring_sizes, feature_rings, H, W, pad=0):
    """-> (tables refused, walk flag, buffer H x (W + pad))."""
    head = struct.pack("<6iq", H, W, xy.shape[0], ring_sizes.size, feature_rings.size, 0, W + pad)
    raw = program("polygons", head + xy.tobytes() + ring_sizes.tobytes() + feature_rings.tobytes())
    refused, flag = struct.unpack("<2i", raw[:8])
    return refused, flag, np.frombuffer(raw[8:], np.uint8).reshape(H, W + pad)


def test_host_launchers_equal_the_restatement(program, expected):
    for name, features, H, W, _options in M.cases():
        tables = ops_mask._polygon_tables(features, name)
        want = expected[name][0] | expected[name][1]
        for pad in (0, 5):
            refused, flag, buf = run_polygons(program, *tables, H, W, pad)
            assert not refused and not flag, (name, pad)
            assert np.array_equal(buf[:, :W], want), (name, pad, np.argwhere(buf[:, :W] != want)[:8])
            assert (buf[:, W:] == 0xAB).all(), (name, pad)                      # nothing outside the window


def test_host_tables_refuse_what_the_abi_refuses(program):
    f64, i32 = np.float64, np.int32
    closed = np.array([[1, 1], [5, 1], [3, 4], [1, 1]], f64)
    assert run_polygons(program, closed, np.array([4], i32), np.array([1], i32), 8, 8)[0] == 0
    assert run_polygons(program, closed[:3], np.array([3], i32), np.array([1], i32), 8, 8)[0] == 1           # not closed
    assert run_polygons(program, closed, np.array([4], i32), np.array([2], i32), 8, 8)[0] == 1               # more rings than there are
    assert run_polygons(program, closed, np.array([3], i32), np.array([1], i32), 8, 8)[0] == 1               # a vertex nobody owns
    assert run_polygons(program, closed, np.array([1, 3], i32), np.array([2], i32), 8, 8)[0] == 1            # a 1-point ring
    for bad in (np.nan, np.inf, 2.0 ** 30 + 1024):
        v = closed.copy()
        v[1, 0] = bad
        assert run_polygons(program, v, np.array([4], i32), np.array([1], i32), 8, 8)[0] == 1


def test_host_mask_and_equals_numpy(program):
    rng = np.random.default_rng(3)
    for H, W, sa, sb, so in ((1, 1, 1, 1, 1), (7, 33, 33, 40, 35), (21, 64, 64, 64, 64), (5, 100, 117, 100, 101)):
        a = (rng.integers(0, 4, (H, sa)) * rng.integers(0, 90, (H, sa))).astype(np.uint8)
        b = (rng.integers(0, 3, (H, sb)) * 255).astype(np.uint8)
        raw = program("and", struct.pack("<2i3q", H, W, sa, sb, so) + a.tobytes() + b.tobytes())
        counts, out = np.frombuffer(raw[:24], np.uint64), np.frombuffer(raw[24:], np.uint8).reshape(H, so)
        want, want_counts = R.combine_masks(a[:, :W], b[:, :W])
        assert np.array_equal(out[:, :W], want) and tuple(int(c) for c in counts) == want_counts and (out[:, W:] == 0xAB).all()
        assert want.max(initial=0) <= 1 and a.max() > 1


# ---- 3. the ABI, the host build, the arguments, the parsing -------------------------------------------------------------------------------
ENTRY_POINTS = ("km_rasterize_polygons", "km_rasterize_polygons_dev", "km_mask_and", "km_mask_and_dev")


def test_abi_carries_the_entry_points():
    import ctypes
    header = open(os.path.join(ROOT, "include", "karios_hip.h")).read()
    api = open(os.path.join(ROOT, "karios_amd", "csrc", "api_prep.hip")).read()        # a file the host build lists
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and f"int {name}(" in header and hasattr(lib, name) and f"int {name}(" in api
    assert "k_mask.hip" in open(os.path.join(ROOT, "karios_amd", "csrc", "Makefile")).read()
    assert ops.MASK_MAX_VERTICES == R.MAX_VERTICES and ops.MASK_MAX_COORD == R.MAX_COORD
    assert all(hasattr(ops, name) for name in ("rasterize_polygons", "combine_masks", "geo_to_pixel"))
    from karios_amd import results
    from karios_amd.core import rasterize_vector_mask
    assert callable(rasterize_vector_mask) and callable(results.load_mask)


def test_host_build_of_the_api_files_still_links():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "hoststub")], capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-4000:]
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "tests", "hoststub", "_build", "libkarios_host_asan.so")], text=True)
    assert all(f" T {name}\n" in syms for name in ENTRY_POINTS)


def test_argument_errors_raise_without_a_device(tmp_path):
    tri = [(1.0, 1.0), (5.0, 1.0), (3.0, 4.0)]
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="not finite"):
            ops.rasterize_polygons([[tri + [(bad, 2.0)]]], (8, 8))
    for bad in (2.0 ** 30 + 1024, -2.0 ** 31):
        with pytest.raises(ValueError, match="beyond 2\\^30"):
            ops.rasterize_polygons([[tri + [(2.0, bad)]]], (8, 8))
    with pytest.raises(ValueError, match="raster of"):
        ops.rasterize_polygons([[tri]], (0, 8))
    with pytest.raises(ValueError, match="raster of"):
        ops.rasterize_polygons([[tri]], (1 << 16, 1 << 16))
    with pytest.raises(ValueError, match="vertices"):
        ops.rasterize_polygons([[[(float(k % 7), float(k % 5)) for k in range((1 << 20) + 1)]]], (8, 8))
    with pytest.raises(ValueError, match="output"):
        ops.rasterize_polygons([[tri]], (8, 8), out=np.zeros((8, 9), np.uint8))
    with pytest.raises(ValueError, match="output"):
        ops.rasterize_polygons([[tri]], (8, 8), out=np.zeros((8, 8), np.int8))
    with pytest.raises(ValueError, match="shape"):
        ops.combine_masks(np.zeros((4, 5), np.uint8), np.zeros((5, 4), np.uint8))
    with pytest.raises(ValueError, match="2-D"):
        ops.combine_masks(np.zeros(4, np.uint8), np.zeros(4, np.uint8))
    from karios_amd.core import NumpyRasterImage, rasterize_vector_mask
    image = NumpyRasterImage(np.zeros((8, 8), np.uint16))
    for geometry in ({"type": "Point", "coordinates": [1, 2]}, {"type": "LineString", "coordinates": [[1, 2], [3, 4]]},
                     {"type": "GeometryCollection", "geometries": [{"type": "MultiPoint", "coordinates": [[1, 2]]}]}):
        with pytest.raises(NotImplementedError, match=geometry.get("geometries", [geometry])[0]["type"]):
            rasterize_vector_mask(geometry, image)
        with pytest.raises(NotImplementedError, match="geometry type"):
            rasterize_vector_mask({"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": geometry}]}, image)
    with pytest.raises(NotImplementedError, match=".shp"):
        rasterize_vector_mask(tmp_path / "aoi.shp", image)
    with pytest.raises(NotImplementedError, match=".gpkg"):
        rasterize_vector_mask(str(tmp_path / "aoi.gpkg"), image)
    from karios_amd import results
    with pytest.raises(ValueError, match="not compatible"):
        results.load_mask(image, raster_mask=NumpyRasterImage(np.zeros((8, 9), np.uint8)))
    assert results.load_mask(image) is None
    only = NumpyRasterImage(np.ones((8, 8), np.uint8))
    assert results.load_mask(image, raster_mask=only) is only


def test_geojson_parsing(tmp_path):
    outer, hole = [[0, 0], [10, 0], [10, 10], [0, 10], [0, 0]], [[2, 2], [2, 4], [4, 4], [4, 2], [2, 2]]
    other = [[20, 20, 7.5], [30, 20, 7.5], [25, 30, 7.5], [20, 20, 7.5]]                                  # (a third ordinate is ignored)
    doc = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [outer, hole]}},
        {"type": "Feature", "properties": {}, "geometry": None},
        {"type": "Feature", "properties": {}, "geometry": {"type": "MultiPolygon", "coordinates": [[outer], [other]]}},
        {"type": "Feature", "properties": {}, "geometry": {"type": "GeometryCollection", "geometries": [
            {"type": "Polygon", "coordinates": [other]}, {"type": "MultiPolygon", "coordinates": [[outer, hole]]}]}}]}
    features = ops.geojson_features(doc)
    assert features == [[outer, hole], [outer, other], [other, outer, hole]]                             # a MultiPolygon is ONE feature
    assert ops.geojson_features(doc["features"][0]) == [[outer, hole]]
    assert ops.geojson_features(doc["features"][2]["geometry"]) == [[outer, other]]
    assert ops.geojson_features({"type": "FeatureCollection", "features": []}) == []
    path = tmp_path / "aoi.geojson"
    path.write_text(json.dumps(doc))
    assert ops.read_vector_features(path) == features and ops.read_vector_features(str(path)) == features
    xy, ring_sizes, feature_rings = ops_mask._polygon_tables(features + [[[[1, 1]], [[3, 3], [4, 5]]]], "t")
    assert list(ring_sizes) == [5, 5, 5, 4, 4, 5, 5, 3] and list(feature_rings) == [2, 2, 3, 1] and xy.shape == (36, 2) and xy.dtype == np.float64
    assert [tuple(p) for p in xy[-3:]] == [(3.0, 3.0), (4.0, 5.0), (3.0, 3.0)]                           # dropped the 1-point ring, closed the open one


def test_geo_to_pixel_against_hand_computed_values():
    north_up = [0, 1, 0, 100, 0, -1]
    assert ops.geo_to_pixel([[10, 90], [50, 50], [0, 100]], north_up) == [(10.0, 10.0), (50.0, 50.0), (0.0, 0.0)]
    s2 = [600000.0, 10.0, 0.0, 5000040.0, 0.0, -10.0]          # inv = (-60000, 0.1, 0, 500004, 0, -0.1)
    assert ops.geo_to_pixel([(600000.0, 5000040.0)], s2) == [(-60000.0 + 600000.0 * 0.1, 500004.0 + 5000040.0 * -0.1)]
    (px, py), = ops.geo_to_pixel([(709800.0, 4890240.0)], s2)
    assert abs(px - 10980.0) < 1e-6 and abs(py - 10980.0) < 1e-6
    rotated = [100.0, 2.0, 0.5, 200.0, 0.25, -4.0]             # X = 100 + 2 px + 0.5 py, Y = 200 + 0.25 px - 4 py: (1, 2) -> (103, 192.25)
    (px, py), = ops.geo_to_pixel([(103.0, 192.25)], rotated)
    assert abs(px - 1.0) < 1e-12 and abs(py - 2.0) < 1e-12
    for gt in (north_up, s2, rotated):
        pts = [(103.0, 192.25), (-7.5, 1e6), (600123.4, 4999876.5)]
        assert ops.geo_to_pixel(pts, gt) == R.geo_to_pixel(pts, gt)
    with pytest.raises(ValueError, match="not invertible"):
        ops.geo_to_pixel([(1.0, 2.0)], [0, 0, 0, 0, 0, 1])
    with pytest.raises(ValueError, match="six"):
        ops.geo_to_pixel([(1.0, 2.0)], [0, 1, 0, 0, 1])
