"""The marching stretch + Laplacian pass (csrc/k_lap.hip lap_march_item) splits an item's march into GENERAL row steps (warm-up,
mirrored rows, tail) and INTERIOR trips of NR rows (static prefetch slots, stores through buffer descriptors).  Outputs must not depend
on where the seams fall: both Laplacians, the mask and the valid count bit for bit the oracle's, at heights that put zero, one and
one-plus-a-remainder interior trips into an item, for every radius, pixel type and strip layout; and a batch of units of different
height in one item space equal to the units one by one.

Where the seams fall follows from the rows per item, which the launcher takes from km_pick_rows_units (common.hpp): the helper below
compiles that function for the host, as tests/test_host_logic.py::test_laplacian_rows_choice_is_km_pick_rows does, and the shape
lists are checked against it - a change of the rule that moves the seams off these shapes fails here instead of passing blind."""
import os
import subprocess

import numpy as np
import pytest

from karios_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAPM_PF_BUILDS = (2, 3, 4)                    # k_lap.hip: rows in flight per wave - 3, and what -DLAPM_PF may set: the shapes below serve all three
DTYPES = [np.uint8, np.uint16, np.int16, np.float32]
# kernel-size pairs (ref, mon): every radius 1 .. 5 (sizes 1 and 3 share radius 1), mixed pairs, 11 beside 1, 9 beside 3
KPAIRS = [(1, 1), (3, 3), (5, 5), (7, 7), (9, 9), (11, 11), (11, 1), (9, 3), (3, 7)]
# every strip of these widths takes the kernel's FAST path, the only one with interior trips: two strips / three with a shifted last
# strip (W % 4 == 2) / three, W % 4 == 0
FAST_WIDTHS = [256, 510, 600]
GENERAL_WIDTH = 253                           # one strip below the shift's minimum: general steps only, whatever the height
BASE_H, BASE_W = 140, 604


def _march_consts(radius, itemsize, lapm_pf):
    """(NR, WARM, PF) of lap_march_item for a radius, a pixel size and a build's LAPM_PF."""
    rh = 4 if radius == 5 else radius
    nr = 2 * rh + 1
    warm = (2 * radius + nr - 1) // nr * nr
    depth = 2 if (radius == 5 and itemsize == 4 and lapm_pf > 2) else lapm_pf
    return nr, warm, min(depth, nr - 1)


def _interior_trips(H, rows, radius, itemsize, lapm_pf):
    """(interior trips, general tail rows behind them) of every item of an image of H rows whose strips take the FAST path (the
    arithmetic of lap_march_item, restated)."""
    nr, warm, pf = _march_consts(radius, itemsize, lapm_pf)
    out = []
    for y0 in range(0, H, rows):
        y1 = min(H, y0 + rows)
        m_end = y1 + radius
        d = min(y1, min(H, m_end) - pf) - (y0 - radius + warm)
        n = d // nr if d > 0 else 0
        out.append((n, m_end - (y0 - radius + warm + n * nr) if n > 0 else None))
    return out


@pytest.fixture(scope="module")
def pick_rows(tmp_path_factory):
    """rows per item for one unit (H, strips) at a radius: km_pick_rows_units itself, compiled for the host.  The launcher's wave
    slots are CUs x 4 SIMDs x workgroups per CU of the instantiation; the choice has to be the same for every plausible occupancy
    (1 .. 8), else the shape lists below pin nothing."""
    import torch
    d = tmp_path_factory.mktemp("rows")
    src, exe = d / "rows.cpp", d / "rows"
    src.write_text(r'''
#include "common.hpp"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char **argv)
{
    int H = atoi(argv[1]), s = atoi(argv[2]), halo = atoi(argv[3]);
    long cus = atol(argv[4]);
    for (int wg = 1; wg <= 8; wg++) printf("%d\n", km_pick_rows_units(&H, &s, 1, halo, cus * 4 * wg, 32, 160));
    return 0;
}
''')
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "karios_amd", "csrc"),
                           "-I", os.path.join(ROOT, "tests", "hoststub"), str(src), "-o", str(exe)])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    memo = {}

    def rows(H, W, radius):
        valid = 240 if radius == 5 else 248
        key = (H, (W + valid - 1) // valid, radius)
        if key not in memo:
            got = set(subprocess.run([str(exe), str(key[0]), str(key[1]), str(2 * radius), str(cus)], capture_output=True, text=True, timeout=60,
                                     check=True).stdout.split())
            assert len(got) == 1, (key, got)
            memo[key] = int(got.pop())
        return memo[key]
    return rows


def _base_pair(dtype):
    """A pair holding every value of its range, exact multiples of the stretch included, zeros, the no-data values 7 / 9 and (float32) NaN."""
    rng = np.random.default_rng(100 + np.dtype(dtype).itemsize + (np.dtype(dtype).kind == "i"))
    n = BASE_H * BASE_W
    if np.dtype(dtype) == np.float32:
        ref = (rng.random((BASE_H, BASE_W)) * 4000).astype(np.float32)
        mon = (rng.random((BASE_H, BASE_W)) * 2800 + 3).astype(np.float32)
        ref[rng.random((BASE_H, BASE_W)) < 0.01] = np.nan
    else:
        span = {"uint8": 255, "uint16": 12345, "int16": 1020}[np.dtype(dtype).name]
        mn = 0 if np.dtype(dtype).kind == "u" else -span // 2
        ref = ((np.arange(n) % (span + 1)) + mn).astype(dtype).reshape(BASE_H, BASE_W)
        mon = ((rng.permutation(n) % (span + 1)) + mn).astype(dtype).reshape(BASE_H, BASE_W)
    ref[rng.random((BASE_H, BASE_W)) < 0.02] = 0
    mon[rng.random((BASE_H, BASE_W)) < 0.02] = 0
    ref[rng.random((BASE_H, BASE_W)) < 0.01] = 7
    mon[rng.random((BASE_H, BASE_W)) < 0.01] = 9
    return ref, mon


_PAIRS = {}


def _want(O, dtype, H, W, x0):
    """The pair's box [0:H, x0:x0+W] and the oracle's stretches and masks of it (the base pair is made once per pixel type)."""
    name = np.dtype(dtype).name
    if name not in _PAIRS:
        _PAIRS.clear()
        _PAIRS[name] = _base_pair(dtype)
    assert x0 + W <= BASE_W and H <= BASE_H
    ref, mon = (a[:H, x0:x0 + W] for a in _PAIRS[name])
    refc, monc = np.ascontiguousarray(ref), np.ascontiguousarray(mon)
    return dict(ref=ref, mon=mon, u8_ref=O.to_uint8(refc), u8_mon={inv: O.to_uint8(monc, invert=inv) for inv in (False, True)},
                mask={nd: O.auto_mask(monc, refc, nodata_mon=nd[1], nodata_ref=nd[0]) for nd in [(None, None), (7.0, 9.0)]})


def _heights(radius):
    """Every height from the marching form's minimum to two items and a row: one item that mirrors at both ends, then a full first
    item + a last item of L = 1 .. 32 rows - both sweep an item through zero interior trips, exactly one, and one plus every
    remainder, for every radius; the last item is shorter than R + PF and shorter than NR at its low end.  Then three to five
    items: items that mirror nowhere between one that mirrors at the top and one that mirrors at the bottom."""
    lo = 16 if radius == 5 else 8
    return list(range(lo, 66)) + [96, 99, 109, 131]


def _classes(items, nr):
    """What an item is to the split: (no trip,), (one trip, the tail's remainder), (several trips, the tail's remainder)."""
    return {(0,) if t == 0 else (min(t, 2), tail % nr) for t, tail in items}


@pytest.mark.parametrize("kpair", KPAIRS, ids=lambda p: f"k{p[0]}-{p[1]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_prefilter_is_bit_exact_at_every_seam_of_the_row_march(ops, O, pick_rows, dtype, kpair):
    kr, km = kpair
    radius = max(max(kr, km) // 2, 1)
    itemsize = np.dtype(dtype).itemsize
    ran = []                                             # (H, rows) of every shape whose strips take the FAST path
    for n, H in enumerate(_heights(radius)):
        # EVERY height at every FAST width - only those shapes enter the interior loop -, every fourth on the general path too
        for k, W in enumerate(FAST_WIDTHS + ([GENERAL_WIDTH] if n % 4 == 0 else [])):
            x0 = (n + k) % 3                             # (the host rows start at different alignments too)
            inv = bool((n + k) & 1)
            nd = (7.0, 9.0) if (n + k) % 3 == 0 else (None, None)
            rows = pick_rows(H, W, radius)
            if W != GENERAL_WIDTH:
                ran.append((H, rows))
            w = _want(O, dtype, H, W, x0)
            want_r, want_m = O.laplacian_u8(w["u8_ref"], kr), O.laplacian_u8(w["u8_mon"][inv], km)
            want_mask, want_valid = w["mask"][nd]
            what = (H, W, x0, rows, inv, nd)
            lr, lm, mk, nv = ops.tile_prefilter(w["ref"], w["mon"], nodata_ref=nd[0], nodata_mon=nd[1], ref_ksize=kr, mon_ksize=km, invert_mon=inv)
            assert np.array_equal(lr, want_r), what
            assert np.array_equal(lm, want_m), what
            assert np.array_equal(mk, want_mask), what
            assert nv == want_valid, what
            lr2, lm2, mk2, nv2 = ops.tile_prefilter(w["ref"], w["mon"], ref_ksize=kr, mon_ksize=km, invert_mon=inv, with_mask=False)
            assert mk2 is None and nv2 is None and np.array_equal(lr2, want_r) and np.array_equal(lm2, want_m), what
    # The FAST shapes reach the seams, whichever LAPM_PF the library was built with: items without an interior trip, with exactly
    # one and with several, and behind the trips a general tail of every remainder 0 .. NR - 1 - every remainder that ANY item of
    # the rule's rows per item can have (all heights up to five items, counted by the same arithmetic), which at radius <= 4 is all
    # of them.  (Radius 5: an item of 32 rows - the rule's choice for every image this small - has 42 source rows, 18 of them
    # warm-up, and with three or four rows in flight cannot hold one trip of 9 rows and the last remainder(s) behind it.)
    rows_used = {r for _, r in ran}
    assert len(rows_used) == 1, rows_used
    rows = rows_used.pop()
    for lapm_pf in LAPM_PF_BUILDS:
        nr, warm, pf = _march_consts(radius, itemsize, lapm_pf)
        seen = _classes([it for H, r in ran for it in _interior_trips(H, r, radius, itemsize, lapm_pf)], nr)
        reachable = _classes([it for H in range(16 if radius == 5 else 8, 5 * rows + 1) for it in _interior_trips(H, rows, radius, itemsize, lapm_pf)], nr)
        assert (0,) in seen and any(c[0] == 1 for c in seen) and any(c[0] == 2 for c in seen), (lapm_pf, sorted(seen))
        assert {c for c in reachable if c[0] == 1} <= seen, (lapm_pf, sorted(reachable - seen))
        if radius <= 4:
            assert {c[1] for c in seen if c[0] == 1} == set(range(nr)), (lapm_pf, sorted(seen))


def same_rows(a, b) -> bool:
    """Two frame blocks hold the same frame: header and, column by column, the first n_rows entries."""
    ia, ib = a.block.view(np.int32), b.block.view(np.int32)
    if not np.array_equal(ia[:4], ib[:4]) or a.cap != b.cap or a.with_zncc != b.with_zncc:
        return False
    n, cap = int(ia[0]), a.cap
    cols32 = all(np.array_equal(ia[4 + k * cap:4 + k * cap + n], ib[4 + k * cap:4 + k * cap + n]) for k in range(6))
    base = 4 + 6 * cap
    cols64 = all(np.array_equal(ia[base + 2 * k * cap:base + 2 * k * cap + 2 * n], ib[base + 2 * k * cap:base + 2 * k * cap + 2 * n]) for k in range(int(a.with_zncc)))
    return cols32 and cols64


# units of different height and width in one item space (the batch form takes units from 512 columns on): boxes of a pair whose uint16
# rows are 2 198 bytes apart (every other row off the dword grid), odd box origins, three and four strips with and without a shifted
# last strip, last items of 13, 8, 5, 20 rows beside full ones.  A small LK window and block, so that units this low are covered.
UNIT_BOXES = [(0, 0, 512, 77), (3, 5, 513, 40), (101, 50, 600, 133), (250, 300, 750, 45), (7, 200, 599, 64), (400, 33, 520, 52)]
UNIT_CONF = dict(matching_winsize=11, blocksize=7)


@pytest.fixture(scope="module")
def unit_pair(ops):
    from karios_amd.resident import ResidentPair
    ctx = ops._lib.default_context()
    mon, ref = synth.make_pair(600, 1099, 0.4, -0.3, seed=21, nodata_wedge=True)
    return ctx, ResidentPair.upload(mon, ref, ctx=ctx), mon, ref


@pytest.mark.parametrize("ksize", [3, 7, 9, 11])
def test_units_in_one_item_space_equal_the_units_one_by_one(ops, O, unit_pair, ksize):
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import submit_units
    ctx, pair, mon, ref = unit_pair
    conf = KLTConfiguration(maxCorners=600, laplacian_kernel_size=ksize, **UNIT_CONF)
    units = [(pair, b, None) for b in UNIT_BOXES]
    want = [p.submit_tile(conf, box=b, origin=o).result() for p, b, o in units]
    assert all(w.flags == 0 for w in want) and sum(w.n_rows for w in want) > 200
    batch = submit_units(units, conf, None, False)
    assert batch is not None and len(batch) == len(units)
    got = list(batch.wait())
    for k, (g, w) in enumerate(zip(got, want)):
        if g.flags:
            got[k] = g = batch.redo(k)
        assert g.flags == 0 and same_rows(g, w), (ksize, k)
    # one unit against the oracle: the batch is not merely self-consistent
    x, y, bw, bh = UNIT_BOXES[2]
    exp = O.klt_tile(mon[y:y + bh, x:x + bw], ref[y:y + bh, x:x + bw], O.default_conf(maxCorners=600, laplacian_kernel_size=ksize, **UNIT_CONF))
    f = got[2].to_frame()
    np.testing.assert_array_equal(f["x0"].to_numpy(), exp["x0"] + x)
    np.testing.assert_array_equal(f["y0"].to_numpy(), exp["y0"] + y)
    np.testing.assert_array_equal(f["dx"].to_numpy(), exp["dx"])


def test_frame_stream_submit_many_equals_submit(ops, unit_pair):
    from karios_amd.core import KLTConfiguration
    from karios_amd.stream import FrameStream
    ctx, pair, _, _ = unit_pair
    conf = KLTConfiguration(maxCorners=500, **UNIT_CONF)
    units = [(pair, b, None) for b in UNIT_BOXES[:5]]
    with FrameStream(0.4, depth=1) as s:
        want = []
        for p, b, o in units:
            want += s.submit(p, conf, b, o)
        want += s.drain()
    with FrameStream(0.4, depth=1) as s:
        got = s.submit_many(units, conf) + s.drain()
    assert len(got) == len(want) == len(units)
    for k, (g, w) in enumerate(zip(got, want)):
        assert same_rows(g.raw, w.raw) and g.frame.equals(w.frame), k
