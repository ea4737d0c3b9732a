"""The 8-pixel eigenvalue kernel's item classes (karios_amd/csrc/k_eig3.hip, km_set_option "eig3_valid_items"): in a batched submission
a strip item reads the valid-pixel counts the Laplacian pass left for the Laplacian items that overlap its mask rectangle
(csrc/lap_items.hpp) and then skips itself (no valid pixel), runs its interior trips without the mask (all valid) or reads the mask as
before.  Option 0 hands the kernel no counts: every item takes the general path, the code the other suites hold to the oracle.

Every case submits the same units with the option on and off and compares everything observable - the four header words (rows,
corners, flags, candidates), every frame column as raw words, and the kernel's tie rows - bit for bit; the per-class item counts
(Context.eig3_item_classes) keep a case from passing on the general path alone.

Shapes: units 300 rows high (items of 48 .. 96 rows: several row blocks; Laplacian items of 32 .. 160 rows).  Widths 1100, 1101 and 1102:
three strips, the last one clamped to the right edge (at 1101 and 1102 off the 4-pixel groups the mask-free trips need: general),
the Laplacian pass's last strip shifted at the odd widths; 1536: four strips; 520: two strips 480 columns apart; one uint8 unit; one
batch of all the uint16 shapes together."""
import numpy as np
import pytest

from karios_amd import synth

pytestmark = pytest.mark.gpu

H = 300
WIDTHS = (1100, 1101, 1102, 1536, 520)
MARGIN, STRIDE = 12, 488                       # EIG3_MARGIN, EIG3_STRIDE of k_eig3.hip


def _strips(W):
    """-> (strips, strips whose column range starts and ends on a 4-pixel group of a lane)."""
    n = -(-(W - 2 * MARGIN) // STRIDE)
    grouped = 0
    for s in range(n):
        xs = min(s * STRIDE, W - 512)
        lo, hi = MARGIN + s * STRIDE, min(MARGIN + (s + 1) * STRIDE, W - MARGIN)
        grouped += (lo - xs) % 4 == 0 and (hi - xs) % 4 == 0
    return n, grouped


_BASE = {}


def _content(W, dtype=np.uint16):
    """An all-valid pair (every pixel >= 1 in both images), made once per shape and never written to."""
    key = (W, np.dtype(dtype).name)
    if key not in _BASE:
        mon, ref = synth.make_pair(H, W, 0.4, -0.3, seed=300 + W)
        if dtype == np.uint8:
            mon, ref = (np.clip(a >> 6, 1, 255).astype(np.uint8) for a in (mon, ref))
        assert mon.min() >= 1 and ref.min() >= 1
        mon.setflags(write=False); ref.setflags(write=False)
        _BASE[key] = (mon, ref)
    return _BASE[key]


def _words(raw):
    """Header and, column by column, the first n_rows entries (what lies behind them is whatever an earlier frame left there)."""
    w = raw.block.view(np.int32)
    n, cap = int(w[0]), raw.cap
    return [w[:4].copy()] + [w[4 + k * cap:4 + k * cap + n].copy() for k in range(6)]


def _run(ops, images, conf=None, pipelined=False):
    """images: [(mon, ref, mask | None)] -> per unit (frame words with the option on, classes on, classes off); asserts on == off."""
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair, submit_units
    ctx = ops._lib.default_context()
    conf = conf or KLTConfiguration(maxCorners=150)
    units = [(ResidentPair.upload(mon, ref, mask, ctx=ctx), None, None) for mon, ref, mask in images]
    got = {}
    try:
        for on in (1, 0):
            ctx.set_option("eig3_valid_items", on)
            batch = submit_units(units, conf)
            assert batch is not None and len(batch) == len(units)
            raws = batch.wait()
            got[on] = [(_words(r), ctx.eig3_item_classes(k)) for k, r in enumerate(raws)]
    finally:
        ctx.set_option("eig3_valid_items", 1)
    out = []
    for k, ((a, ca), (b, cb)) in enumerate(zip(got[1], got[0])):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (k, a[0].tolist(), b[0].tolist())
        assert ca["tie_rows"] == cb["tie_rows"], (k, ca, cb)
        assert a[0][2] == 0, (k, a[0].tolist())                  # not flagged: the rows are the result
        assert cb["all"] == 0 and cb["none"] == 0 and cb["general"] > 0, (k, cb)
        assert ca["all"] + ca["none"] + ca["general"] == cb["general"], (k, ca, cb)
        out.append((a, ca, cb))
    return out


def _batches():
    return [[W] for W in WIDTHS] + [[1100, 1101, 1102, 1536]]


def test_all_valid_units_run_their_unclamped_strips_without_the_mask(ops):
    for widths in _batches():
        res = _run(ops, [(*_content(W), None) for W in widths])
        for W, (words, on, off) in zip(widths, res):
            n, grouped = _strips(W)
            per_strip = off["general"] // n
            assert off["general"] == per_strip * n and per_strip >= 3, (W, off)
            assert on["none"] == 0 and on["all"] == grouped * per_strip and on["general"] == (n - grouped) * per_strip, (W, on, n, grouped)
            assert grouped >= n - 1 and words[0][0] > 50, (W, words[0].tolist())
    res = _run(ops, [(*_content(1100, np.uint8), None)])
    words, on, off = res[0]
    assert on["none"] == 0 and on["general"] == 0 and on["all"] == off["general"] and words[0][0] > 50, (on, off, words[0].tolist())


PIXELS = [(0, 0), (0, 12), (1, 499), (1, -1), (47, 11), (47, 500), (48, 511), (48, -13), (95, 512), (95, 0), (96, -12), (96, 499),
          (97, 12), (97, 511), (299, 500), (299, -1), (299, 0), (48, 12)]


def test_one_nodata_pixel_takes_the_items_around_it_to_the_general_path(ops):
    """Rows at the items' and the Laplacian items' seams, columns at a strip's halo, its first and last output column, the seam of two
    strips and the right border."""
    for W in WIDTHS:
        mon0, ref0 = _content(W)
        clean = _run(ops, [(mon0, ref0, None)])[0][1]
        for k, (r, c) in enumerate(PIXELS):
            c = c % W
            mon, ref = mon0.copy(), ref0.copy()
            (mon if k & 1 else ref)[r, c] = 0
            words, on, off = _run(ops, [(mon, ref, None)])[0]
            total = off["general"]
            assert on["none"] == 0 and 0 < on["general"] < total, (W, r, c, on, clean)
            # the Laplacian strip (248 columns at this kernel size) that counts the pixel overlaps these strips' column ranges: where one
            # of them ran without the mask on the clean pair, the item(s) holding the pixel have left that class
            k0 = c // 248 * 248
            hit = [s for s in range(_strips(W)[0]) if MARGIN + s * STRIDE < k0 + 248 and min(MARGIN + (s + 1) * STRIDE, W - MARGIN) > k0]
            was_all = [s for s in hit if (MARGIN + s * STRIDE - min(s * STRIDE, W - 512)) % 4 == 0]
            assert hit, (W, c)
            if was_all:
                assert on["all"] < clean["all"] and on["general"] > clean["general"], (W, r, c, on, clean)
            else:
                assert all(on[k] == clean[k] for k in ("none", "all", "general")), (W, r, c, on, clean)


def test_nodata_wedge_band_and_user_mask(ops):
    # the wedge: items without a valid pixel, with some, and with nothing else
    for W in (1101, 1536):
        mon, ref = synth.make_pair(H, W, 0.4, -0.3, seed=300 + W, nodata_wedge=True)
        words, on, off = _run(ops, [(mon, ref, None)])[0]
        assert on["general"] > 0 and on["none"] + on["all"] > 0 and words[0][0] > 20, (W, on, words[0].tolist())
    # a band of nodata rows that holds whole Laplacian items (at most 160 rows each) and whole items of the eigenvalue pass
    for widths in ([1100, 1101, 1102, 1536], [520]):
        images = []
        for W in widths:
            mon, ref = (a.copy() for a in _content(W))
            mon[:200] = 0
            ref[:200] = 0
            images.append((mon, ref, None))
        from karios_amd.core import KLTConfiguration
        for W, (words, on, off) in zip(widths, _run(ops, images, KLTConfiguration(maxCorners=40))):       # (100 rows are left: few corners)
            assert on["none"] > 0 and on["none"] + on["all"] + on["general"] == off["general"] and words[0][0] > 20, (W, on, words[0].tolist())
    # a user mask: the counts are not the Laplacian items' - nothing is classified
    rng = np.random.default_rng(9)
    for W in (1101, 520):
        mon, ref = _content(W)
        mask = np.ones((H, W), np.uint8)
        for _ in range(6):
            y, x = int(rng.integers(0, H - 20)), int(rng.integers(0, W - 40))
            mask[y:y + int(rng.integers(10, 120)), x:x + int(rng.integers(20, 300))] = 0
        words, on, off = _run(ops, [(mon, ref, mask)])[0]
        assert on["all"] == 0 and on["none"] == 0 and on["general"] == off["general"] and words[0][0] > 50, (W, on)


def test_pipelined_submissions_read_their_own_lanes_counts(ops):
    """Two batches of the same shapes alternate on the two workspace lanes: one all valid, one with the band.  A submission that read
    the other lane's counts would skip items that hold corners, or run masked rows without the mask."""
    from karios_amd.core import KLTConfiguration
    from karios_amd.resident import ResidentPair, submit_units
    ctx = ops._lib.default_context()
    conf = KLTConfiguration(maxCorners=40)                # (the band leaves 100 rows: few corners)
    widths = [1100, 1101, 1536]
    clear = [(ResidentPair.upload(*_content(W), ctx=ctx), None, None) for W in widths]
    band = []
    for W in widths:
        mon, ref = (a.copy() for a in _content(W))
        mon[:200] = 0
        band.append((ResidentPair.upload(mon, ref, ctx=ctx), None, None))
    want = {}
    ctx.set_option("eig3_valid_items", 0)
    try:
        for name, units in (("clear", clear), ("band", band)):
            want[name] = [_words(r) for r in submit_units(units, conf).wait()]
        ctx.set_option("eig3_valid_items", 1)
        ctx.set_option("units_pipeline", 1)
        def check(name, p):
            for k, r in enumerate(p.wait()):
                got = _words(r)
                assert got[0][2] == 0 and all(np.array_equal(x, y) for x, y in zip(got, want[name][k])), (name, k, got[0].tolist(), want[name][k][0].tolist())

        prev = None                  # submission i is waited for after submission i + 1 went in (its tail travels with that one)
        for name in ("clear", "band", "band", "clear", "band", "clear"):
            cur = (name, submit_units(clear if name == "clear" else band, conf))
            if prev is not None:
                check(*prev)
            prev = cur
        check(*prev)
        assert ctx.eig3_item_classes(0)["none"] == 0 and ctx.eig3_item_classes(0)["all"] > 0      # (the last one: clear)
    finally:
        ctx.set_option("units_pipeline", 0)
        ctx.set_option("eig3_valid_items", 1)
