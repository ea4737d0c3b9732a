"""The 8-pixel eigenvalue kernel's row update (karios_amd/csrc/k_eig3.hip, eig3_item): the source row that enters the box window
and the one that leaves it travel as the two 16-bit halves of one dword, and the three box sums take `entering - leaving` as one
dot product each.  Every case asks goodFeaturesToTrack for EVERY candidate (maxCorners 0, minDistance 0), in rank order, and holds
the answer array_equal to the oracle: positions pin the box sums' sign and zero, the order pins the eigenvalues' order.

Which path a shape takes (a single tile this small is cut into items of 32 rows - km_pick_rows with every item in one round; item i
marches the product rows 32 i - bs // 2 ... min(H - 1, 32 i + 33) + bs // 2; block sizes below 5 have no early warm-up path):
  * H = 77: three items.  Item 0 starts above row 0 (bs >= 3): mirrored general steps, the steady loop, no leaving row for its first
    bs steps.  Item 1 starts inside the image: three general steps, then (bs >= 5) the warm-up groups of the sliding march, whose
    leaving halves are loaded but must not count before step bs, then the steady loop.  Item 2 ends on general steps over the
    mirrored bottom rows.  The band of extremes (rows 19 .. 34) enters item 0 in the steady loop, is met by item 1 in its warm-up and
    leaves it in the steady loop.
  * H = 38: two items; the second one never reaches the steady loop (general steps, at bs 15 two warm-up groups, general steps over
    the mirrored bottom).
  * H = 2 bs + 8, the smallest height the 8-pixel kernel takes: one item (two at bs 15), the fewest steady trips there are - 1, 1, 3
    and 5 groups of three rows at bs 1, 3, 7, 15.  No height the kernel accepts keeps the first item out of the steady loop
    altogether: its general steps end at row bs + 1 and the loop runs while three rows fit below H - 5.
  * W = 512: one strip; W = 1000: two strips, the second one shifted left to end at the image's edge (both widths: plus the two
    12-column border strips of the 2-pixel item).
The library's statistics do not name the kernel that ran; they do tell when the fused kernel's result was NOT used (stage overflow:
PATH_STAGE_FALLBACK), and every case asserts that this did not happen."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q = 1e-3
FLAT = 77                    # grey level outside the band


def _band(H):
    y0 = H // 4
    return y0, y0 + H // 5 + 1     # rows [y0, y1)


def _col_ranges(W):
    """Column ranges that carry a pattern, 48 wide: each crosses lane boundaries (every 8 columns); at W = 1000 one crosses the seam
    of the two strips.  Patterns of exact ties stay this narrow because their candidates form plateaus many rows tall, and a wave
    stages at most 1024 candidates between two flushes: wider, the call falls back to the map kernel and tests nothing here."""
    return [(36, 84), (W - 148, W - 100)] + ([(476, 524)] if W >= 1000 else [])


def _cells(H, W, cell, along_x, along_y):
    yy, xx = np.mgrid[0:H, 0:W]
    v = np.zeros((H, W), np.int64)
    if along_x:
        v += xx // cell
    if along_y:
        v += yy // cell
    return ((v & 1) * 255).astype(np.uint8)


def _content(kind, H, W, bs):
    """-> (image, first row of the region that must hold no candidate, or None)."""
    rng = np.random.default_rng(1000 * H + W + bs)
    if kind == "random":
        return rng.integers(0, 256, (H, W), dtype=np.uint8), None
    if kind == "vperiod":
        # vertical period bs: the entering and the leaving row are the same row, every update of the box sums is exactly zero
        base = np.full((bs, W), FLAT, np.uint8)
        for x0, x1 in _col_ranges(W):
            base[:, x0:x1] = rng.integers(0, 256, (bs, x1 - x0), dtype=np.uint8)
        return np.ascontiguousarray(base[np.arange(H) % bs]), None
    # a band of 0 / 255 cells in a constant image.  cell 1: neighbouring pixels alternate (the Sobel taps two apart cancel: the
    # extremes appear at the band's edges only); cell 2: |dx| / |dy| = 1020 all through the band, in one half of the packed
    # registers while the other half is 0, and bs rows later the reverse
    name, cell = kind[:-1], int(kind[-1])
    pat = _cells(H, W, cell, name in ("cols", "check"), name in ("rows", "check"))
    y0, y1 = _band(H)
    img = np.full((H, W), FLAT, np.uint8)
    for x0, x1 in _col_ranges(W):
        img[y0:y1, x0:x1] = pat[y0:y1, x0:x1]
    # Sobel rows up to y1 see the band; the window of row y spans the product rows y - bs // 2 ... y + bs // 2
    return img, y1 + bs // 2 + 1


def _mask(H, W):
    return ((np.random.default_rng(H + W).integers(0, 4, (H, W)) > 0) * 255).astype(np.uint8)


@pytest.mark.parametrize("bs", [1, 3, 7, 15])
@pytest.mark.parametrize("kind", ["random", "cols1", "cols2", "rows1", "rows2", "check1", "check2", "vperiod"])
@pytest.mark.parametrize("shape", [(None, 512), (38, 1000), (77, 512), (77, 1000)])
def test_all_candidates_in_rank_order(ops, O, shape, kind, bs):
    from karios_amd._lib import PATH_STAGE_FALLBACK, default_context
    H, W = shape
    H = 2 * bs + 8 if H is None else H
    img, flat_from = _content(kind, H, W, bs)
    for mask in (None, _mask(H, W)):
        exp = O.good_features(img, mask, 0, Q, 0, bs)
        got = ops.good_features_to_track(img, 0, Q, 0, blockSize=bs, mask=mask)
        assert not default_context().stats().path_flags & PATH_STAGE_FALLBACK
        if exp is None:
            assert got is None
            continue
        np.testing.assert_array_equal(got, exp)
        if flat_from is not None and flat_from < H:
            # below the band, once it has left every window, all three box sums are exactly 0 again: no candidate
            assert not (got[:, 0, 1] >= flat_from).any()
