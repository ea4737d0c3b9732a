"""The definition of the vector-mask burn: what `gdal.RasterizeLayer(..., options=['BURN=1', 'ALL_TOUCHED=TRUE'])` does to polygons
(karios/core/image.py:104-191 rasterize_vector_mask), restated in plain Python on float64 scalars - no numpy arithmetic decides anything.

It restates GDAL's GDALdllImageFilledPolygon and GDALdllImageLineAllTouched (alg/llrasterize.cpp) and the way gv_rasterize_one_shape
calls them for polygons with ALL_TOUCHED: the scan-line fill at pixel centres, then the all-touched line pass over every ring; the
raster is the OR of both over all features.  The text was written from knowledge of GDAL 3.x, NOT from a source tree, and GDAL itself
was never run against it (it is installed nowhere this project is tested): parity with GDAL is unpinned, this file is the contract the
device is held to bit for bit.  What the text is checked against is exact geometry (tests/test_mask_host.py): the fill equals the
even-odd rule at pixel centres, the line pass the set of pixels whose closed square meets a segment.

Points this restatement is unsure of, in the order they appear:
  * the horizontal-edge span of the fill is skipped when `floor(x[ind1] + 0.5) <= 0` (GDAL: `horizontal_x2 <= minx`); with the clamp of a
    burn to [0, W - 1] and empty spans ignored the skip changes nothing, so either reading gives these bytes;
  * the Y clip of the general line case MOVES `xe` outward when `ye >= H` (`xe += (ye - H) / s`, with s > 0) - as remembered from GDAL;
    the walk then runs past the raster's right edge below its last row, where nothing burns;
  * GDAL's walk has no test of the column: `ix < W` holds whenever a row in [0, H) is burnt on every input tried here (the walk is
    below the raster once it is right of it).  The definition burns only with `ix < W` and counts the burns it refused
    (`Stats.refused_columns`): the tests assert the count is 0, and the device carries the same test as a memory guard.

Input: a list of features; a feature is a list of rings - ALL rings of ALL polygons of a MultiPolygon are one feature, so overlapping
members cancel under the even-odd rule; a ring is a closed list of (x, y) in pixel / line space, last point == first point
(`normalize` closes an open ring and drops rings of fewer than 2 points).  The raster is H x W uint8, zeros, burn value 1.
"""
import math

import numpy as np

MAX_COORD = float(2 ** 30)       # |v| beyond it: the C casts of the rounded crossings would be undefined
MAX_VERTICES = 1 << 20
TINY = 0.000000001               # the walk's smallest step along y


def walk_cap(H, W):
    return 4 * (H + W) + 64


class Stats:
    """What the self-tests look at: the longest walk, as steps and as a fraction of its cap; burns refused for their column."""

    def __init__(self):
        self.max_steps, self.max_cap_fraction, self.refused_columns, self.walks = 0, 0.0, 0, 0


def normalize(features, H, W):
    """-> the features as lists of closed rings of (float, float); ValueError for what lies outside the domain."""
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 32 - 1:
        raise ValueError(f"rasterize_polygons: a raster of {H} x {W} (at least 1 x 1, fewer than 2^32 - 1 pixels)")
    out, total = [], 0
    for feature in features:
        rings = []
        for ring in feature:
            pts = [(float(p[0]), float(p[1])) for p in ring]
            for x, y in pts:
                if not (math.isfinite(x) and math.isfinite(y)):
                    raise ValueError("rasterize_polygons: a vertex is not finite")
                if abs(x) > MAX_COORD or abs(y) > MAX_COORD:
                    raise ValueError("rasterize_polygons: a vertex lies beyond 2^30")
            if len(pts) < 2:
                continue
            if pts[0] != pts[-1]:
                pts.append(pts[0])
            total += len(pts)
            rings.append(pts)
        out.append(rings)
    if total > MAX_VERTICES:
        raise ValueError(f"rasterize_polygons: {total} vertices (at most 2^20)")
    return out


def burn_span(row, first, last, W):
    """A burn clamps to [0, W - 1] and ignores an empty span."""
    first, last = max(first, 0), min(last, W - 1)
    for x in range(first, last + 1):
        row[x] = 1


# ---- the fill --------------------------------------------------------------------------------------------------------------------------
def crossing(x1, y1, x2, y2, dy):
    """Edge ind1 = (x1, y1) -> ind2 = (x2, y2) against the centre line dy -> ("x", rounded crossing) | ("h", first, last) | None."""
    if (y1 < dy and y2 < dy) or (y1 > dy and y2 > dy):
        return None
    if y1 < y2:
        dy1, dy2, dx1, dx2 = y1, y2, x1, x2
    elif y1 > y2:
        dy1, dy2, dx1, dx2 = y2, y1, x2, x1
    else:                                   # a horizontal edge on the centre line: a span only when it runs from ind2 rightwards to ind1
        if x1 > x2:
            return ("h", math.floor(x2 + 0.5), math.floor(x1 + 0.5) - 1)
        return None
    if dy1 <= dy < dy2:
        t = dy - dy1                        # every operation rounds on its own, in this order
        t = t * (dx2 - dx1)
        t = t / (dy2 - dy1)
        t = t + dx1
        return ("x", math.floor(t + 0.5))
    return None


def feature_edges(rings):
    """Edge i of a ring joins vertex i - 1 (ind1) to vertex i (ind2); the edge of the first vertex joins the last to the first (the
    same point twice in a closed ring: it never counts)."""
    for ring in rings:
        n = len(ring)
        for i in range(n):
            (x1, y1), (x2, y2) = ring[i - 1 if i else n - 1], ring[i]
            yield x1, y1, x2, y2


def row_range(rings, H):
    ys = [p[1] for ring in rings for p in ring]
    if not ys:
        return 0, -1
    return max(int(min(ys)), 0), min(int(max(ys)), H - 1)       # int(): the C cast, toward zero


def fill_feature(rings, H, W, out, parity=False, counts=None):
    """The sorted-pairs rule; `parity` True: the equivalent form (below).  counts: list that takes every row's number of crossings."""
    miny, maxy = row_range(rings, H)
    for y in range(miny, maxy + 1):
        dy = y + 0.5
        xs = []
        for x1, y1, x2, y2 in feature_edges(rings):
            c = crossing(x1, y1, x2, y2, dy)
            if c is None:
                continue
            if c[0] == "h":
                if not (c[1] > W - 1 or c[2] + 1 <= 0):
                    burn_span(out[y], c[1], c[2], W)
            else:
                xs.append(c[1])
        if counts is not None:
            counts.append(len(xs))
        if parity:
            # Pixel x is burnt by the pairs rule iff the number of values <= x is odd, GIVEN an even count.  Proof: sort the values,
            # a_0 <= a_1 <= ...; pair k burns [a_2k, a_2k+1 - 1].  With m = #{a <= x}: x in pair k  <=>  a_2k <= x < a_2k+1  <=>
            # m >= 2k + 1 and m <= 2k + 1, so x is burnt iff m is odd (k = (m - 1) / 2; with an even count a_2k+1 exists).  The count
            # is even per closed ring: an edge is collected iff exactly one of its ends has y <= dy (the tests are pure
            # comparisons: min <= dy < max), a horizontal edge never, and around a closed ring that predicate changes an even
            # number of times.  Values <= 0 act on pixel 0, values > W - 1 on nothing.
            odd = 0
            marks = {}
            for v in xs:
                if v <= W - 1:
                    marks[max(v, 0)] = marks.get(max(v, 0), 0) ^ 1
            for x in range(W):
                odd ^= marks.get(x, 0)
                if odd:
                    out[y][x] = 1
        else:
            xs.sort()
            for i in range(0, len(xs) - 1, 2):
                if xs[i] <= W - 1 and xs[i + 1] > 0:
                    burn_span(out[y], xs[i], xs[i + 1] - 1, W)


# ---- the lines -------------------------------------------------------------------------------------------------------------------------
def line_pair(x, y, xe, ye, H, W, out, stats):
    """One consecutive vertex pair (x, y) -> (xe, ye) of a ring."""
    if (y < 0 and ye < 0) or (y > H and ye > H) or (x < 0 and xe < 0) or (x > W and xe > W):
        return
    if x > xe:
        x, y, xe, ye = xe, ye, x, y
    if math.floor(x) == math.floor(xe) or abs(x - xe) < .01:            # vertical
        ix = math.floor(xe)
        if 0 <= ix < W:
            for iy in range(max(math.floor(min(y, ye)), 0), min(math.floor(max(y, ye)), H - 1) + 1):
                out[iy][ix] = 1
        return
    if math.floor(y) == math.floor(ye) or abs(y - ye) < .01:            # horizontal
        iy = math.floor(y)
        if 0 <= iy < H:
            for ix in range(max(math.floor(x), 0), min(math.floor(xe), W - 1) + 1):
                out[iy][ix] = 1
        return
    s = (ye - y) / (xe - x)
    if xe > W:
        ye -= (xe - W) * s
        xe = float(W)
    if x < 0:
        y += (0.0 - x) * s
        x = 0.0
    if ye > y:
        if y < 0:
            x += (0.0 - y) / s
            y = 0.0
        if ye >= H:
            xe += (ye - H) / s
    else:
        if y >= H:
            x += (H - y) / s
            y = float(H)
        if ye < 0:
            xe -= ye / s
    steps, cap = 0, walk_cap(H, W)
    while x >= 0 and x < xe:
        ix, iy = math.floor(x), math.floor(y)
        if (s > 0 and iy >= H) or (s < 0 and iy < 0):                   # y is monotone: nothing further can burn
            break
        steps += 1
        if steps > cap:
            raise RuntimeError("rasterize_polygons: a walk exceeded its cap")
        if 0 <= iy < H:
            if ix < W:
                out[iy][ix] = 1
            else:
                stats.refused_columns += 1
        sx = math.floor(x + 1.0) - x
        sy = sx * s
        if math.floor(y + sy) == iy:
            x += sx
            y += sy
        elif s < 0:
            sy = iy - y
            if sy > -TINY:
                sy = -TINY
            sx = sy / s
            x += sx
            y += sy
        else:
            sy = (iy + 1) - y
            if sy < TINY:
                sy = TINY
            sx = sy / s
            x += sx
            y += sy
    stats.walks += 1
    stats.max_steps = max(stats.max_steps, steps)
    stats.max_cap_fraction = max(stats.max_cap_fraction, steps / cap)


def lines_feature(rings, H, W, out, stats):
    for ring in rings:
        for j in range(1, len(ring)):
            line_pair(ring[j - 1][0], ring[j - 1][1], ring[j][0], ring[j][1], H, W, out, stats)


# ---- the raster ------------------------------------------------------------------------------------------------------------------------
def rasterize_parts(features, H, W, parity=False, stats=None):
    """-> (fill, lines): two H x W uint8 arrays, each the OR over the features."""
    stats = stats if stats is not None else Stats()
    features = normalize(features, H, W)
    fill = [bytearray(W) for _ in range(H)]
    lines = [bytearray(W) for _ in range(H)]
    for rings in features:
        fill_feature(rings, H, W, fill, parity)
        lines_feature(rings, H, W, lines, stats)
    as_array = lambda rows: np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8).reshape(H, W).copy()
    return as_array(fill), as_array(lines)


def rasterize(features, H, W, stats=None):
    fill, lines = rasterize_parts(features, H, W, stats=stats)
    return fill | lines


def combine_masks(raster_mask, vector_mask):
    """_load_mask (karios/api/core.py:593-612): the AND and the three logged counts."""
    a, b = np.asarray(raster_mask) > 0, np.asarray(vector_mask) > 0
    both = np.logical_and(a, b).astype(np.uint8)
    return both, (int(np.sum(a)), int(np.sum(b)), int(np.sum(both > 0)))


# ---- world -> pixel ----------------------------------------------------------------------------------------------------------------------
def inv_geo_transform(gt):
    """GDALInvGeoTransform."""
    gt = [float(v) for v in gt]
    if gt[2] == 0.0 and gt[4] == 0.0 and gt[1] != 0.0 and gt[5] != 0.0:
        return (-gt[0] / gt[1], 1.0 / gt[1], 0.0, -gt[3] / gt[5], 0.0, 1.0 / gt[5])
    det = gt[1] * gt[5] - gt[2] * gt[4]
    if det == 0.0:
        raise ValueError("geo_to_pixel: the geotransform is not invertible")
    inv_det = 1.0 / det
    o1, o2, o4, o5 = gt[5] * inv_det, -gt[2] * inv_det, -gt[4] * inv_det, gt[1] * inv_det
    return (gt[2] * gt[3] - gt[0] * gt[5]) * inv_det, o1, o2, (-gt[1] * gt[3] + gt[0] * gt[4]) * inv_det, o4, o5


def geo_to_pixel(xy, gt):
    """GDALApplyGeoTransform of the inverse: a list of (X, Y) -> a list of (pixel, line)."""
    inv = inv_geo_transform(gt)
    return [(inv[0] + float(X) * inv[1] + float(Y) * inv[2], inv[3] + float(X) * inv[4] + float(Y) * inv[5]) for X, Y in xy]
