"""The shared case list of the vector-mask tests (tests/test_mask_host.py, tests/test_gpu_mask.py): small rasters, every path the fill
and the line pass of csrc/k_mask.hip take.  A case is (name, features, H, W, options); options: `chunk` = the "mask_edge_chunk" option
the device runs under (edges staged in LDS at a time; 0: the default), `window` = the output is a window of a wider buffer."""
import math
import random


def rect(x0, y0, x1, y1, clockwise=True):
    ring = [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]
    return ring if clockwise else ring[::-1]


def star(cx, cy, r_out, r_in, n):
    """A closed star of n vertices around (cx, cy)."""
    pts = []
    for k in range(n):
        r = r_out if k % 2 == 0 else r_in
        a = 2.0 * math.pi * k / n
        pts.append((cx + r * math.cos(a), cy + r * math.sin(a)))
    return pts + [pts[0]]


def random_polygon(rng, H, W, margin=6.0):
    """1 - 2 rings of 3 - 8 vertices, uniform in [-margin, W + margin] x [-margin, H + margin]."""
    rings = []
    for _ in range(rng.randint(1, 2)):
        pts = [(rng.uniform(-margin, W + margin), rng.uniform(-margin, H + margin)) for _ in range(rng.randint(3, 8))]
        rings.append(pts + [pts[0]])
    return rings


def cases():
    rng = random.Random(11)
    H, W = 45, 67
    out = []

    def add(name, features, h=H, w=W, **options):
        out.append((name, features, h, w, options))

    add("reference_input", [[[(10.0, 10.0), (50.0, 10.0), (50.0, 50.0), (10.0, 50.0), (10.0, 10.0)]]], 100, 100)
    add("half_open_rules", [[[(2.5, 2.5), (7.5, 2.5), (7.5, 6.5), (2.5, 6.5)]]], 10, 10)
    # the shapes
    add("1x1_covered", [[rect(-1.0, -1.0, 2.0, 2.0)]], 1, 1)
    add("1x1_missed", [[rect(1.25, 0.0, 3.0, 1.0)]], 1, 1)
    add("1x67", [[[(3.2, -2.0), (60.7, 0.4), (30.0, 3.0)]]], 1, 67)
    add("67x1", [[[(-2.0, 3.2), (0.4, 60.7), (3.0, 30.0)]]], 67, 1)
    add("45x67", [random_polygon(rng, H, W) for _ in range(3)])
    # 4099 columns: 129 bitmap words, beyond one wavefront's 64; crossings in the first, the 64th, the 65th and the last word
    add("3x4099", [[[(5.3, -1.0), (4090.6, 0.2), (4098.7, 2.9), (2049.5, 1.5), (2040.2, 3.7), (100.0, 3.7)]],
                   [[(2047.6, -0.5), (2080.3, 0.7), (2050.1, 4.0)]], [[(4097.2, -3.0), (4110.0, 1.0), (4096.4, 5.0)]]], 3, 4099)
    # many LDS chunks per feature
    add("star_5000", [[star(31.7, 32.2, 40.0, 11.0, 5000)]], 64, 64, chunk=256)
    add("stars_chunk_1",[[star(20.0, 7.0, 9.0, 4.0, 12)], [star(40.0, 20.0, 19.0, 8.0, 7)]], chunk=1)
    # the rules between features and rings
    add("two_features_or", [[rect(5.3, 4.2, 30.6, 25.1)], [rect(20.2, 15.7, 50.9, 40.4)]])
    add("hole", [[rect(6.4, 5.3, 58.2, 39.6), rect(20.7, 12.1, 41.3, 30.8, clockwise=False)]])
    add("multipolygon_cancel", [[rect(5.3, 4.2, 30.6, 25.1), rect(20.2, 15.7, 50.9, 40.4)]])
    add("same_ring_twice", [[rect(5.3, 4.2, 30.6, 25.1), rect(5.3, 4.2, 30.6, 25.1)]])
    # vertices on pixel centres and on integer grid lines
    add("on_centres", [[[(3.5, 2.5), (40.5, 7.5), (33.5, 30.5), (8.5, 22.5)]]])
    add("on_grid_lines", [[[(3.0, 2.0), (40.0, 7.0), (33.0, 30.0), (8.0, 22.0)]], [rect(50.0, 30.0, 60.0, 40.0)]])
    add("on_centres_rect", [[rect(10.5, 10.5, 20.5, 20.5)], [rect(30.5, 10.5, 40.5, 20.5, clockwise=False)]])
    # horizontal edges on a centre line, running both ways, at the raster's edges too
    add("horizontal_both_ways", [[[(4.5, 3.5), (30.5, 3.5), (30.5, 9.5), (20.0, 9.5), (20.0, 15.5), (4.5, 15.5)]],
                                 [[(60.0, 20.5), (60.0, 30.5), (-5.0, 30.5), (-5.0, 20.5)]],
                                 [[(50.2, 35.5), (80.0, 35.5), (80.0, 44.5), (50.2, 44.5)]],
                                 [[(70.0, 1.5), (90.0, 1.5), (90.0, 5.5), (70.0, 5.5)], [(-9.0, 40.5), (-0.6, 40.5), (-0.6, 42.5), (-9.0, 42.5)]]])
    # the axis-parallel shortcuts of the line pass, on both sides of their thresholds
    add("near_vertical", [[[(10.998, 3.3), (11.003, 40.2), (30.4, 20.0)]], [[(40.2, 2.0), (40.2, 30.0), (50.0, 10.0)]],
                          [[(20.995, -7.0), (21.006, 60.0), (60.0, 33.0)]], [[(5.0, 5.0), (5.011, 35.0), (-3.0, 12.0)]]])
    add("near_horizontal", [[[(3.3, 10.998), (60.2, 11.003), (20.0, 30.4)]], [[(2.0, 40.2), (30.0, 40.2), (10.0, 44.9)]],
                            [[(-7.0, 20.995), (80.0, 21.006), (33.0, 5.0)]], [[(5.0, 5.0), (35.0, 5.011), (12.0, -3.0)]]])
    add("both_slopes", [[[(33.3, 2.2), (64.8, 22.9), (30.1, 43.7), (2.6, 21.4)]], [[(10.2, 3.1), (12.9, 40.8), (15.3, 2.7)]],
                        [[(2.1, 30.3), (66.2, 33.1), (1.7, 35.6)]]])
    # outside and across the borders
    add("outside", [[rect(-40.0, -30.0, -3.5, -2.5)], [rect(70.5, 50.5, 90.0, 80.0)], [rect(10.0, 46.5, 20.0, 50.0)], [rect(68.2, 10.0, 75.0, 20.0)],
                    [[(-20.0, 10.0), (-1.5, 30.0), (-30.0, 44.0)]]])
    add("cross_left", [[[(-10.3, 8.8), (20.6, 15.2), (-4.4, 38.1)]]])
    add("cross_right", [[[(77.3, 8.8), (46.6, 15.2), (71.4, 38.1)]]])
    add("cross_top", [[[(8.8, -10.3), (15.2, 20.6), (38.1, -4.4)]]])
    add("cross_bottom", [[[(8.8, 55.3), (15.2, 24.6), (38.1, 49.4)]]])
    add("cross_all", [[[(33.0, -30.0), (110.0, 22.0), (35.0, 80.0), (-45.0, 24.0)]]])
    add("cover_all", [[rect(-100.0, -100.0, 200.0, 200.0)]])
    add("corner_cuts", [[[(-8.0, 5.5), (6.2, -7.0), (-3.0, -4.0)]], [[(60.3, 50.0), (75.0, 38.6), (73.0, 52.0)]],
                        [[(60.0, -5.0), (72.0, 9.0), (80.0, -3.0)]], [[(-6.0, 37.0), (9.0, 52.0), (-5.0, 50.0)]]])
    add("far_vertices", [[[(-1.0e6, -2.0e5), (2.0e6, 3.0e5), (33.0, 1.0e6)]], [[(-2.0 ** 30, 10.5), (2.0 ** 30, 12.25), (2.0 ** 30, 2.0 ** 30)]]])
    # degenerate rings
    add("two_point_rings", [[[(3.0, 3.0), (20.5, 17.2)]], [[(40.2, 5.5), (40.2, 5.5)]], [[(50.0, 40.0)]], [[(30.1, 30.2), (55.5, 10.9), (30.1, 30.2)]]])
    add("zero_area", [[[(2.0, 2.0), (30.0, 20.0), (58.0, 38.0), (30.0, 20.0), (2.0, 2.0)]], [[(5.5, 40.5), (25.5, 40.5), (15.5, 40.5)]]])
    add("no_features", [])
    add("empty_feature", [[], [rect(3.3, 3.3, 9.9, 9.9)], [[]]])
    add("random_many", [random_polygon(rng, H, W) for _ in range(12)])
    # the output as a window of a wider buffer
    add("window", [random_polygon(rng, 21, 37), [rect(-3.0, 4.4, 50.0, 9.6)]], 21, 37, window=True)
    add("window_wide", [[[(5.3, -1.0), (600.6, 0.2), (640.7, 2.9), (300.5, 1.5), (100.0, 3.7)]]], 3, 641, window=True)
    return out
