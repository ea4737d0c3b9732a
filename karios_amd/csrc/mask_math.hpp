// mask_math.hpp: the arithmetic of the vector-mask burn - GDAL's polygon fill at pixel centres and its all-touched line pass, as
// gdal.RasterizeLayer(..., ['BURN=1', 'ALL_TOUCHED=TRUE']) applies them (karios/core/image.py:104-191) - as plain C++ on doubles, shared
// by the kernels (k_mask.hip), the host build of the launchers (k_mask.hpp) and the CPU test (tests/test_mask_host.py compiles this
// file with g++).  tests/rasterize_restatement.py is the definition; every function here is held to it bit for bit, which needs
// -ffp-contract=off and correctly rounded division on every compiler that reads this text.
// Domain (checked on the host before anything runs): every coordinate finite with |v| <= 2^30, so every rounded value fits an int.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MK_HD __host__ __device__
#else
#define MK_HD
#endif

namespace mk {

constexpr double MAX_COORD = 1073741824.0;
constexpr int MAX_VERTICES = 1 << 20;
constexpr double TINY = 0.000000001;       // the walk's smallest step along y

// one edge of a ring: vertex i - 1 (the fill's ind1, the line pass's start) -> vertex i (ind2, the end); 32 bytes
struct edge {
    double x1, y1, x2, y2;
};

// ---- the fill: an edge against the centre line dy = row + 0.5
enum { NONE = 0, CROSS = 1, SPAN = 2 };
// CROSS: a = the rounded crossing.  SPAN: a horizontal edge on the centre line that runs leftwards, columns [a, b] before the clamp
MK_HD inline int crossing(const edge &e, double dy, int &a, int &b)
{
    if ((e.y1 < dy && e.y2 < dy) || (e.y1 > dy && e.y2 > dy)) return NONE;
    double dy1, dy2, dx1, dx2;
    if (e.y1 < e.y2) { dy1 = e.y1; dy2 = e.y2; dx1 = e.x1; dx2 = e.x2; }
    else if (e.y1 > e.y2) { dy1 = e.y2; dy2 = e.y1; dx1 = e.x2; dx2 = e.x1; }
    else {
        if (e.x1 > e.x2) { a = (int)floor(e.x2 + 0.5); b = (int)floor(e.x1 + 0.5) - 1; return SPAN; }
        return NONE;
    }
    if (dy1 <= dy && dy < dy2) {
        double t = dy - dy1;                // every operation rounds on its own, in this order
        t = t * (dx2 - dx1);
        t = t / (dy2 - dy1);
        t = t + dx1;
        a = (int)floor(t + 0.5);
        return CROSS;
    }
    return NONE;
}

// the rows whose centre lines a feature's fill visits, from the extremes of its vertices: (int) is the C cast, toward zero
MK_HD inline void row_range(double min_y, double max_y, int H, int &miny, int &maxy)
{
    miny = (int)min_y; if (miny < 0) miny = 0;
    maxy = (int)max_y; if (maxy > H - 1) maxy = H - 1;
}

// ---- the line pass: one consecutive vertex pair
enum { L_SKIP = 0, L_COLUMN = 1, L_ROW = 2, L_WALK = 3 };
struct line_plan {
    int kind;
    int fixed, lo, hi;        // L_COLUMN: rows lo .. hi of column `fixed`; L_ROW: columns lo .. hi of row `fixed` (clamped, lo <= hi)
    double x, y, xe, s;       // L_WALK: the clipped start, the end along x, the slope
};

MK_HD inline void plan_line(const edge &e, int H, int W, line_plan &p)
{
    double x = e.x1, y = e.y1, xe = e.x2, ye = e.y2;
    p.kind = L_SKIP;
    if ((y < 0 && ye < 0) || (y > H && ye > H) || (x < 0 && xe < 0) || (x > W && xe > W)) return;
    if (x > xe) { double t = x; x = xe; xe = t; t = y; y = ye; ye = t; }
    if (floor(x) == floor(xe) || fabs(x - xe) < .01) {
        const int ix = (int)floor(xe);
        int lo = (int)floor(y < ye ? y : ye), hi = (int)floor(y < ye ? ye : y);
        if (lo < 0) lo = 0;
        if (hi > H - 1) hi = H - 1;
        if (ix < 0 || ix >= W || lo > hi) return;
        p.kind = L_COLUMN; p.fixed = ix; p.lo = lo; p.hi = hi;
        return;
    }
    if (floor(y) == floor(ye) || fabs(y - ye) < .01) {
        const int iy = (int)floor(y);
        int lo = (int)floor(x), hi = (int)floor(xe);
        if (lo < 0) lo = 0;
        if (hi > W - 1) hi = W - 1;
        if (iy < 0 || iy >= H || lo > hi) return;
        p.kind = L_ROW; p.fixed = iy; p.lo = lo; p.hi = hi;
        return;
    }
    const double s = (ye - y) / (xe - x);
    if (xe > W) { ye -= (xe - W) * s; xe = W; }
    if (x < 0) { y += (0.0 - x) * s; x = 0; }
    if (ye > y) {
        if (y < 0) { x += (0.0 - y) / s; y = 0; }
        if (ye >= H) xe += (ye - H) / s;
    } else {
        if (y >= H) { x += (H - y) / s; y = H; }
        if (ye < 0) xe -= ye / s;
    }
    p.kind = L_WALK; p.x = x; p.y = y; p.xe = xe; p.s = s;
}

// One step of the walk.  false: the walk has ended (x has left [0, xe), or the row has left the raster in the direction of travel -
// y is monotone, nothing further can burn).  Else (ix, iy) is the pixel of this step and `burn` says whether it lies in the raster;
// the walk then moves on.  The column test of `burn` is a memory guard: the definition counts the burns it would refuse, none is known.
MK_HD inline bool walk_step(line_plan &p, int H, int W, int &ix, int &iy, bool &burn)
{
    if (!(p.x >= 0.0 && p.x < p.xe)) return false;
    const double fx = floor(p.x), fy = floor(p.y);
    if ((p.s > 0 && fy >= H) || (p.s < 0 && fy < 0)) return false;
    burn = fy >= 0 && fy < H && fx < W;
    ix = burn ? (int)fx : 0;
    iy = burn ? (int)fy : 0;
    double sx = floor(p.x + 1.0) - p.x, sy = sx * p.s;
    if (floor(p.y + sy) == fy) { p.x += sx; p.y += sy; return true; }
    if (p.s < 0) {
        sy = fy - p.y;
        if (sy > -TINY) sy = -TINY;
    } else {
        sy = (fy + 1) - p.y;
        if (sy < TINY) sy = TINY;
    }
    sx = sy / p.s;
    p.x += sx;
    p.y += sy;
    return true;
}

MK_HD inline long long walk_cap(int H, int W) { return 4 * ((long long)H + W) + 64; }

}  // namespace mk
