// The work items of the marching stretch + Laplacian pass (k_lap.hip, lap_march_item) as a grid over the image, and the pixels whose
// validity each item COUNTS (valid_partial[item]).  One statement of that rule for the kernel that counts, for the fused eigenvalue
// pass (k_eig3.hip), which reads the counts of the items that overlap its own mask rectangle instead of the mask where they decide
// it, and for the host test that holds the count domains to a partition of the image (tests/hoststub/lap_items_main.cpp).
// Plain C++: no HIP type, no device builtin.
//
//   item (strip, rowblock), index rowblock * nstrips + strip (strips fastest)
//   rows     rowblock * rows .. min(H, (rowblock + 1) * rows) - 1
//   columns  strip * strip_w .. min(W, (strip + 1) * strip_w) - 1
// The last strip of a width that is no multiple of 4 is SHIFTED left so that its last lane ends at the image's edge: it recomputes
// columns of its left neighbour and counts only from the column where that neighbour's domain ends - the same first column as an
// unshifted strip's.  The count domains therefore partition the image whatever the width.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LAPI_FN __host__ __device__ inline
#else
#define LAPI_FN inline
#endif

// output columns of a strip: 64 lanes x 4 columns less the halo lanes (one either side; two for radius 5)
#define LAPM_VALID_OF(R) ((R) == 5 ? 240 : 248)

struct lap_item_grid {
    int H, W;          // the image
    int rows;          // rows per item
    int strip_w;       // LAPM_VALID_OF(radius)
    int nstrips;       // lapi_nstrips(W, strip_w)
};
// item indices [s0, s1] x [rb0, rb1], both ends included
struct lap_item_range {
    int s0, s1, rb0, rb1;
};

LAPI_FN int lapi_min(int a, int b) { return a < b ? a : b; }
LAPI_FN int lapi_nstrips(int W, int strip_w) { return (W + strip_w - 1) / strip_w; }
LAPI_FN int lapi_nrowblocks(int H, int rows) { return (H + rows - 1) / rows; }
LAPI_FN lap_item_grid lapi_grid(int H, int W, int rows, int strip_w)
{
    lap_item_grid g = {H, W, rows, strip_w, lapi_nstrips(W, strip_w)};
    return g;
}
// the strip that is shifted left (its lane 0 at column W - 256 + halo lies inside the image)
LAPI_FN bool lapi_shifted(int W, int strip, int nstrips) { return (W % 4 != 0) && strip == nstrips - 1 && W >= 256; }
// count domain of an item: columns [lapi_col0, lapi_col1), rows [lapi_row0, lapi_row1)
LAPI_FN int lapi_col0(const lap_item_grid &g, int strip) { return strip * g.strip_w; }
LAPI_FN int lapi_col1(const lap_item_grid &g, int strip) { return lapi_min(g.W, (strip + 1) * g.strip_w); }
LAPI_FN int lapi_row0(const lap_item_grid &g, int rowblock) { return rowblock * g.rows; }
LAPI_FN int lapi_row1(const lap_item_grid &g, int rowblock) { return lapi_min(g.H, (rowblock + 1) * g.rows); }
// first column a SHIFTED strip counts (everything left of it belongs to its neighbour); an unshifted strip counts all its output columns
LAPI_FN int lapi_count_from(const lap_item_grid &g, int strip) { return lapi_shifted(g.W, strip, g.nstrips) ? lapi_col0(g, strip) : 0; }
LAPI_FN int lapi_index(const lap_item_grid &g, int strip, int rowblock) { return rowblock * g.nstrips + strip; }
LAPI_FN unsigned lapi_area(const lap_item_grid &g, int strip, int rowblock)
{
    return (unsigned)(lapi_col1(g, strip) - lapi_col0(g, strip)) * (unsigned)(lapi_row1(g, rowblock) - lapi_row0(g, rowblock));
}
// the items whose count domains meet the rectangle rows [y0, y1] x columns [x0, x1) (non-empty, inside the image)
LAPI_FN lap_item_range lapi_items_of_rect(const lap_item_grid &g, int y0, int y1, int x0, int x1)
{
    lap_item_range r = {x0 / g.strip_w, (x1 - 1) / g.strip_w, y0 / g.rows, y1 / g.rows};
    return r;
}
