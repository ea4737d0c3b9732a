// The item geometry of the marching Laplacian pass (karios_amd/csrc/lap_items.hpp) as plain C++, held to the kernel's lane rule.
// A program of its own (g++ -fsanitize=address,undefined; tests/test_lap_items_host.py builds and runs it).  For every height 1 .. 200,
// every width 8 .. 700, 8 / 32 / 33 / 160 rows per item and both strip widths:
//   * the columns a strip COUNTS by the kernel's rule - lane l of a strip holds the four columns gx0 .. gx0 + 3, gx0 from the strip's
//     (or the shifted last strip's) origin; output lanes only, inside the image, from lapi_count_from on - are exactly
//     [lapi_col0, lapi_col1), every column of the image is counted by exactly one strip, every row by exactly one row block, and the
//     areas of the items add up to the image;
//   * the items lapi_items_of_rect returns for a rectangle cover it, and none of them misses it: for every column range and every row
//     range of the image.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../karios_amd/csrc/lap_items.hpp"

static long long checks = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        checks++;                                                                 \
        if (!(cond)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } \
    } while (0)

// the columns strip `strip` counts, as lap_march_item's lanes do (k_lap.hip: gx0, out_lane, cnt_from / cnt_mask, `gx0 + j < W`)
static void count_columns_of_strip(const lap_item_grid &g, int strip, std::vector<int> &hits, int &first, int &last)
{
    const int halo = (256 - g.strip_w) / 2;
    const bool shifted = lapi_shifted(g.W, strip, g.nstrips);
    const int cnt_from = lapi_count_from(g, strip);
    first = g.W; last = -1;
    for (int lane = 0; lane < 64; lane++) {
        const int gx0 = (shifted ? g.W - (256 - halo) : strip * g.strip_w - halo) + 4 * lane;
        const bool out_lane = lane >= halo / 4 && lane <= 63 - halo / 4 && gx0 < g.W;
        if (!out_lane) continue;
        for (int j = 0; j < 4; j++) {
            const int x = gx0 + j;
            if (x < 0 || x >= g.W || x < cnt_from) continue;
            hits[(size_t)x]++;
            first = x < first ? x : first;
            last = x > last ? x : last;
        }
    }
}

int main()
{
    const int rows_of[4] = {8, 32, 33, 160};
    const int strip_w_of[2] = {LAPM_VALID_OF(3), LAPM_VALID_OF(5)};
    for (int sw = 0; sw < 2; sw++) {
        const int strip_w = strip_w_of[sw];
        for (int W = 8; W <= 700; W++) {
            // ---- columns: independent of the height and of the rows per item
            const lap_item_grid g = lapi_grid(1, W, 8, strip_w);
            CHECK(g.nstrips == (W + strip_w - 1) / strip_w && g.nstrips >= 1, "W %d", W);
            std::vector<int> hits((size_t)W, 0);
            for (int s = 0; s < g.nstrips; s++) {
                int first, last;
                count_columns_of_strip(g, s, hits, first, last);
                CHECK(first == lapi_col0(g, s) && last + 1 == lapi_col1(g, s), "W %d strip_w %d strip %d: lanes count %d .. %d, header %d .. %d", W, strip_w, s,
                      first, last, lapi_col0(g, s), lapi_col1(g, s) - 1);
                CHECK(lapi_col0(g, s) < lapi_col1(g, s), "W %d strip %d: empty", W, s);
                if (s) CHECK(lapi_col0(g, s) == lapi_col1(g, s - 1), "W %d strip %d: gap or overlap", W, s);
            }
            CHECK(lapi_col0(g, 0) == 0 && lapi_col1(g, g.nstrips - 1) == W, "W %d", W);
            for (int x = 0; x < W; x++) CHECK(hits[(size_t)x] == 1, "W %d strip_w %d: column %d counted %d times", W, strip_w, x, hits[(size_t)x]);
            // every column range [x0, x1): the strips returned cover it, and the first and the last one meet it
            for (int x0 = 0; x0 < W; x0++)
                for (int x1 = x0 + 1; x1 <= W; x1++) {
                    const lap_item_range r = lapi_items_of_rect(g, 0, 0, x0, x1);
                    CHECK(r.s0 >= 0 && r.s0 <= r.s1 && r.s1 < g.nstrips, "W %d [%d, %d)", W, x0, x1);
                    CHECK(lapi_col0(g, r.s0) <= x0 && x0 < lapi_col1(g, r.s0), "W %d [%d, %d): first strip %d", W, x0, x1, r.s0);
                    CHECK(lapi_col0(g, r.s1) < x1 && x1 <= lapi_col1(g, r.s1), "W %d [%d, %d): last strip %d", W, x0, x1, r.s1);
                }
        }
    }
    for (int ri = 0; ri < 4; ri++) {
        const int rows = rows_of[ri];
        for (int H = 1; H <= 200; H++) {
            const lap_item_grid g = lapi_grid(H, 8, rows, strip_w_of[0]);
            const int nrb = lapi_nrowblocks(H, rows);
            for (int rb = 0; rb < nrb; rb++) {
                CHECK(lapi_row0(g, rb) < lapi_row1(g, rb), "H %d rows %d block %d: empty", H, rows, rb);
                if (rb) CHECK(lapi_row0(g, rb) == lapi_row1(g, rb - 1), "H %d rows %d block %d", H, rows, rb);
            }
            CHECK(lapi_row0(g, 0) == 0 && lapi_row1(g, nrb - 1) == H, "H %d rows %d", H, rows);
            // every row range [y0, y1], both ends included
            for (int y0 = 0; y0 < H; y0++)
                for (int y1 = y0; y1 < H; y1++) {
                    const lap_item_range r = lapi_items_of_rect(g, y0, y1, 0, 1);
                    CHECK(r.rb0 >= 0 && r.rb0 <= r.rb1 && r.rb1 < nrb, "H %d rows %d [%d, %d]", H, rows, y0, y1);
                    CHECK(lapi_row0(g, r.rb0) <= y0 && y0 < lapi_row1(g, r.rb0), "H %d rows %d [%d, %d]", H, rows, y0, y1);
                    CHECK(lapi_row0(g, r.rb1) <= y1 && y1 < lapi_row1(g, r.rb1), "H %d rows %d [%d, %d]", H, rows, y0, y1);
                }
            // both directions together: indices are distinct and dense, areas add up to the image
            for (int sw = 0; sw < 2; sw++)
                for (int W = 8; W <= 700; W++) {
                    const lap_item_grid q = lapi_grid(H, W, rows, strip_w_of[sw]);
                    unsigned long long area = 0;
                    int next = 0;
                    for (int rb = 0; rb < nrb; rb++)
                        for (int s = 0; s < q.nstrips; s++) {
                            if (lapi_index(q, s, rb) != next++) CHECK(false, "H %d W %d rows %d: index of (%d, %d)", H, W, rows, s, rb);
                            area += lapi_area(q, s, rb);
                        }
                    CHECK(area == (unsigned long long)H * (unsigned long long)W, "H %d W %d rows %d strip_w %d: areas %llu", H, W, rows, strip_w_of[sw], area);
                }
        }
    }
    std::printf("%lld checks\nLAP-ITEMS OK\n", checks);
    return 0;
}
