// TEST INFRASTRUCTURE (tests/test_frame_layout_host.py): the frame block's one layout, the arena of the kernel-size search and the search
// itself in every form.  A program of its own (no python, no preload) linked from the host objects of the sanitizer build and the
// stand-in HIP layer:
//   1. km_frame_layout against the words karios_amd.frames.block_words / block_to_frame read;
//   2. km_auto_arena_of: regions ascending, disjoint, aligned, large enough, the total the formula the search always used;
//   3. km_klt_auto_ksize_frame_dev on the stand-in - all batched, corners batched + trackers one by one, all one by one, flagged units
//      repaired - per case the same ratios, winner and frame block in every form;
//   4. a blocking tile frame call and a three-unit batched submission with ZNCC and MI columns: every column at its word.
//   5. km_frame_from_tracks (the frame stage alone, tests/test_frame_host.py): a handful of cases with their expected rows written out;
//      `frame --tracks IN OUT` runs the records of a file through it instead and prints 'FRAME-TRACKS OK'.
// 3 to 5 use the public C ABI only and print one digest line per case.  Prints 'FRAME-LAYOUT OK' at the end.
#ifdef FRAME_MAIN_ABI_ONLY      // (parts 3 and 4 alone: they build against any csrc/ with the same C ABI)
#include "../../karios_amd/csrc/common.hpp"
#else
#include "../../karios_amd/csrc/api_internal.hpp"
#endif

#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

static int g_failures = 0;
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "frame_main.cpp:%d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); g_failures++; } } while (0)
#define CALL(expr) do { const int rc_ = (expr); REQUIRE(rc_ == KM_OK, "%s -> %d (%s)", #expr, rc_, km_last_error(c)); } while (0)

// the words of a block as karios_amd.frames reads them: float32 column i, float64 score column k (in 4-byte words)
static size_t word_of_col(int cap, int i) { return 4 + (size_t)i * cap; }
static size_t word_of_score(int cap, int k) { return 4 + (size_t)(6 + 2 * k) * cap; }
static size_t block_words(int cap, int n_scores) { return 4 + (size_t)(6 + 2 * n_scores) * cap; }

static unsigned long long fnv(unsigned long long h, const void *p, size_t n)
{
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
    return h;
}

#ifndef FRAME_MAIN_ABI_ONLY
static void check_layout()
{
    static_assert(std::is_trivially_copyable<km_frame_layout>::value && !std::is_polymorphic<km_frame_layout>::value, "km_frame_layout is a plain struct");
    for (int cap : {1, 7, 64, 32768})
        for (int k : {0, 1, 3}) {
            const km_frame_layout L(cap, k >= 1, k == 3);
            REQUIRE(L.ob == 4 * block_words(cap, k) && L.ob == 4 * (4 + (size_t)(6 + 2 * k) * cap), "cap %d, %d score columns: ob %zu", cap, k, L.ob);
            REQUIRE(L.fb == 16 + (size_t)24 * cap, "cap %d: fb %zu", cap, L.fb);
            REQUIRE(L.ob_al % 256 == 0 && L.ob_al >= L.ob && L.ob_al - L.ob < 256, "cap %d, %d score columns: ob_al %zu of ob %zu", cap, k, L.ob_al, L.ob);
            std::vector<char> block(L.ob);
            char *b = block.data();
            REQUIRE((const char *)L.header(b) == b, "header");
            for (int i = 0; i < 6; i++) REQUIRE((const char *)L.col(b, i) == b + 4 * word_of_col(cap, i), "cap %d: float32 column %d", cap, i);
            for (int s = 0; s < k; s++) REQUIRE((char *)L.score_col(b, s) == b + 4 * word_of_score(cap, s), "cap %d: score column %d", cap, s);
            if (k >= 1) {
                km_score_unit z, m;
                L.score_unit(z, b, false);
                REQUIRE(z.d_n == (const int *)b && z.x0 == L.col(b, 0) && z.y0 == L.col(b, 1) && z.dx == L.col(b, 2) && z.dy == L.col(b, 3) && z.score == L.col(b, 4) &&
                            z.out == L.score_col(b, 0) && !z.out2, "cap %d: the ZNCC rows of a score unit", cap);
                if (k == 3) {
                    L.score_unit(m, b, true);
                    REQUIRE(m.x0 == z.x0 && m.score == z.score && m.out == L.score_col(b, 1) && m.out2 == L.score_col(b, 2), "cap %d: the MI rows of a score unit", cap);
                }
            }
        }
}

static void check_arena()
{
    for (int nk : {1, 2, 5, 8})
        for (size_t pyr_bytes : {(size_t)0, (size_t)8192})
            for (int cap : {1, 64, 20000}) {
                const int H = 64, W = 512;
                const km_auto_arena a = km_auto_arena_of(nk, H, W, pyr_bytes, cap);
                const size_t k = (size_t)nk, px = (size_t)H * W, pb = (size_t)cap * 2 * sizeof(float);
                const size_t start[6] = {a.lap_ref, a.lap_mon, a.pyr, a.p0, a.trk, a.counts};
                const size_t use[6] = {(k - 1) * a.na + px, (k - 1) * a.na + px, pyr_bytes ? (2 * k - 1) * a.pyr_bytes + pyr_bytes : 0, (k - 1) * a.pts + pb,
                                       (2 * k * k - 1) * a.pts + pb, (k + k * k) * sizeof(int)};
                for (int r = 0; r < 6; r++) {
                    const size_t end = r < 5 ? start[r + 1] : a.total;
                    REQUIRE(start[r] <= end && start[r] + use[r] <= end, "nk %d, pyramid %zu, cap %d: region %d [%zu, %zu) holds %zu bytes", nk, pyr_bytes, cap, r, start[r],
                            end, use[r]);
                    if (r < 5) REQUIRE(start[r] % 256 == 0, "nk %d, pyramid %zu, cap %d: region %d starts at %zu", nk, pyr_bytes, cap, r, start[r]);
                }
                REQUIRE(a.pyr_bytes == pyr_bytes && a.na >= px && a.pts >= pb && a.counts_bytes >= (k + k * k) * sizeof(int) && a.counts + a.counts_bytes == a.total,
                        "nk %d, pyramid %zu, cap %d: pitches and counters", nk, pyr_bytes, cap);
                const size_t na = (px + 255) & ~(size_t)255, pts = (pb + 255) & ~(size_t)255;
                REQUIRE(a.total == 2 * k * (na + pyr_bytes) + k * pts + 2 * k * k * pts + 4096, "nk %d, pyramid %zu, cap %d: total %zu", nk, pyr_bytes, cap, a.total);
            }
}
#endif

// device memory of the caller (km_dev_alloc), filled from host memory
struct dev_buf {
    km_ctx *c;
    void *p = nullptr;
    dev_buf(km_ctx *ctx, const void *src, size_t bytes) : c(ctx)
    {
        if (km_dev_alloc(c, bytes, &p) != KM_OK) p = nullptr;
        REQUIRE(p && km_h2d(c, p, src, bytes) == KM_OK, "device buffer of %zu bytes", bytes);
    }
    ~dev_buf() { if (p) (void)km_dev_free(c, p); }
    dev_buf(const dev_buf &) = delete;
};

static void fill_pair(std::vector<uint16_t> &ref, std::vector<uint16_t> &mon)
{
    for (size_t i = 0; i < ref.size(); i++) { ref[i] = (uint16_t)(1 + (i * 2654435761u >> 20) % 9000); mon[i] = (uint16_t)(1 + (i * 40503u >> 7) % 9000); }
}

static km_klt_params params(int cap)
{
    km_klt_params prm = {};
    prm.max_corners = cap; prm.block_size = 15; prm.win_size = 21; prm.max_level = 1; prm.max_count = 30;
    prm.ksize_mon = prm.ksize_ref = 7; prm.quality_level = 0.1; prm.min_distance = 10.0; prm.epsilon = 0.03;
    return prm;
}

struct search_result {
    std::vector<double> ratios;
    int best[2] = {0, 0};
    std::vector<char> block;
    int path_flags = 0;
    bool same(const search_result &o) const
    {
        return ratios.size() == o.ratios.size() && !memcmp(ratios.data(), o.ratios.data(), ratios.size() * sizeof(double)) && best[0] == o.best[0] && best[1] == o.best[1] &&
               block == o.block;
    }
    unsigned long long digest() const { return fnv(fnv(fnv(14695981039346656037ull, ratios.data(), ratios.size() * sizeof(double)), best, sizeof best), block.data(), block.size()); }
};

// the four forms of the search (the stand-in's knobs and the library's options), for every shape, candidate count and mask
static void check_search(km_ctx *c)
{
    static const int all_ksizes[8] = {3, 5, 7, 9, 11, 13, 15, 17};
    const int cap = 64;
    const km_klt_params prm = params(cap);
    const char *const form_name[4] = {"batched", "corners batched, trackers one by one", "one by one", "flagged and repaired"};
    stub().corners_like_exact = true;
    for (int W : {512, 40}) {
        const int H = 64;
        const bool batchable = W >= 512;          // (40 columns: no pyramid level exists, every form runs one by one)
        std::vector<uint16_t> ref((size_t)H * W), mon(ref.size());
        fill_pair(ref, mon);
        const ptrdiff_t wide = W + 24;
        std::vector<uint8_t> mask_dense((size_t)H * W, 1), mask_wide((size_t)H * wide, 0);
        for (int y = 0; y < 20; y++) for (int x = 0; x < 17; x++) mask_dense[(size_t)y * W + x] = 0;
        for (int y = 0; y < H; y++) memcpy(&mask_wide[(size_t)y * wide], &mask_dense[(size_t)y * W], (size_t)W);
        dev_buf dr(c, ref.data(), ref.size() * 2), dm(c, mon.data(), mon.size() * 2), dmd(c, mask_dense.data(), mask_dense.size()), dmw(c, mask_wide.data(), mask_wide.size());
        struct { const char *name; const uint8_t *d; ptrdiff_t stride; } const masks[3] = {{"dense", (const uint8_t *)dmd.p, W}, {"strided", (const uint8_t *)dmw.p, wide}, {"none", nullptr, 0}};
        for (int nk : {1, 3, 8}) {
            if (!batchable && nk != 3) continue;
            unsigned long long digest_of_mask[3] = {0, 0, 0};
            for (int mk = 0; mk < 3; mk++) {
                search_result r[4];
                for (int form = 0; form < 4; form++) {
                    stub().lk_jobs_unsupported = form == 1;
                    CALL(km_set_option(c, "lk2", form == 2 ? 0 : 1));
                    CALL(km_set_option(c, "spec_flag", form == 3 ? 32 : 0));
                    r[form].ratios.assign((size_t)nk * nk, -7.0);
                    r[form].block.assign(4 * block_words(cap, 0), 0x5a);
                    CALL(km_klt_auto_ksize_frame_dev(c, dr.p, dm.p, KM_U16, H, W, W, W, masks[mk].d, masks[mk].stride, nullptr, nullptr, &prm, all_ksizes, nk, 3.f, 5.f,
                                                     r[form].block.data(), cap, r[form].ratios.data(), r[form].best));
                    km_klt_stats st;
                    CALL(km_get_klt_stats(c, &st));
                    r[form].path_flags = st.path_flags;
                    REQUIRE(((st.path_flags & KM_PATH_SPEC_RETRY) != 0) == (batchable && form == 3), "%dx%d nk %d mask %s, %s: path_flags %d", H, W, nk, masks[mk].name,
                            form_name[form], st.path_flags);
                    REQUIRE(r[form].same(r[0]), "%dx%d nk %d mask %s: '%s' differs from '%s'", H, W, nk, masks[mk].name, form_name[form], form_name[0]);
                }
                stub().lk_jobs_unsupported = false;
                CALL(km_set_option(c, "lk2", 1));
                CALL(km_set_option(c, "spec_flag", 0));
                const int *hdr = (const int *)r[0].block.data();
                REQUIRE(hdr[1] == cap && hdr[0] > 0 && hdr[0] <= cap && r[0].best[0] == all_ksizes[0] && r[0].best[1] == all_ksizes[0], "%dx%d nk %d mask %s: %d of %d rows, best (%d, %d)",
                        H, W, nk, masks[mk].name, hdr[0], hdr[1], r[0].best[0], r[0].best[1]);
                digest_of_mask[mk] = r[0].digest();
                printf("search %dx%d nk=%d mask=%s best=(%d,%d) ratio0=%.6f rows=%d/%d digest=%016llx\n", H, W, nk, masks[mk].name, r[0].best[0], r[0].best[1], r[0].ratios[0],
                       hdr[0], hdr[1], digest_of_mask[mk]);
            }
            REQUIRE(digest_of_mask[0] == digest_of_mask[1], "%dx%d nk %d: the strided mask gives another result than the same mask in dense rows", H, W, nk);
        }
    }
    stub().corners_like_exact = false;
}

// the score columns of one block at the words block_to_frame reads; rows_all: the MI stand-in filled every row (tile form) or the kept ones
static void check_scores(const char *what, const char *block, int cap, float thr, bool mi_rows_all)
{
    const int *hdr = (const int *)block;
    const float *f = (const float *)block;
    const int kept = hdr[0];
    REQUIRE(kept > 0 && kept <= hdr[1] && hdr[1] <= cap, "%s: header %d / %d", what, hdr[0], hdr[1]);
    const float *x0 = f + word_of_col(cap, 0), *score = f + word_of_col(cap, 4);
    double z[2], s[2], m[2];
    for (int e = 0; e < 2; e++) {      // first and last element of every score column
        const size_t i = e ? (size_t)cap - 1 : 0;
        memcpy(&z[e], f + word_of_score(cap, 0) + 2 * i, 8); memcpy(&s[e], f + word_of_score(cap, 1) + 2 * i, 8); memcpy(&m[e], f + word_of_score(cap, 2) + 2 * i, 8);
        const bool row = (int)i < kept;
        if (row && score[i] >= thr) REQUIRE(z[e] == (double)x0[i], "%s: zncc[%zu] = %g", what, i, z[e]);
        else REQUIRE(std::isnan(z[e]), "%s: zncc[%zu] = %g", what, i, z[e]);
        if (row || mi_rows_all) REQUIRE(s[e] == (double)x0[i] && m[e] == -(double)x0[i], "%s: mi[%zu] = %g, %g", what, i, s[e], m[e]);
        else REQUIRE(std::isnan(s[e]) && std::isnan(m[e]), "%s: mi[%zu] = %g, %g", what, i, s[e], m[e]);
    }
}

static void check_tile_and_units(km_ctx *c)
{
    const int H = 64, W = 512, cap = 64;
    const float thr = 0.4f;
    const km_klt_params prm = params(cap);
    std::vector<uint16_t> ref((size_t)H * W), mon(ref.size());
    fill_pair(ref, mon);
    dev_buf dr(c, ref.data(), ref.size() * 2), dm(c, mon.data(), mon.size() * 2);
    const size_t ob = 4 * block_words(cap, 3);
    CALL(km_set_option(c, "frame_mi", 1));
    {
        std::vector<char> block(ob, 0x5a);
        CALL(km_klt_tile_frame_zncc_dev(c, dr.p, dm.p, KM_U16, H, W, W, W, nullptr, 0, nullptr, nullptr, &prm, 3.f, 5.f, dr.p, dm.p, H, W, W, W, thr, block.data(), cap));
        check_scores("tile frame", block.data(), cap, thr, true);
        printf("tile-frame 64x512 rows=%d/%d digest=%016llx\n", ((const int *)block.data())[0], ((const int *)block.data())[1], fnv(14695981039346656037ull, block.data(), ob));
    }
    km_unit units[3] = {};
    const int box[3][2] = {{0, H}, {8, H - 16}, {4, H - 8}};    // {first row, rows}: 512 columns, the narrowest the batch form takes
    for (int u = 0; u < 3; u++) {
        units[u].d_ref = (const uint16_t *)dr.p + (size_t)box[u][0] * W; units[u].d_mon = (const uint16_t *)dm.p + (size_t)box[u][0] * W;
        units[u].sref = units[u].smon = units[u].sref_f = units[u].smon_f = W;
        units[u].d_ref_full = dr.p; units[u].d_mon_full = dm.p;
        units[u].H = box[u][1]; units[u].W = W; units[u].Hf = H; units[u].Wf = W; units[u].y_off = (float)box[u][0];
    }
    int ticket = -1;
    const void *blocks = nullptr;
    size_t nb = 0;
    CALL(km_klt_units_frame_submit(c, units, 3, KM_U16, nullptr, nullptr, &prm, thr, cap, &ticket));
    CALL(km_frame_wait(c, ticket, &blocks, &nb));
    REQUIRE(nb == 3 * ob, "three blocks of %zu bytes: %zu", ob, nb);
    if (blocks && nb == 3 * ob) {
        for (int u = 0; u < 3; u++) {
            const char *b = (const char *)blocks + ob * u;
            REQUIRE(((const int *)b)[1] == 40 + u, "unit %d: %d corners", u, ((const int *)b)[1]);
            check_scores(u == 0 ? "unit 0" : u == 1 ? "unit 1" : "unit 2", b, cap, thr, false);
        }
        printf("units-frame 3x512 digest=%016llx\n", fnv(14695981039346656037ull, blocks, nb));
    }
    CALL(km_set_option(c, "frame_mi", 0));
}

// ---- km_frame_from_tracks (the frame stage alone, tests/test_frame_host.py)
struct track_unit {
    std::vector<float> p0, p1, p0r;
    int n = 0, width = 0;
    float x_off = 0.f, y_off = 0.f;
};
static int run_tracks(km_ctx *c, const std::vector<track_unit> &units, int n_max, int cap, std::vector<char> &blocks)
{
    const size_t k = units.size(), pts = (size_t)n_max * 2;
    std::vector<float> p0(k * pts), p1(k * pts), p0r(k * pts), xo(k), yo(k);
    std::vector<int> n(k), width(k);
    for (size_t u = 0; u < k; u++) {
        REQUIRE(units[u].p0.size() == pts && units[u].p1.size() == pts && units[u].p0r.size() == pts, "unit %zu: %d points each", u, n_max);
        memcpy(&p0[u * pts], units[u].p0.data(), pts * 4); memcpy(&p1[u * pts], units[u].p1.data(), pts * 4); memcpy(&p0r[u * pts], units[u].p0r.data(), pts * 4);
        n[u] = units[u].n; width[u] = units[u].width; xo[u] = units[u].x_off; yo[u] = units[u].y_off;
    }
    blocks.assign(k * 4 * block_words(cap, 0), 0x5a);
    return km_frame_from_tracks(c, (int)k, p0.data(), p1.data(), p0r.data(), n.data(), xo.data(), yo.data(), width.data(), n_max, cap, blocks.data());
}
struct want_row { float x0, y0, dx, dy, score; int label; };
static unsigned bits_of(float v) { unsigned u; memcpy(&u, &v, 4); return u; }
static void expect_block(const char *what, const char *block, int cap, int n_init, const std::vector<want_row> &rows)
{
    const int *hdr = (const int *)block;
    const float *f = (const float *)block;
    REQUIRE(hdr[0] == (int)rows.size() && hdr[1] == n_init && hdr[2] == 0 && hdr[3] == 0, "%s: header %d %d %d %d, expected %zu rows of %d", what, hdr[0], hdr[1], hdr[2], hdr[3],
            rows.size(), n_init);
    if (hdr[0] != (int)rows.size()) return;
    for (size_t i = 0; i < rows.size(); i++) {
        const float got[5] = {f[word_of_col(cap, 0) + i], f[word_of_col(cap, 1) + i], f[word_of_col(cap, 2) + i], f[word_of_col(cap, 3) + i], f[word_of_col(cap, 4) + i]};
        const float exp[5] = {rows[i].x0, rows[i].y0, rows[i].dx, rows[i].dy, rows[i].score};
        for (int c2 = 0; c2 < 5; c2++) REQUIRE(bits_of(got[c2]) == bits_of(exp[c2]), "%s: row %zu column %d = %g (%08x), expected %g (%08x)", what, i, c2, (double)got[c2], bits_of(got[c2]),
                                               (double)exp[c2], bits_of(exp[c2]));
        int label;
        memcpy(&label, &f[word_of_col(cap, 5) + i], 4);
        REQUIRE(label == rows[i].label, "%s: row %zu label %d, expected %d", what, i, label, rows[i].label);
    }
}
// one unit of n_max rows: corner (x, y) tracked to (x + 0.5, y - 0.25), back to (x + ex, y + ey)
static track_unit unit_of(const std::vector<float> &x, const std::vector<float> &y, const std::vector<float> &ex, const std::vector<float> &ey)
{
    track_unit u;
    for (size_t i = 0; i < x.size(); i++) {
        u.p0.push_back(x[i]); u.p0.push_back(y[i]);
        u.p1.push_back(x[i] + 0.5f); u.p1.push_back(y[i] - 0.25f);
        u.p0r.push_back(x[i] + ex[i]); u.p0r.push_back(y[i] + ey[i]);
    }
    u.n = (int)x.size();
    return u;
}
// a handful of the cases of tests/frame_cases.py, expected values written out by hand
static void check_tracks(km_ctx *c)
{
    const float thr = 0.1f, below = std::nextafterf(thr, 0.f), above = std::nextafterf(thr, 1.f), nan = NAN, inf = INFINITY;
    std::vector<char> blocks;
    {   // the cut at the threshold, in x alone, in y alone, NaN / inf in one component; every corner at 0 (the distance is exact there)
        const std::vector<float> ex = {0.f, below, thr, above, 0.f, 0.f, nan, 0.05f, inf, -0.f, 0.f}, ey = {0.f, 0.f, 0.f, 0.f, below, thr, 0.05f, nan, 0.f, 0.f, 0.f};
        const std::vector<float> z(ex.size(), 0.f);
        track_unit u = unit_of(z, z, ex, ey);
        u.n = (int)ex.size() - 1;                       // (the last row lies behind the count word)
        CALL(run_tracks(c, {u}, (int)ex.size(), 16, blocks));
        const float s_below = 1.f - below / thr;
        // all corners equal: the rows keep their list order, the labels count up
        expect_block("cut", blocks.data(), 16, u.n, {{0, 0, .5f, -.25f, 1.f, 0}, {0, 0, .5f, -.25f, s_below, 1}, {0, 0, .5f, -.25f, s_below, 2}, {0, 0, .5f, -.25f, 1.f, 3}});
    }
    {   // order, ties, origin, capacity: corners (3,1) (1,2) (3,1) (1,0) (2,9), capacity 4, origin (10, 20), no count word
        track_unit u = unit_of({3, 1, 3, 1, 2}, {1, 2, 1, 0, 9}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0});
        u.n = -1; u.x_off = 10.f; u.y_off = 20.f; u.width = 4;
        CALL(run_tracks(c, {u}, 5, 4, blocks));
        expect_block("order", blocks.data(), 4, 5, {{11, 20, .5f, -.25f, 1.f, 3}, {11, 22, .5f, -.25f, 1.f, 1}, {13, 21, .5f, -.25f, 1.f, 0}, {13, 21, .5f, -.25f, 1.f, 2}});
    }
    {   // three units of different length in one call, a count word above n_max, an empty unit; each as when submitted alone
        track_unit a = unit_of({5, 4, 3}, {0, 0, 0}, {0, 0.2f, 0}, {0, 0, 0}), b = unit_of({7, 7, 7}, {2, 1, 0}, {0, 0, 0}, {0, 0, 0}), e = b;
        a.n = 5000; b.n = 2; e.n = 0; b.y_off = 67108864.f; a.width = b.width = e.width = 8;
        CALL(run_tracks(c, {a, b, e}, 3, 3, blocks));
        const size_t ob = 4 * block_words(3, 0);
        expect_block("units[0]", blocks.data(), 3, 3, {{3, 0, .5f, -.25f, 1.f, 1}, {5, 0, .5f, -.25f, 1.f, 0}});
        // (2^26 + 2 and 2^26 + 1 both round to 2^26 in float32: a tie, the rows keep their list order)
        expect_block("units[1]", blocks.data() + ob, 3, 2, {{7, 67108864.f, .5f, -.25f, 1.f, 0}, {7, 67108864.f, .5f, -.25f, 1.f, 1}});
        expect_block("units[2]", blocks.data() + 2 * ob, 3, 0, {});
        for (const track_unit *u : {&a, &b, &e}) {
            std::vector<char> alone;
            CALL(run_tracks(c, {*u}, 3, 3, alone));
            REQUIRE(alone.size() == ob && !memcmp(alone.data(), blocks.data() + ob * (size_t)(u == &a ? 0 : u == &b ? 1 : 2), ob), "a unit alone differs");
        }
    }
    {   // refused on the host: too many units, a negative width, a width beyond the ordering's
        track_unit u = unit_of({1}, {1}, {0}, {0});
        std::vector<track_unit> many(17, u);
        REQUIRE(run_tracks(c, many, 1, 1, blocks) == KM_E_ARG, "17 units");
        u.width = 65536;
        REQUIRE(run_tracks(c, {u}, 1, 1, blocks) == KM_E_ARG, "width 65536");
        u.width = -1;
        REQUIRE(run_tracks(c, {u}, 1, 1, blocks) == KM_E_ARG, "width -1");
    }
    printf("tracks 4 groups\n");
}

// `frame --tracks IN OUT`: every record of IN {int32 n_units, n_max, cap; per unit int32 n, int32 width, float32 x_off, y_off; then the
// units' p0, p1, p0r lists} through km_frame_from_tracks on ONE context; OUT gets {int32 status; the blocks if status == 0} per record
static int tracks_from_file(km_ctx *c, const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) { fprintf(stderr, "cannot open %s / %s\n", in_path, out_path); return 1; }
    int head[3], records = 0;
    while (fread(head, sizeof head, 1, in) == 1) {
        const int k = head[0], n_max = head[1], cap = head[2];
        if (k < 1 || k > 64 || n_max < 1 || cap < 1) { fprintf(stderr, "record %d: bad header\n", records); return 1; }
        std::vector<int> meta(4 * (size_t)k);
        std::vector<float> pts((size_t)3 * k * n_max * 2);
        if (fread(meta.data(), 16, (size_t)k, in) != (size_t)k || fread(pts.data(), 4, pts.size(), in) != pts.size()) { fprintf(stderr, "record %d: truncated\n", records); return 1; }
        std::vector<int> n((size_t)k), width((size_t)k);
        std::vector<float> xo((size_t)k), yo((size_t)k);
        for (int u = 0; u < k; u++) { n[u] = meta[4 * u]; width[u] = meta[4 * u + 1]; memcpy(&xo[u], &meta[4 * u + 2], 4); memcpy(&yo[u], &meta[4 * u + 3], 4); }
        const size_t list = (size_t)k * n_max * 2;
        std::vector<char> blocks((size_t)k * 4 * block_words(cap, 0), 0x5a);
        const int rc = km_frame_from_tracks(c, k, pts.data(), pts.data() + list, pts.data() + 2 * list, n.data(), xo.data(), yo.data(), width.data(), n_max, cap, blocks.data());
        fwrite(&rc, sizeof rc, 1, out);
        if (rc == KM_OK) fwrite(blocks.data(), 1, blocks.size(), out);
        records++;
    }
    fclose(in);
    if (fclose(out)) return 1;
    printf("tracks-file %d records\n", records);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "--tracks")) {
        km_ctx *c = nullptr;
        if (km_ctx_create(0, &c) != KM_OK) { fprintf(stderr, "km_ctx_create failed: %s\n", km_last_error(nullptr)); return 1; }
        const int rc = tracks_from_file(c, argv[2], argv[3]);
        REQUIRE(km_ctx_destroy(c) == KM_OK, "km_ctx_destroy");
        if (rc || g_failures) return 1;
        printf("FRAME-TRACKS OK\n");
        return 0;
    }
#ifndef FRAME_MAIN_ABI_ONLY
    check_layout();
    check_arena();
#endif
    km_ctx *c = nullptr;
    if (km_ctx_create(0, &c) != KM_OK) { fprintf(stderr, "km_ctx_create failed: %s\n", km_last_error(nullptr)); return 1; }
    check_search(c);
    check_tile_and_units(c);
    check_tracks(c);
    REQUIRE(km_ctx_destroy(c) == KM_OK, "km_ctx_destroy");
    const stub_state &s = stub();
    REQUIRE(s.streams == 0 && s.events == 0 && s.device_allocs == 0 && s.host_allocs == 0, "left behind %ld streams, %ld events, %ld device, %ld page-locked allocations", s.streams,
            s.events, s.device_allocs, s.host_allocs);
    if (g_failures) return 1;
    printf("FRAME-LAYOUT OK\n");
    return 0;
}
