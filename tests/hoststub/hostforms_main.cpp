// TEST INFRASTRUCTURE (tests/test_host_forms_host.py): the host form of an entry point computes what its _dev form computes.  A program of
// its own (no python, no preload) linked from the host objects of the sanitizer build and the stand-in HIP layer, where device memory is host
// memory: every host form that places caller columns in a workspace slot (upload_columns, csrc/api.hip) - and the profile and box forms, which
// place theirs inside a larger block - is called beside its _dev form on the same data, and the outputs are compared byte for byte.  The
// sanitizers check the copies.  Shapes are the smallest at which a column's pitch or a null column can go wrong: n in {0, 1, 3, 65}, rasters
// seen as windows of wider buffers.  The score launchers of the stand-in write a function of their four columns, km_dn_keep_dev (host columns,
// no twin) is held to its return code on a raster whose x range is no y range.  Uses the public C ABI only.  Prints 'HOST-FORMS OK' at the end.
#include "../../karios_amd/csrc/common.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static int g_failures = 0;
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "hostforms_main.cpp:%d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); g_failures++; } } while (0)
#define CALL(expr) do { const int rc_ = (expr); REQUIRE(rc_ == KM_OK, "%s -> %d (%s)", #expr, rc_, km_last_error(c)); } while (0)

static const int ROWS[4] = {0, 1, 3, 65};

static unsigned g_seed = 12345u;
static unsigned next_u32() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(next_u32() & 0xffff) / 65536.f; }
static std::vector<float> column(int n, float lo, float hi)
{
    std::vector<float> v((size_t)n);
    for (float &x : v) x = uniform(lo, hi);
    return v;
}
template <typename T> static std::vector<T> pixels(size_t count, unsigned span)
{
    std::vector<T> v(count);
    for (T &x : v) x = (T)(next_u32() % span);
    return v;
}

// device memory of the caller (km_dev_alloc), filled from host memory; `back` reads all of it
struct dev_buf {
    km_ctx *c;
    void *p = nullptr;
    size_t bytes;
    dev_buf(km_ctx *ctx, const void *src, size_t n) : c(ctx), bytes(n)
    {
        if (km_dev_alloc(c, n ? n : 1, &p) != KM_OK) p = nullptr;
        REQUIRE(p && (!n || km_h2d(c, p, src, n) == KM_OK), "device buffer of %zu bytes", n);
    }
    template <typename T> dev_buf(km_ctx *ctx, const std::vector<T> &v) : dev_buf(ctx, v.data(), v.size() * sizeof(T)) {}
    ~dev_buf() { if (p) (void)km_dev_free(c, p); }
    dev_buf(const dev_buf &) = delete;
    template <typename T> T *as() const { return (T *)p; }
    std::vector<char> back() const
    {
        std::vector<char> h(bytes);
        REQUIRE(!bytes || km_d2h(c, h.data(), p, bytes) == KM_OK, "read-back of %zu bytes", bytes);
        return h;
    }
};
// (memcmp takes no null pointer, not even for no bytes)
static bool same(const void *a, const void *b, size_t bytes) { return !bytes || !memcmp(a, b, bytes); }
template <typename T> static bool same_bytes(const std::vector<T> &host, const dev_buf &d)
{
    const std::vector<char> b = d.back();
    return host.size() * sizeof(T) == b.size() && same(host.data(), b.data(), b.size());
}
// (the host forms take neither a column nor an output for n == 0)
template <typename T> static const T *or_null(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
template <typename T> static T *or_null(std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

// ---- ZNCC, MI (the stand-in launchers write a function of the four columns) and the DN filter
static void check_scores(km_ctx *c)
{
    const int H = 40, W = 80, stride = 96;
    const std::vector<uint16_t> ref = pixels<uint16_t>((size_t)H * stride, 9000), mon = pixels<uint16_t>((size_t)H * stride, 9000);
    const dev_buf d_ref(c, ref), d_mon(c, mon);
    for (int n : ROWS) {
        const std::vector<float> x0 = column(n, 40.f, 80.f), y0 = column(n, 0.f, 40.f), dx = column(n, -2.f, 2.f), dy = column(n, -2.f, 2.f);
        const dev_buf d_x0(c, x0), d_y0(c, y0), d_dx(c, dx), d_dy(c, dy);
        const std::vector<double> fill((size_t)n, -7.0);
        {
            std::vector<double> out = fill;
            const dev_buf d_out(c, fill);
            CALL(km_zncc_batch(c, ref.data(), mon.data(), KM_U16, H, W, H, W, stride, stride, or_null(x0), or_null(y0), or_null(dx), or_null(dy), n, or_null(out)));
            CALL(km_zncc_batch_dev(c, d_ref.p, d_mon.p, KM_U16, H, W, H, W, stride, stride, d_x0.as<float>(), d_y0.as<float>(), d_dx.as<float>(), d_dy.as<float>(), n,
                                   d_out.as<double>()));
            REQUIRE(same_bytes(out, d_out), "zncc, %d rows: the host form differs from the device form", n);
        }
        for (int which = 1; which <= 3; which++) {      // the total score alone, the normalised one alone, both
            std::vector<double> st = fill, nmi = fill;
            const dev_buf d_st(c, fill), d_nmi(c, fill);
            CALL(km_mi_batch(c, ref.data(), mon.data(), KM_U16, H, W, H, W, stride, stride, or_null(x0), or_null(y0), or_null(dx), or_null(dy), n,
                             which & 1 ? st.data() : nullptr, which & 2 ? nmi.data() : nullptr));
            CALL(km_mi_batch_dev(c, d_ref.p, d_mon.p, KM_U16, H, W, H, W, stride, stride, d_x0.as<float>(), d_y0.as<float>(), d_dx.as<float>(), d_dy.as<float>(), n,
                                 which & 1 ? d_st.as<double>() : nullptr, which & 2 ? d_nmi.as<double>() : nullptr));
            REQUIRE(same_bytes(st, d_st) && same_bytes(nmi, d_nmi), "mi, %d rows, outputs %d: the host form differs from the device form", n, which);
        }
        // every x0 is a column but no row of the 40-row raster: a y column read at the wrong pitch is refused
        const double no_values[2] = {0.0, 65535.0};
        std::vector<uint8_t> keep((size_t)n, 9);
        CALL(km_dn_keep_dev(c, d_ref.p, d_mon.p, KM_U16, H, W, stride, stride, or_null(x0), or_null(y0), n, no_values, 2, nullptr, nullptr, or_null(keep)));
        for (int i = 0; i < n; i++) REQUIRE(keep[i] <= 1, "dn_keep, %d rows: keep[%d] = %d", n, i, keep[i]);
    }
    printf("scores: zncc, mi, dn_keep\n");
}

// ---- analyze_accuracy's statistics
static void check_accuracy(km_ctx *c)
{
    const double percents[2] = {0.9, 0.95};
    for (int n : ROWS)
        for (int n_percent : {0, 2}) {
            const std::vector<float> dx = column(n, -3.f, 3.f), dy = column(n, -3.f, 3.f), score = column(n, 0.f, 1.f);
            const dev_buf d_dx(c, dx), d_dy(c, dy), d_score(c, score);
            km_accuracy_result a, b;
            memset(&a, 0x5a, sizeof a); memset(&b, 0x5a, sizeof b);
            CALL(km_accuracy_stats(c, or_null(dx), or_null(dy), or_null(score), n, 0.25, 1, 10.0, n_percent, n_percent ? percents : nullptr, &a));
            CALL(km_accuracy_stats_dev(c, d_dx.as<float>(), d_dy.as<float>(), d_score.as<float>(), n, 0.25, 1, 10.0, n_percent, n_percent ? percents : nullptr, &b));
            REQUIRE(a.sample == b.sample && a.n_nan == b.n_nan && same(a.stats, b.stats, sizeof a.stats) && same(a.order, b.order, (size_t)n_percent * 2 * sizeof(float)),
                    "accuracy_stats, %d rows, %d percents: the host form differs from the device form", n, n_percent);
            REQUIRE(a.sample <= n && (n < 65 || a.sample > 0), "accuracy_stats, %d rows: a sample of %lld", n, (long long)a.sample);
        }
    printf("accuracy: statistics\n");
}

// ---- key-point chips: the selection, the chips of 57 x 57 rasters seen as windows of 57 x 60 buffers
static void check_chips(km_ctx *c)
{
    const int rows = 2, cols = 3, cap = rows * cols * KM_CHIP_PICKS;
    for (int n : ROWS) {
        const std::vector<float> x0 = column(n, 0.f, 200.f), y0 = column(n, 0.f, 100.f), score = column(n, 0.f, 1.f);
        const dev_buf d_x0(c, x0), d_y0(c, y0), d_score(c, score);
        const std::vector<int32_t> fill((size_t)cap, -1);
        std::vector<int32_t> index = fill;
        const dev_buf d_index(c, fill);
        int32_t count = -1, d_count = -1;
        CALL(km_chip_select(c, or_null(x0), or_null(y0), or_null(score), n, 200, 100, 0.3, 0, rows, cols, index.data(), &count));
        CALL(km_chip_select_dev(c, d_x0.as<float>(), d_y0.as<float>(), d_score.as<float>(), n, 200, 100, 0.3, 0, rows, cols, d_index.as<int32_t>(), &d_count));
        const std::vector<char> got = d_index.back();
        REQUIRE(count == d_count && count >= 0 && count <= cap && count <= n && (n < 65 || count > 0) && same(index.data(), got.data(), (size_t)count * sizeof(int32_t)),
                "chip_select, %d rows: %d and %d picks, or other picks", n, count, d_count);
    }
    const int S = KM_CHIP_SIZE, stride = 60;
    const std::vector<uint16_t> ref = pixels<uint16_t>((size_t)S * stride, 60000), mon = pixels<uint16_t>((size_t)S * stride, 60000);
    const dev_buf d_ref(c, ref), d_mon(c, mon);
    for (int n : ROWS)
        for (int lap = 0; lap < 2; lap++) {
            const int kref = lap ? 3 : 0, kmon = lap ? 5 : 0;
            // the one window a 57 x 57 raster holds has its centre at (28, 28): about half the rows are ok, the rest zero
            const std::vector<float> x0 = column(n, 27.5f, 29.5f), y0 = column(n, 28.f, 29.f), dx = column(n, -0.4f, 0.4f), dy = column(n, -0.4f, 0.4f);
            const dev_buf d_x0(c, x0), d_y0(c, y0), d_dx(c, dx), d_dy(c, dy);
            const size_t px = (size_t)n * S * S;
            const std::vector<uint16_t> raw_fill(px, 0x5a5a);
            const std::vector<uint8_t> u8_fill(px, 0x5a), ok_fill((size_t)n, 0x5a);
            const std::vector<int32_t> win_fill((size_t)n * 4, -1);
            std::vector<uint16_t> ref_raw = raw_fill, mon_raw = raw_fill;
            std::vector<uint8_t> ref_u8 = u8_fill, mon_u8 = u8_fill, ref_lap = u8_fill, mon_lap = u8_fill, ok = ok_fill;
            std::vector<int32_t> windows = win_fill;
            const dev_buf d_ref_raw(c, raw_fill), d_mon_raw(c, raw_fill), d_ref_u8(c, u8_fill), d_mon_u8(c, u8_fill), d_ref_lap(c, u8_fill), d_mon_lap(c, u8_fill),
                d_ok(c, ok_fill), d_windows(c, win_fill);
            const km_chip_outputs out = {or_null(ref_raw), or_null(mon_raw), or_null(ref_u8), or_null(mon_u8), lap ? or_null(ref_lap) : nullptr,
                                         lap ? or_null(mon_lap) : nullptr, or_null(ok), or_null(windows)};
            const km_chip_outputs d_out = {d_ref_raw.p, d_mon_raw.p, d_ref_u8.as<uint8_t>(), d_mon_u8.as<uint8_t>(), lap ? d_ref_lap.as<uint8_t>() : nullptr,
                                           lap ? d_mon_lap.as<uint8_t>() : nullptr, d_ok.as<uint8_t>(), d_windows.as<int32_t>()};
            CALL(km_chips(c, ref.data(), mon.data(), KM_U16, S, S, S, S, stride, stride, or_null(x0), or_null(y0), or_null(dx), or_null(dy), n, kref, kmon, &out));
            CALL(km_chips_dev(c, d_ref.p, d_mon.p, KM_U16, S, S, S, S, stride, stride, d_x0.as<float>(), d_y0.as<float>(), d_dx.as<float>(), d_dy.as<float>(), n, kref, kmon,
                              &d_out));
            REQUIRE(same_bytes(ref_raw, d_ref_raw) && same_bytes(mon_raw, d_mon_raw) && same_bytes(ref_u8, d_ref_u8) && same_bytes(mon_u8, d_mon_u8) &&
                        same_bytes(ref_lap, d_ref_lap) && same_bytes(mon_lap, d_mon_lap) && same_bytes(ok, d_ok) && same_bytes(windows, d_windows),
                    "chips, %d rows, Laplacian %d / %d: the host form differs from the device form", n, kref, kmon);
            int n_ok = 0;
            for (int i = 0; i < n; i++) n_ok += ok[i] == 1;
            REQUIRE(n < 65 || (n_ok > 0 && n_ok < n), "chips, %d rows: %d ok", n, n_ok);
            REQUIRE(lap || ref_lap == u8_fill, "chips, %d rows: a Laplacian nobody asked for", n);
        }
    printf("chips: selection, extraction\n");
}

// ---- mean profiles and box statistics (their columns lie inside a larger block)
static void check_profiles_and_boxes(km_ctx *c)
{
    for (int n : ROWS) {
        const std::vector<float> v0 = column(n, -4.f, 4.f), p0 = column(n, -80.f, 220.f), v1 = column(n, 0.f, 9.f), p1 = column(n, 0.f, 1000.f);
        const dev_buf d_v0(c, v0), d_p0(c, p0), d_v1(c, v1), d_p1(c, p1);
        const std::vector<uint32_t> fill((size_t)n, 0x5a5a5a5au);
        std::vector<uint32_t> h[2][5];
        std::vector<dev_buf *> d;
        km_profile prof[2] = {}, d_prof[2] = {};
        for (int k = 0; k < 2; k++) {
            for (int j = 0; j < 5; j++) { h[k][j] = fill; d.push_back(new dev_buf(c, fill)); }
            void *o[5], *dv[5];
            for (int j = 0; j < 5; j++) { o[j] = or_null(h[k][j]); dv[j] = d[(size_t)k * 5 + j]->p; }
            prof[k].values = or_null(k ? v1 : v0); prof[k].positions = or_null(k ? p1 : p0); prof[k].bin_size = k ? 1 : 20;
            prof[k].key = (float *)o[0]; prof[k].position = (int32_t *)o[1]; prof[k].count = (int32_t *)o[2]; prof[k].mean = (float *)o[3]; prof[k].std = (float *)o[4];
            d_prof[k].values = (k ? d_v1 : d_v0).as<float>(); d_prof[k].positions = (k ? d_p1 : d_p0).as<float>(); d_prof[k].bin_size = prof[k].bin_size;
            d_prof[k].key = (float *)dv[0]; d_prof[k].position = (int32_t *)dv[1]; d_prof[k].count = (int32_t *)dv[2]; d_prof[k].mean = (float *)dv[3]; d_prof[k].std = (float *)dv[4];
        }
        int32_t groups[2] = {-1, -1}, oor[2] = {-1, -1}, d_groups[2] = {-1, -1}, d_oor[2] = {-1, -1};
        CALL(km_mean_profiles(c, n, 2, prof, groups, oor));
        CALL(km_mean_profiles_dev(c, n, 2, d_prof, d_groups, d_oor));
        for (int k = 0; k < 2; k++) {
            REQUIRE(groups[k] == d_groups[k] && oor[k] == d_oor[k] && groups[k] >= 0 && groups[k] <= n && (n == 0 || groups[k] > 0), "mean_profiles, %d rows: %d and %d groups of profile %d",
                    n, groups[k], d_groups[k], k);
            for (int j = 0; j < 5 && groups[k] == d_groups[k]; j++) {
                const std::vector<char> got = d[(size_t)k * 5 + j]->back();
                REQUIRE(same(h[k][j].data(), got.data(), (size_t)groups[k] * sizeof(uint32_t)), "mean_profiles, %d rows: output %d of profile %d", n, j, k);
            }
        }
        for (dev_buf *b : d) delete b;

        std::vector<float> key((size_t)n, -7.f), mean((size_t)n, -7.f);
        std::vector<int32_t> count((size_t)n, -1);
        std::vector<double> stats((size_t)n * KM_BOX_STATS, -7.0);
        std::vector<int8_t> cls((size_t)n, 9);
        const dev_buf d_key(c, key), d_mean(c, mean), d_count(c, count), d_stats(c, stats), d_cls(c, cls);
        int32_t g = -1, d_g = -1;
        CALL(km_box_stats(c, n, or_null(v0), or_null(p0), 20, or_null(key), or_null(count), or_null(mean), or_null(stats), or_null(cls), &g));
        CALL(km_box_stats_dev(c, n, d_v0.as<float>(), d_p0.as<float>(), 20, d_key.as<float>(), d_count.as<int32_t>(), d_mean.as<float>(), d_stats.as<double>(),
                              d_cls.as<int8_t>(), &d_g));
        REQUIRE(g == d_g && g == groups[0], "box_stats, %d rows: %d and %d groups (%d in the profile)", n, g, d_g, groups[0]);
        if (g == d_g && n > 0) {
            const std::vector<char> bk = d_key.back(), bc = d_count.back(), bm = d_mean.back(), bs = d_stats.back();
            bool eq = same(key.data(), bk.data(), (size_t)g * 4) && same(count.data(), bc.data(), (size_t)g * 4) && same(mean.data(), bm.data(), (size_t)g * 4) &&
                      same_bytes(cls, d_cls);
            for (int s = 0; s < KM_BOX_STATS; s++) eq = eq && same(stats.data() + (size_t)s * n, bs.data() + (size_t)s * n * sizeof(double), (size_t)g * sizeof(double));
            REQUIRE(eq, "box_stats, %d rows: the host form differs from the device form", n);
        }
    }
    printf("report: mean profiles, box statistics\n");
}

// ---- the report's products: point rasters on 5 x 7 in windows of wider buffers, samples of every pixel type
template <typename T> static void check_samples_of(km_ctx *c, int dtype, const char *name)
{
    const int H = 5, W = 7, stride = 10;
    const std::vector<T> raster = pixels<T>((size_t)H * stride, 200);
    const dev_buf d_raster(c, raster);
    for (int n : ROWS) {
        const std::vector<float> x0 = column(n, -7.5f, 7.5f), y0 = column(n, -5.5f, 5.5f);
        const dev_buf d_x0(c, x0), d_y0(c, y0);
        const std::vector<T> fill((size_t)n, (T)90);
        std::vector<T> out = fill;
        const dev_buf d_out(c, fill);
        int32_t bad = -1, d_bad = -1;
        CALL(km_sample_points(c, raster.data(), dtype, H, W, stride, n, or_null(x0), or_null(y0), or_null(out), &bad));
        CALL(km_sample_points_dev(c, d_raster.p, dtype, H, W, stride, n, d_x0.as<float>(), d_y0.as<float>(), d_out.p, &d_bad));
        REQUIRE(bad == d_bad && bad >= 0 && bad <= n && (n < 65 || (bad > 0 && bad < n)) && same_bytes(out, d_out), "sample_points of %s, %d rows: %d and %d rows out of range, or other samples",
                name, n, bad, d_bad);
    }
}

static void check_products(km_ctx *c)
{
    const int H = 5, W = 7;
    for (int n : ROWS)
        for (int ms : {7, 10})
            for (int rs : {7, 10})
                for (int form = 1; form <= 3; form++) {      // the mask alone (no dx, no dy), the delta raster alone, both
                    const bool with_mask = form & 1, with_delta = form & 2;
                    const ptrdiff_t band = (ptrdiff_t)H * rs + 3;
                    const std::vector<float> x0 = column(n, -7.5f, 7.5f), y0 = column(n, -0.5f, 5.5f), dx = column(n, -2.f, 2.f), dy = column(n, -2.f, 2.f);
                    const dev_buf d_x0(c, x0), d_y0(c, y0), d_dx(c, dx), d_dy(c, dy);
                    std::vector<uint8_t> mask((size_t)H * ms, 0xab);
                    std::vector<float> delta((size_t)2 * band, -7.f);
                    const dev_buf d_mask(c, mask), d_delta(c, delta);
                    int32_t bad = -1, d_bad = -1;
                    CALL(km_point_rasters(c, n, or_null(x0), or_null(y0), with_delta ? or_null(dx) : nullptr, with_delta ? or_null(dy) : nullptr, H, W, with_mask ? mask.data() : nullptr,
                                          ms, with_delta ? delta.data() : nullptr, band, rs, &bad));
                    CALL(km_point_rasters_dev(c, n, d_x0.as<float>(), d_y0.as<float>(), with_delta ? d_dx.as<float>() : nullptr, with_delta ? d_dy.as<float>() : nullptr, H, W,
                                              with_mask ? d_mask.as<uint8_t>() : nullptr, ms, with_delta ? d_delta.as<float>() : nullptr, band, rs, &d_bad));
                    // the whole buffers: what lies outside the 5 x 7 windows stays as it was in both forms
                    REQUIRE(bad == d_bad && bad >= 0 && bad <= n && (n < 65 || (bad > 0 && bad < n)) && same_bytes(mask, d_mask) && same_bytes(delta, d_delta),
                            "point_rasters, %d rows, strides %d / %d, form %d: %d and %d rows out of range, or other rasters", n, ms, rs, form, bad, d_bad);
                    REQUIRE(with_mask == (mask[0] != 0xab) && with_delta == (delta[0] != -7.f) && (ms == W || mask[W] == 0xab) && delta[(size_t)H * rs] == -7.f,
                            "point_rasters, %d rows, strides %d / %d, form %d: a raster nobody asked for, or a write outside the window", n, ms, rs, form);
                }
    check_samples_of<uint8_t>(c, KM_U8, "uint8");
    check_samples_of<uint16_t>(c, KM_U16, "uint16");
    check_samples_of<int16_t>(c, KM_I16, "int16");
    check_samples_of<float>(c, KM_F32, "float32");
    printf("products: point rasters, samples\n");
}

int main()
{
    km_ctx *c = nullptr;
    if (km_ctx_create(0, &c) != KM_OK) { fprintf(stderr, "km_ctx_create failed: %s\n", km_last_error(nullptr)); return 1; }
    check_scores(c);
    check_accuracy(c);
    check_chips(c);
    check_profiles_and_boxes(c);
    check_products(c);
    REQUIRE(km_ctx_destroy(c) == KM_OK, "km_ctx_destroy");
    const stub_state &s = stub();
    REQUIRE(s.streams == 0 && s.events == 0 && s.device_allocs == 0 && s.host_allocs == 0, "left behind %ld streams, %ld events, %ld device, %ld page-locked allocations", s.streams,
            s.events, s.device_allocs, s.host_allocs);
    if (g_failures) return 1;
    printf("HOST-FORMS OK\n");
    return 0;
}
