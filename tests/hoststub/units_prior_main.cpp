// TEST INFRASTRUCTURE (tests/test_units_prior_host.py): km_klt_units_frame_prior_submit on the stand-in HIP layer, as a program of its own
// (no python, no preload) linked from the host objects of the sanitizer build.
//   1. every refusal, each followed by a clean km_ctx_sync and an empty frame ring;
//   2. prior, non-prior and prior submissions with "units_pipeline" on, the deferred tail flushed by km_frame_flush, by another entry
//      point and by km_ctx_sync;
//   1 and 2 run with the happens-before checker of stub_order.hpp ON and must leave no report.  What the checker sees: every stand-in
//   launcher's declared buffers - the lanes' LK tables (kl_units_prepare / kl_units_launch on WS_UNITS_LK), the tails enqueued by the
//   next submission of either kind, the Laplacian stand-in's read of U.user_mask == U.mask beside its write of U.mask, the copies and
//   events of the streams.  What it cannot see: the host form of the batched mask launcher writes U.mask with plain loops and declares
//   nothing, and the seeded prepare / launch are the unseeded stand-ins (same slot, same size: the seeds behind the table are not declared).
//   3. the host form of the batched mask launcher (csrc/k_prior.hpp) for two units with different origins and priors: the masks are
//      written to argv[1], the test compares them with the restatement's byte for byte.
// Prints 'UNITS-PRIOR OK' at the end.
#include "../../karios_amd/csrc/common.hpp"
#include "../../karios_amd/csrc/k_prior.hpp"
#include "stub_order.hpp"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int g_failures = 0;
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "units_prior_main.cpp:%d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); g_failures++; } } while (0)
#define OK(expr) do { const int rc_ = (expr); REQUIRE(rc_ == KM_OK, "%s -> %d (%s)", #expr, rc_, km_last_error(c)); } while (0)

enum { H = 64, W = 512, CAP = 64 };

// the rasters of the mask comparison (tests/test_units_prior_host.py builds the same ones): no-data zeros sprinkled over both
static uint16_t pixel(size_t i, unsigned mul, unsigned shift) { const unsigned v = (unsigned)((i * mul) >> shift) % 9000u; return (uint16_t)(v % 17u == 0 ? 0 : v); }

int main(int argc, char **argv)
{
    stub_order::enable(true);      // (in front of the first allocation: the checker tracks what it saw allocated)
    auto no_reports = [&](const char *where) {
        const auto &r = stub_order::reports();
        REQUIRE(r.empty(), "%s: %zu happens-before report(s), the first: %s", where, r.size(), r.empty() ? "" : r[0].text.c_str());
        stub_order::clear_log();
    };
    km_ctx *c = nullptr;
    if (km_ctx_create(0, &c) != KM_OK) { fprintf(stderr, "km_ctx_create failed: %s\n", km_last_error(nullptr)); return 1; }
    std::vector<uint16_t> ref((size_t)H * W), mon((size_t)H * W);
    for (size_t i = 0; i < ref.size(); i++) { ref[i] = pixel(i, 2654435761u, 20); mon[i] = pixel(i, 40503u, 7); }
    const size_t bytes = ref.size() * sizeof(uint16_t);
    void *dr = nullptr, *dm = nullptr;
    OK(km_dev_alloc(c, bytes, &dr));
    OK(km_dev_alloc(c, bytes, &dm));
    OK(km_h2d(c, dr, ref.data(), bytes));
    OK(km_h2d(c, dm, mon.data(), bytes));

    km_klt_params prm = {};
    prm.max_corners = CAP; prm.block_size = 15; prm.win_size = 21; prm.max_level = 1; prm.max_count = 30;
    prm.ksize_mon = prm.ksize_ref = 7; prm.quality_level = 0.1; prm.min_distance = 10.0; prm.epsilon = 0.03;
    km_unit units[2] = {};
    const int box[2][2] = {{0, H}, {8, H - 16}};      // {first row, rows}: 512 columns, the narrowest the batch form takes
    for (int u = 0; u < 2; u++) {
        units[u].d_ref = (const uint16_t *)dr + (size_t)box[u][0] * W; units[u].d_mon = (const uint16_t *)dm + (size_t)box[u][0] * W;
        units[u].sref = units[u].smon = units[u].sref_f = units[u].smon_f = W;
        units[u].d_ref_full = dr; units[u].d_mon_full = dm;
        units[u].H = box[u][1]; units[u].W = W; units[u].Hf = H; units[u].Wf = W; units[u].y_off = (float)box[u][0];
    }
    const double priors[18] = {1, 0, 3, 0, 1, -2, 0, 0, 1, 0.9999, -0.01, 5.5, 0.01, 0.9999, 1.25, 0, 0, 1};
    const double nodata = 0.0;
    int ticket = -5;
    const void *block = nullptr;
    size_t nb = 0;

    // ---- 1. refusals: nothing queued, the ticket untouched, the context synchronises cleanly
    auto refused = [&](int want, const char *needle, int rc) {
        REQUIRE(rc == want, "refusal: status %d, expected %d (%s)", rc, want, km_last_error(c));
        if (needle) REQUIRE(strstr(km_last_error(c), needle) != nullptr, "refusal: '%s' lacks '%s'", km_last_error(c), needle);
        REQUIRE(ticket == -5, "a refused call wrote the ticket");
        OK(km_ctx_sync(c));
    };
    refused(KM_E_ARG, "null priors", km_klt_units_frame_prior_submit(c, units, 2, KM_U16, &nodata, &nodata, &prm, 0.4, CAP, nullptr, &ticket));
    for (double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()}) {
        double p[18];
        memcpy(p, priors, sizeof p);
        p[9 + 3] = bad;
        refused(KM_E_ARG, "unit 1: prior[3]", km_klt_units_frame_prior_submit(c, units, 2, KM_U16, &nodata, &nodata, &prm, 0.4, CAP, p, &ticket));
    }
    OK(km_set_option(c, "frame_clip", 1));
    refused(KM_E_UNSUPPORTED, "frame_clip", km_klt_units_frame_prior_submit(c, units, 2, KM_U16, &nodata, &nodata, &prm, 0.4, CAP, priors, &ticket));
    OK(km_set_option(c, "frame_clip", 0));
    {
        km_unit w[2] = {units[0], units[1]};
        w[1].win_H = H; w[1].win_W = W;
        refused(KM_E_UNSUPPORTED, "unit 1", km_klt_units_frame_prior_submit(c, w, 2, KM_U16, &nodata, &nodata, &prm, 0.4, CAP, priors, &ticket));
        w[1] = units[1]; w[1].W = 256;               // what the unseeded batch refuses, without a text
        refused(KM_E_UNSUPPORTED, nullptr, km_klt_units_frame_prior_submit(c, w, 2, KM_U16, &nodata, &nodata, &prm, 0.4, CAP, priors, &ticket));
    }
    refused(KM_E_ARG, nullptr, km_klt_units_frame_prior_submit(c, units, 0, KM_U16, &nodata, &nodata, &prm, 0.4, CAP, priors, &ticket));
    refused(KM_E_ARG, nullptr, km_klt_units_frame_prior_submit(c, nullptr, 2, KM_U16, &nodata, &nodata, &prm, 0.4, CAP, priors, &ticket));

    no_reports("refusals");

    // ---- 2. unpipelined, then prior / plain / prior in the pipeline; three ways of flushing the deferred tail
    auto submit = [&](bool with_priors, int *t) {
        *t = -1;
        if (with_priors) OK(km_klt_units_frame_prior_submit(c, units, 2, KM_U16, &nodata, &nodata, &prm, 0.4, CAP, priors, t));
        else OK(km_klt_units_frame_submit(c, units, 2, KM_U16, &nodata, &nodata, &prm, 0.4, CAP, t));
    };
    auto wait = [&](int t) {
        if (t < 0) return;
        OK(km_frame_wait(c, t, &block, &nb));
        REQUIRE(block && nb > 0, "km_frame_wait handed out nothing");
    };
    int tk[3];
    submit(true, &tk[0]);
    wait(tk[0]);
    OK(km_set_option(c, "units_pipeline", 1));
    for (int round = 0; round < 3; round++) {
        submit(true, &tk[0]);
        submit(false, &tk[1]);                       // (enqueues the seeded tail of the first on the other lane's table)
        submit(true, &tk[2]);                        // (... and this one the plain tail of the second)
        if (round == 0) OK(km_frame_flush(c, tk[2]));
        else if (round == 1) {                       // another entry point flushes the deferred tail and joins the lanes
            double mm[2] = {0, 0};
            OK(km_minmax_dev(c, dr, KM_U16, H, W, W, mm));
        } else OK(km_ctx_sync(c));
        for (int k = 0; k < 3; k++) wait(tk[k]);
    }
    OK(km_set_option(c, "units_pipeline", 0));
    submit(false, &tk[0]);                           // (the unseeded form behind all that)
    wait(tk[0]);
    OK(km_ctx_sync(c));
    no_reports("prior / plain / prior submissions");
    REQUIRE(stub_order::on(), "the happens-before checker went off");
    {   // the control: the checker of THIS program does report - two writes of one buffer on two streams with no event between them
        hipStream_t s[2];
        char *buf = nullptr;
        (void)hipStreamCreateWithFlags(&s[0], hipStreamNonBlocking); (void)hipStreamCreateWithFlags(&s[1], hipStreamNonBlocking);
        (void)hipMalloc((void **)&buf, 256);
        (void)hipMemsetAsync(buf, 0, 256, s[0]); (void)hipMemsetAsync(buf, 1, 256, s[1]);
        REQUIRE(stub_order::reports().size() == 1, "control: %zu report(s) for two unordered writes, expected 1", stub_order::reports().size());
        stub_order::clear_log();
        (void)hipFree(buf); (void)hipStreamDestroy(s[0]); (void)hipStreamDestroy(s[1]);
    }

    // ---- 3. the host form of the batched mask launcher
    if (argc > 1) {
        kp_mask_units M;
        memset(&M, 0, sizeof M);
        M.n = 2;
        std::vector<uint8_t> masks((size_t)H * W + (size_t)(H - 16) * W, 0xee), base((size_t)H * W);
        for (size_t i = 0; i < base.size(); i++) base[i] = (uint8_t)((i * 7u) % 5u ? 3 : 0);
        size_t at = 0;
        for (int u = 0; u < 2; u++) {
            kp_mask_args &a = M.a[u];
            a.ref = units[u].d_ref; a.mon = units[u].d_mon; a.dtype = KM_U16; a.H = units[u].H; a.W = W; a.sref = a.smon = W;
            a.base = u == 1 ? base.data() + (size_t)box[u][0] * W : nullptr; a.sbase = W;
            a.has_nd_ref = a.has_nd_mon = 1; a.nd_ref = a.nd_mon = 0.0;
            memcpy(a.P, priors + 9 * u, sizeof a.P);
            a.x_off = u == 1 ? 100.0 : 0.0; a.y_off = (double)box[u][0];
            a.mask = masks.data() + at;
            at += (size_t)a.H * W;
        }
        OK(kp_prior_mask_units(c, M));
        FILE *f = fopen(argv[1], "wb");
        REQUIRE(f && fwrite(masks.data(), 1, masks.size(), f) == masks.size(), "cannot write %s", argv[1]);
        if (f) fclose(f);
    }

    OK(km_dev_free(c, dr));
    OK(km_dev_free(c, dm));
    km_ctx_destroy(c);
    if (g_failures) { fprintf(stderr, "%d failure(s)\n", g_failures); return 1; }
    puts("UNITS-PRIOR OK");
    return 0;
}
