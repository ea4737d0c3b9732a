// TEST INFRASTRUCTURE (tests/test_stream_order_host.py): stream order.  The library decides with record / wait statements which kernel may
// read which buffer; the stand-in HIP layer executes everything at once, so a missing wait changes nothing there - unless the layer keeps
// vector clocks (stub_order.hpp).  A program of its own (no python, no preload) linked from the host objects of the sanitizer build, the only
// one that switches the checker on:
//   a. the model's own controls, through the stand-in API alone;
//   b. scenarios through the C ABI, each on a fresh context: zero reports;
//   c. a sweep over every hipStreamWaitEvent the scenarios issue: with that one wait ignored the scenario must produce a report, or the wait
//      is listed in kCovered below with what covers it.  A listed wait that IS reported fails too: the table cannot go stale.
// Prints 'STREAM-ORDER OK' at the end.
#include "../../karios_amd/csrc/common.hpp"

#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace so = stub_order;

static int g_failures = 0;
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "order_main.cpp:%d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); g_failures++; } } while (0)

// ------------------------------------------------------------------ names: streams and events by their km_ctx member, buffers by slot and lane
static km_ctx *g_ctx = nullptr;
static const char *const kLaneEvent[KM_LANE_EVENTS] = {"EV_MM", "EV_FORK", "EV_JOIN", "EV_E_DONE", "EV_C_DONE", "EV_K_DONE", "EV_F_DONE", "EV_SETUP"};   // (api_units.hip)
struct ctx_names : so::namer {
    std::string stream(const void *s) override
    {
        const km_ctx *c = g_ctx;
        if (!c) return "";
        if (s == c->main_stream.h) return "main_stream";
        if (s == c->copy_stream.h) return "copy_stream";
        if (s == c->aux_stream.h) return "aux_stream";
        if (s == c->d2h_stream.h) return "d2h_stream";
        if (s == c->chain_stream.h) return "chain_stream";
        return "";
    }
    std::string event(const void *e) override
    {
        const km_ctx *c = g_ctx;
        if (!c) return "";
#define EV(member) if (e == c->member.h) return #member
        EV(ev_copy); EV(ev_tail); EV(ev_lk_start); EV(ev_mm); EV(ev_fork); EV(ev_join); EV(ev_readback); EV(ev_units_start); EV(land_ev[0]); EV(land_ev[1]);
#undef EV
        for (int l = 0; l < 2; l++)
            for (int i = 0; i < KM_LANE_EVENTS; i++)
                if (e == c->ev_lane[l][i].h) return "ev_lane[" + std::to_string(l) + "][" + kLaneEvent[i] + "]";
        for (int k = 0; k < KM_FRAME_SLOTS; k++) {
            if (e == c->fslot[k].done.h) return "fslot[" + std::to_string(k) + "].done";
            if (e == c->fslot[k].sunk.h) return "fslot[" + std::to_string(k) + "].sunk";
        }
        for (int k = 0; k < KM_RING_SLOTS; k++) if (e == c->ring.slot[k].done.h) return "ring.slot[" + std::to_string(k) + "].done";
        for (const km_event_h &m : c->upload_marks) if (e == m.h) return "upload_marks[]";
        for (const km_event_h &m : c->free_marks) if (e == m.h) return "upload_marks[]";
        return "";
    }
    std::string buffer(const void *base) override
    {
        const km_ctx *c = g_ctx;
        if (!c) return "";
        static const std::map<int, const char *> known = {{WS_U8_A, "WS_U8_A"}, {WS_U8_B, "WS_U8_B"}, {WS_MASK, "WS_MASK"}, {WS_PYR_A, "WS_PYR_A"}, {WS_PYR_B, "WS_PYR_B"},
            {WS_KEYS0, "WS_KEYS0"}, {WS_MM_PARTIAL, "WS_MM_PARTIAL"}, {WS_MM_EARLY, "WS_MM_EARLY"}, {WS_GRID, "WS_GRID"}, {WS_PTS0, "WS_PTS0"}, {WS_PTS1, "WS_PTS1"},
            {WS_PTS2, "WS_PTS2"}, {WS_SCALARS, "WS_SCALARS"}, {WS_PARTIAL, "WS_PARTIAL"}, {WS_MISC0, "WS_MISC0"}, {WS_MISC1, "WS_MISC1"}, {WS_MISC2, "WS_MISC2"},
            {WS_MISC3, "WS_MISC3"}, {WS_FRAME, "WS_FRAME"}, {WS_MI_TABLE, "WS_MI_TABLE"}, {WS_LAP_VALID, "WS_LAP_VALID"}, {WS_FRAME_CNT, "WS_FRAME_CNT"},
            {WS_UNITS_LK, "WS_UNITS_LK"}, {WS_UNITS_MM, "WS_UNITS_MM"}, {WS_CL_COLS, "WS_CL_COLS"}};
        for (int lane = 0; lane < 2; lane++)
            for (int i = 0; i < WS_COUNT; i++)
                if (base == (lane ? c->ws_b[i].p : c->ws[i].p)) {
                    const auto it = known.find(i);
                    return "workspace slot " + std::to_string(i) + (it != known.end() ? std::string(" (") + it->second + ")" : std::string()) + " of lane " + std::to_string(lane);
                }
        for (const km_dev_mem &m : c->retired) if (base == m.p) return "a retired workspace buffer";
        return "";
    }
};

// ------------------------------------------------------------------ a. the model's own controls
struct control_fixture {
    hipStream_t s[2];
    hipEvent_t e;
    char *buf = nullptr, *host = nullptr;
    control_fixture()
    {
        (void)hipStreamCreateWithFlags(&s[0], hipStreamNonBlocking); (void)hipStreamCreateWithFlags(&s[1], hipStreamNonBlocking);
        (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
        (void)hipMalloc((void **)&buf, 4096);
        (void)hipHostMalloc((void **)&host, 4096, hipHostMallocDefault);
        so::clear_log();
    }
    ~control_fixture() { (void)hipFree(buf); (void)hipHostFree(host); (void)hipEventDestroy(e); (void)hipStreamDestroy(s[0]); (void)hipStreamDestroy(s[1]); }
};
static void expect_reports(const char *name, size_t want)
{
    const size_t got = so::reports().size();
    REQUIRE(got == want, "control '%s': %zu report(s), expected %zu%s%s", name, got, want, got ? ": " : "", got ? so::reports()[0].text.c_str() : "");
    printf("control %-58s %zu report(s)\n", name, got);
}
static void controls()
{
    { control_fixture f; (void)hipMemsetAsync(f.buf, 0, 256, f.s[0]); (void)hipMemsetAsync(f.buf, 1, 256, f.s[1]); expect_reports("two memsets, two streams, no event", 1); }
    {
        control_fixture f;
        (void)hipMemsetAsync(f.buf, 0, 256, f.s[0]); (void)hipEventRecord(f.e, f.s[0]); (void)hipStreamWaitEvent(f.s[1], f.e, 0); (void)hipMemsetAsync(f.buf, 1, 256, f.s[1]);
        expect_reports("the same with record + wait", 0);
    }
    {
        control_fixture f;
        (void)hipEventRecord(f.e, f.s[0]); (void)hipMemsetAsync(f.buf, 0, 256, f.s[0]); (void)hipStreamWaitEvent(f.s[1], f.e, 0); (void)hipMemsetAsync(f.buf, 1, 256, f.s[1]);
        expect_reports("a wait on an event recorded BEFORE the write", 1);
    }
    {
        control_fixture f;
        (void)hipStreamWaitEvent(f.s[1], f.e, 0); (void)hipMemsetAsync(f.buf, 0, 256, f.s[0]); (void)hipMemsetAsync(f.buf, 1, 256, f.s[1]);
        expect_reports("a wait on a never-recorded event orders nothing", 1);
    }
    { control_fixture f; (void)hipMemsetAsync(f.buf, 0, 256, f.s[0]); (void)hipStreamSynchronize(f.s[0]); (void)hipMemsetAsync(f.buf, 1, 256, f.s[1]); expect_reports("write, hipStreamSynchronize, another stream", 0); }
    {
        control_fixture f;
        (void)hipMemsetAsync(f.buf, 0, 256, f.s[0]); (void)hipEventRecord(f.e, f.s[0]); (void)hipEventSynchronize(f.e); (void)hipMemsetAsync(f.buf, 1, 256, f.s[1]);
        expect_reports("write, record, hipEventSynchronize, another stream", 0);
    }
    { control_fixture f; (void)hipMemsetAsync(f.buf, 0, 256, f.s[0]); (void)hipMemsetAsync(f.buf + 256, 1, 256, f.s[1]); expect_reports("disjoint byte ranges of one allocation", 0); }
    { control_fixture f; (void)hipMemsetAsync(f.buf, 0, 256, f.s[0]); (void)hipMemsetAsync(f.buf + 255, 1, 16, f.s[1]); expect_reports("ranges that share one byte", 1); }
    {
        control_fixture f;
        (void)hipMemcpyAsync(f.host, f.buf, 256, hipMemcpyDeviceToHost, f.s[0]); (void)hipMemcpyAsync(f.host + 256, f.buf, 256, hipMemcpyDeviceToHost, f.s[1]);
        expect_reports("read / read", 0);
    }
    {
        control_fixture f;
        (void)hipMemcpyAsync(f.host, f.buf, 256, hipMemcpyDeviceToHost, f.s[0]); (void)hipMemsetAsync(f.buf, 1, 256, f.s[1]);
        expect_reports("read, then an unordered write", 1);
    }
    {
        control_fixture f;
        { const so::op a(f.s[0], "accumulate A"); a.accum(f.buf, 8); }
        { const so::op b(f.s[1], "accumulate B"); b.accum(f.buf, 8); }
        expect_reports("accumulate / accumulate", 0);
    }
    {
        control_fixture f;
        { const so::op a(f.s[0], "accumulate A"); a.accum(f.buf, 8); }
        (void)hipMemcpyAsync(f.host, f.buf, 8, hipMemcpyDeviceToHost, f.s[1]);
        expect_reports("accumulate / read", 1);
    }
    {
        control_fixture f;
        (void)hipMemsetAsync(f.buf, 0, 8, f.s[0]);
        { const so::op a(f.s[1], "accumulate A"); a.accum(f.buf, 8); }
        expect_reports("write / accumulate", 1);
    }
    {
        control_fixture f;
        // (the sanitizer's allocator keeps a freed block in quarantine and would never hand the address out again: the two hooks hipFree and
        // hipMalloc call, on one address)
        char *p = nullptr;
        (void)hipMalloc((void **)&p, 512);
        (void)hipMemsetAsync(p, 0, 512, f.s[0]);
        so::on_free(p);
        so::on_malloc(p, 512);
        (void)hipMemsetAsync(p, 1, 512, f.s[1]);
        (void)hipFree(p);
        expect_reports("free and re-allocation at the same address", 0);
    }
    {
        control_fixture f;
        (void)hipMemsetAsync(f.buf, 0, 256, f.s[0]); (void)hipMemcpy(f.host, f.buf, 256, hipMemcpyDeviceToHost);
        expect_reports("blocking hipMemcpy of what a non-blocking stream wrote", 1);
    }
    {
        control_fixture f;
        (void)hipMemcpy(f.buf, f.host, 256, hipMemcpyHostToDevice); (void)hipMemcpyAsync(f.host, f.buf, 256, hipMemcpyDeviceToHost, f.s[0]);
        expect_reports("blocking hipMemcpy, then a stream reads it", 0);
    }
    {
        control_fixture f;
        (void)hipMemcpy2DAsync(f.buf, 64, f.host, 64, 16, 8, hipMemcpyHostToDevice, f.s[0]); (void)hipMemcpy2DAsync(f.buf + 16, 64, f.host, 64, 16, 8, hipMemcpyHostToDevice, f.s[1]);
        expect_reports("two strided boxes side by side", 0);
    }
    {
        control_fixture f;
        so::ignore_wait_after(0);
        (void)hipMemsetAsync(f.buf, 0, 256, f.s[0]); (void)hipEventRecord(f.e, f.s[0]); (void)hipStreamWaitEvent(f.s[1], f.e, 0); (void)hipMemsetAsync(f.buf, 1, 256, f.s[1]);
        so::ignore_wait_after(-1);
        expect_reports("record + wait with the wait ignored (the sweep's knob)", 1);
    }
}

// ------------------------------------------------------------------ b. scenarios through the C ABI
enum { H = 64, W = 512, CAP = 64 };      // 64 x 512: the narrowest unit the batched form takes
#define CALL(expr) do { const int rc_ = (expr); REQUIRE(rc_ == KM_OK, "%s -> %d (%s)", #expr, rc_, km_last_error(c)); } while (0)

struct dev_buf {
    km_ctx *c;
    void *p = nullptr;
    dev_buf(km_ctx *ctx, size_t bytes) : c(ctx) { if (km_dev_alloc(c, bytes, &p) != KM_OK) p = nullptr; REQUIRE(p, "km_dev_alloc"); }
    ~dev_buf() { if (p) (void)km_dev_free(c, p); }
    dev_buf(const dev_buf &) = delete;
};
struct host_buf {
    km_ctx *c;
    void *p = nullptr;
    host_buf(km_ctx *ctx, size_t bytes) : c(ctx) { if (km_host_alloc(c, bytes, &p) != KM_OK) p = nullptr; REQUIRE(p, "km_host_alloc"); }
    ~host_buf() { if (p) (void)km_host_free(c, p); }
    host_buf(const host_buf &) = delete;
};
static void fill_pair(uint16_t *ref, uint16_t *mon)
{
    for (size_t i = 0; i < (size_t)H * W; i++) { ref[i] = (uint16_t)(1 + (i * 2654435761u >> 20) % 9000); mon[i] = (uint16_t)(1 + (i * 40503u >> 7) % 9000); }
}
static km_klt_params params()
{
    km_klt_params prm = {};
    prm.max_corners = CAP; prm.block_size = 15; prm.win_size = 21; prm.max_level = 1; prm.max_count = 30;
    prm.ksize_mon = prm.ksize_ref = 7; prm.quality_level = 0.1; prm.min_distance = 10.0; prm.epsilon = 0.03;
    return prm;
}
// a resident uint16 pair and what the scenarios do with it
struct pair16 {
    km_ctx *c;
    dev_buf dr, dm, dmask;
    km_klt_params prm = params();
    km_unit units[2];
    pair16(km_ctx *ctx) : c(ctx), dr(ctx, (size_t)H * W * 2), dm(ctx, (size_t)H * W * 2), dmask(ctx, (size_t)H * W)
    {
        const int box[2][2] = {{0, H}, {8, H - 16}};      // {first row, rows}
        for (int u = 0; u < 2; u++) {
            units[u] = km_unit();
            units[u].d_ref = (const uint16_t *)dr.p + (size_t)box[u][0] * W; units[u].d_mon = (const uint16_t *)dm.p + (size_t)box[u][0] * W;
            units[u].sref = units[u].smon = units[u].sref_f = units[u].smon_f = W;
            units[u].d_ref_full = dr.p; units[u].d_mon_full = dm.p;
            units[u].H = box[u][1]; units[u].W = W; units[u].Hf = H; units[u].Wf = W; units[u].y_off = (float)box[u][0];
        }
    }
    void upload_blocking()      // through the ring on the main stream; the call completes the stream
    {
        std::vector<uint16_t> ref((size_t)H * W), mon((size_t)H * W);
        fill_pair(ref.data(), mon.data());
        std::vector<uint8_t> mask((size_t)H * W, 1);
        CALL(km_h2d(c, dr.p, ref.data(), ref.size() * 2)); CALL(km_h2d(c, dm.p, mon.data(), mon.size() * 2)); CALL(km_h2d(c, dmask.p, mask.data(), mask.size()));
    }
    void upload_async(const host_buf &hr, const host_buf &hm)      // page-locked sources: DMA'd in place on the copy stream
    {
        fill_pair((uint16_t *)hr.p, (uint16_t *)hm.p);
        CALL(km_upload_async(c, dr.p, W * 2, hr.p, W * 2, W * 2, H)); CALL(km_upload_async(c, dm.p, W * 2, hm.p, W * 2, W * 2, H));
    }
    // leaves a write of the monitored raster in flight on the main stream (km_shift_image_dev from a copy of it): whatever reads the raster
    // next on another stream has to be ordered behind it.  The scenarios put one in front of every pipeline start, so that the wait the
    // second stream owes the main stream there always has something to wait for
    std::unique_ptr<dev_buf> mon_copy;
    void rewrite_mon()
    {
        if (!mon_copy) {
            mon_copy.reset(new dev_buf(c, (size_t)H * W * 2));
            CALL(km_shift_image_dev(c, dm.p, 2, H, W, W, 0, 0, mon_copy->p));
        }
        CALL(km_shift_image_dev(c, mon_copy->p, 2, H, W, W, 0, 0, dm.p));
    }
    int submit_units(bool user_mask = false)
    {
        int t = -1;
        km_unit q[2] = {units[0], units[1]};
        if (user_mask) for (int u = 0; u < 2; u++) { q[u].d_mask = (const uint8_t *)dmask.p + (size_t)(u ? 8 : 0) * W; q[u].smask = W; }
        CALL(km_klt_units_frame_submit(c, q, 2, KM_U16, nullptr, nullptr, &prm, 0.4, CAP, &t));
        return t;
    }
    int submit_tile()
    {
        int t = -1;
        CALL(km_klt_tile_frame_submit(c, dr.p, dm.p, KM_U16, H, W, W, W, nullptr, 0, nullptr, nullptr, &prm, 0.f, 0.f, dr.p, dm.p, H, W, W, W, 0.4, CAP, &t));
        return t;
    }
    void wait(int t)
    {
        const void *block = nullptr;
        size_t nb = 0;
        if (t < 0) return;
        CALL(km_frame_flush(c, t));
        CALL(km_frame_wait(c, t, &block, &nb));
    }
};

// 1: upload + ticket, joined on a fresh context, then a PIPELINED submission as the first compute call
static void sc_upload_ticket(km_ctx *c)
{
    pair16 P(c);
    host_buf hr(c, (size_t)H * W * 2), hm(c, (size_t)H * W * 2);
    int ticket = -1;
    CALL(km_set_option(c, "units_pipeline", 1));
    P.upload_async(hr, hm);
    CALL(km_upload_mark(c, &ticket));
    CALL(km_upload_join(c, ticket));
    P.wait(P.submit_units());
}
// 2: the same with the upload left to begin_call's join_uploads
static void sc_upload_implicit(km_ctx *c)
{
    pair16 P(c);
    host_buf hr(c, (size_t)H * W * 2), hm(c, (size_t)H * W * 2);
    CALL(km_set_option(c, "units_pipeline", 1));
    P.upload_async(hr, hm);
    P.wait(P.submit_units());
}
// 3: a pipelined submission behind two tiles still in flight.  The warm-up brings every workspace slot to its final size: a slot regrown
// under the in-flight tiles would retire the buffer they use and hide the conflict
static void sc_behind_tiles(km_ctx *c)
{
    pair16 P(c);
    P.upload_blocking();
    CALL(km_set_option(c, "units_pipeline", 1));
    P.rewrite_mon(); P.wait(P.submit_units());
    P.wait(P.submit_tile());
    P.rewrite_mon(); P.wait(P.submit_units());
    const void *scalars_before = c->ws[WS_SCALARS].p;
    const size_t retired_before = c->retired.size();
    const int t0 = P.submit_tile(), t1 = P.submit_tile();
    const int t2 = P.submit_units();
    REQUIRE(c->ws[WS_SCALARS].p == scalars_before && c->retired.size() == retired_before, "a workspace slot was regrown under the in-flight tiles");
    P.wait(t2); P.wait(t0); P.wait(t1);
}
// 4: km_shift_image_dev writes the monitored raster on the main stream, a pipelined submission reads it; then the same with an unpipelined
// uint8 batch in between
static void sc_behind_shift(km_ctx *c)
{
    pair16 P(c);
    P.upload_blocking();
    dev_buf r8(c, (size_t)H * W), m8(c, (size_t)H * W);
    std::vector<uint8_t> a8((size_t)H * W), b8((size_t)H * W);
    for (size_t i = 0; i < a8.size(); i++) { a8[i] = (uint8_t)(i * 31 >> 3); b8[i] = (uint8_t)(i * 17 >> 2); }
    CALL(km_h2d(c, r8.p, a8.data(), a8.size())); CALL(km_h2d(c, m8.p, b8.data(), b8.size()));
    CALL(km_set_option(c, "units_pipeline", 1));
    P.rewrite_mon(); P.wait(P.submit_units());
    P.rewrite_mon();
    km_unit q = P.units[0];
    q.d_ref = q.d_ref_full = r8.p; q.d_mon = q.d_mon_full = m8.p;
    int t8 = -1;
    CALL(km_klt_units_frame_submit(c, &q, 1, KM_U8, nullptr, nullptr, &P.prm, 0.4, CAP, &t8));
    const int t = P.submit_units();
    P.wait(t); P.wait(t8);
}
// 5: steady state - six pipelined submissions on alternating lanes, with and without a user mask, clip and MI columns on, blocks into a
// pitched frame sink; waited for in submission order, then in reverse
static void sc_steady_state(km_ctx *c)
{
    pair16 P(c);
    P.upload_blocking();
    const size_t pitch = 16 + (size_t)CAP * (6 * 4 + 3 * 8) + 512;
    dev_buf sink(c, pitch * 2);
    CALL(km_set_frame_sink_pitch(c, sink.p, pitch * 2, pitch));
    CALL(km_set_option(c, "units_pipeline", 1));
    CALL(km_set_option(c, "frame_clip", 1));
    CALL(km_set_option(c, "frame_mi", 1));
    int t[3];
    P.rewrite_mon();
    for (int k = 0; k < 3; k++) t[k] = P.submit_units(k == 1);
    for (int k = 0; k < 3; k++) P.wait(t[k]);
    P.rewrite_mon();
    for (int k = 0; k < 3; k++) t[k] = P.submit_units(k != 1);
    for (int k = 2; k >= 0; k--) P.wait(t[k]);
    CALL(km_set_frame_sink(c, nullptr, 0));
}
// 6: the tile path alone - blocking, then three submissions through the frame ring with the early min / max, with the pyramids on and off
// the second stream, with and without the speculative corner path; the kernel-size search
static void sc_tile_path(km_ctx *c)
{
    pair16 P(c);
    P.upload_blocking();
    std::vector<char> block(16 + (size_t)CAP * (6 * 4 + 8));
    for (int variant = 0; variant < 3; variant++) {
        CALL(km_set_option(c, "aux_pyramid", variant != 1));
        CALL(km_set_option(c, "speculative", variant != 2));
        CALL(km_klt_tile_frame_zncc_dev(c, P.dr.p, P.dm.p, KM_U16, H, W, W, W, nullptr, 0, nullptr, nullptr, &P.prm, 0.f, 0.f, P.dr.p, P.dm.p, H, W, W, W, 0.4, block.data(), CAP));
        // (a tile on the speculative path marks the start of its LK - the blocking call above too: the tile behind it starts its min / max there, on
        // the second stream)
        int t[3];
        unsigned early = 0;
        for (int k = 0; k < 3; k++) {
            t[k] = P.submit_tile();
            km_klt_stats st;
            CALL(km_get_klt_stats(c, &st));
            early += (st.path_flags & KM_PATH_MM_EARLY) != 0;
        }
        REQUIRE(early == (variant != 2 ? 3u : 0u), "variant %d: %u of three submitted tiles took the early min / max", variant, early);
        for (int k = 0; k < 3; k++) P.wait(t[k]);
    }
    const int ksizes[3] = {3, 5, 7};
    double ratios[9];
    int best[2];
    std::vector<char> out(16 + (size_t)CAP * 6 * 4);
    CALL(km_klt_auto_ksize_frame_dev(c, P.dr.p, P.dm.p, KM_U16, H, W, W, W, nullptr, 0, nullptr, nullptr, &P.prm, ksizes, 3, 0.f, 0.f, out.data(), CAP, ratios, best));
}
// 7: pair B's upload queued (marked, not joined) while pair A is matched, joined before B's first call - pipelined and not
static void sc_next_pair_upload(km_ctx *c)
{
    pair16 A(c), B(c);
    A.upload_blocking();
    host_buf hr(c, (size_t)H * W * 2), hm(c, (size_t)H * W * 2);
    for (int piped = 0; piped < 2; piped++) {
        CALL(km_set_option(c, "units_pipeline", piped));
        int ticket = -1;
        if (piped) A.rewrite_mon();
        const int ta = A.submit_units();
        B.upload_async(hr, hm);
        CALL(km_upload_mark(c, &ticket));
        const int ta2 = A.submit_units();
        CALL(km_upload_join(c, ticket));
        const int tb = B.submit_units();
        A.wait(ta); A.wait(ta2); B.wait(tb);
        B.wait(B.submit_tile());
    }
}

struct scenario {
    const char *name;
    void (*run)(km_ctx *);
};
static const scenario kScenarios[] = {{"1 upload ticket, pipelined first call", sc_upload_ticket}, {"2 upload joined by begin_call, pipelined first call", sc_upload_implicit},
                                      {"3 pipelined submission behind in-flight tiles", sc_behind_tiles}, {"4 pipelined submission behind km_shift_image_dev", sc_behind_shift},
                                      {"5 steady state", sc_steady_state}, {"6 tile path", sc_tile_path}, {"7 next pair's upload", sc_next_pair_upload}};

struct outcome {
    std::vector<so::report> reports;
    std::vector<so::wait_entry> waits;
};
// one scenario on a fresh context; ignore >= 0: the checker ignores that hipStreamWaitEvent of the scenario
static outcome run_scenario(const scenario &s, int ignore)
{
    outcome o;
    km_ctx *c = nullptr;
    so::enable(false);      // (nothing of the previous run is alive: its clocks - an entry per stream there ever was - go with it)
    so::enable(true);
    if (km_ctx_create(0, &c) != KM_OK) { REQUIRE(false, "km_ctx_create: %s", km_last_error(nullptr)); return o; }
    g_ctx = c;
    so::clear_log();
    so::ignore_wait_after(ignore);
    s.run(c);
    so::ignore_wait_after(-1);
    o.reports = so::reports(); o.waits = so::waits();
    REQUIRE(km_ctx_destroy(c) == KM_OK, "km_ctx_destroy");
    g_ctx = nullptr;
    return o;
}

// ------------------------------------------------------------------ c. waits whose removal no scenario can see, and what covers each
// scenario: its number; occurrence: which wait of that (stream, event) pair within the scenario, counted from 0 (-1: every one)
struct covered_wait {
    int scenario;
    const char *stream, *event;
    int occurrence;
    const char *covered_by;
};
// the host had waited for every frame in flight (km_frame_wait: a successful hipEventQuery of the slot's `done`) or completed a blocking call
// (km_d2h_flush) before the call that issues the wait: the device-side wait orders what the host already knows to be through
#define HOST_WAITED "the host waited for the frames in flight before this call (km_frame_wait / the flush of a blocking call)"
// units_tail waits for the lane's pyramids and valid-pixel sums (EV_JOIN, second stream) in front of LK.  When the NEXT submission enqueues
// this tail, its min / max already sits on the second stream BEHIND those pyramids and the main stream has waited for it (EV_MM) a few lines
// up.  The wait carries the order when km_frame_flush enqueues the tail: those occurrences are reported
#define NEXT_MINMAX "the next submission's min / max runs on aux_stream behind these pyramids, and main_stream waited for it (ev_lane[][EV_MM]) before this tail"
// the early min / max waits for the start of the previous unit's LK so that it runs BESIDE LK: timing.  For order it needs to stay behind the
// previous unit's Laplacian pass, which reads the previous early result - and the previous unit's fork (ev_fork / EV_FORK, recorded behind
// that pass) put aux_stream there already.  With "aux_pyramid" 0 there is no fork: those occurrences (scenario 6) are reported
#define FORKED "the previous unit's fork (ev_fork / ev_lane[][EV_FORK]) already put aux_stream behind its Laplacian pass; the wait decides when the min / max starts"
// km_upload_join makes both streams wait for the ticket.  The first kernel that reads the rasters is the early min / max on aux_stream; the
// main stream's first reader, the Laplacian pass, waits for that min / max (EV_MM).  aux_stream's wait for the ticket is reported
#define AUX_JOINED "aux_stream waits for the same ticket, and main_stream waits for the min / max that ran there (ev_lane[][EV_MM]) before it reads the rasters"
static const std::vector<covered_wait> kCovered = {
    {3, "main_stream", "ev_lane[0][EV_F_DONE]", 0, HOST_WAITED}, {3, "aux_stream", "ev_lane[0][EV_F_DONE]", 0, HOST_WAITED},
    {3, "main_stream", "ev_lane[0][EV_F_DONE]", 1, HOST_WAITED}, {3, "aux_stream", "ev_lane[0][EV_F_DONE]", 1, HOST_WAITED},
    {3, "chain_stream", "fslot[1].done", 0, HOST_WAITED},
    {3, "aux_stream", "ev_lk_start", 0, FORKED},
    {4, "main_stream", "ev_lane[0][EV_F_DONE]", 0, HOST_WAITED}, {4, "aux_stream", "ev_lane[0][EV_F_DONE]", 0, HOST_WAITED},
    {5, "main_stream", "ev_lane[0][EV_JOIN]", 0, NEXT_MINMAX}, {5, "main_stream", "ev_lane[1][EV_JOIN]", 0, NEXT_MINMAX},
    {5, "main_stream", "ev_lane[0][EV_JOIN]", 2, NEXT_MINMAX}, {5, "main_stream", "ev_lane[1][EV_JOIN]", 1, NEXT_MINMAX},
    {5, "main_stream", "ev_lane[0][EV_F_DONE]", 0, HOST_WAITED}, {5, "aux_stream", "ev_lane[0][EV_F_DONE]", 1, HOST_WAITED},
    {5, "main_stream", "ev_lane[1][EV_F_DONE]", 0, HOST_WAITED}, {5, "aux_stream", "ev_lane[1][EV_F_DONE]", 0, HOST_WAITED},
    {6, "aux_stream", "ev_lk_start", 0, HOST_WAITED}, {6, "aux_stream", "ev_lk_start", 1, FORKED}, {6, "aux_stream", "ev_lk_start", 2, FORKED},
    {6, "aux_stream", "ev_lk_start", 3, HOST_WAITED},
    {6, "main_stream", "fslot[2].done", -1, HOST_WAITED},
    {7, "aux_stream", "ev_lk_start", 0, FORKED}, {7, "aux_stream", "ev_lk_start", 1, FORKED}, {7, "aux_stream", "ev_lk_start", 2, FORKED},
    {7, "main_stream", "upload_marks[]", -1, AUX_JOINED},
    {7, "main_stream", "fslot[2].done", 0, HOST_WAITED},
    {7, "main_stream", "ev_lane[0][EV_JOIN]", 3, NEXT_MINMAX}, {7, "main_stream", "ev_lane[1][EV_JOIN]", 0, NEXT_MINMAX},
    {7, "main_stream", "ev_lane[0][EV_F_DONE]", 0, HOST_WAITED}, {7, "aux_stream", "ev_lane[0][EV_F_DONE]", 1, HOST_WAITED},
    {7, "main_stream", "ev_lane[1][EV_F_DONE]", 0, HOST_WAITED}, {7, "aux_stream", "ev_lane[1][EV_F_DONE]", 0, HOST_WAITED},
    {7, "chain_stream", "fslot[0].done", 0, HOST_WAITED},
};

int main()
{
    static ctx_names names;
    so::enable(true);
    so::set_namer(&names);
    controls();
    if (g_failures) return 1;

    const bool list_only = getenv("ORDER_LIST_REPORTS") != nullptr;      // print every scenario's reports and go on (how the reports of a library under repair are read)
    const int n_sc = (int)(sizeof kScenarios / sizeof kScenarios[0]);
    const int only = getenv("ORDER_ONLY") ? atoi(getenv("ORDER_ONLY")) : 0;      // one scenario's number: that one alone, and no verdict
    std::vector<outcome> clean;
    for (int i = 0; i < n_sc; i++) {
        if (only && only != i + 1) { clean.push_back(outcome()); continue; }
        clean.push_back(run_scenario(kScenarios[i], -1));
        printf("scenario %-52s %3zu wait(s), %zu report(s)\n", kScenarios[i].name, clean[i].waits.size(), clean[i].reports.size());
        for (const so::report &r : clean[i].reports) printf("    %s\n", r.text.c_str());
        if (!list_only) REQUIRE(clean[i].reports.empty(), "scenario %s: %zu report(s), the first: %s", kScenarios[i].name, clean[i].reports.size(), clean[i].reports[0].text.c_str());
    }
    if (list_only) { printf("STREAM-ORDER LISTED\n"); return 0; }
    if (g_failures) return 1;

    size_t walked = 0, reported = 0, tabled = 0;
    std::vector<bool> entry_used(kCovered.size(), false);
    for (int i = 0; i < n_sc; i++) {
        std::map<std::string, int> seen;
        for (size_t w = 0; w < clean[i].waits.size(); w++) {
            const so::wait_entry &we = clean[i].waits[w];
            const int occurrence = seen[we.stream + "|" + we.event]++;
            const outcome o = run_scenario(kScenarios[i], (int)w);
            REQUIRE(o.waits.size() == clean[i].waits.size() && o.waits[w].ignored && o.waits[w].stream == we.stream && o.waits[w].event == we.event,
                    "scenario %s: the rerun did not issue the same waits", kScenarios[i].name);
            walked++;
            int entry = -1;
            for (size_t k = 0; k < entry_used.size(); k++)
                if (kCovered[k].scenario == i + 1 && we.stream == kCovered[k].stream && we.event == kCovered[k].event && (kCovered[k].occurrence < 0 || kCovered[k].occurrence == occurrence))
                    entry = (int)k;
            if (!o.reports.empty()) {
                reported++;
                REQUIRE(entry < 0, "scenario %s: wait %d of %s for %s is listed as covered (%s) but ignoring it is reported: %s", kScenarios[i].name, occurrence,
                        we.stream.c_str(), we.event.c_str(), kCovered[entry < 0 ? 0 : entry].covered_by, o.reports[0].text.c_str());
            } else {
                REQUIRE(entry >= 0, "scenario %s: wait %d of %s for %s can be ignored without a report and is not listed", kScenarios[i].name, occurrence, we.stream.c_str(),
                        we.event.c_str());
                if (entry >= 0) { entry_used[(size_t)entry] = true; tabled++; }
            }
        }
    }
    for (size_t k = 0; k < entry_used.size() && !only; k++)
        REQUIRE(entry_used[k], "the table lists a wait no scenario issues: scenario %d, %s for %s", kCovered[k].scenario, kCovered[k].stream, kCovered[k].event);
    printf("waits walked %zu, reported %zu, tabled %zu\n", walked, reported, tabled);
    if (g_failures || only) return 1;
    printf("STREAM-ORDER OK\n");
    return 0;
}
