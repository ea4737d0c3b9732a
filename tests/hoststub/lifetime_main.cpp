// TEST INFRASTRUCTURE (tests/test_ctx_lifetime_host.py): who releases what a context creates.  A program of its own (no python, no
// preload) linked from the host objects of the sanitizer build and the stand-in HIP layer, whose counters of live streams, events,
// device and page-locked allocations must all be back at zero after km_ctx_destroy -
//   1. once after a context has been through every lazy creation site of the library (checked member by member);
//   2. again with every device allocation, every page-locked allocation and every stream / event creation failing in turn: no call
//      may crash, whatever it returns, and the half-built context must still destroy cleanly.
// Prints 'CTX-LIFETIME OK' at the end.
#include "../../karios_amd/csrc/common.hpp"

#include <cstdio>
#include <vector>

static int g_failures = 0;
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "lifetime_main.cpp:%d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); g_failures++; } } while (0)

// device memory of the caller (km_dev_alloc): released through the context it came from
struct dev_buf {
    km_ctx *c;
    void *p = nullptr;
    dev_buf(km_ctx *ctx, size_t bytes) : c(ctx) { if (km_dev_alloc(c, bytes, &p) != KM_OK) p = nullptr; }
    ~dev_buf() { if (p) (void)km_dev_free(c, p); }
    dev_buf(const dev_buf &) = delete;
};

// every owner of a context that is created on first use (clean pass: all of them must exist before the context goes)
static void require_all_created(const km_ctx *c)
{
#define HAS(member) REQUIRE((member), "never created: %s", #member)
    HAS(c->main_stream); HAS(c->copy_stream); HAS(c->aux_stream); HAS(c->d2h_stream); HAS(c->chain_stream);
    HAS(c->ev_copy); HAS(c->ev_tail); HAS(c->ev_lk_start); HAS(c->ev_mm); HAS(c->ev_fork); HAS(c->ev_join); HAS(c->ev_units_start); HAS(c->ev_readback);
    for (int l = 0; l < 2; l++) for (int i = 0; i < KM_LANE_EVENTS; i++) HAS(c->ev_lane[l][i]);
    HAS(c->ev_ready); HAS(c->evs[0][0][0]); HAS(c->evs[KM_FRAME_SLOTS][ST_COUNT - 1][1]);
    HAS(c->land_ev[0]); HAS(c->land_ev[1]); HAS(c->land); HAS(c->chk_dev); HAS(c->chk_host); HAS(c->pinned_rb);
    for (const km_ring_slot &s : c->ring.slot) { HAS(s.buf); HAS(s.done); }
    for (const km_frame_slot &f : c->fslot) { HAS(f.host); HAS(f.done); }
    HAS(c->ws[WS_SCALARS]); HAS(c->ws_b[WS_SCALARS]); HAS(c->utail.get());
    HAS(!c->free_marks.empty() || !c->upload_marks.empty());      // (retired buffers: checked where one is retired - a later flush releases them)
#undef HAS
}

// One context from km_ctx_create to km_ctx_destroy.  strict: every call must succeed and every lazy owner must exist at the end;
// otherwise a knob of the stand-in makes some call fail, and whatever depends on it is skipped or fails in turn
static void life_of_a_context(bool strict)
{
#define CALL(expr) do { const int rc_ = (expr); if (strict) REQUIRE(rc_ == KM_OK, "%s -> %d (%s)", #expr, rc_, km_last_error(c)); if (rc_ != KM_OK) ok = false; } while (0)
    km_ctx *c = nullptr;
    if (km_ctx_create(0, &c) != KM_OK) { REQUIRE(!strict && !c, "km_ctx_create failed: %s", km_last_error(nullptr)); return; }
    bool ok = true;
    CALL(km_set_profiling(c, 1));
    {
        const int H = 64, W = 512, cap = 64;
        std::vector<uint16_t> ref((size_t)H * W), mon((size_t)H * W);
        for (size_t i = 0; i < ref.size(); i++) { ref[i] = (uint16_t)(1 + (i * 2654435761u >> 20) % 9000); mon[i] = (uint16_t)(1 + (i * 40503u >> 7) % 9000); }
        const size_t bytes = ref.size() * sizeof(uint16_t);
        dev_buf dr(c, bytes), dm(c, bytes);
        if (dr.p && dm.p) {
            // ---- the copy stream with its tickets; the page-locked ring (pageable source) and the landing arena, in two halves for a large result
            int ticket = -1;
            CALL(km_upload_async(c, dr.p, W * 2, ref.data(), W * 2, W * 2, H));
            CALL(km_upload_mark(c, &ticket));
            CALL(km_upload_join(c, ticket));
            CALL(km_h2d(c, dm.p, mon.data(), bytes));
            std::vector<uint16_t> back(ref.size());
            CALL(km_d2h(c, back.data(), dr.p, bytes));
            if (strict) REQUIRE(back == ref, "the raster did not survive upload_async + d2h");
            const size_t big = ((size_t)4 << 20) + 64;      // more than half the arena
            dev_buf dbig(c, big);
            std::vector<char> hbig(big);
            if (dbig.p) CALL(km_d2h(c, hbig.data(), dbig.p, big));

            km_klt_params prm = {};
            prm.max_corners = cap; prm.block_size = 15; prm.win_size = 21; prm.max_level = 1; prm.max_count = 30;
            prm.ksize_mon = prm.ksize_ref = 7; prm.quality_level = 0.1; prm.min_distance = 10.0; prm.epsilon = 0.03;
            const void *block = nullptr;
            size_t nb = 0;
            auto submit_tile = [&]() {      // the second stream, the block-copy stream, a frame slot
                int t = -1;
                CALL(km_klt_tile_frame_submit(c, dr.p, dm.p, KM_U16, H, W, W, W, nullptr, 0, nullptr, nullptr, &prm, 0.f, 0.f, dr.p, dm.p, H, W, W, W, 0.4, cap, &t));
                if (t >= 0) CALL(km_frame_wait(c, t, &block, &nb));
            };
            submit_tile();
            // ---- batched units: one submission in stream order (it marks the start of its LK: the tile behind it starts its min / max
            // there), then two pipelined ones: both lanes, the chain stream, the deferred tail
            km_unit units[2] = {};
            const int box[2][2] = {{0, H}, {8, H - 16}};    // {first row, rows}: 512 columns, the narrowest the batch form takes
            for (int u = 0; u < 2; u++) {
                units[u].d_ref = (const uint16_t *)dr.p + (size_t)box[u][0] * W; units[u].d_mon = (const uint16_t *)dm.p + (size_t)box[u][0] * W;
                units[u].sref = units[u].smon = units[u].sref_f = units[u].smon_f = W;
                units[u].d_ref_full = dr.p; units[u].d_mon_full = dm.p;
                units[u].H = box[u][1]; units[u].W = W; units[u].Hf = H; units[u].Wf = W; units[u].y_off = (float)box[u][0];
            }
            int tk[2] = {-1, -1};
            CALL(km_klt_units_frame_submit(c, units, 2, KM_U16, nullptr, nullptr, &prm, 0.4, cap, &tk[0]));
            if (ok) submit_tile();
            if (tk[0] >= 0) CALL(km_frame_wait(c, tk[0], &block, &nb));
            tk[0] = -1;
            CALL(km_set_option(c, "units_pipeline", 1));
            for (int k = 0; k < 2 && ok; k++) CALL(km_klt_units_frame_submit(c, units, 2, KM_U16, nullptr, nullptr, &prm, 0.4, cap, &tk[k]));
            for (int k = 0; k < 2; k++) {
                if (tk[k] < 0) continue;
                CALL(km_frame_flush(c, tk[k]));
                CALL(km_frame_wait(c, tk[k], &block, &nb));
            }
            CALL(km_set_option(c, "units_pipeline", 0));
        } else
            ok = false;
    }
    // ---- host forms (their uploads are checksummed: KARIOS_HIP_UPLOAD_CHECKSUM); the larger image regrows workspace slots, whose old buffers are retired
    for (int side : {24, 96}) {
        std::vector<uint8_t> a((size_t)side * side, 7), out(a.size());
        const long before = stub().device_allocs;
        CALL(km_laplacian_u8(c, a.data(), side, side, 7, out.data()));
        if (strict && side == 96) REQUIRE(stub().device_allocs > before && !c->retired.empty(), "no workspace buffer was retired");
    }
    {
        const int side = 40, cap = 256;
        std::vector<uint8_t> img((size_t)side * side), desc((size_t)cap * 128);
        for (size_t i = 0; i < img.size(); i++) img[i] = (uint8_t)(((i % side) / 8 + (i / side) / 8) % 2 ? 200 : 30);
        std::vector<float> f((size_t)5 * cap);
        std::vector<int> octave(cap);
        int count = 0;
        int64_t stats[160];
        const int rc = km_sift_detect_and_compute(c, img.data(), side, side, side, 0, 3, 0.04, 10.0, 1.6, cap, &f[0], &f[cap], &f[2 * cap], &f[3 * cap], &f[4 * cap],
                                                  octave.data(), desc.data(), KM_U8, 128, &count, stats);
        if (strict) REQUIRE(rc == KM_OK || rc == KM_E_CAPACITY, "km_sift_detect_and_compute -> %d (%s)", rc, km_last_error(c));
    }
    // (the stand-in has no kernels of the exact corner path, k_select.hip, whose read-backs alone create these two: asked for directly)
    CALL(km_wait_readback(c));
    CALL(km_pinned_rb(c, 64) && km_pinned_rb(c, 4096) ? KM_OK : KM_E_NOMEM);
    if (strict) require_all_created(c);
    REQUIRE(km_ctx_destroy(c) == KM_OK, "km_ctx_destroy");
#undef CALL
}

static bool nothing_alive(const char *when, int k)
{
    const stub_state &s = stub();
    REQUIRE(s.streams == 0 && s.events == 0 && s.device_allocs == 0 && s.host_allocs == 0,
            "%s %d: left behind %ld streams, %ld events, %ld device allocations, %ld page-locked allocations", when, k, s.streams, s.events, s.device_allocs,
            s.host_allocs);
    return g_failures == 0;
}

int main()
{
    setenv("KARIOS_HIP_UPLOAD_CHECKSUM", "1", 1);
    life_of_a_context(true);
    if (!nothing_alive("clean pass", 0)) return 1;
    struct { const char *what; int stub_state::*knob; } const sweeps[] = {{"device allocation", &stub_state::fail_malloc_after},
                                                                          {"page-locked allocation", &stub_state::fail_host_malloc_after},
                                                                          {"stream / event creation", &stub_state::fail_create_after}};
    for (const auto &sw : sweeps) {
        int k = 0;
        for (;; k++) {
            stub().*sw.knob = k;
            life_of_a_context(false);
            const bool fired = stub().*sw.knob < 0;      // (a knob disarms itself when it makes a call fail)
            stub().*sw.knob = -1;
            if (!nothing_alive(sw.what, k)) return 1;
            if (!fired) break;
            if (k > 2000) { fprintf(stderr, "%s: the sweep does not end\n", sw.what); return 1; }
        }
        printf("%s: %d failures walked\n", sw.what, k);
        if (k < 8) { fprintf(stderr, "%s: only %d creations in a context's life?\n", sw.what, k); return 1; }
    }
    printf("CTX-LIFETIME OK\n");
    return 0;
}
