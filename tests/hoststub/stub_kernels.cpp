// TEST INFRASTRUCTURE (tests/test_host_asan.py): the stand-in HIP layer of hip/hip_runtime.h and do-little replacements of every
// kernel launcher of csrc/common.hpp that api*.hip / staging.hip call (the launchers of the align step's k_*.hpp headers have
// their stand-ins in stub_kernels_align.cpp).  "Device" memory is malloc'ed host memory, so AddressSanitizer
// sees every access: the stand-ins READ their inputs completely and WRITE their outputs completely, at the sizes the launchers
// are entitled to - an undersized workspace slot, a short upload or a read-back beyond a buffer is a sanitizer report.
//
// Stream order (stub_order.hpp, on in tests/hoststub/order_main.cpp only): every stand-in DECLARES, as one operation on c->stream, what the
// REAL launcher of csrc/k_*.hip reads and writes - which is not what the stand-in happens to touch: rasters as strided boxes row by row,
// a km_scalars block by the fields the kernels touch, and the workspace slots the real launcher reserves by id (partials, tables, scratch
// of the selection and frame stages), reserved here on the same lane so that slots shared between the tile path and the batched path meet
// in the checker.  With the checker off `launch` does nothing and reserves nothing: the stand-ins are what they were.
#include "../../karios_amd/csrc/common.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

stub_state &stub()
{
    static stub_state s;
    return s;
}

namespace so = stub_order;
// one launcher's operation on c->stream
struct launch : so::op {
    km_ctx *c;
    launch(km_ctx *ctx, const char *name) : so::op(ctx->stream, name), c(ctx) {}
    // the workspace slot the real launcher reserves (current lane), touched as a whole; nullptr with the checker off
    void *slot(int id, size_t bytes, so::kind k = so::WRITE) const
    {
        if (!live) return nullptr;
        void *p = km_ws(c, id, bytes);
        touch(k, p, bytes);
        return p;
    }
    void box(so::kind k, const void *img, size_t es, int H, int W, ptrdiff_t stride) const { touch_rows(k, img, (size_t)stride * es, (size_t)W * es, (size_t)H); }
    // fields [first, last] of a scalar block
    void fields(so::kind k, const km_scalars *sc, size_t first, size_t end) const { touch(k, (const char *)sc + first, end - first); }
    void pyramid(const km_pyr &P) const
    {
        for (int l = 0; l <= P.levels; l++) {
            const int h = P.Hres[l] ? P.Hres[l] : P.H[l], oy = P.Hres[l] ? P.oy[l] : 0;
            read(P.img[l] + (size_t)oy * P.W[l], (size_t)h * P.W[l]);
        }
    }
};
#define SC_FIELD(name) offsetof(km_scalars, name), offsetof(km_scalars, name) + sizeof(((km_scalars *)0)->name)
#define SC_CORNERS offsetof(km_scalars, max_eig_key), sizeof(km_scalars)      // everything behind the min / max and the valid-pixel count
static size_t dtype_bytes(int dtype) { return km_any_dtype_size(dtype); }
static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
enum { LK_TABLE_ENTRY = 512 };      // bytes of one entry of the LK argument table (lk_device.hpp lk_args: two pyramids and a dozen words; the stand-in's own figure)

static bool is_pinned(const void *p)
{
    stub_state &s = stub();
    std::lock_guard<std::mutex> g(s.m);
    auto it = s.pinned.upper_bound((const char *)p);
    if (it == s.pinned.begin()) return false;
    --it;
    return (const char *)p < it->first + it->second;
}

hipError_t hipMalloc(void **p, size_t n)
{
    stub_state &s = stub();
    if (stub_fails_now(s.fail_malloc_after)) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(n ? n : 1);
    s.device_allocs++;
    so::on_malloc(*p, n ? n : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void *p) { if (p) { so::on_free(p); free(p); stub().device_allocs--; } return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned)
{
    *p = stub_fails_now(stub().fail_host_malloc_after) ? nullptr : malloc(n ? n : 1);
    if (!*p) return hipErrorOutOfMemory;
    stub_state &s = stub();
    std::lock_guard<std::mutex> g(s.m);
    s.pinned[(const char *)*p] = n ? n : 1;
    s.host_allocs++;
    return hipSuccess;
}
hipError_t hipHostFree(void *p)
{
    if (!p) return hipSuccess;
    stub_state &s = stub();
    {
        std::lock_guard<std::mutex> g(s.m);
        if (!s.pinned.erase((const char *)p)) return hipErrorInvalidValue;
        s.host_allocs--;
    }
    free(p);
    return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *at, const void *p)
{
    if (!is_pinned(p)) return hipErrorInvalidValue;      // like the runtime: unregistered host memory is an error
    at->type = hipMemoryTypeHost; at->device = 0; at->devicePointer = at->hostPointer = (void *)p;
    return hipSuccess;
}
// the property under test: the library never hands PAGEABLE memory to an asynchronous runtime copy
static void note_copy(const void *host_side)
{
    if (!is_pinned(host_side)) { std::lock_guard<std::mutex> g(stub().m); stub().pageable_async_copies++; }
}
// (the copies declare both ends whatever their kind: an end in host memory lies in no device allocation and is ignored)
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
    if (kind == hipMemcpyHostToDevice) note_copy(src);
    if (kind == hipMemcpyDeviceToHost) note_copy(dst);
    { const so::op o(s, s ? "hipMemcpyAsync" : "hipMemcpy"); o.read(src, n); o.write(dst, n); }
    memmove(dst, src, n);
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t s)
{
    if (dpitch < width || spitch < width) return hipErrorInvalidValue;
    { const so::op o(s, "hipMemcpy2DAsync"); o.touch_rows(so::READ, src, spitch, width, height); o.touch_rows(so::WRITE, dst, dpitch, width, height); }
    if (kind == hipMemcpyHostToDevice) note_copy(src);
    if (kind == hipMemcpyDeviceToHost) note_copy(dst);
    for (size_t y = 0; y < height; y++) memmove((char *)dst + y * dpitch, (const char *)src + y * spitch, width);
    return hipSuccess;
}

extern "C" {
// counters for the test: {device allocations alive, page-locked allocations alive, asynchronous copies that touched pageable memory}
void stub_counters(long out[3])
{
    out[0] = stub().device_allocs; out[1] = stub().host_allocs; out[2] = stub().pageable_async_copies;
}
void stub_fail_malloc_after(int n) { stub().fail_malloc_after = n; }
void stub_lk_jobs_unsupported(int on) { stub().lk_jobs_unsupported = on != 0; }
}

// ------------------------------------------------------------------ pixel access
static double px(const void *img, int dtype, size_t i)
{
    switch (dtype) {
    case KM_U8: return ((const uint8_t *)img)[i];
    case KM_U16: return ((const uint16_t *)img)[i];
    case KM_I16: return ((const int16_t *)img)[i];
    case KM_F32: return ((const float *)img)[i];
    case KM_F64: return ((const double *)img)[i];
    case KM_I32: return ((const int32_t *)img)[i];
    case KM_U32: return ((const uint32_t *)img)[i];
    default: return 0;
    }
}
static void minmax_of(const void *img, int dtype, int H, int W, ptrdiff_t stride, double *mm)
{
    double mn = INFINITY, mx = -INFINITY;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const double v = px(img, dtype, (size_t)y * stride + x);
            if (v == v) { mn = std::min(mn, v); mx = std::max(mx, v); }
        }
    mm[0] = mn; mm[1] = mx;
}

// (k_raster.hip: 2048 workgroups per image leave a {min, max} pair each in the slot of the caller's choice; a final launch reduces them)
int kd_minmax(km_ctx *c, const void *a, int dtype, int H, int W, ptrdiff_t sa, double *mm, const void *b, ptrdiff_t sb, int ws_slot)
{
    const launch L(c, "kd_minmax");
    L.box(so::READ, a, dtype_bytes(dtype), H, W, sa);
    if (b) L.box(so::READ, b, dtype_bytes(dtype), H, W, sb);
    L.slot(ws_slot, (size_t)2 * 2048 * (b ? 2 : 1) * sizeof(double));
    L.write(mm, (b ? 4 : 2) * sizeof(double));
    minmax_of(a, dtype, H, W, sa, mm);
    if (b) minmax_of(b, dtype, H, W, sb, mm + 2);
    return KM_OK;
}
static void to_uint8_of(const void *d, int dtype, int H, int W, ptrdiff_t s, const double *mm, int invert, uint8_t *out);
int kd_to_uint8(km_ctx *c, const void *d, int dtype, int H, int W, ptrdiff_t s, const double *mm, int invert, uint8_t *out)
{
    const launch L(c, "kd_to_uint8");
    L.box(so::READ, d, dtype_bytes(dtype), H, W, s);
    L.read(mm, 2 * sizeof(double));
    L.write(out, (size_t)H * W);
    to_uint8_of(d, dtype, H, W, s, mm, invert, out);
    return KM_OK;
}
static void to_uint8_of(const void *d, int dtype, int H, int W, ptrdiff_t s, const double *mm, int invert, uint8_t *out)
{
    const double r = mm[1] - mm[0];
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const double v = px(d, dtype, (size_t)y * s + x);
            uint8_t u = dtype == KM_U8 ? (uint8_t)v : (r > 0 && v == v ? (uint8_t)((v - mm[0]) / r * 255.0) : 0);
            out[(size_t)y * W + x] = invert ? 255 - u : u;
        }
}
static void auto_mask_of(const void *m, const void *r, int dtype, int H, int W, ptrdiff_t sm, ptrdiff_t sr, uint8_t *mask, unsigned long long *valid);
// (the count: a memset, then atomics of the same launcher - a write)
int kd_auto_mask(km_ctx *c, const void *m, const void *r, int dtype, int H, int W, ptrdiff_t sm, ptrdiff_t sr, const double *, const double *, uint8_t *mask,
                 unsigned long long *valid)
{
    const launch L(c, "kd_auto_mask");
    L.box(so::READ, m, dtype_bytes(dtype), H, W, sm);
    L.box(so::READ, r, dtype_bytes(dtype), H, W, sr);
    L.write(mask, (size_t)H * W);
    L.write(valid, sizeof *valid);
    auto_mask_of(m, r, dtype, H, W, sm, sr, mask, valid);
    return KM_OK;
}
static void auto_mask_of(const void *m, const void *r, int dtype, int H, int W, ptrdiff_t sm, ptrdiff_t sr, uint8_t *mask, unsigned long long *valid)
{
    unsigned long long n = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const bool ok = px(m, dtype, (size_t)y * sm + x) != 0 && px(r, dtype, (size_t)y * sr + x) != 0;
            mask[(size_t)y * W + x] = ok; n += ok;
        }
    *valid += n;
}
// (4096 per-workgroup counts in WS_PARTIAL, summed by one workgroup that WRITES the total)
int kd_count_nonzero(km_ctx *c, const uint8_t *m, size_t n, unsigned long long *valid)
{
    const launch L(c, "kd_count_nonzero");
    L.read(m, n);
    L.slot(WS_PARTIAL, 4096 * sizeof(unsigned));
    L.write(valid, sizeof *valid);
    unsigned long long k = 0;
    for (size_t i = 0; i < n; i++) k += m[i] != 0;
    *valid += k;
    return KM_OK;
}
int kd_laplacian_u8(km_ctx *c, const uint8_t *s, int H, int W, int, uint8_t *d)
{
    const launch L(c, "kd_laplacian_u8");
    L.read(s, (size_t)H * W); L.write(d, (size_t)H * W);
    memmove(d, s, (size_t)H * W);
    return KM_OK;
}
// work items of the marching Laplacian pass, each of which leaves one count of valid pixels (the stand-in's own figure: k_lap.hip sizes them by
// occupancy) - what matters is the slot, WS_LAP_VALID, and who sums it on which stream
static size_t lap_items(int H, int W) { return (size_t)((H + 31) / 32) * (size_t)((W + 255) / 256); }
// (k_lap.hip launch_lap_march: the per-item counts go to WS_LAP_VALID; their sum into *valid is this launcher's last launch, or - defer - the
// caller's job, kd_run_valid_sum on whatever stream it chooses)
int kd_stretch_laplacian_pair(km_ctx *c, const void *ref, const void *mon, int dtype, int H, int W, ptrdiff_t sr, ptrdiff_t sm, const double *mm, int, int, int inv,
                              const double *, const double *, uint8_t *lr, uint8_t *lm, uint8_t *mask, unsigned long long *valid, km_valid_job *defer)
{
    const launch L(c, "kd_stretch_laplacian_pair");
    L.box(so::READ, ref, dtype_bytes(dtype), H, W, sr);
    L.box(so::READ, mon, dtype_bytes(dtype), H, W, sm);
    L.read(mm, 4 * sizeof(double));
    L.write(lr, (size_t)H * W); L.write(lm, (size_t)H * W);
    if (mask) {
        L.write(mask, (size_t)H * W);
        const size_t items = lap_items(H, W);
        const unsigned *partial = (const unsigned *)L.slot(WS_LAP_VALID, (items + 4) * sizeof(unsigned));
        if (defer && partial) { defer->partial = partial; defer->n = (unsigned)items; defer->out = valid; }
        else L.write(valid, sizeof *valid);
    }
    to_uint8_of(ref, dtype, H, W, sr, mm, 0, lr);
    to_uint8_of(mon, dtype, H, W, sm, mm + 2, inv, lm);
    if (mask) auto_mask_of(mon, ref, dtype, H, W, sm, sr, mask, valid);
    return KM_OK;
}
// (k_eigmap.hip: per-workgroup maxima in WS_PARTIAL, reduced into *max_key)
int kd_min_eigen(km_ctx *c, const uint8_t *s, const uint8_t *mask, int H, int W, int, float *eig, unsigned *max_key)
{
    const launch L(c, "kd_min_eigen");
    L.read(s, (size_t)H * W);
    if (mask) L.read(mask, (size_t)H * W);
    L.write(eig, (size_t)H * W * sizeof(float));
    L.slot(WS_PARTIAL, lap_items(H, W) * sizeof(unsigned));
    L.write(max_key, sizeof *max_key);
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)H * W; i++) { eig[i] = (float)s[i]; if (!mask || mask[i]) mx = std::max(mx, eig[i]); }
    unsigned k; memcpy(&k, &mx, 4);
    *max_key = k | 0x80000000u;
    return KM_OK;
}
int k2_min_eigen(km_ctx *, const uint8_t *, const uint8_t *, int, int, int, float *, unsigned *) { return KM_E_UNSUPPORTED; }
// With the checker on, the synchronisation-free corner path of a tile (k2_eig_candidates with partials -> kf_rank -> kf_select) has stand-ins
// too: it is the path on which a tile forks its pyramids onto the second stream and marks the start of its LK for the next tile's early
// min / max.  With the checker off the three stay unsupported, as they were: the tile entry points then take the exact path.
// (k_eig3.hip launch_eig3_units for one unit: what k3_eig_candidates_units declares below)
int k2_eig_candidates(km_ctx *c, const uint8_t *src, const uint8_t *mask, int H, int W, int, double, km_scalars *sc, unsigned long long *keys, size_t cap, bool,
                      km_eig_partials *partials)
{
    if (!so::on() || !partials) return KM_E_UNSUPPORTED;
    const launch L(c, "k2_eig_candidates");
    L.read(src, (size_t)H * W);
    if (mask) L.read(mask, (size_t)H * W);
    L.write(keys, cap * sizeof *keys);
    L.fields(so::WRITE, sc, offsetof(km_scalars, pad0), offsetof(km_scalars, cut));
    L.fields(so::WRITE, sc, SC_FIELD(run_max_shard));
    L.fields(so::WRITE, sc, offsetof(km_scalars, tie_rows), sizeof(km_scalars));
    partials->partial = (const unsigned *)L.slot(WS_PARTIAL, (lap_items(H, W) + 16) * sizeof(unsigned));
    partials->n = (unsigned)lap_items(H, W);
    keys[0] = 1ull; keys[cap - 1] = 2ull;
    return KM_OK;
}
int k3_eig_candidates(km_ctx *, const uint8_t *, const uint8_t *, int, int, int, double, km_scalars *, unsigned long long *, size_t, km_eig_partials *) { return KM_E_UNSUPPORTED; }
// candidates: every 7th pixel of every 5th row, keys written up to the capacity the caller reserved
int kd_candidates(km_ctx *c, const float *eig, const uint8_t *mask, int H, int W, double, km_scalars *sc, unsigned long long *keys, size_t cap, bool)
{
    const launch L(c, "kd_candidates");
    L.read(eig, (size_t)H * W * sizeof(float));
    if (mask) L.read(mask, (size_t)H * W);
    L.fields(so::READ, sc, SC_FIELD(max_eig_key));
    L.fields(so::WRITE, sc, SC_FIELD(n_cand)); L.fields(so::WRITE, sc, SC_FIELD(thr)); L.fields(so::WRITE, sc, SC_FIELD(max_eig)); L.fields(so::WRITE, sc, SC_FIELD(shard_cnt));
    L.write(keys, cap * sizeof *keys);
    size_t n = 0;
    for (int y = 1; y < H - 1; y += 5)
        for (int x = 1; x < W - 1; x += 7) {
            unsigned b; const float v = eig[(size_t)y * W + x] + 1.f; memcpy(&b, &v, 4);
            if (n < cap) keys[n] = ((unsigned long long)b << 32) | (unsigned)((size_t)y * W + x);
            n++;
        }
    sc->n_cand = (unsigned)n;
    return KM_OK;
}
// (k_select.hip: histogram + cut in the scalar block, the WHOLE block read back behind km_wait_readback - the host knows the stream is
// through - then the compaction of the kept keys into WS_MISC3)
int ks_topk_prefilter(km_ctx *c, const unsigned long long *keys, size_t cap, size_t, km_scalars *sc, double, unsigned long long **kept, size_t *n_kept, size_t *n_total,
                      km_scalars *hs, bool)
{
    if (so::on()) {
        {
            const launch L(c, "ks_topk_prefilter");
            L.read(keys, cap * sizeof *keys);
            L.fields(so::READ, sc, SC_FIELD(max_eig_key)); L.fields(so::READ, sc, SC_FIELD(shard_cnt));
            L.fields(so::WRITE, sc, SC_FIELD(hist)); L.fields(so::WRITE, sc, SC_FIELD(cut));
        }
        { const so::op back(c->stream, "ks_topk_prefilter (read-back)"); back.read(sc, sizeof *sc); }
        { const int rc = km_wait_readback(c); if (rc) return rc; }
        const launch L(c, "ks_topk_prefilter (compaction)");
        L.read(keys, cap * sizeof *keys);
        L.fields(so::READ, sc, SC_FIELD(cut));
        L.slot(WS_MISC3, (std::min((size_t)sc->n_cand, cap) + 16) * sizeof *keys);
    }
    *hs = *sc;
    hs->pad0 = 0;
    const size_t n = std::min((size_t)sc->n_cand, cap);
    *kept = const_cast<unsigned long long *>(keys); *n_kept = n; *n_total = n;
    hs->cut[1] = (unsigned)n; hs->cut[3] = (unsigned)n;
    return KM_OK;
}
// (k_select.hip / k_sort.hip: the second key buffer in WS_KEYS1, the digit tables in WS_SORT_TMP)
int ks_sort_keys_desc(km_ctx *c, unsigned long long *k, size_t n, unsigned long long **sorted)
{
    const launch L(c, "ks_sort_keys_desc");
    L.write(k, n * sizeof *k);
    L.slot(WS_KEYS1, n * sizeof *k);
    L.slot(WS_SORT_TMP, ((size_t)256 * ((n + 2047) / 2048) + 8 * 256) * sizeof(unsigned));
    std::sort(k, k + n, std::greater<unsigned long long>());
    *sorted = k;
    return KM_OK;
}
// (k_select.hip: cell lists in WS_GRID, items / states / positions in WS_MISC2, the scan's tile sums in WS_SORT_TMP; the undecided counters
// and the corner count are read back behind km_wait_readback)
int ks_select(km_ctx *c, const unsigned long long *sorted, size_t n, int H, int W, int max_corners, double min_distance, float *xy, int cap, km_scalars *sc, int *found,
              bool)
{
    if (so::on()) {
        const launch L(c, "ks_select");
        L.fields(so::WRITE, sc, SC_FIELD(n_corners)); L.fields(so::WRITE, sc, SC_FIELD(n_batches));
        if (n > 0) {
            const int cell = min_distance >= 1 ? (int)lrint(min_distance) : 1;
            const size_t cells = (size_t)((W + cell - 1) / cell) * (size_t)((H + cell - 1) / cell);
            L.read(sorted, n * sizeof *sorted);
            L.slot(WS_GRID, (3 * cells + 4) * sizeof(unsigned));
            L.slot(WS_MISC2, n * 3 * sizeof(unsigned));
            L.slot(WS_SORT_TMP, (n / 2048 + cells / 2048 + 2) * sizeof(unsigned));
            L.fields(so::WRITE, sc, SC_FIELD(und));
            L.write(xy, (size_t)cap * 2 * sizeof(float));
            { const so::op back(c->stream, "ks_select (read-back)"); back.touch(so::READ, sc->und, sizeof sc->und); }
            { const int rc = km_wait_readback(c); if (rc) return rc; }
        }
    }
    int m = 0;
    for (size_t i = 0; i < n && (max_corners <= 0 || m < max_corners) && m < cap; i++, m++) {
        const unsigned idx = (unsigned)(sorted[i] & 0xffffffffu);
        xy[2 * m] = (float)(idx % (unsigned)W); xy[2 * m + 1] = (float)(idx / (unsigned)W);
    }
    sc->n_corners = m;
    if (found) *found = m;
    return KM_OK;
}
int km_sort_u64(km_ctx *c, unsigned long long *ka, unsigned long long *kb, unsigned *va, unsigned *vb, size_t n, bool desc)
{
    const launch L(c, "km_sort_u64");
    L.write(ka, n * 8); L.write(kb, n * 8);
    if (va) { L.write(va, n * 4); L.write(vb, n * 4); }
    L.slot(WS_SORT_TMP, ((size_t)256 * ((n + 2047) / 2048) + 8 * 256) * sizeof(unsigned));
    std::vector<size_t> o(n);
    std::iota(o.begin(), o.end(), (size_t)0);
    std::stable_sort(o.begin(), o.end(), [&](size_t a, size_t b) { return desc ? ka[a] > ka[b] : ka[a] < ka[b]; });
    for (size_t i = 0; i < n; i++) { kb[i] = ka[o[i]]; if (va) vb[i] = va[o[i]]; }
    memcpy(ka, kb, n * 8);
    if (va) memcpy(va, vb, n * 4);
    return KM_OK;
}
int km_exclusive_scan(km_ctx *c, const unsigned *in, unsigned *out, size_t n, int mode, int tmp_slot)
{
    const launch L(c, "km_exclusive_scan");
    L.read(in, n * sizeof *in); L.write(out, n * sizeof *out);
    L.slot(tmp_slot, ((n + 2047) / 2048 + 1) * sizeof(unsigned));
    unsigned s = 0;
    for (size_t i = 0; i < n; i++) { out[i] = s; s += mode == KM_SCAN_IS_ONE ? (in[i] == 1) : in[i]; }
    return KM_OK;
}
size_t kf_kept_capacity(int max_corners) { return (size_t)max_corners * 8; }
// k_select2.hip kf_layout_units: n units' slices of WS_MISC3 (kept + accepted keys), WS_GRID (cell records) and WS_MISC2 (states, counters),
// sized for the largest unit
static void kf_scratch(const launch &L, int n, int Hm, int Wm, int max_corners, double min_distance)
{
    const size_t kept_cap = kf_kept_capacity(max_corners), cell = (size_t)std::max(1L, lrint(min_distance));
    const size_t cells = ((Wm + cell - 1) / cell) * ((Hm + cell - 1) / cell);
    L.slot(WS_MISC3, up256((2 * kept_cap + 32) * sizeof(unsigned long long)) * n);
    L.slot(WS_GRID, up256((cells + 1) * 10 * sizeof(unsigned)) * n);
    L.slot(WS_MISC2, up256((kept_cap + 4 * KM_TK_NB + 16) * sizeof(unsigned)) * n);
}
int kf_rank(km_ctx *c, const unsigned long long *keys, size_t cap_keys, int H, int W, int max_corners, double, double min_distance, km_scalars *sc, km_eig_partials partials)
{
    if (!so::on()) return KM_E_UNSUPPORTED;
    const launch L(c, "kf_rank");
    kf_scratch(L, 1, H, W, max_corners, min_distance);
    L.read(keys, cap_keys * sizeof *keys);
    if (partials.partial) L.read(partials.partial, (size_t)partials.n * sizeof(unsigned));
    L.fields(so::WRITE, sc, SC_CORNERS);
    return KM_OK;
}
int kf_select(km_ctx *c, int H, int W, int max_corners, double min_distance, float *xy, int cap, km_scalars *sc)
{
    if (!so::on()) return KM_E_UNSUPPORTED;
    const launch L(c, "kf_select");
    kf_scratch(L, 1, H, W, max_corners, min_distance);
    L.fields(so::WRITE, sc, SC_CORNERS);
    L.write(xy, (size_t)cap * 2 * sizeof(float));
    const int n = std::min(std::min(max_corners, cap), 40);
    for (int i = 0; i < n; i++) { xy[2 * i] = (float)(20 + 7 * i % (W - 40)); xy[2 * i + 1] = (float)(20 + 11 * i % (H - 40)); }
    sc->n_corners = n; sc->cut[3] = 1000u; sc->flags = (unsigned)c->opt_spec_flag;
    return KM_OK;
}
static void pyrdown_of(const uint8_t *s, int H, int W, uint8_t *d)
{
    const int h = (H + 1) / 2, w = (W + 1) / 2;
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) d[(size_t)y * w + x] = s[(size_t)std::min(2 * y, H - 1) * W + std::min(2 * x, W - 1)];
}
int kd_pyrdown_u8(km_ctx *c, const uint8_t *s, int H, int W, uint8_t *d)
{
    const launch L(c, "kd_pyrdown_u8");
    L.read(s, (size_t)H * W); L.write(d, (size_t)((H + 1) / 2) * ((W + 1) / 2));
    pyrdown_of(s, H, W, d);
    return KM_OK;
}
int kd_pyrdown_u8_pair(km_ctx *c, const uint8_t *a, const uint8_t *b, int H, int W, uint8_t *da, uint8_t *db)
{
    const launch L(c, "kd_pyrdown_u8_pair");
    const size_t n = (size_t)H * W, m = (size_t)((H + 1) / 2) * ((W + 1) / 2);
    L.read(a, n); L.read(b, n); L.write(da, m); L.write(db, m);
    pyrdown_of(a, H, W, da); pyrdown_of(b, H, W, db);
    return KM_OK;
}
int kd_shift_image(km_ctx *c, const void *img, int es, int H, int W, ptrdiff_t stride, int yo, int xo, void *out)
{
    const launch L(c, "kd_shift_image");
    L.box(so::READ, img, (size_t)es, H, W, stride);
    L.write(out, (size_t)H * W * es);
    memset(out, 0, (size_t)H * W * es);
    for (int y = 0; y < H; y++) {
        const int sy = y + yo;
        if (sy < 0 || sy >= H) continue;
        for (int x = 0; x < W; x++) {
            const int sx = x + xo;
            if (sx >= 0 && sx < W) memcpy((char *)out + ((size_t)y * W + x) * es, (const char *)img + ((size_t)sy * stride + sx) * es, es);
        }
    }
    return KM_OK;
}
// what one tracker run touches: both pyramids, the corner list and its count, the two track lists
static void lk_declare(const launch &L, const km_pyr &A, const km_pyr &B, const float *p, const int *d_n, int n_max, bool back, float *p1, float *p0r)
{
    L.pyramid(A); L.pyramid(B);
    L.read(p, (size_t)n_max * 2 * sizeof(float));
    if (d_n) L.read(d_n, sizeof *d_n);
    L.write(p1, (size_t)n_max * 2 * sizeof(float));
    if (back && p0r) L.write(p0r, (size_t)n_max * 2 * sizeof(float));
}
static int track_of(const km_pyr &A, const km_pyr &B, const float *p, const int *d_n, int n_max, bool back, float *p1, float *p0r);
int kl_track(km_ctx *c, const km_pyr &A, const km_pyr &B, const float *p, const int *d_n, int n_max, int, int, double, bool back, float *p1, float *p0r, int *)
{
    const launch L(c, "kl_track");
    lk_declare(L, A, B, p, d_n, n_max, back, p1, p0r);
    return track_of(A, B, p, d_n, n_max, back, p1, p0r);
}
static int track_of(const km_pyr &A, const km_pyr &B, const float *p, const int *d_n, int n_max, bool back, float *p1, float *p0r)
{
    // touch the last pixel of every pyramid level: the level buffers must be as large as the geometry says
    for (int l = 0; l <= A.levels; l++) {
        const int h = A.Hres[l] ? A.Hres[l] : A.H[l], oy = A.Hres[l] ? A.oy[l] : 0;
        volatile uint8_t t = A.img[l][(size_t)(oy + h - 1) * A.W[l] + A.W[l] - 1] ^ B.img[l][(size_t)(oy + h - 1) * B.W[l] + B.W[l] - 1];
        (void)t;
    }
    const int n = d_n ? std::min(*d_n, n_max) : n_max;
    for (int i = 0; i < 2 * n; i++) { p1[i] = p[i] + 0.25f; if (back && p0r) p0r[i] = p[i] + (i % 8 == 0 ? 0.5f : 0.01f); }
    return KM_OK;
}
int kl_oscillation_probe(km_ctx *c, const float *q, int n, uint8_t *out)
{
    { const launch L(c, "kl_oscillation_probe"); L.read(q, (size_t)n * 4 * sizeof(float)); L.write(out, (size_t)n); }
    for (int i = 0; i < n; i++) out[i] = (double)fabsf(q[4 * i] + q[4 * i + 1]) < 0.01 && (double)fabsf(q[4 * i + 2] + q[4 * i + 3]) < 0.01;
    return KM_OK;
}
static void count_kept_of(const float *p0, const float *p0r, const int *d_n, int n_max, float thr, int *cnt)
{
    const int n = std::min(*d_n, n_max);
    int k = 0;
    for (int i = 0; i < n; i++) {
        const float ax = fabsf(p0[2 * i] - p0r[2 * i]), ay = fabsf(p0[2 * i + 1] - p0r[2 * i + 1]);
        k += ((ax > ay || ax != ax) ? ax : ay) < thr;      // (numpy's max: a NaN in either component is the distance)
    }
    *cnt = k;
}
static void count_kept_declare(const launch &L, const float *p0, const float *p0r, const int *d_n, int n_max, int *cnt, so::kind how)
{
    L.read(p0, (size_t)n_max * 2 * sizeof(float)); L.read(p0r, (size_t)n_max * 2 * sizeof(float)); L.read(d_n, sizeof *d_n);
    L.touch(how, cnt, sizeof *cnt);
}
int kf_count_kept(km_ctx *c, const float *p0, const float *p0r, const int *d_n, int n_max, float thr, int *cnt)
{
    const launch L(c, "kf_count_kept");
    count_kept_declare(L, p0, p0r, d_n, n_max, cnt, so::WRITE);
    count_kept_of(p0, p0r, d_n, n_max, thr, cnt);
    return KM_OK;
}
int kf_dn_keep(km_ctx *c, const void *ref, const void *mon, int dtype, int H, int W, ptrdiff_t sref, ptrdiff_t smon, const float *x0, const float *y0, int n, const double *nv,
               int n_no, const double *, const double *, uint8_t *keep)
{
    {
        const launch L(c, "kf_dn_keep");
        L.box(so::READ, ref, dtype_bytes(dtype), H, W, sref); L.box(so::READ, mon, dtype_bytes(dtype), H, W, smon);
        L.read(x0, (size_t)n * sizeof(float)); L.read(y0, (size_t)n * sizeof(float)); L.read(nv, (size_t)n_no * sizeof(double));
        L.write(keep, (size_t)n);
    }
    for (int i = 0; i < n; i++) keep[i] = (x0[i] < 0 || y0[i] < 0 || x0[i] >= W || y0[i] >= H) ? 2 : 1;
    return KM_OK;
}
// frame block: 16-byte header + 6 * cap float32 columns (x0 | y0 | dx | dy | score | index bits); every column written to `cap`
// (k_frame.hip frame_launch: n units' order keys, ranks, staged columns and per-workgroup counts are slices of WS_MISC0 / WS_MISC1 / WS_MISC2 /
// WS_FRAME_CNT; the header takes the flags and the candidate count from the scalar block)
static void frame_unit_declare(const launch &L, const float *p0, const float *p1, const float *p0r, const int *d_n, int n_max, int cap, void *out, const km_scalars *hdr)
{
    const size_t pts = (size_t)n_max * 2 * sizeof(float);
    L.read(p0, pts); L.read(p1, pts); L.read(p0r, pts);
    if (d_n) L.read(d_n, sizeof *d_n);
    if (hdr) { L.fields(so::READ, hdr, SC_FIELD(flags)); L.fields(so::READ, hdr, SC_FIELD(cut)); }
    L.write(out, 16 + (size_t)cap * 6 * sizeof(float));
}
static void frame_scratch(const launch &L, int n, int n_max, int cap)
{
    L.slot(WS_MISC0, up256((size_t)cap * 2 * sizeof(unsigned long long)) * n);
    L.slot(WS_MISC1, up256((size_t)cap * 2 * sizeof(unsigned)) * n);
    L.slot(WS_MISC2, up256((size_t)cap * 5 * sizeof(float)) * n);
    L.slot(WS_FRAME_CNT, up256((size_t)((n_max + 255) / 256) * sizeof(unsigned)) * n);
}
static int frame_of(const float *p0, const float *p1, const float *p0r, const int *d_n, int n_max, int cap, float thr, float xo, float yo, void *out, const km_scalars *hdr);
int kf_frame(km_ctx *c, const float *p0, const float *p1, const float *p0r, const int *d_n, int n_max, int cap, float thr, float xo, float yo, void *out, const km_scalars *hdr, int /*width*/)
{
    const launch L(c, "kf_frame");
    frame_scratch(L, 1, n_max, cap);
    frame_unit_declare(L, p0, p1, p0r, d_n, n_max, cap, out, hdr);
    return frame_of(p0, p1, p0r, d_n, n_max, cap, thr, xo, yo, out, hdr);
}
// the frame stage as the device code defines it (k_frame.hip), in plain loops: d = max(|p0 - p0r|) with numpy's NaN rule (a NaN in either
// component is the distance), the cut d < thr, at most `cap` kept rows (the first in list order), rows behind the count word ignored
// (no count word: n_max rows), then the stable (x0, y0) order with the row's position in the kept list as its label
static int frame_of(const float *p0, const float *p1, const float *p0r, const int *d_n, int n_max, int cap, float thr, float xo, float yo, void *out, const km_scalars *hdr)
{
    const int n = d_n ? std::min(*d_n, n_max) : n_max;
    int *h = (int *)out;
    float *f = (float *)((char *)out + 16);
    for (size_t i = 0; i < (size_t)6 * cap; i++) f[i] = 0.f;
    std::vector<float> col[5];
    for (int i = 0; i < n; i++) {
        const float ax = fabsf(p0[2 * i] - p0r[2 * i]), ay = fabsf(p0[2 * i + 1] - p0r[2 * i + 1]);
        const float d = (ax > ay || ax != ax) ? ax : ay;
        if (!(d < thr) || (int)col[0].size() >= cap) continue;
        col[0].push_back(p0[2 * i] + xo); col[1].push_back(p0[2 * i + 1] + yo);
        col[2].push_back(p1[2 * i] - p0[2 * i]); col[3].push_back(p1[2 * i + 1] - p0[2 * i + 1]);
        col[4].push_back(1.f - d / thr);
    }
    const int k = (int)col[0].size();
    std::vector<int> order((size_t)k);
    for (int i = 0; i < k; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return col[0][a] < col[0][b] || (col[0][a] == col[0][b] && col[1][a] < col[1][b]); });
    for (int i = 0; i < k; i++) {
        const int r = order[(size_t)i];
        for (int c2 = 0; c2 < 5; c2++) f[(size_t)c2 * cap + i] = col[c2][(size_t)r];
        memcpy(&f[(size_t)5 * cap + i], &r, sizeof r);
    }
    h[0] = k; h[1] = n; h[2] = hdr ? (int)hdr->flags : 0; h[3] = hdr ? (int)hdr->cut[3] : 0;
    return KM_OK;
}
int kf_row_checksum(km_ctx *c, const void *d, size_t rb, int rows, unsigned long long *out)
{
    { const launch L(c, "kf_row_checksum"); L.read(d, rb * rows); L.write(out, (size_t)rows * sizeof *out); }
    for (int y = 0; y < rows; y++) {
        const uint8_t *p = (const uint8_t *)d + (size_t)y * rb;
        unsigned long long s = 0;
        for (size_t i = 0; i < rb; i++) s += (unsigned long long)(p[i] + 1u) * (unsigned long long)(2 * i + 1);
        out[y] = s;
    }
    return KM_OK;
}
// what a score kernel touches: the two rasters the chips are cut from, the four key-point columns [and the row count and the score column
// of a frame block], the score column(s) it writes
static void score_declare(const launch &L, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref, ptrdiff_t smon,
                          const float *x0, const float *y0, const float *dx, const float *dy, int n, const int *d_n, const float *score, double *out, double *out2)
{
    L.box(so::READ, ref, dtype_bytes(dtype), Href, Wref, sref);
    L.box(so::READ, mon, dtype_bytes(dtype), Hmon, Wmon, smon);
    for (const float *col : {x0, y0, dx, dy, score}) if (col) L.read(col, (size_t)n * sizeof(float));
    if (d_n) L.read(d_n, sizeof *d_n);
    if (out) L.write(out, (size_t)n * sizeof(double));
    if (out2) L.write(out2, (size_t)n * sizeof(double));
}
// k_mi.hip mi_table: c ln c in the LANE-0 slot WS_MI_TABLE whatever the lane, uploaded on c->stream by the first call that needs it
static void mi_table_declare(const launch &L)
{
    if (!L.live) return;
    km_ctx *c = L.c;
    const int lane = c->lane;
    c->lane = 0;
    const void *tab = km_ws(c, WS_MI_TABLE, (size_t)(57 * 57 + 1) * sizeof(double));
    c->lane = lane;
    L.touch(c->mi_table_ready ? so::READ : so::WRITE, tab, (size_t)(57 * 57 + 1) * sizeof(double));
    c->mi_table_ready = tab != nullptr;
}
int kz_zncc(km_ctx *c, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref, ptrdiff_t smon, const float *x0, const float *y0,
            const float *dx, const float *dy, int n, double *out)
{
    { const launch L(c, "kz_zncc"); score_declare(L, ref, mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, x0, y0, dx, dy, n, nullptr, nullptr, out, nullptr); }
    for (int i = 0; i < n; i++) out[i] = (double)(x0[i] + y0[i] + dx[i] + dy[i]);
    return KM_OK;
}
int kz_zncc_filtered(km_ctx *c, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref, ptrdiff_t smon, const float *x0,
                     const float *y0, const float *dx, const float *dy, int n, const int *d_n, const float *score, float thr, double *out)
{
    { const launch L(c, "kz_zncc_filtered"); score_declare(L, ref, mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, x0, y0, dx, dy, n, d_n, score, out, nullptr); }
    const int m = std::min(*d_n, n);
    for (int i = 0; i < n; i++) out[i] = i < m && score[i] >= thr ? (double)x0[i] : NAN;      // (the whole column: blocks compare byte for byte)
    return KM_OK;
}
int kz_zncc_windows(km_ctx *c, const void *i1, const void *i2, int dt1, int dt2, int H1, int W1, int H2, int W2, ptrdiff_t s1, ptrdiff_t s2, const int *uv, int, int count,
                    double *out, uint8_t *fl)
{
    {
        const launch L(c, "kz_zncc_windows");
        L.box(so::READ, i1, dtype_bytes(dt1), H1, W1, s1); L.box(so::READ, i2, dtype_bytes(dt2), H2, W2, s2);
        L.read(uv, (size_t)count * 4 * sizeof(int)); L.write(out, (size_t)count * sizeof(double)); L.write(fl, (size_t)count);
    }
    for (int i = 0; i < count; i++) { out[i] = uv[4 * i] + uv[4 * i + 3]; fl[i] = 0; }
    return KM_OK;
}
int kmi_batch(km_ctx *c, const void *ref, const void *mon, int dtype, int Href, int Wref, int Hmon, int Wmon, ptrdiff_t sref, ptrdiff_t smon, const float *x0, const float *y0,
              const float *dx, const float *dy, int n, const int *d_n, const float *score, float, double *st, double *nmi)
{
    {
        const launch L(c, "kmi_batch");
        mi_table_declare(L);
        score_declare(L, ref, mon, dtype, Href, Wref, Hmon, Wmon, sref, smon, x0, y0, dx, dy, n, d_n, score, st, nmi);
    }
    for (int i = 0; i < n; i++) { if (st) st[i] = x0[i]; if (nmi) nmi[i] = -x0[i]; }
    return KM_OK;
}
// (the transforms' workspace - the WS_FFT_* / WS_F64_* slots - is used by this launcher alone, on c->stream: the two rasters are what it shares)
int kp_phase_shift(km_ctx *c, const void *a, const void *b, int dtype, int H, int W, ptrdiff_t sa, ptrdiff_t sb, double rc[2])
{
    { const launch L(c, "kp_phase_shift"); L.box(so::READ, a, dtype_bytes(dtype), H, W, sa); L.box(so::READ, b, dtype_bytes(dtype), H, W, sb); }
    rc[0] = px(a, dtype, (size_t)(H - 1) * sa + W - 1) - px(b, dtype, (size_t)(H - 1) * sb + W - 1);
    rc[1] = 0;
    c->phase_path = 1;
    return KM_OK;
}
// (the deferred sum of the Laplacian pass's per-item counts, on whatever stream the caller is on)
int kd_run_valid_sum(km_ctx *c, km_valid_job *job)
{
    if (job->partial) { const launch L(c, "kd_run_valid_sum"); L.read(job->partial, (size_t)job->n * sizeof(unsigned)); L.write(job->out, sizeof *job->out); }
    *job = km_valid_job();
    return KM_OK;
}

// ---- batched units (api_units.hip): every stage touches the first and last byte / element of what the host laid out for it
// (k_raster.hip: the partials of all units in the slot of the caller's choice, one {min, max} pair per workgroup, raster and unit)
int kd_minmax_units(km_ctx *c, const km_units &U, double *const *out, int ws_slot)
{
    {
        const launch L(c, "kd_minmax_units");
        L.slot(ws_slot, (size_t)2 * 1024 * 2 * U.n * sizeof(double));
        for (int u = 0; u < U.n; u++) {
            L.box(so::READ, U.ref[u], dtype_bytes(U.dtype), U.H[u], U.W[u], U.sref[u]);
            L.box(so::READ, U.mon[u], dtype_bytes(U.dtype), U.H[u], U.W[u], U.smon[u]);
            L.write(out[u], 4 * sizeof(double));
        }
    }
    for (int u = 0; u < U.n; u++) {
        minmax_of(U.ref[u], U.dtype, U.H[u], U.W[u], U.sref[u], out[u]);
        minmax_of(U.mon[u], U.dtype, U.H[u], U.W[u], U.smon[u], out[u] + 2);
    }
    return KM_OK;
}
// (k_lap.hip launch_lap_march_units: the per-item counts of valid pixels - with user masks: the per-workgroup counts of the pack launch, 256 a
// unit - go to WS_LAP_VALID, the caller sums them per unit with kd_valid_sum_units; a user mask is read as a strided box and packed into the
// unit's dense mask plane)
int kd_stretch_laplacian_units(km_ctx *c, const km_units &U, int, int, int, const double *, const double *, km_valid_units *job)
{
    const launch L(c, "kd_stretch_laplacian_units");
    size_t item0[KM_UNITS_MAX + 1] = {0};
    for (int u = 0; u < U.n; u++) item0[u + 1] = item0[u] + (U.has_user_mask ? 256 : lap_items(U.H[u], U.W[u]));
    const unsigned *partial = (const unsigned *)L.slot(WS_LAP_VALID, (item0[U.n] + (U.has_user_mask ? 0 : 4 * KM_UNITS_MAX)) * sizeof(unsigned));
    job->n = U.n;
    for (int u = 0; u < U.n; u++) {
        const size_t n = (size_t)U.H[u] * U.W[u];
        L.box(so::READ, U.ref[u], dtype_bytes(U.dtype), U.H[u], U.W[u], U.sref[u]);
        L.box(so::READ, U.mon[u], dtype_bytes(U.dtype), U.H[u], U.W[u], U.smon[u]);
        L.read(U.mm[u], 4 * sizeof(double));
        if (U.has_user_mask) L.box(so::READ, U.user_mask[u], 1, U.H[u], U.W[u], U.user_smask[u]);
        L.write(U.lap_ref[u], n); L.write(U.lap_mon[u], n); L.write(U.mask[u], n);
        for (size_t i = 0; i < n; i++) { U.lap_ref[u][i] = (uint8_t)i; U.lap_mon[u][i] = (uint8_t)(i + 1); U.mask[u][i] = 1; }
        volatile double m = U.mm[u][0] + U.mm[u][3];
        (void)m;
        job->partial[u] = partial ? partial + item0[u] : nullptr; job->n_partial[u] = partial ? (unsigned)(item0[u + 1] - item0[u]) : 0; job->out[u] = &U.sc[u]->valid;
    }
    return KM_OK;
}
int kd_valid_sum_units(km_ctx *c, const km_valid_units &J)
{
    const launch L(c, "kd_valid_sum_units");
    for (int u = 0; u < J.n; u++) {
        if (J.partial[u]) L.read(J.partial[u], (size_t)J.n_partial[u] * sizeof(unsigned));
        L.write(J.out[u], sizeof *J.out[u]);
        *J.out[u] = 12345ull;
    }
    return KM_OK;
}
// (k_eig3.hip launch_eig3_units: per-wave maxima of every unit in WS_PARTIAL, left for the ranking's first launch; of the scalar block the
// shard counters and the overflow word, the sharded running maxima, the tie rows and the development counters)
int k3_eig_candidates_units(km_ctx *c, km_units &U, int, double)
{
    const launch L(c, "k3_eig_candidates_units");
    size_t item0[KM_UNITS_MAX + 1] = {0};
    for (int u = 0; u < U.n; u++) item0[u + 1] = item0[u] + lap_items(U.H[u], U.W[u]);
    const unsigned *partial = (const unsigned *)L.slot(WS_PARTIAL, (item0[U.n] + 16) * sizeof(unsigned));
    for (int u = 0; u < U.n; u++) {
        const size_t n = (size_t)U.H[u] * U.W[u];
        L.read(U.lap_ref[u], n); L.read(U.mask[u], n);
        L.write(U.keys[u], U.capk * sizeof(unsigned long long));
        L.fields(so::WRITE, U.sc[u], offsetof(km_scalars, pad0), offsetof(km_scalars, cut));                  // pad0, shard_cnt
        L.fields(so::WRITE, U.sc[u], SC_FIELD(run_max_shard));
        L.fields(so::WRITE, U.sc[u], offsetof(km_scalars, tie_rows), sizeof(km_scalars));                     // tie_rows .. skip_hit
        U.keys[u][0] = 1ull; U.keys[u][U.capk - 1] = 2ull;
        U.eig_partial[u] = partial ? partial + item0[u] : nullptr; U.eig_npartial[u] = partial ? (unsigned)(item0[u + 1] - item0[u]) : 0;
    }
    return KM_OK;
}
int kd_pyrdown_units(km_ctx *c, const km_units &U, int level)
{
    const launch L(c, "kd_pyrdown_units");
    for (int u = 0; u < U.n; u++) {
        for (const km_pyr *P : {&U.A[u], &U.B[u]}) {
            L.read(P->img[level - 1], (size_t)P->H[level - 1] * P->W[level - 1]);
            L.write(P->img[level], (size_t)P->H[level] * P->W[level]);
        }
    }
    for (int u = 0; u < U.n; u++) {
        uint8_t *a = (uint8_t *)U.A[u].img[level], *b = (uint8_t *)U.B[u].img[level];
        const size_t n = (size_t)U.A[u].H[level] * U.A[u].W[level];
        memset(a, 3, n); memset(b, 4, n);
    }
    return KM_OK;
}
// corners_like_exact (tests/hoststub/frame_main.cpp): the corners the stand-ins of the exact path (kd_min_eigen, kd_candidates, the sort,
// ks_select) find in the unit's Laplacian, so that every form of the kernel-size search must agree; "spec_flag" flags every unit
int kf_rank_select_units(km_ctx *c, const km_units &U, int max_corners, double, double min_distance, int cap)
{
    if (so::on()) {
        // the ranking's first launch reduces the eigenvalue pass's maxima (WS_PARTIAL) into max_eig_key, and the chain goes through every counter
        // of the scalar block behind it
        const launch L(c, "kf_rank_select_units");
        int Hm = 0, Wm = 0;
        for (int u = 0; u < U.n; u++) { Hm = std::max(Hm, U.H[u]); Wm = std::max(Wm, U.W[u]); }
        kf_scratch(L, U.n, Hm, Wm, max_corners, min_distance);
        for (int u = 0; u < U.n; u++) {
            L.read(U.keys[u], U.capk * sizeof(unsigned long long));
            if (U.eig_partial[u]) L.read(U.eig_partial[u], (size_t)U.eig_npartial[u] * sizeof(unsigned));
            L.fields(so::WRITE, U.sc[u], SC_CORNERS);
            L.write(U.p0[u], (size_t)cap * 2 * sizeof(float));
        }
    }
    for (int u = 0; u < U.n && stub().corners_like_exact; u++) {
        const int H = U.H[u], W = U.W[u];
        std::vector<float> eig((size_t)H * W);
        std::vector<unsigned long long> keys((size_t)H * W / 8 + 4096 * KM_NSHARD);
        km_scalars sc = {};
        unsigned max_key;
        unsigned long long *sorted;
        kd_min_eigen(c, U.lap_ref[u], U.mask[u], H, W, 0, eig.data(), &max_key);
        kd_candidates(c, eig.data(), U.mask[u], H, W, 0.0, &sc, keys.data(), keys.size(), false);
        ks_sort_keys_desc(c, keys.data(), std::min((size_t)sc.n_cand, keys.size()), &sorted);
        ks_select(c, sorted, std::min((size_t)sc.n_cand, keys.size()), H, W, max_corners, 0.0, U.p0[u], cap, &sc, nullptr, true);
        U.sc[u]->n_corners = sc.n_corners; U.sc[u]->flags = (unsigned)c->opt_spec_flag;
    }
    if (stub().corners_like_exact) return KM_OK;
    for (int u = 0; u < U.n; u++) {
        const int n = std::min(std::min(max_corners, cap), 40 + u);
        for (int i = 0; i < n; i++) { U.p0[u][2 * i] = (float)(20 + 7 * i % (U.W[u] - 40)); U.p0[u][2 * i + 1] = (float)(20 + 11 * i % (U.H[u] - 40)); }
        U.p0[u][2 * (size_t)cap - 1] = 0.f;
        U.sc[u]->n_corners = n; U.sc[u]->cut[3] = 1000u + (unsigned)u;
    }
    return KM_OK;
}
// per job what kl_track / kf_count_kept do; the knob lk_jobs_unsupported: refused (the search then runs its trackers one by one)
int kl_jobs_launch(km_ctx *c, const km_lk_job *jobs, int n_jobs, int n_max, int win, int max_count, double eps)
{
    if (stub().lk_jobs_unsupported) return KM_E_UNSUPPORTED;
    (void)win; (void)max_count; (void)eps;
    const launch L(c, "kl_jobs_launch");
    L.slot(WS_UNITS_LK, LK_TABLE_ENTRY * KM_LK_JOBS_MAX);      // (k_lk2.hip: the jobs' argument table, uploaded on c->stream)
    for (int j = 0; j < n_jobs; j++) {
        lk_declare(L, jobs[j].A, jobs[j].B, jobs[j].pts_in, jobs[j].d_n, n_max, true, jobs[j].p1, jobs[j].p0r);
        const int rc = track_of(jobs[j].A, jobs[j].B, jobs[j].pts_in, jobs[j].d_n, n_max, true, jobs[j].p1, jobs[j].p0r);
        if (rc) return rc;
    }
    return KM_OK;
}
int kf_count_kept_jobs(km_ctx *c, const km_count_jobs &J, int n_jobs, int n_max, float thr, int *counts)
{
    const launch L(c, "kf_count_kept_jobs");
    for (int j = 0; j < n_jobs; j++) {
        count_kept_declare(L, J.p0[j], J.p0r[j], J.d_n[j], n_max, &counts[j], so::ACCUM);      // (k_frame.hip: counts[j] += ...)
        count_kept_of(J.p0[j], J.p0r[j], J.d_n[j], n_max, thr, &counts[j]);
    }
    return KM_OK;
}
static km_units g_lk_units[2];       // (per workspace lane: a pipelined submission prepares its table before the previous one's LK is launched)
// (k_lk2.hip: the per-unit argument table is uploaded into the lane's WS_UNITS_LK on c->stream; the launch reads it from there)
int kl_units_prepare(km_ctx *c, const km_units &U, int, int, int, double)
{
    const launch L(c, "kl_units_prepare");
    L.slot(WS_UNITS_LK, LK_TABLE_ENTRY * KM_UNITS_MAX);
    g_lk_units[c->lane & 1] = U;
    return KM_OK;
}
int kl_units_launch(km_ctx *c, int n_units, int n_max, int)
{
    const km_units &U = g_lk_units[c->lane & 1];
    const launch L(c, "kl_units_launch");
    if (L.live) L.read(km_ws_peek(c, WS_UNITS_LK), LK_TABLE_ENTRY * KM_UNITS_MAX);
    for (int u = 0; u < n_units; u++) {
        lk_declare(L, U.A[u], U.B[u], U.p0[u], &U.sc[u]->n_corners, n_max, true, U.p1[u], U.p0r[u]);
        const int rc = track_of(U.A[u], U.B[u], U.p0[u], &U.sc[u]->n_corners, n_max, true, U.p1[u], U.p0r[u]);
        if (rc) return rc;
    }
    return KM_OK;
}
int kf_frame_units(km_ctx *c, const km_units &U, int n_max, int cap, float thr)
{
    if (std::min(n_max, cap) > 32768 && U.n != 1) return km_fail(c, KM_E_UNSUPPORTED, "frame: batched units hold at most 32768 rows each");      // (k_frame.hip frame_launch)
    const launch L(c, "kf_frame_units");
    frame_scratch(L, U.n, n_max, cap);
    for (int u = 0; u < U.n; u++) {
        frame_unit_declare(L, U.p0[u], U.p1[u], U.p0r[u], &U.sc[u]->n_corners, n_max, cap, U.frame[u], U.sc[u]);
        const int rc = frame_of(U.p0[u], U.p1[u], U.p0r[u], &U.sc[u]->n_corners, n_max, cap, thr, U.x_off[u], U.y_off[u], U.frame[u], U.sc[u]);
        if (rc) return rc;
    }
    return KM_OK;
}
static void score_units_declare(const launch &L, const km_score_units &A, int n_units, int dtype, int n)
{
    for (int u = 0; u < n_units; u++) {
        const km_score_unit &s = A.u[u];
        score_declare(L, s.ref, s.mon, dtype, s.Href, s.Wref, s.Hmon, s.Wmon, s.sref, s.smon, s.x0, s.y0, s.dx, s.dy, n, s.d_n, s.score, s.out, s.out2);
    }
}
int kz_zncc_units(km_ctx *c, const km_score_units &A, int n_units, int dtype, int n, float thr)
{
    { const launch L(c, "kz_zncc_units"); score_units_declare(L, A, n_units, dtype, n); }
    for (int u = 0; u < n_units; u++) {
        const km_score_unit &s = A.u[u];
        const int m = std::min(*s.d_n, n);
        for (int i = 0; i < n; i++) s.out[i] = i < m && s.score[i] >= thr ? (double)s.x0[i] : NAN;
    }
    return KM_OK;
}
int kmi_units(km_ctx *c, const km_score_units &A, int n_units, int dtype, int n, float)
{
    { const launch L(c, "kmi_units"); mi_table_declare(L); score_units_declare(L, A, n_units, dtype, n); }
    for (int u = 0; u < n_units; u++) {
        const km_score_unit &s = A.u[u];
        const int m = std::min(*s.d_n, n);
        for (int i = 0; i < n; i++) { s.out[i] = i < m ? (double)s.x0[i] : NAN; s.out2[i] = i < m ? -(double)s.x0[i] : NAN; }      // (the whole columns)
    }
    return KM_OK;
}
