// The numbers the report step needs of resident data (karios/report/overview_plot.py:134-194, karios/report/commons.py:49-71);
// tests/report_restatement.py is the definition, report_math.hpp the arithmetic.
//
// Display range: the radix select of k_prep.hip (12 + 10 + 10 key bits, three passes, select_pick_kernel after each) with a keep-rule
// of its own: a pixel is kept when it is finite, not zero, its mask byte (if there is a mask) is not zero and it equals none of the
// DN values / the no-data value.  The rule is evaluated in every pass; the first pass also counts the invalid pixels and takes the
// raster's minimum and maximum as order keys.  Every counter is an integer: two runs give the same bits.
//
// Mean profiles: rows -> (order key of the group << 32 | row), km_sort_u64, the values gathered in that order, the group heads
// compacted by a scan; one lane per group then walks its rows in row order carrying pandas' Kahan (float32) and Welford (float64)
// recurrences - the definition's own sequential order.
#include "k_report.hpp"

#include "common.hpp"
#include "k_prep_select.hpp"

#include <algorithm>
#include <type_traits>

namespace {

struct kr_state {
    kp_state sel;
    unsigned long long n_invalid;
    unsigned min_key, max_key;      // order keys; min_key > max_key: no pixel but NaN
};

// Pass PASS of the select under the report's keep-rule.  FLAT: raster (and mask) dense and aligned, read as one run of 16-byte vectors
// of pixels (and the VEC mask bytes beside them); else row by row, one element per lane, the mask at a pitch of its own.
template <typename T, int PASS>
__global__ __launch_bounds__(kSelThreads) void range_pass_kernel(const T *__restrict__ src, ptrdiff_t ss, const uint8_t *__restrict__ mask, ptrdiff_t ms,
                                                                  int H, int W, int flat, rp::tests t, kr_state *__restrict__ st)
{
    constexpr int NB = PASS == 1 ? KP_NB1 : KP_MAX_RANKS * KP_NB23;
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ unsigned h[NB];
    __shared__ unsigned long long s_invalid;
    __shared__ unsigned s_min, s_max;
    const int tid = threadIdx.x;
    for (int i = tid; i < NB; i += kSelThreads) h[i] = 0;
    if (tid == 0) { s_invalid = 0; s_min = 0xFFFFFFFFu; s_max = 0; }
    unsigned prefix[KP_MAX_RANKS];
#pragma unroll
    for (int s = 0; s < KP_MAX_RANKS; s++) prefix[s] = PASS == 1 ? kNone : st->sel.prefix[s];
    __syncthreads();

    unsigned long long my_invalid = 0;
    unsigned my_min = 0xFFFFFFFFu, my_max = 0;

    auto bin = [&](T raw, unsigned mbyte, bool inb) -> unsigned {
        if (!inb) return kNone;
        const bool invalid = mbyte == 0 || rp::listed<T>(raw, t);
        const unsigned k = key_of((float)raw);
        if (PASS == 1) {
            my_invalid += invalid;
            if (!rp::is_nan<T>(raw)) { my_min = min(my_min, k); my_max = max(my_max, k); }
        }
        if (invalid || !rp::countable<T>(raw)) return kNone;
        if (PASS == 1) return k >> (32 - KP_BITS1);
        const unsigned p = PASS == 2 ? k >> (32 - KP_BITS1) : k >> KP_BITS23;
        const unsigned low = PASS == 2 ? (k >> KP_BITS23) & (KP_NB23 - 1) : k & (KP_NB23 - 1);
        unsigned r = kNone;
#pragma unroll
        for (int s = 0; s < KP_MAX_RANKS; s++)
            if (prefix[s] == p) r = (unsigned)s * KP_NB23 + low;   // (prefixes are distinct, unused slots hold kNone)
        return r;
    };

    if (flat) {
        const size_t n = (size_t)H * W, nvec = n / VEC;
        const uint4 *__restrict__ v4 = reinterpret_cast<const uint4 *>(src);
        for (size_t base = (size_t)blockIdx.x * kSelThreads; base < nvec; base += (size_t)gridDim.x * kSelThreads) {
            const size_t v = base + tid;
            const bool inb = v < nvec;
            union { uint4 q; T e[VEC]; } u;
            union { uint4 q; uint2 d; unsigned w; uint8_t b[16]; } m;
            u.q = inb ? v4[v] : make_uint4(0, 0, 0, 0);
            m.q = make_uint4(~0u, ~0u, ~0u, ~0u);
            if (mask && inb) {
                if (VEC == 16) m.q = reinterpret_cast<const uint4 *>(mask)[v];
                else if (VEC == 8) m.d = reinterpret_cast<const uint2 *>(mask)[v];
                else m.w = reinterpret_cast<const unsigned *>(mask)[v];
            }
#pragma unroll
            for (int k = 0; k < VEC; k++) lds_add_runs(h, bin(u.e[k], m.b[k], inb));
        }
        if (blockIdx.x == 0) {   // the n % VEC (< 16) elements behind the last whole vector
            const size_t i = nvec * VEC + tid;
            const bool inb = i < n;
            lds_add_runs(h, bin(inb ? src[i] : T(0), inb && mask ? mask[i] : 1u, inb));
        }
    } else {
        const size_t chunks = ((size_t)W + kSelThreads - 1) / kSelThreads, items = (size_t)H * chunks;
        for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
            const size_t y = item / chunks;
            const int x = (int)(item - y * chunks) * kSelThreads + tid;
            const bool inb = x < W;
            lds_add_runs(h, bin(inb ? src[(ptrdiff_t)y * ss + x] : T(0), inb && mask ? mask[(ptrdiff_t)y * ms + x] : 1u, inb));
        }
    }
    if (PASS == 1) {
        if (my_invalid) atomicAdd(&s_invalid, my_invalid);
        if (my_min <= my_max) { atomicMin(&s_min, my_min); atomicMax(&s_max, my_max); }
    }
    __syncthreads();
    unsigned long long *g = PASS == 1 ? st->sel.hist1 : PASS == 2 ? &st->sel.hist2[0][0] : &st->sel.hist3[0][0];
    for (int i = tid; i < NB; i += kSelThreads) {
        const unsigned cnt = h[i];
        if (cnt) atomicAdd(&g[i], (unsigned long long)cnt);
    }
    if (PASS == 1 && tid == 0) {
        if (s_invalid) atomicAdd(&st->n_invalid, s_invalid);
        if (s_min <= s_max) { atomicMin(&st->min_key, s_min); atomicMax(&st->max_key, s_max); }
    }
}

__global__ void range_finish_kernel(const kr_state *__restrict__ st, kr_range_result *__restrict__ res)
{
    if (threadIdx.x || blockIdx.x) return;
    res->n_valid = st->sel.n;
    res->n_invalid = (long long)st->n_invalid;
    for (int j = 0; j < KR_MAX_Q; j++) { res->vi[j] = st->sel.vi[j]; res->v0[j] = st->sel.v0[j]; res->v1[j] = st->sel.v1[j]; }
    const bool none = st->min_key > st->max_key;
    const float mn = value_of(st->min_key), mx = value_of(st->max_key);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    res->raster_min = none ? nan : mn == 0.0f ? 0.0 : (double)mn;
    res->raster_max = none ? nan : mx == 0.0f ? 0.0 : (double)mx;
}

template <typename T>
int range_run(km_ctx *c, const T *d_src, int H, int W, ptrdiff_t ss, const uint8_t *d_mask, ptrdiff_t ms, const rp::tests &t, const kp_q4 &q, int n_q,
              kr_state *st, kr_range_result *d_res)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    const bool flat = (ss == W || H == 1) && ((uintptr_t)d_src & 15) == 0 && (!d_mask || ((ms == W || H == 1) && ((uintptr_t)d_mask & (VEC - 1)) == 0));
    const size_t n = (size_t)H * W;
    const size_t work = flat ? n / VEC / kSelThreads + 1 : (size_t)H * (((size_t)W + kSelThreads - 1) / kSelThreads);
    const unsigned blocks = (unsigned)std::min<size_t>(std::max<size_t>(work, 1), kSelMaxBlocks);
    range_pass_kernel<T, 1><<<blocks, kSelThreads, 0, c->stream>>>(d_src, ss, d_mask, ms, H, W, flat, t, st);
    KM_LAUNCH_CHECK(c);
    select_pick_kernel<1, std::is_same<T, float>::value><<<1, 256, 0, c->stream>>>(&st->sel, q, n_q);   // (numpy's float32 virtual index)
    KM_LAUNCH_CHECK(c);
    range_pass_kernel<T, 2><<<blocks, kSelThreads, 0, c->stream>>>(d_src, ss, d_mask, ms, H, W, flat, t, st);
    KM_LAUNCH_CHECK(c);
    select_pick_kernel<2><<<1, 256, 0, c->stream>>>(&st->sel, q, n_q);
    KM_LAUNCH_CHECK(c);
    range_pass_kernel<T, 3><<<blocks, kSelThreads, 0, c->stream>>>(d_src, ss, d_mask, ms, H, W, flat, t, st);
    KM_LAUNCH_CHECK(c);
    select_pick_kernel<3><<<1, 256, 0, c->stream>>>(&st->sel, q, n_q);
    KM_LAUNCH_CHECK(c);
    range_finish_kernel<<<1, 64, 0, c->stream>>>(st, d_res);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

// ---- mean profiles
constexpr int kProfThreads = 256;

__global__ __launch_bounds__(kProfThreads) void profile_keys_kernel(const float *__restrict__ positions, int n, float bin, unsigned long long *__restrict__ keys)
{
    const int i = blockIdx.x * kProfThreads + threadIdx.x;
    if (i >= n) return;
    keys[i] = ((unsigned long long)rp::group_key(positions[i], bin) << 32) | (unsigned)i;
}

// sorted keys -> the values in that order, the head flag of every row, the number of rows with a key
__global__ __launch_bounds__(kProfThreads) void profile_gather_kernel(const unsigned long long *__restrict__ keys, const float *__restrict__ values, int n,
                                                                       float *__restrict__ sorted, unsigned *__restrict__ flags, int32_t *__restrict__ counts)
{
    const int j = blockIdx.x * kProfThreads + threadIdx.x;
    if (j >= n) return;
    const unsigned long long k = keys[j];
    const unsigned okey = (unsigned)(k >> 32);
    const bool has = okey != rp::DROPPED;
    sorted[j] = has ? values[(unsigned)k] : 0.0f;
    flags[j] = has && (j == 0 || (unsigned)(keys[j - 1] >> 32) != okey) ? 1u : 0u;
    if (has && (j == n - 1 || (unsigned)(keys[j + 1] >> 32) == rp::DROPPED)) counts[KR_KEPT] = j + 1;   // (one row at the most)
}

// flags scanned in place: a head's word is its group's index.  The heads' positions, the groups' number
__global__ __launch_bounds__(kProfThreads) void profile_heads_kernel(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ gid, int n,
                                                                      int32_t *__restrict__ heads, int32_t *__restrict__ counts)
{
    const int j = blockIdx.x * kProfThreads + threadIdx.x;
    if (j >= n) return;
    const unsigned okey = (unsigned)(keys[j] >> 32);
    if (okey == rp::DROPPED || (j > 0 && (unsigned)(keys[j - 1] >> 32) == okey)) return;
    heads[gid[j]] = j;
    atomicMax(&counts[KR_GROUPS], (int32_t)gid[j] + 1);
}

// one lane per group: its rows in row order through both recurrences
__global__ __launch_bounds__(64) void profile_walk_kernel(const unsigned long long *__restrict__ keys, const float *__restrict__ sorted,
                                                           const int32_t *__restrict__ heads, int32_t *__restrict__ counts, kr_profile p)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    const int groups = counts[KR_GROUPS];
    if (g >= groups) return;
    const int start = heads[g], end = g + 1 < groups ? heads[g + 1] : counts[KR_KEPT];
    rp::accum a = rp::accum_zero();
    int j = start;
    for (; j + 4 <= end; j += 4) {          // (the loads of four rows in flight beside the dependent chain of the recurrences)
        const float x0 = sorted[j], x1 = sorted[j + 1], x2 = sorted[j + 2], x3 = sorted[j + 3];
        rp::accum_add(a, x0); rp::accum_add(a, x1); rp::accum_add(a, x2); rp::accum_add(a, x3);
    }
    for (; j < end; j++) rp::accum_add(a, sorted[j]);
    const float key = rp::key_value((unsigned)(keys[start] >> 32));
    int32_t pos;
    if (!rp::group_position(key, p.bin, pos)) atomicAdd(&counts[KR_OUT_OF_RANGE], 1);
    p.key[g] = key; p.position[g] = pos; p.count[g] = a.n; p.mean[g] = rp::accum_mean(a); p.std[g] = rp::accum_std(a);
}

}  // namespace

size_t kr_range_ws_bytes() { return sizeof(kr_state); }

int kr_display_range(km_ctx *c, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, const uint8_t *d_mask, ptrdiff_t ms, const rp::tests &t,
                     int n_q, const double *q, void *d_ws, kr_range_result *d_res)
{
    kr_state *st = (kr_state *)d_ws;
    kp_q4 q4;
    for (int j = 0; j < KP_MAX_Q; j++) q4.q[j] = j < n_q ? q[j] : 0.0;
    static_assert(KR_MAX_Q == KP_MAX_Q, "one group of quantiles is one selection");
    KM_HIP(c, hipMemsetAsync(st, 0, sizeof(kr_state), c->stream));
    KM_HIP(c, hipMemsetAsync(&st->min_key, 0xFF, sizeof(unsigned), c->stream));
    return km_with_pixel_type(c, dtype, "display_range: dtype %d (uint8, uint16, int16 and float32 only)", [&](auto tv) {
        using T = decltype(tv);
        return range_run<T>(c, (const T *)d_src, H, W, ss, d_mask, ms, t, q4, n_q, st, d_res);
    });
}

int kr_mean_profile(km_ctx *c, const kr_profile &p, int n, const kr_profile_ws &ws, int32_t *d_counts)
{
    KM_HIP(c, hipMemsetAsync(d_counts, 0, KR_COUNTS * sizeof(int32_t), c->stream));
    if (n == 0) return KM_OK;
    const unsigned blocks = (unsigned)((n + kProfThreads - 1) / kProfThreads);
    profile_keys_kernel<<<blocks, kProfThreads, 0, c->stream>>>(p.positions, n, (float)p.bin, ws.keys_a);
    KM_LAUNCH_CHECK(c);
    int rc;
    if ((rc = km_sort_u64(c, ws.keys_a, ws.keys_b, nullptr, nullptr, (size_t)n, false))) return rc;
    float *sorted = (float *)ws.keys_b;                 // keys_b is free once the sort has left its result in keys_a
    int32_t *heads = (int32_t *)(sorted + n);
    profile_gather_kernel<<<blocks, kProfThreads, 0, c->stream>>>(ws.keys_a, p.values, n, sorted, ws.flags, d_counts);
    KM_LAUNCH_CHECK(c);
    if ((rc = km_exclusive_scan(c, ws.flags, ws.flags, (size_t)n, KM_SCAN_PLAIN, WS_RP_SCAN))) return rc;
    profile_heads_kernel<<<blocks, kProfThreads, 0, c->stream>>>(ws.keys_a, ws.flags, n, heads, d_counts);
    KM_LAUNCH_CHECK(c);
    profile_walk_kernel<<<(unsigned)((n + 63) / 64), 64, 0, c->stream>>>(ws.keys_a, sorted, heads, d_counts, p);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
