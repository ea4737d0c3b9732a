// The report's products and the altitude figure's numbers on resident data (karios/report/product_generator.py:138-218,
// karios/api/core.py:1049-1053, karios/report/shift_by_alt_plot.py:127-171); tests/products_restatement.py is the definition,
// products_math.hpp the arithmetic.
//
// Point rasters: one fill pass over the mask and the two bands (16-byte stores over every run of bytes - the whole plane when its rows
// are dense, else row by row - with an element-wide head and tail where a run starts or ends off the 16-byte grid), then the scatter.
// The rows that are out of range are counted, one integer atomic per workgroup; the mask takes its ones in that pass (every writer
// stores the same byte).  The bands need the last row of every pixel: (pixel << 32 | row) through km_sort_u64, the last entry of every
// run of equal pixels stores.
//
// Box statistics: the grouping of k_report.hip - (order key of the group << 32 | row), km_sort_u64, head flags, km_exclusive_scan.
// The values gathered in that order feed numpy's pairwise sum: every 8192-block of a group, counted from the group's first row, is
// summed by the wavefront that holds its first row (a leaf of up to 128 by one lane, a full block as 64 leaves and the butterfly over
// the lanes), the block sums of a group folded left to right.  The row half of the keys is then replaced by the value's order key
// (NaN last) and the same buffers sorted again: every group is a sorted run, read by one lane per group for the percentiles and the
// whisker ends.  The classes go back per row through the row's group index.
#include "k_products.hpp"

#include "common.hpp"

#include <algorithm>

namespace {

constexpr int kT = 256;

// ---- fill
struct fill_plane {
    char *base;                 // null: no plane
    size_t run_bytes;           // bytes of one run
    ptrdiff_t pitch_bytes;      // from run to run
    unsigned n_runs;
    unsigned unit;              // bytes of one element: what the head and the tail are stored by (1 or 4)
    unsigned pattern;           // the element, repeated over 32 bits
    unsigned long long chunks;  // per run: kT 16-byte vectors each, at least one
};
struct fill_plan {
    fill_plane p[3];
};

__global__ __launch_bounds__(kT) void fill_kernel(fill_plan plan, unsigned long long total)
{
    for (unsigned long long item = blockIdx.x; item < total; item += gridDim.x) {
        unsigned long long at = item;
        int k = 0;
        for (; k < 2; k++) {
            const unsigned long long items = plan.p[k].base ? plan.p[k].chunks * plan.p[k].n_runs : 0ull;
            if (at < items) break;
            at -= items;
        }
        const fill_plane &P = plan.p[k];
        const unsigned long long run = at / P.chunks, chunk = at - run * P.chunks;
        char *p = P.base + (ptrdiff_t)run * P.pitch_bytes;
        size_t head = (size_t)(-(uintptr_t)p & 15u);
        if (head > P.run_bytes) head = P.run_bytes;
        const size_t nvec = (P.run_bytes - head) >> 4, tail = P.run_bytes - head - (nvec << 4);
        const size_t v = (size_t)chunk * kT + threadIdx.x;
        if (v < nvec) reinterpret_cast<uint4 *>(p + head)[v] = make_uint4(P.pattern, P.pattern, P.pattern, P.pattern);
        if (chunk == 0) {       // fewer than 16 bytes on either side: the lanes of the run's first chunk store them by elements
            const size_t o = (size_t)threadIdx.x * P.unit;
            char *t = p + head + (nvec << 4);
            if (P.unit == 4) {
                if (o < head) *reinterpret_cast<unsigned *>(p + o) = P.pattern;
                if (o < tail) *reinterpret_cast<unsigned *>(t + o) = P.pattern;
            } else {
                if (o < head) p[o] = (char)P.pattern;
                if (o < tail) t[o] = (char)P.pattern;
            }
        }
    }
}

fill_plane make_plane(void *base, int H, int W, ptrdiff_t stride, unsigned unit, unsigned pattern)
{
    fill_plane P;
    const bool dense = stride == W || H == 1;
    P.base = (char *)base;
    P.run_bytes = (dense ? (size_t)H * W : (size_t)W) * unit;
    P.pitch_bytes = stride * (ptrdiff_t)unit;
    P.n_runs = dense ? 1u : (unsigned)H;
    P.unit = unit;
    P.pattern = pattern;
    P.chunks = std::max<unsigned long long>(((P.run_bytes >> 4) + kT - 1) / kT, 1ull);
    return P;
}

// ---- scatter
// every row: its pixel; the out-of-range count; the mask's ones; the sort keys when a delta raster follows
__global__ __launch_bounds__(kT) void raster_rows_kernel(kpd_rasters r, unsigned long long *__restrict__ keys, int32_t *__restrict__ out_of_range)
{
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const int i = blockIdx.x * kT + threadIdx.x;
    bool bad = false;
    if (i < r.n) {
        const uint32_t px = pm::raster_pixel(r.x0[i], r.y0[i], r.H, r.W);
        bad = px == pm::NO_PIXEL;
        if (keys) keys[i] = ((unsigned long long)px << 32) | (unsigned)i;
        if (!bad && r.mask) r.mask[(ptrdiff_t)(px / (uint32_t)r.W) * r.mask_stride + (ptrdiff_t)(px % (uint32_t)r.W)] = 1;
    }
    const unsigned long long b = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&s_bad, (int)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && s_bad) atomicAdd(out_of_range, s_bad);
}

// sorted keys: the last entry of every run of equal pixels stores its row's dx / dy
__global__ __launch_bounds__(kT) void raster_delta_kernel(kpd_rasters r, const unsigned long long *__restrict__ keys)
{
    const int j = blockIdx.x * kT + threadIdx.x;
    if (j >= r.n) return;
    const unsigned long long k = keys[j];
    const uint32_t px = (uint32_t)(k >> 32);
    if (px == pm::NO_PIXEL || (j + 1 < r.n && (uint32_t)(keys[j + 1] >> 32) == px)) return;
    const uint32_t row = (uint32_t)k;
    float *at = r.delta + (ptrdiff_t)(px / (uint32_t)r.W) * r.row_stride + (ptrdiff_t)(px % (uint32_t)r.W);
    at[0] = r.dx[row];
    at[r.band_stride] = r.dy[row];
}

// ---- sampling
template <typename T>
__global__ __launch_bounds__(kT) void sample_kernel(const T *__restrict__ src, int H, int W, ptrdiff_t stride, int n, const float *__restrict__ x0,
                                                   const float *__restrict__ y0, T *__restrict__ out, int32_t *__restrict__ out_of_range)
{
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const int i = blockIdx.x * kT + threadIdx.x;
    bool bad = false;
    if (i < n) {
        int x, y;
        bad = !(pm::wrapped(x0[i], W, x) && pm::wrapped(y0[i], H, y));
        out[i] = bad ? T(0) : src[(ptrdiff_t)y * stride + x];
    }
    const unsigned long long b = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&s_bad, (int)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && s_bad) atomicAdd(out_of_range, s_bad);
}

// ---- box statistics
struct box_misc {
    float *sorted;        // n: the values in (group, row) order
    int32_t *heads;       // n: first position of every group
    int32_t *group_at;    // n: the group of every position
    int32_t *row_group;   // n: the group of every row, -1 for a dropped one
    float *bsum;          // n: a block's sum at the position of its first row
};

__global__ __launch_bounds__(kT) void box_keys_kernel(const float *__restrict__ positions, int n, float bin, unsigned long long *__restrict__ keys)
{
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    keys[i] = ((unsigned long long)rp::group_key(positions[i], bin) << 32) | (unsigned)i;
}

// sorted keys -> the values in that order, the head flag of every position, the number of rows with a key
__global__ __launch_bounds__(kT) void box_gather_kernel(const unsigned long long *__restrict__ keys, const float *__restrict__ values, int n,
                                                       float *__restrict__ sorted, unsigned *__restrict__ flags, int32_t *__restrict__ counts)
{
    const int j = blockIdx.x * kT + threadIdx.x;
    if (j >= n) return;
    const unsigned long long k = keys[j];
    const unsigned okey = (unsigned)(k >> 32);
    const bool has = okey != rp::DROPPED;
    sorted[j] = has ? values[(unsigned)k] : 0.0f;
    flags[j] = has && (j == 0 || (unsigned)(keys[j - 1] >> 32) != okey) ? 1u : 0u;
    if (has && (j == n - 1 || (unsigned)(keys[j + 1] >> 32) == rp::DROPPED)) counts[KPD_KEPT] = j + 1;   // (one position at the most)
}

// scan[j] = heads in front of position j.  The heads' positions, every position's and every row's group, the groups' keys and number
__global__ __launch_bounds__(kT) void box_heads_kernel(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ scan, int n, box_misc m,
                                                      float *__restrict__ key_out, int32_t *__restrict__ counts)
{
    const int j = blockIdx.x * kT + threadIdx.x;
    if (j >= n) return;
    const unsigned long long k = keys[j];
    const unsigned okey = (unsigned)(k >> 32), row = (unsigned)k;
    if (okey == rp::DROPPED) { m.row_group[row] = -1; return; }
    const bool head = j == 0 || (unsigned)(keys[j - 1] >> 32) != okey;
    const int g = (int)scan[j] - (head ? 0 : 1);
    m.group_at[j] = g;
    m.row_group[row] = g;
    if (head) {
        m.heads[g] = j;
        key_out[g] = rp::key_value(okey);
        atomicMax(&counts[KPD_GROUPS], g + 1);
    }
}

constexpr int BS_STRIDE = ac::LEAF + 4;   // words between the leaves in LDS (k_accuracy.hip: 128-word strides would share their banks)

// one wavefront per 64 positions: every block of 8192 values of a group, counted from the group's head, whose first value lies here
__global__ __launch_bounds__(64) void box_block_sums_kernel(box_misc m, int n, const int32_t *__restrict__ counts)
{
    __shared__ float lds[64 * BS_STRIDE];
    const int kept = counts[KPD_KEPT], groups = counts[KPD_GROUPS];
    const int lane = threadIdx.x, j = blockIdx.x * 64 + lane;
    if (blockIdx.x * 64 >= kept) return;
    int len = 0;
    if (j < kept) {
        const int g = m.group_at[j];
        const int start = m.heads[g], end = g + 1 < groups ? m.heads[g + 1] : kept;
        if ((j - start) % ac::BLOCK == 0) len = end - j < ac::BLOCK ? end - j : ac::BLOCK;
    }
    if (len > 0 && len <= ac::LEAF) m.bsum[j] = ac::leaf_sum(m.sorted + j, len);
    unsigned long long wide = __ballot(len > ac::LEAF);
    while (wide) {                                   // (wave-uniform: the blocks that need the whole wavefront, one after the other)
        const int src = __ffsll((long long)wide) - 1;
        wide &= wide - 1;
        const int blen = __shfl(len, src), first = blockIdx.x * 64 + src;
        const float *a = m.sorted + first;
        if (blen == ac::BLOCK) {
            for (int e = lane; e < ac::BLOCK; e += 64) lds[(e >> 7) * BS_STRIDE + (e & 127)] = a[e];
            __syncthreads();
            float v = ac::leaf_sum(lds + lane * BS_STRIDE, ac::LEAF);
            for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
            if (lane == 0) m.bsum[first] = v;
        } else {
            for (int e = lane; e < blen; e += 64) lds[e] = a[e];
            __syncthreads();
            if (lane == 0) m.bsum[first] = ac::block_sum(lds, blen);
        }
        __syncthreads();
    }
}

// the row half of every kept key becomes the value's order key: the next sort orders the values inside the groups
__global__ __launch_bounds__(kT) void box_rekey_kernel(unsigned long long *__restrict__ keys, const float *__restrict__ sorted, int n)
{
    const int j = blockIdx.x * kT + threadIdx.x;
    if (j >= n) return;
    const unsigned long long k = keys[j];
    if ((unsigned)(k >> 32) == rp::DROPPED) return;
    keys[j] = (k & 0xFFFFFFFF00000000ull) | pm::value_key(sorted[j]);
}

// one lane per group: the block sums folded, the percentiles and the whisker ends out of the sorted run
__global__ __launch_bounds__(64) void box_groups_kernel(const unsigned long long *__restrict__ keys, box_misc m, int n, const int32_t *__restrict__ counts, kpd_box b)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    const int groups = counts[KPD_GROUPS];
    if (g >= groups) return;
    const int start = m.heads[g], end = g + 1 < groups ? m.heads[g + 1] : counts[KPD_KEPT];
    const int cnt = end - start;
    float acc = 0.0f;
    for (int o = start; o < end; o += ac::BLOCK) acc += m.bsum[o];
    b.count[g] = cnt;
    b.mean[g] = ac::mean_of(acc, cnt);
    double st[pm::N_STATS];
    const unsigned long long *run = keys + start;
    pm::box_of_sorted([run](int i) { return (uint32_t)run[i]; }, cnt, st);
#pragma unroll
    for (int s = 0; s < pm::N_STATS; s++) b.stats[(size_t)s * n + g] = st[s];
}

__global__ __launch_bounds__(kT) void box_classes_kernel(const int32_t *__restrict__ row_group, int n, kpd_box b)
{
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int g = row_group[i];
    b.cls[i] = g < 0 ? (int8_t)-1 : pm::flier_class(b.values[i], b.stats[(size_t)pm::WHISLO * n + g], b.stats[(size_t)pm::WHISHI * n + g]);
}

}  // namespace

int kpd_point_rasters(km_ctx *c, const kpd_rasters &r, const kpd_rasters_ws &ws, int32_t *d_out_of_range)
{
    if (r.mask || r.delta) {
        fill_plan plan;
        plan.p[0] = make_plane(r.mask, r.H, r.W, r.mask_stride, 1, 0u);
        plan.p[1] = make_plane(r.delta, r.H, r.W, r.row_stride, 4, pm::NAN_FILL);
        plan.p[2] = make_plane(r.delta ? r.delta + r.band_stride : nullptr, r.H, r.W, r.row_stride, 4, pm::NAN_FILL);
        unsigned long long total = 0;
        for (int k = 0; k < 3; k++) total += plan.p[k].base ? plan.p[k].chunks * plan.p[k].n_runs : 0ull;
        fill_kernel<<<(unsigned)std::min<unsigned long long>(total, 8192ull), kT, 0, c->stream>>>(plan, total);
        KM_LAUNCH_CHECK(c);
    }
    KM_HIP(c, hipMemsetAsync(d_out_of_range, 0, sizeof(int32_t), c->stream));
    if (r.n == 0) return KM_OK;
    const unsigned blocks = (unsigned)((r.n + kT - 1) / kT);
    raster_rows_kernel<<<blocks, kT, 0, c->stream>>>(r, r.delta ? ws.keys_a : nullptr, d_out_of_range);
    KM_LAUNCH_CHECK(c);
    if (!r.delta) return KM_OK;
    int rc;
    if ((rc = km_sort_u64(c, ws.keys_a, ws.keys_b, nullptr, nullptr, (size_t)r.n, false))) return rc;
    raster_delta_kernel<<<blocks, kT, 0, c->stream>>>(r, ws.keys_a);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kpd_sample_points(km_ctx *c, const void *d_raster, int dtype, int H, int W, ptrdiff_t stride, int n, const float *d_x0, const float *d_y0,
                      void *d_out, int32_t *d_out_of_range)
{
    KM_HIP(c, hipMemsetAsync(d_out_of_range, 0, sizeof(int32_t), c->stream));
    return km_with_pixel_type(c, dtype, "sample_points: dtype %d (uint8, uint16, int16 and float32 only)", [&](auto tv) {
        using T = decltype(tv);
        if (n == 0) return (int)KM_OK;
        sample_kernel<T><<<(unsigned)((n + kT - 1) / kT), kT, 0, c->stream>>>((const T *)d_raster, H, W, stride, n, d_x0, d_y0, (T *)d_out, d_out_of_range);
        KM_LAUNCH_CHECK(c);
        return (int)KM_OK;
    });
}

int kpd_box_stats(km_ctx *c, const kpd_box &b, int n, const kpd_box_ws &ws, int32_t *d_counts)
{
    KM_HIP(c, hipMemsetAsync(d_counts, 0, KPD_COUNTS * sizeof(int32_t), c->stream));
    if (n == 0) return KM_OK;
    box_misc m;
    m.sorted = (float *)ws.misc;
    m.heads = (int32_t *)(ws.misc + (size_t)n);
    m.group_at = (int32_t *)(ws.misc + 2 * (size_t)n);
    m.row_group = (int32_t *)(ws.misc + 3 * (size_t)n);
    m.bsum = (float *)(ws.misc + 4 * (size_t)n);
    const unsigned blocks = (unsigned)((n + kT - 1) / kT), waves = (unsigned)((n + 63) / 64);
    int rc;
    box_keys_kernel<<<blocks, kT, 0, c->stream>>>(b.positions, n, (float)b.bin, ws.keys_a);
    KM_LAUNCH_CHECK(c);
    if ((rc = km_sort_u64(c, ws.keys_a, ws.keys_b, nullptr, nullptr, (size_t)n, false))) return rc;
    box_gather_kernel<<<blocks, kT, 0, c->stream>>>(ws.keys_a, b.values, n, m.sorted, ws.flags, d_counts);
    KM_LAUNCH_CHECK(c);
    if ((rc = km_exclusive_scan(c, ws.flags, ws.flags, (size_t)n, KM_SCAN_PLAIN, WS_RP_SCAN))) return rc;
    box_heads_kernel<<<blocks, kT, 0, c->stream>>>(ws.keys_a, ws.flags, n, m, b.key, d_counts);
    KM_LAUNCH_CHECK(c);
    box_block_sums_kernel<<<waves, 64, 0, c->stream>>>(m, n, d_counts);
    KM_LAUNCH_CHECK(c);
    box_rekey_kernel<<<blocks, kT, 0, c->stream>>>(ws.keys_a, m.sorted, n);
    KM_LAUNCH_CHECK(c);
    if ((rc = km_sort_u64(c, ws.keys_a, ws.keys_b, nullptr, nullptr, (size_t)n, false))) return rc;
    box_groups_kernel<<<waves, 64, 0, c->stream>>>(ws.keys_a, m, n, d_counts, b);
    KM_LAUNCH_CHECK(c);
    box_classes_kernel<<<blocks, kT, 0, c->stream>>>(m.row_group, n, b);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
