// Device half of KariosAPI.analyze_accuracy (karios/api/core.py:268-328), see k_accuracy.hpp.  Every float32 operation that decides a
// bit is accuracy_math.hpp's; the library's -ffp-contract=off and correctly rounded division / square root apply.
//   ka_count_valid   one pass over the raster (+ mask): 16-byte loads from any address, integer partial per workgroup, integer sum
//   ka_compact       flag (double)score > thr, exclusive scan (k_sort.hip), ordered scatter of x, +-y, c; NaN count
//   ka_block_sums    one wavefront per 8192-block of a column: a full block is the perfect tree over 64 leaves of 128 - leaf sums by
//                    lanes, then a xor-butterfly (float addition is commutative, so every lane ends with the tree's value); the last,
//                    irregular block walks the header's tree from LDS
//   ka_finish        one lane per column: the block sums left to right, the division, the square root
//   ka_order         one radix sort (k_sort.hip) of the order keys of x, y, c and the radial error, 2^33 apart per column and the rows
//                    beyond the sample behind each column's own: rank r of column j sits at j n_max + r.  Exact ranks, no selection
#include "k_accuracy.hpp"
#include "common.hpp"

namespace {

constexpr int CV_T = 256;            // threads of a counting workgroup
constexpr int CV_CHUNKS = 2;         // 16-byte chunks a thread takes per step

template <typename T> __device__ __forceinline__ unsigned cv_nonzero(T v) { return v != 0 ? 1u : 0u; }
template <> __device__ __forceinline__ unsigned cv_nonzero<float>(float v) { return ac::nonzero_f32_bits(ac::f32_bits(v)) ? 1u : 0u; }

// P = 16 / sizeof(T) pixels from any address (alignment of T): one 16-byte load; the P mask bytes as packed words
template <typename T, bool MASK>
__device__ __forceinline__ unsigned cv_chunk(const T *p, const uint8_t *m)
{
    constexpr int P = 16 / (int)sizeof(T);
    T v[P];
    __builtin_memcpy(v, p, 16);
    uint8_t k[P];
    if (MASK) __builtin_memcpy(k, m, P);
    unsigned n = 0;
#pragma unroll
    for (int i = 0; i < P; i++) n += MASK ? (cv_nonzero(v[i]) & (k[i] ? 1u : 0u)) : cv_nonzero(v[i]);
    return n;
}

// work item = (row, group of CV_T * CV_CHUNKS chunks); a workgroup walks items grid-stride and leaves one partial
template <typename T, bool MASK>
__global__ __launch_bounds__(CV_T) void ka_count_valid_kernel(const T *__restrict__ img, int H, int W, ptrdiff_t stride, const uint8_t *__restrict__ mask,
                                                              ptrdiff_t ms, unsigned groups, unsigned long long *__restrict__ partial)
{
    constexpr int P = 16 / (int)sizeof(T);
    const unsigned long long items = (unsigned long long)H * groups;
    unsigned long long mine = 0;
    for (unsigned long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int y = (int)(it / groups);
        const unsigned g = (unsigned)(it % groups);
        const T *row = img + (ptrdiff_t)y * stride;
        const uint8_t *mrow = MASK ? mask + (ptrdiff_t)y * ms : nullptr;
        unsigned n = 0;
#pragma unroll
        for (int k = 0; k < CV_CHUNKS; k++) {
            const long long x0 = ((long long)(g * CV_CHUNKS + k) * CV_T + threadIdx.x) * P;
            if (x0 + P <= W) n += cv_chunk<T, MASK>(row + x0, MASK ? mrow + x0 : nullptr);
            else
                for (long long x = x0; x < W; x++) n += MASK ? (cv_nonzero(row[x]) & (mrow[x] ? 1u : 0u)) : cv_nonzero(row[x]);
        }
        mine += n;
    }
    __shared__ unsigned long long part[CV_T / 64];
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < CV_T / 64; w++) s += part[w];
        partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(CV_T) void ka_count_sum_kernel(const unsigned long long *__restrict__ partial, unsigned n, unsigned long long *__restrict__ out)
{
    unsigned long long mine = 0;
    for (unsigned i = threadIdx.x; i < n; i += CV_T) mine += partial[i];
    __shared__ unsigned long long part[CV_T / 64];
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < CV_T / 64; w++) s += part[w];
        *out = s;
    }
}

template <typename T>
int count_valid_t(km_ctx *c, const void *d_img, int H, int W, ptrdiff_t stride, const uint8_t *d_mask, ptrdiff_t ms, unsigned long long *d_count)
{
    constexpr int P = 16 / (int)sizeof(T);
    const unsigned per_group = CV_T * CV_CHUNKS * P;
    const unsigned groups = ((unsigned)W + per_group - 1) / per_group;
    const unsigned long long items = (unsigned long long)H * groups;
    const unsigned long long want = (unsigned long long)c->n_cu * 8;
    const unsigned grid = (unsigned)(items < want ? items : want);
    unsigned long long *partial = (unsigned long long *)km_ws(c, WS_AC_PART, (size_t)grid * sizeof(unsigned long long));
    if (!partial) return KM_E_NOMEM;
    if (d_mask) ka_count_valid_kernel<T, true><<<grid, CV_T, 0, c->stream>>>((const T *)d_img, H, W, stride, d_mask, ms, groups, partial);
    else ka_count_valid_kernel<T, false><<<grid, CV_T, 0, c->stream>>>((const T *)d_img, H, W, stride, nullptr, 0, groups, partial);
    KM_LAUNCH_CHECK(c);
    ka_count_sum_kernel<<<1, CV_T, 0, c->stream>>>(partial, grid, d_count);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

// ---- the sample
constexpr int KC_T = 256;

__global__ __launch_bounds__(KC_T) void ka_flag_kernel(const float *__restrict__ score, int n, double thr, unsigned *__restrict__ flag, ka_state *st)
{
    const int i = blockIdx.x * KC_T + threadIdx.x;
    if (i == 0) *st = ka_state();
    if (i < n) flag[i] = ac::above(score[i], thr) ? 1u : 0u;
}

__global__ __launch_bounds__(KC_T) void ka_scatter_kernel(const float *__restrict__ dx, const float *__restrict__ dy, const float *__restrict__ score,
                                                          int n, const unsigned *__restrict__ flag, const unsigned *__restrict__ at, int carto,
                                                          float *__restrict__ cols, ka_state *st)
{
    const int i = blockIdx.x * KC_T + threadIdx.x;
    bool nan = false;
    if (i < n && flag[i]) {
        const unsigned p = at[i];
        const float x = dx[i], y = dy[i];
        cols[p] = x;
        cols[(size_t)n + p] = carto ? -y : y;
        cols[2 * (size_t)n + p] = score[i];
        nan = ac::is_nan(x) || ac::is_nan(y);
    }
    const unsigned long long nans = __ballot(nan);
    if ((threadIdx.x & 63) == 0 && nans) atomicAdd(&st->n_nan, (int)__popcll(nans));
    if (i == n - 1) st->n = (int)(at[i] + flag[i]);
}

// ---- block sums
constexpr int BS_STRIDE = ac::LEAF + 4;   // words between the leaves in LDS: 128-word strides would put every lane's float4 on the same banks

__global__ __launch_bounds__(64) void ka_block_sums_kernel(const float *__restrict__ cols, int n_max, int nb_max, const ka_state *__restrict__ st,
                                                           int dev_sq, float *__restrict__ bsum)
{
    __shared__ float lds[64 * BS_STRIDE];
    const int n = st->n, blk = blockIdx.x, col = blockIdx.y, lane = threadIdx.x;
    const int first = blk * ac::BLOCK;
    if (first >= n) return;
    const int len = n - first < ac::BLOCK ? n - first : ac::BLOCK;
    const float *a = cols + (size_t)col * n_max + first;
    const float mean = st->mean[col];
    if (len == ac::BLOCK) {
        // coalesced float4 loads; element e goes to leaf e / 128 at e % 128
        const float4 *a4 = (const float4 *)a;      // (the columns start 4 n_max bytes apart: 16-byte alignment is not given)
        const bool aligned = (((uintptr_t)a) & 15u) == 0;
        for (int e = lane * 4; e < ac::BLOCK; e += 256) {
            float v[4];
            if (aligned) { const float4 q = a4[e >> 2]; v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
            else { v[0] = a[e]; v[1] = a[e + 1]; v[2] = a[e + 2]; v[3] = a[e + 3]; }
            float *dst = lds + (e >> 7) * BS_STRIDE + (e & 127);
#pragma unroll
            for (int k = 0; k < 4; k++) dst[k] = dev_sq ? ac::dev_sq(v[k], mean) : v[k];
        }
        __syncthreads();
        float v = ac::leaf_sum(lds + lane * BS_STRIDE, ac::LEAF);
        for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
        if (lane == 0) bsum[(size_t)col * nb_max + blk] = v;
    } else {
        for (int e = lane; e < len; e += 64) lds[e] = dev_sq ? ac::dev_sq(a[e], mean) : a[e];
        __syncthreads();
        if (lane == 0) bsum[(size_t)col * nb_max + blk] = ac::block_sum(lds, len);
    }
}

__global__ __launch_bounds__(64) void ka_finish_kernel(const float *__restrict__ bsum, int nb_max, ka_state *st, int dev_sq)
{
    const int col = threadIdx.x;
    if (col >= 3) return;
    const int n = st->n;
    const float s = ac::fold_blocks(bsum + (size_t)col * nb_max, ka_nblocks(n));
    st->sum[col] = s;
    if (n > 0) {
        if (dev_sq) st->std[col] = ac::std_of(s, n);
        else st->mean[col] = ac::mean_of(s, n);
    }
}

// ---- order statistics
__global__ __launch_bounds__(KC_T) void ka_keys_kernel(const float *__restrict__ cols, int n_max, float factor, const ka_state *__restrict__ st,
                                                       unsigned long long *__restrict__ keys)
{
    const int i = blockIdx.x * KC_T + threadIdx.x;
    if (i >= n_max) return;
    const int n = st->n;
    const unsigned long long pad = 1ull << 32;
#pragma unroll
    for (int col = 0; col < 4; col++) {
        unsigned long long k = ((unsigned long long)col << 33) | pad | (unsigned)i;
        if (i < n) {
            const float v = col < 3 ? cols[(size_t)col * n_max + i] : ac::radial(cols[i], cols[(size_t)n_max + i], factor);
            k = ((unsigned long long)col << 33) | ac::order_key(v);
        }
        keys[(size_t)col * n_max + i] = k;
    }
}

__global__ __launch_bounds__(64) void ka_gather_kernel(const unsigned long long *__restrict__ keys, int n_max, ka_percents pc,
                                                       const ka_state *__restrict__ st, km_accuracy_result *__restrict__ out)
{
    const int t = threadIdx.x, n = st->n;
    const float nanv = ac::bits_f32(0x7fc00000u);
    if (t == 0) { out->sample = n; out->n_nan = st->n_nan; out->pad = 0.0f; }
    if (t < 3) {
        const unsigned long long *k = keys + (size_t)t * n_max;
        float *s = out->stats + 5 * t;
        if (n > 0) {
            s[0] = ac::order_value((uint32_t)k[0]);
            s[1] = ac::order_value((uint32_t)k[n - 1]);
            s[2] = (n & 1) ? ac::order_value((uint32_t)k[n / 2])
                           : ac::median_even(ac::order_value((uint32_t)k[n / 2 - 1]), ac::order_value((uint32_t)k[n / 2]));
            s[3] = st->mean[t];
            s[4] = st->std[t];
        } else {
            for (int i = 0; i < 5; i++) s[i] = nanv;
        }
    }
    if (t >= 8 && t < 8 + KM_ACC_MAX_PERCENTS) {
        const int q = t - 8;
        const unsigned long long *k = keys + 3 * (size_t)n_max;
        long long lo, hi;
        const bool ok = q < pc.n && n > 0 && ac::ce_ranks(pc.q[q], n, lo, hi);
        out->order[2 * q] = ok ? ac::order_value((uint32_t)k[lo]) : nanv;
        out->order[2 * q + 1] = ok ? ac::order_value((uint32_t)k[hi]) : nanv;
    }
}

__global__ void ka_empty_kernel(ka_state *st, km_accuracy_result *out)
{
    const float nanv = ac::bits_f32(0x7fc00000u);
    if (st) *st = ka_state();
    if (out) {
        out->sample = 0; out->n_nan = 0; out->pad = 0.0f;
        for (int i = 0; i < 15; i++) out->stats[i] = nanv;
        for (int i = 0; i < 2 * KM_ACC_MAX_PERCENTS; i++) out->order[i] = nanv;
    }
}

}  // namespace

int ka_count_valid(km_ctx *c, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, const uint8_t *d_mask, ptrdiff_t mask_stride,
                   unsigned long long *d_count)
{
    return km_with_pixel_type(c, dtype, "count_valid_pixels: bad dtype %d",
                              [&](auto t) { return count_valid_t<decltype(t)>(c, d_img, H, W, stride, d_mask, mask_stride, d_count); });
}

int ka_compact(km_ctx *c, const float *d_dx, const float *d_dy, const float *d_score, int n_max, double thr, int carto, float *d_cols, ka_state *st)
{
    if (n_max <= 0) {
        ka_empty_kernel<<<1, 1, 0, c->stream>>>(st, nullptr);
        KM_LAUNCH_CHECK(c);
        return KM_OK;
    }
    unsigned *flag = (unsigned *)km_ws(c, WS_AC_FLAG, (size_t)n_max * 2 * sizeof(unsigned));
    if (!flag) return KM_E_NOMEM;
    unsigned *at = flag + n_max;
    const unsigned grid = (unsigned)((n_max + KC_T - 1) / KC_T);
    ka_flag_kernel<<<grid, KC_T, 0, c->stream>>>(d_score, n_max, thr, flag, st);
    KM_LAUNCH_CHECK(c);
    const int rc = km_exclusive_scan(c, flag, at, (size_t)n_max, KM_SCAN_PLAIN, WS_AC_SCAN);
    if (rc) return rc;
    ka_scatter_kernel<<<grid, KC_T, 0, c->stream>>>(d_dx, d_dy, d_score, n_max, flag, at, carto, d_cols, st);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ka_block_sums(km_ctx *c, const float *d_cols, int n_max, const ka_state *st, int dev_sq, float *d_bsum)
{
    if (n_max <= 0) return KM_OK;
    const int nb = ka_nblocks(n_max);
    ka_block_sums_kernel<<<dim3((unsigned)nb, 3), 64, 0, c->stream>>>(d_cols, n_max, nb, st, dev_sq, d_bsum);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ka_finish(km_ctx *c, const float *d_bsum, int n_max, ka_state *st, int dev_sq)
{
    if (n_max <= 0) return KM_OK;
    ka_finish_kernel<<<1, 64, 0, c->stream>>>(d_bsum, ka_nblocks(n_max), st, dev_sq);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ka_order(km_ctx *c, const float *d_cols, int n_max, float factor, ka_percents pc, const ka_state *st, km_accuracy_result *d_out)
{
    if (n_max <= 0) {
        ka_empty_kernel<<<1, 1, 0, c->stream>>>(nullptr, d_out);
        KM_LAUNCH_CHECK(c);
        return KM_OK;
    }
    const size_t nk = (size_t)n_max * 4;
    unsigned long long *k0 = (unsigned long long *)km_ws(c, WS_AC_KEYS0, nk * sizeof(unsigned long long));
    unsigned long long *k1 = (unsigned long long *)km_ws(c, WS_AC_KEYS1, nk * sizeof(unsigned long long));
    if (!k0 || !k1) return KM_E_NOMEM;
    ka_keys_kernel<<<(unsigned)((n_max + KC_T - 1) / KC_T), KC_T, 0, c->stream>>>(d_cols, n_max, factor, st, k0);
    KM_LAUNCH_CHECK(c);
    const int rc = km_sort_u64(c, k0, k1, nullptr, nullptr, nk, false);
    if (rc) return rc;
    ka_gather_kernel<<<1, 64, 0, c->stream>>>(k0, n_max, pc, st, d_out);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
