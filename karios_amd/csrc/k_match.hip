// Brute-force L2 matching of 128-element integer descriptors (cv2.BFMatcher(NORM_L2).knnMatch with k <= 2, reference
// karios/matcher/global_align.py:178-197) and the Lowe / mutual filter behind it (:179-202).  The definition is
// tests/match_restatement.py; every result is exact.
//
// The squared distance of two rows of integers 0 .. 255 is an integer <= 128 * 255^2 < 2^24.  With x' = x - 128 (int8):
//   d2 = |q'|^2 + |t'|^2 - 2 q'.t'      (the offset cancels in the difference)
// and q'.t' is one v_mfma_i32_32x32x32_i8 contraction, exact in int32.  The distance OpenCV ranks by is the float32 nearest to
// sqrt(d2); neighbouring d2 can share one float32 distance, and among equal distances the lower train index wins.  Every candidate is
// therefore a 64-bit key (float bits << 32 | train index): the k best are the k smallest keys, and merging partial results is a
// minimum of keys - order-free, bitwise repeatable.
//
// Operand roles of the MFMA (D = A B, checked with asymmetric data by tests/test_gpu_match.py): A = 32 TRAIN rows (lane l: row l & 31,
// 16 consecutive k of group l >> 5), B = 32 QUERY rows (lane l: query l & 31, the same 16 k).  Both operands take the same 16-byte
// piece of their row, so the order of k inside the instruction does not matter.  D: query on the lane (l & 31), train rows in the 16
// registers: row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  A lane so keeps the running k-best of ITS queries in registers; the two
// half-waves see different train rows of the same query and are merged once at the end.
#include "k_match.hpp"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int KT = 256;                      // threads of a workgroup (4 waves, 64 query rows each)
constexpr int THR_OPEN = 0x1fffffff;         // threshold of a row whose k-th best is still missing (> every real d2)
constexpr int NORM_ABSENT = 0x40000000;      // |t'|^2 of a train row beyond the end: its d2 exceeds THR_OPEN whatever the product holds
constexpr u64 KEY_NONE = ~0ull;

__device__ __forceinline__ u64 make_key(int d2, int j)
{
    // (float)d2 is exact (d2 < 2^24); sqrtf is correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt)
    return ((u64)__float_as_uint(sqrtf((float)d2)) << 32) | (unsigned)j;
}

// The largest integer d with sqrtf(d) <= f (f = the float32 distance of the k-th best): d2 above it has a strictly larger distance and
// cannot enter; d2 at or below it goes through the exact key comparison.  f^2 is within d * 2^-23 <= 1 of every d that rounds to f.
__device__ __forceinline__ int threshold_of(unsigned fbits)
{
    const float f = __uint_as_float(fbits);
    int d = (int)((double)f * (double)f) + 3;
    while (sqrtf((float)d) > f) d--;
    return d;
}

template <int K>
struct best_t {
    u64 b1 = KEY_NONE, b2 = KEY_NONE;
    int thr = THR_OPEN;
    __device__ __forceinline__ void insert(int d2, int j)
    {
        const u64 key = make_key(d2, j);
        if (K == 1) {
            if (key < b1) { b1 = key; thr = threshold_of((unsigned)(key >> 32)); }
        } else {
            if (key < b2) {
                if (key < b1) { b2 = b1; b1 = key; }
                else b2 = key;
                if (b2 != KEY_NONE) thr = threshold_of((unsigned)(b2 >> 32));
            }
        }
    }
};

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int mask)
{
    const unsigned lo = __shfl_xor((unsigned)v, mask), hi = __shfl_xor((unsigned)(v >> 32), mask);
    return ((u64)hi << 32) | lo;
}

// grid (query blocks, chunks of the train rows).  part[(query * nchunks + chunk) * K + rank]
template <int K>
__global__ __launch_bounds__(KT) void knn_kernel(const int8_t *__restrict__ qrows, const int *__restrict__ qnorm, int nq,
                                                 const int8_t *__restrict__ trows, const int *__restrict__ tnorm, int nt, int chunk_rows,
                                                 int nchunks, u64 *__restrict__ part)
{
    __shared__ v4i lds_rows[2][KMT_TILE * 8];   // a row's 16-byte piece c sits at slot c ^ (row & 7): the 32 rows of an A read spread over the banks
    __shared__ int lds_norm[2][KMT_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r = lane & 31;
    const int chunk = blockIdx.y;
    const int t0 = chunk * chunk_rows, t1 = min(nt, t0 + chunk_rows);
    const long long qbase = (long long)blockIdx.x * KMT_QBLOCK + wave * 64;

    // the wave's 64 query rows stay in registers for the whole launch
    v4i bq[2][4];
    int nqv[2];
    best_t<K> best[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const long long qi = min(qbase + s * 32 + r, (long long)nq - 1);
#pragma unroll
        for (int ks = 0; ks < 4; ks++) bq[s][ks] = *(const v4i *)(qrows + qi * KMT_DIM + (ks * 2 + h) * 16);
        nqv[s] = qnorm[qi];
    }

    v4i stage[4];
    int stage_norm = NORM_ABSENT;
    auto load_tile = [&](int start) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = tid + KT * u, row = e >> 3, cc = e & 7;
            const int g = min(start + row, nt - 1);
            stage[u] = *(const v4i *)(trows + (size_t)g * KMT_DIM + cc * 16);
        }
        if (tid < KMT_TILE) stage_norm = start + tid < t1 ? tnorm[start + tid] : NORM_ABSENT;
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = tid + KT * u, row = e >> 3, cc = e & 7;
            lds_rows[buf][row * 8 + (cc ^ (row & 7))] = stage[u];
        }
        if (tid < KMT_TILE) lds_norm[buf][tid] = stage_norm;
    };

    const int ntiles = (t1 - t0 + KMT_TILE - 1) / KMT_TILE;
    if (ntiles > 0) {
        load_tile(t0);
        store_tile(0);
    }
    __syncthreads();
    for (int it = 0; it < ntiles; it++) {
        const int buf = it & 1, start = t0 + it * KMT_TILE;
        if (it + 1 < ntiles) load_tile(start + KMT_TILE);   // in flight under this tile's products
#pragma unroll 1
        for (int g = 0; g < KMT_TILE / 32; g++) {
            const int row = g * 32 + r;
            v4i a[4];
#pragma unroll
            for (int ks = 0; ks < 4; ks++) a[ks] = lds_rows[buf][row * 8 + ((ks * 2 + h) ^ (row & 7))];
            int ntv[16];
#pragma unroll
            for (int reg = 0; reg < 16; reg++) ntv[reg] = lds_norm[buf][g * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h];
#pragma unroll
            for (int s = 0; s < 2; s++) {
                v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < 4; ks++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[ks], bq[s][ks], acc, 0, 0, 0);
                // one branch per 16 elements: the smallest d2 of the lane's column decides whether any of them can enter
                int d2[16], least = 0x7fffffff;
#pragma unroll
                for (int reg = 0; reg < 16; reg++) {
                    d2[reg] = nqv[s] + ntv[reg] - 2 * acc[reg];
                    least = min(least, d2[reg]);
                }
                if (least <= best[s].thr) {
#pragma unroll
                    for (int reg = 0; reg < 16; reg++)
                        if (d2[reg] <= best[s].thr) best[s].insert(d2[reg], start + g * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h);
                }
            }
        }
        if (it + 1 < ntiles) store_tile(buf ^ 1);   // (every wave left that buffer before the barrier that ended the previous tile)
        __syncthreads();
    }

    // the two half-waves hold the same queries over different train rows
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const u64 o1 = shfl_xor_u64(best[s].b1, 32);
        u64 m1 = min(best[s].b1, o1), m2 = max(best[s].b1, o1);
        if (K == 2) {
            const u64 o2 = shfl_xor_u64(best[s].b2, 32);
            m2 = min(m2, min(best[s].b2, o2));
        }
        const long long qi = qbase + s * 32 + r;
        if (h == 0 && qi < nq) {
            u64 *p = part + ((size_t)qi * nchunks + chunk) * K;
            p[0] = m1;
            if (K == 2) p[1] = m2;
        }
    }
}

template <int K>
__global__ __launch_bounds__(256) void knn_merge_kernel(const u64 *__restrict__ part, int nq, int nchunks, int *__restrict__ idx,
                                                        float *__restrict__ dist)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    u64 b1 = KEY_NONE, b2 = KEY_NONE;
    const u64 *p = part + (size_t)q * nchunks * K;
    for (int i = 0; i < nchunks * K; i++) {
        const u64 key = p[i];
        if (key < b1) { b2 = b1; b1 = key; }
        else if (key < b2) b2 = key;
    }
    idx[q * K] = b1 == KEY_NONE ? -1 : (int)(unsigned)b1;
    dist[q * K] = b1 == KEY_NONE ? __uint_as_float(0x7f800000u) : __uint_as_float((unsigned)(b1 >> 32));
    if (K == 2) {
        idx[q * K + 1] = b2 == KEY_NONE ? -1 : (int)(unsigned)b2;
        dist[q * K + 1] = b2 == KEY_NONE ? __uint_as_float(0x7f800000u) : __uint_as_float((unsigned)(b2 >> 32));
    }
}

// 8 threads per row, 16 elements each: rows as int8 x - 128 and the row's sum of (x - 128)^2.  float32 elements must be integers
// 0 .. 255: anything else is counted, its smallest position kept, and packed as 0.
template <typename T>
__global__ __launch_bounds__(256) void pack_kernel(const T *__restrict__ src, int n, ptrdiff_t stride, int8_t *__restrict__ rows,
                                                   int *__restrict__ norm, kmt_state *st, int which)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long row = e >> 3;
    const int piece = (int)(e & 7);
    int sum = 0;
    if (row < n) {
        const T *p = src + row * stride + piece * 16;
        int w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 16; i++) {
            int x;
            if constexpr (sizeof(T) == 1) x = (int)p[i];
            else {
                const float v = p[i];
                const bool ok = v >= 0.f && v <= 255.f && v == truncf(v);   // (NaN fails every comparison)
                if (!ok) {
                    atomicAdd(&st->n_bad[which], 1u);
                    atomicMin(&st->first_bad[which], (u64)row * KMT_DIM + (u64)(piece * 16 + i));
                }
                x = ok ? (int)v : 0;
            }
            const int y = x - 128;
            sum += y * y;
            w[i >> 2] |= (y & 0xff) << (8 * (i & 3));
        }
        *(v4i *)(rows + row * KMT_DIM + piece * 16) = v4i{w[0], w[1], w[2], w[3]};
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    sum += __shfl_xor(sum, 4);
    if (row < n && piece == 0) norm[row] = sum;
}

__global__ void state_reset_kernel(kmt_state *st)
{
    st->first_bad[0] = st->first_bad[1] = KEY_NONE;
    st->n_bad[0] = st->n_bad[1] = 0u;
    st->counts[0] = st->counts[1] = st->counts[2] = 0;
    st->pad = 0;
}

// Lowe's test as Python evaluates it on the two float32 attributes: float64(d1) < ratio * float64(d2), one float64 product
// (-ffp-contract=off); then the mutual check against the backward nearest neighbour.  Grid-stride rows, one pair of atomics per
// workgroup: a counter sustains ~90 atomics per microsecond, one pair per wavefront cost 0.36 ms at 10^6 rows.
__global__ __launch_bounds__(256) void filter_flag_kernel(const int *__restrict__ fwd_idx, const float *__restrict__ fwd_dist,
                                                          const int *__restrict__ bwd_idx, int n_mon, int n_ref, double ratio,
                                                          unsigned *__restrict__ flag, kmt_state *st)
{
    __shared__ int s_lowe, s_mutual;
    if (threadIdx.x == 0) { s_lowe = 0; s_mutual = 0; }
    __syncthreads();
    int n_lowe = 0, n_mutual = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_mon; i += (long long)gridDim.x * blockDim.x) {
        bool lowe = false;
        if (n_ref >= 2) {
            const double limit = ratio * (double)fwd_dist[2 * i + 1];
            lowe = (double)fwd_dist[2 * i] < limit;
        }
        const bool mutual = lowe && bwd_idx[fwd_idx[2 * i]] == (int)i;
        flag[i] = mutual ? 1u : 0u;
        n_lowe += lowe;
        n_mutual += mutual;
    }
    if (n_lowe) atomicAdd(&s_lowe, n_lowe);
    if (n_mutual) atomicAdd(&s_mutual, n_mutual);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_lowe) atomicAdd(&st->counts[1], s_lowe);
        if (s_mutual) atomicAdd(&st->counts[2], s_mutual);
        if (blockIdx.x == 0) st->counts[0] = n_mon;
    }
}

__global__ __launch_bounds__(256) void filter_scatter_kernel(const int *__restrict__ fwd_idx, const float *__restrict__ fwd_dist,
                                                             const unsigned *__restrict__ flag, const unsigned *__restrict__ offs, int n_mon,
                                                             int cap, int *__restrict__ qi, int *__restrict__ ti, float *__restrict__ dist)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_mon || !flag[i]) return;
    const unsigned o = offs[i];
    if (o >= (unsigned)cap) return;
    qi[o] = i;
    ti[o] = fwd_idx[2 * i];
    dist[o] = fwd_dist[2 * i];
}

}  // namespace

int kmt_state_reset(km_ctx *c, kmt_state *st)
{
    state_reset_kernel<<<1, 1, 0, c->stream>>>(st);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kmt_pack(km_ctx *c, const void *d_src, int dtype, int n, ptrdiff_t stride, void *d_dst, kmt_state *st, int which, kmt_packed *out)
{
    int8_t *rows = (int8_t *)d_dst;
    int *norm = (int *)(rows + (((size_t)n * KMT_DIM + 255) & ~(size_t)255));
    const unsigned blocks = (unsigned)(((size_t)n * 8 + 255) / 256);
    if (dtype == KM_U8) pack_kernel<uint8_t><<<blocks, 256, 0, c->stream>>>((const uint8_t *)d_src, n, stride, rows, norm, st, which);
    else if (dtype == KM_F32) pack_kernel<float><<<blocks, 256, 0, c->stream>>>((const float *)d_src, n, stride, rows, norm, st, which);
    else return km_fail(c, KM_E_ARG, "descriptor dtype %d (uint8 and float32 only)", dtype);
    KM_LAUNCH_CHECK(c);
    out->rows = rows; out->norm = norm; out->n = n;
    return KM_OK;
}

// A grid of query blocks alone fills the device only for large n_q: the train rows are split until about four workgroups per CU
// exist; a chunk is a whole number of tiles.
static void chunking(const km_ctx *c, int n_q, int n_t, int *chunk_rows, int *nchunks)
{
    const long long blocks = ((long long)n_q + KMT_QBLOCK - 1) / KMT_QBLOCK;
    const long long tiles = ((long long)n_t + KMT_TILE - 1) / KMT_TILE;
    long long want = (4ll * c->n_cu + blocks - 1) / blocks;
    if (want > tiles) want = tiles;
    if (want > KMT_MAX_CHUNKS) want = KMT_MAX_CHUNKS;
    if (want < 1) want = 1;
    const long long per = (tiles + want - 1) / want;
    *chunk_rows = (int)(per * KMT_TILE);
    *nchunks = (int)((tiles + per - 1) / per);
}

int kmt_chunks(const km_ctx *c, int n_q, int n_t)
{
    int rows, n;
    chunking(c, n_q, n_t, &rows, &n);
    return n;
}

int kmt_knn(km_ctx *c, const kmt_packed &q, const kmt_packed &t, int k, unsigned long long *d_part, int *d_idx, float *d_dist)
{
    if (q.n <= 0 || t.n <= 0) return km_fail(c, KM_E_INTERNAL, "knn: empty descriptor set");
    int chunk_rows, nchunks;
    chunking(c, q.n, t.n, &chunk_rows, &nchunks);
    const dim3 grid((unsigned)((q.n + KMT_QBLOCK - 1) / KMT_QBLOCK), (unsigned)nchunks);
    const unsigned mblocks = (unsigned)((q.n + 255) / 256);
    if (k == 1) {
        knn_kernel<1><<<grid, KT, 0, c->stream>>>(q.rows, q.norm, q.n, t.rows, t.norm, t.n, chunk_rows, nchunks, d_part);
        KM_LAUNCH_CHECK(c);
        knn_merge_kernel<1><<<mblocks, 256, 0, c->stream>>>(d_part, q.n, nchunks, d_idx, d_dist);
    } else {
        knn_kernel<2><<<grid, KT, 0, c->stream>>>(q.rows, q.norm, q.n, t.rows, t.norm, t.n, chunk_rows, nchunks, d_part);
        KM_LAUNCH_CHECK(c);
        knn_merge_kernel<2><<<mblocks, 256, 0, c->stream>>>(d_part, q.n, nchunks, d_idx, d_dist);
    }
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kmt_filter(km_ctx *c, const int *d_fwd_idx, const float *d_fwd_dist, const int *d_bwd_idx, int n_mon, int n_ref, double ratio, unsigned *d_flag,
               int cap, int *d_qi, int *d_ti, float *d_dist, kmt_state *st)
{
    const unsigned blocks = (unsigned)((n_mon + 255) / 256);
    unsigned *d_offs = d_flag + n_mon;
    filter_flag_kernel<<<blocks < 1024u ? blocks : 1024u, 256, 0, c->stream>>>(d_fwd_idx, d_fwd_dist, d_bwd_idx, n_mon, n_ref, ratio, d_flag, st);
    KM_LAUNCH_CHECK(c);
    int rc;
    if ((rc = km_exclusive_scan(c, d_flag, d_offs, (size_t)n_mon, KM_SCAN_PLAIN, WS_MT_SCAN))) return rc;
    filter_scatter_kernel<<<blocks, 256, 0, c->stream>>>(d_fwd_idx, d_fwd_dist, d_flag, d_offs, n_mon, cap, d_qi, d_ti, d_dist);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
