// The tracker's iterative outlier clip (karios/matcher/klt.py:52-71) on the device, see k_clip.hpp.  Every float32 operation that decides a
// bit is clip_math.hpp's / accuracy_math.hpp's; the library's -ffp-contract=off and correctly rounded division / square root apply.
//
// clip_units_kernel: unit = blockIdx.y, ONE 256-thread workgroup per unit (the stage runs on the chain stream beside the next submission's
// dense kernels: see FB_T in k_frame.hip for what a larger workgroup costs there), the whole loop inside one launch - no host
// synchronisation, no read-back.  The working set (dx, dy, the row's name; <= 32768 rows) lives in the unit's workspace columns and stays in
// L2.  A round:
//   leaf sums     the leaves of numpy's pairwise tree - 64 of 128 elements per full 8192-block, the leaf table (clip_math.hpp) of the last,
//                 shorter block - one (leaf, column) per lane, eight accumulators each, straight from the columns
//   block sums    one lane per (block, column) combines <= 65 leaf sums along the tree; one lane per column folds the blocks, divides
//   the same for the squared deviations -> the 3-sigma limits
//   compaction    in place, in ascending chunks of 2048 rows (eight per thread): flags, a workgroup-wide exclusive scan of the counts,
//                 the reads of a chunk in front of its barrier and the writes behind it (a chunk writes below its own first row)
// The loop ends when a round keeps every row or none is left, after rows + 1 rounds at the latest (every other round drops a row).
// A frame block is scattered into kept-list order first and compacted (rows, labels, header) at the end, in the same chunked way.
#include "k_clip.hpp"
#include "common.hpp"

static_assert(KC_UNITS_MAX == KM_UNITS_MAX, "units of a clip launch");

namespace {

constexpr int KC_T = 256;
constexpr int KC_PER = KC_CHUNK / KC_T;                // rows a thread takes per chunk of the column compaction
constexpr int KC_FPER = 4;                             // ... of the frame compaction (six columns each)
constexpr int KC_BLOCKS = cl::MAX_ROWS / ac::BLOCK;    // 8192-blocks of a column at most
constexpr int KC_LEAVES = (KC_BLOCKS - 1) * cl::FULL_LEAVES + cl::LEAVES_MAX;   // leaves of a column at most (KC_BLOCKS full blocks hold fewer)
static_assert(KC_PER * KC_T == KC_CHUNK && cl::MAX_ROWS % KC_CHUNK == 0 && KC_BLOCKS * cl::FULL_LEAVES <= KC_LEAVES, "clip geometry");

struct kc_shared {
    unsigned short off[cl::LEAVES_MAX], len[cl::LEAVES_MAX];   // leaf table of the last block
    int nl_last;
    float lsum[2][KC_LEAVES];                                  // leaf sums of dx, dy
    float bsum[2][KC_BLOCKS];
    float mean[2], lim[2];
    int wtot[2][KC_T / 64];                                    // kept rows per wavefront of a chunk (two sets alternate: one barrier per chunk)
};

// sums of both columns (DEV: of their squared deviations) -> s.mean (s.lim).  n > 0; s.nl_last / off / len describe n % 8192
template <bool DEV>
__device__ void kc_stats(kc_shared &s, const float *u, const float *v, int n)
{
    const int tid = threadIdx.x;
    const int nfull = cl::full_blocks_of(n), last = n - nfull * ac::BLOCK, nb = cl::blocks_of(n);
    const int n_leaves = nfull * cl::FULL_LEAVES + (last ? s.nl_last : 0);
    for (int item = tid; item < 2 * n_leaves; item += KC_T) {
        const int col = item & 1, leaf = item >> 1;
        int off = leaf * ac::LEAF, len = ac::LEAF;
        if (leaf >= nfull * cl::FULL_LEAVES) {
            const int k = leaf - nfull * cl::FULL_LEAVES;
            off = nfull * ac::BLOCK + s.off[k]; len = s.len[k];
        }
        s.lsum[col][leaf] = cl::leaf_sum<DEV>((col ? v : u) + off, len, DEV ? s.mean[col] : 0.0f);
    }
    __syncthreads();
    if (tid < 2 * nb) {
        const int col = tid & 1, b = tid >> 1;
        s.bsum[col][b] = cl::combine(s.lsum[col] + b * cl::FULL_LEAVES, b < nfull ? (int)ac::BLOCK : last);
    }
    __syncthreads();
    if (tid < 2) {
        const float sum = ac::fold_blocks(s.bsum[tid], nb);
        if (DEV) s.lim[tid] = cl::limit_of(ac::std_of(sum, n));
        else s.mean[tid] = ac::mean_of(sum, n);
    }
    __syncthreads();
}

// exclusive position of this thread's `cnt` kept rows among the workgroup's of chunk k, and the chunk's total (one barrier inside)
__device__ __forceinline__ int kc_scan(kc_shared &s, int k, int cnt, int &total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (lane == 63) s.wtot[k & 1][wv] = incl;
    __syncthreads();
    int at = incl - cnt;
    total = 0;
#pragma unroll
    for (int w = 0; w < KC_T / 64; w++) { const int t = s.wtot[k & 1][w]; if (w < wv) at += t; total += t; }
    return at;
}

// one round's stable compaction of the working columns -> rows kept.  The columns hold whole chunks (kc_ws_rows)
__device__ int kc_compact(kc_shared &s, float *u, float *v, int32_t *idx, int n)
{
    const float mu = s.mean[0], mv = s.mean[1], lu = s.lim[0], lv = s.lim[1];
    int base = 0;
    for (int c0 = 0, k = 0; c0 < n; c0 += KC_CHUNK, k++) {
        const int e0 = c0 + (int)threadIdx.x * KC_PER;
        float a[KC_PER], b[KC_PER];
        int32_t id[KC_PER];
#pragma unroll
        for (int j = 0; j < KC_PER; j++) { a[j] = u[e0 + j]; b[j] = v[e0 + j]; id[j] = idx[e0 + j]; }
        unsigned keep = 0;
#pragma unroll
        for (int j = 0; j < KC_PER; j++)
            if (e0 + j < n && cl::keeps(a[j], mu, lu, b[j], mv, lv)) keep |= 1u << j;
        int total;
        int at = base + kc_scan(s, k, __popc(keep), total);
#pragma unroll
        for (int j = 0; j < KC_PER; j++)
            if ((keep >> j) & 1u) { u[at] = a[j]; v[at] = b[j]; idx[at] = id[j]; at++; }
        base += total;
    }
    __syncthreads();                                    // the compacted columns are complete before the next round reads them
    return base;
}

__global__ __launch_bounds__(KC_T) void clip_units_kernel(kc_units A)
{
    __shared__ kc_shared s;
    const kc_unit &U = A.u[blockIdx.y];
    float *u = U.u, *v = U.v;
    int32_t *idx = U.idx, *lab = U.lab;
    const int tid = threadIdx.x, cap = U.cap;
    int32_t *hdr = (int32_t *)U.frame;
    float *col = U.frame ? (float *)(U.frame + 16) : nullptr;
    int rows = U.frame ? cl::frame_rows(hdr, cap) : U.n;
    rows = rows < 0 ? 0 : (rows > cl::MAX_ROWS ? (int)cl::MAX_ROWS : rows);      // (the launchers' callers refuse more)
    if (U.frame) {
        // the kept list in corner order: row j of the frame carries its position there in column 5
        for (int l = tid; l < rows; l += KC_T) { u[l] = 0.0f; v[l] = 0.0f; idx[l] = 0; lab[l] = -1; }
        __syncthreads();
        for (int j = tid; j < rows; j += KC_T) {
            const uint32_t l = ac::f32_bits(col[(size_t)5 * cap + j]);
            if (l < (uint32_t)rows) { u[l] = col[(size_t)2 * cap + j]; v[l] = col[(size_t)3 * cap + j]; idx[l] = j; }
        }
    } else {
        for (int i = tid; i < rows; i += KC_T) { u[i] = U.dx[i]; v[i] = U.dy[i]; idx[i] = i; }
    }
    __syncthreads();
    int n = rows, rounds = 0;
    for (int round = 0; round <= rows && n > 0; round++) {
        if (tid == 0) {
            const int last = n % ac::BLOCK;
            s.nl_last = last ? cl::leaf_table(last, s.off, s.len) : 0;
        }
        __syncthreads();
        kc_stats<false>(s, u, v, n);
        kc_stats<true>(s, u, v, n);
        rounds++;
        const int m = kc_compact(s, u, v, idx, n);
        if (m == n) break;
        n = m;
    }
    if (!U.frame) {
        for (int i = tid; i < n; i += KC_T) U.keep_index[i] = idx[i];
    } else if (n != rows) {
        // survivor p of the kept list is frame row idx[p]: its new label.  Then the frame's rows close up, in frame order
        for (int p = tid; p < n; p += KC_T) {
            const uint32_t j = (uint32_t)idx[p];
            if (j < (uint32_t)rows) lab[j] = p;
        }
        __syncthreads();
        int base = 0;
        for (int c0 = 0, k = 0; c0 < rows; c0 += KC_T * KC_FPER, k++) {
            const int e0 = c0 + tid * KC_FPER;
            float val[KC_FPER][5];
            int32_t nl[KC_FPER];
            unsigned keep = 0;
#pragma unroll
            for (int j = 0; j < KC_FPER; j++) {
                nl[j] = e0 + j < rows ? lab[e0 + j] : -1;
                if (nl[j] >= 0) {
                    keep |= 1u << j;
#pragma unroll
                    for (int c2 = 0; c2 < 5; c2++) val[j][c2] = col[(size_t)c2 * cap + e0 + j];
                }
            }
            int total;
            int at = base + kc_scan(s, k, __popc(keep), total);
#pragma unroll
            for (int j = 0; j < KC_FPER; j++)
                if ((keep >> j) & 1u) {
#pragma unroll
                    for (int c2 = 0; c2 < 5; c2++) col[(size_t)c2 * cap + at] = val[j][c2];
                    col[(size_t)5 * cap + at] = ac::bits_f32((uint32_t)nl[j]);
                    at++;
                }
            base += total;
        }
        if (tid == 0) hdr[0] = base;
    }
    if (tid == 0 && U.rec) { U.rec->count = n; U.rec->rounds = rounds; }
}

}  // namespace

int kc_clip_units(km_ctx *c, const kc_units &A, int n_units)
{
    if (n_units <= 0) return KM_OK;
    if (n_units > KC_UNITS_MAX) return km_fail(c, KM_E_ARG, "clip: %d units (1 .. %d per launch)", n_units, KC_UNITS_MAX);
    clip_units_kernel<<<dim3(1, (unsigned)n_units), KC_T, 0, c->stream>>>(A);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
