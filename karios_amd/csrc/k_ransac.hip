// Kernels of the RANSAC homography (k_ransac.hpp).  Every formula is ransac_math.hpp's, compiled here for the device.
#include "k_ransac.hpp"
#include "ransac_math.hpp"

namespace {

struct krs_model { float h[9]; };

__global__ __launch_bounds__(256) void pack_kernel(const float *__restrict__ src, ptrdiff_t ss, const float *__restrict__ dst, ptrdiff_t sd, int n,
                                                   float4 *__restrict__ pairs)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *s = src + (size_t)i * ss, *d = dst + (size_t)i * sd;
    pairs[i] = make_float4(s[0], s[1], d[0], d[1]);
}

// One lane's working set of the eigen-solver, strided through LDS: element i of lane t sits at word i * 64 + t, so the 64 lanes of
// a (divergent) wave read 64 neighbouring words whatever subscripts they computed.  Private memory would serve too, but every
// rotation is a chain of dependent accesses with computed subscripts and the launch lasts as long as one such chain.
struct lds_store {
    double *d;   // 171 doubles a lane: A 81, V 81, W 9
    int *n;      // 18 ints a lane: indR 9, indC 9
    __device__ double &a(int i) { return d[i * 64]; }
    __device__ double &v(int i) { return d[(81 + i) * 64]; }
    __device__ double &w(int i) { return d[(162 + i) * 64]; }
    __device__ int &r(int i) { return n[i * 64]; }
    __device__ int &c(int i) { return n[(9 + i) * 64]; }
};

// kernel A: one iteration per lane, one wave per workgroup (its working sets fill 92 KB of LDS).  The 9 x 9 Jacobi iteration is
// divergent and short; it is bounded by its 30 n^2 rotations (rs::jacobi).
__global__ __launch_bounds__(64) void solve_kernel(const float4 *__restrict__ pairs, const int4 *__restrict__ idx, int first, int count,
                                                   double *__restrict__ H64, float *__restrict__ Hf, int *__restrict__ valid, int *__restrict__ counts)
{
    __shared__ double sd[171 * 64];
    __shared__ int sn[18 * 64];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    lds_store st = {sd + threadIdx.x, sn + threadIdx.x};
    const size_t it = (size_t)first + i;
    const int4 id = idx[it];
    const int ids[4] = {id.x, id.y, id.z, id.w};
    float M[8], m[8];
    for (int k = 0; k < 4; k++) {
        const float4 p = pairs[ids[k]];
        M[2 * k] = p.x; M[2 * k + 1] = p.y; m[2 * k] = p.z; m[2 * k + 1] = p.w;
    }
    double H[9];
    const int ok = rs::dlt(M, m, 4, H, st);
    for (int k = 0; k < 9; k++) {
        H64[it * 9 + k] = ok ? H[k] : 0.;
        Hf[it * KRS_HSTRIDE + k] = ok ? (float)H[k] : __builtin_nanf("");
    }
    valid[it] = ok;
    counts[it] = 0;
}

// kernel B: a workgroup = KRS_TILE pairs (a lane holds KRS_PTS of them in registers) x `hc` iterations.  The coefficients of an
// iteration are wave-uniform (scalar loads from the table); the inliers of a wave are a ballot + population count per pair slot,
// kept by lane (iteration - h0); one LDS add per lane and one global integer atomic per (workgroup, iteration) at the end.
__global__ __launch_bounds__(KRS_BLOCK) void score_kernel(const float4 *__restrict__ pairs, int n, const float *__restrict__ Hf, int first, int count,
                                                          int hc, float thr, int *__restrict__ counts)
{
    __shared__ int acc[KRS_HC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < KRS_HC) acc[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * KRS_TILE + (long long)wave * KRS_WAVE_PAIRS;
    float x[KRS_PTS], y[KRS_PTS], mx[KRS_PTS], my[KRS_PTS];
#pragma unroll
    for (int p = 0; p < KRS_PTS; p++) {
        const long long i = base + p * 64 + lane;
        // a slot beyond n holds NaN: its error is NaN and never passes err <= thr
        float4 v = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
        if (i < n) v = pairs[i];
        x[p] = v.x; y[p] = v.y; mx[p] = v.z; my[p] = v.w;
    }
    const int h0 = blockIdx.y * hc, h1 = h0 + hc < count ? h0 + hc : count;
    int mine = 0;
    if (base < n) {
        for (int h = h0; h < h1; h++) {
            const float *H = Hf + (size_t)(first + h) * KRS_HSTRIDE;
            int cnt = 0;
#pragma unroll
            for (int p = 0; p < KRS_PTS; p++) cnt += __popcll(__ballot(rs::reproj_err(H, x[p], y[p], mx[p], my[p]) <= thr));
            mine = lane == h - h0 ? cnt : mine;
        }
        if (mine) atomicAdd(&acc[lane], mine);
    }
    __syncthreads();
    if ((int)threadIdx.x < h1 - h0 && acc[threadIdx.x]) atomicAdd(&counts[first + h0 + threadIdx.x], acc[threadIdx.x]);
}

// kernel C: the winner's mask, the same expression
__global__ __launch_bounds__(256) void mask_kernel(const float4 *__restrict__ pairs, int n, krs_model H, float thr, uint8_t *__restrict__ mask,
                                                   int *__restrict__ total)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool in = false;
    if (i < n) {
        const float4 v = pairs[i];
        in = rs::reproj_err(H.h, v.x, v.y, v.z, v.w) <= thr;
        mask[i] = in ? 1 : 0;
    }
    const int cnt = __popcll(__ballot(in));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(total, cnt);
}

}  // namespace

int krs_pack(km_ctx *c, const float *d_src, ptrdiff_t ss, const float *d_dst, ptrdiff_t sd, int n, float *d_pairs)
{
    pack_kernel<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(d_src, ss, d_dst, sd, n, (float4 *)d_pairs);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int krs_solve(km_ctx *c, const float *d_pairs, int n, const int *d_idx, int first, int count, double *d_H64, float *d_Hf, int *d_valid, int *d_count)
{
    (void)n;
    solve_kernel<<<(unsigned)((count + 63) / 64), 64, 0, c->stream>>>((const float4 *)d_pairs, (const int4 *)d_idx, first, count, d_H64, d_Hf, d_valid, d_count);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int krs_score(km_ctx *c, const float *d_pairs, int n, const float *d_Hf, int first, int count, float thr, int *d_count)
{
    const long long tiles = ((long long)n + KRS_TILE - 1) / KRS_TILE;
    const long long waves = ((long long)n + KRS_WAVE_PAIRS - 1) / KRS_WAVE_PAIRS;
    // KRS_HC iterations per wave when that still gives every SIMD a wave, KRS_HC_SMALL otherwise
    const int hc = waves * ((count + KRS_HC - 1) / KRS_HC) >= 4ll * c->n_cu ? KRS_HC : KRS_HC_SMALL;
    const dim3 grid((unsigned)tiles, (unsigned)((count + hc - 1) / hc));
    score_kernel<<<grid, KRS_BLOCK, 0, c->stream>>>((const float4 *)d_pairs, n, d_Hf, first, count, hc, thr, d_count);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int krs_mask(km_ctx *c, const float *d_pairs, int n, const float *Hf, float thr, uint8_t *d_mask, int *d_total)
{
    krs_model H;
    for (int k = 0; k < 9; k++) H.h[k] = Hf[k];
    KM_HIP(c, hipMemsetAsync(d_total, 0, sizeof(int), c->stream));
    mask_kernel<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>((const float4 *)d_pairs, n, H, thr, d_mask, d_total);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
