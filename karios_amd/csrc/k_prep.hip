// The dense front half of the global align step (karios/matcher/global_align.py:87-108) and the quality check's percentiles
// (karios/api/core.py:491-506): exact order statistics of a raster, the percentile stretch to uint8 and CLAHE.  The arithmetic is
// restated in numpy in tests/prep_restatement.py, which is the definition these kernels are held to bit for bit.
//
// Order statistics: a radix select.  Every pixel becomes a float32 (exact for uint8 / uint16 / int16), its bit pattern an
// order-preserving uint32 key, and three passes over the raster narrow the key by 12 + 10 + 10 bits: pass 1 counts the top 12 bits of
// every kept key, passes 2 and 3 the next 10 bits of the keys under one of up to KP_MAX_RANKS tracked prefixes.  A one-workgroup kernel
// after each pass scans the merged histogram and picks, for every rank wanted, the bin and the rank inside it.  Counters are integers
// (LDS per workgroup, 64-bit global atomics to merge): the result does not depend on any order and is bitwise repeatable.
//
// CLAHE's interpolation is a chain of separately rounded float32 operations (OpenCV's expression, no fused multiply-add): this file
// relies on the library's -ffp-contract=off (csrc/Makefile); one contracted add changes pixels.
#include "k_prep.hpp"
#include "k_prep_select.hpp"   // the key mapping, lds_add_runs, select_pick_kernel: shared with k_report.hip

#include <limits.h>
#include <math.h>

#include <algorithm>
#include <type_traits>

namespace {

template <typename T>
__device__ __forceinline__ bool kept(float f, int exclude)
{
    if constexpr (std::is_same<T, float>::value) {
        const unsigned a = __float_as_uint(f) & 0x7FFFFFFFu;
        return exclude ? a < 0x7F800000u : a <= 0x7F800000u;   // 1: finite only; 0: everything but NaN
    } else {
        return true;
    }
}

template <bool PLAIN>
__device__ __forceinline__ void lds_add(unsigned *h, unsigned idx)
{
    if (PLAIN) {
        if (idx != kNone) atomicAdd(&h[idx], 1u);
    } else {
        lds_add_runs(h, idx);
    }
}

// Pass PASS of the select.  Contiguous 16-byte-aligned rasters are read as one flat run of 16-byte vectors (FLAT); anything else row
// by row, one element per lane.
template <typename T, int PASS, bool PLAIN>
__global__ __launch_bounds__(kSelThreads) void select_pass_kernel(const T *__restrict__ src, ptrdiff_t ss, int H, int W, int flat, int exclude,
                                                                   kp_state *__restrict__ st)
{
    constexpr int NB = PASS == 1 ? KP_NB1 : KP_MAX_RANKS * KP_NB23;
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ unsigned h[NB];
    const int tid = threadIdx.x;
    for (int i = tid; i < NB; i += kSelThreads) h[i] = 0;
    unsigned prefix[KP_MAX_RANKS];
#pragma unroll
    for (int s = 0; s < KP_MAX_RANKS; s++) prefix[s] = PASS == 1 ? kNone : st->prefix[s];
    __syncthreads();

    auto bin = [&](T raw, bool inb) -> unsigned {
        const float f = (float)raw;
        if (!inb || !kept<T>(f, exclude)) return kNone;
        const unsigned k = key_of(f);
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
            u.q = inb ? v4[v] : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int k = 0; k < VEC; k++) lds_add<PLAIN>(h, bin(u.e[k], inb));
        }
        if (blockIdx.x == 0) {   // the n % VEC (< 16) elements behind the last whole vector
            const size_t i = nvec * VEC + tid;
            const bool inb = i < n;
            lds_add<PLAIN>(h, bin(inb ? src[i] : T(0), inb));
        }
    } else {
        const size_t chunks = ((size_t)W + kSelThreads - 1) / kSelThreads, items = (size_t)H * chunks;
        for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
            const size_t y = item / chunks;
            const int x = (int)(item - y * chunks) * kSelThreads + tid;
            const bool inb = x < W;
            lds_add<PLAIN>(h, bin(inb ? src[(ptrdiff_t)y * ss + x] : T(0), inb));
        }
    }
    __syncthreads();
    unsigned long long *g = PASS == 1 ? st->hist1 : PASS == 2 ? &st->hist2[0][0] : &st->hist3[0][0];
    for (int i = tid; i < NB; i += kSelThreads) {
        const unsigned cnt = h[i];
        if (cnt) atomicAdd(&g[i], (unsigned long long)cnt);
    }
}

template <typename T, bool PLAIN>
int select_run(km_ctx *c, const T *d_src, int H, int W, ptrdiff_t ss, int exclude, const kp_q4 &q, int n_q, kp_state *st)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    const bool flat = (ss == W || H == 1) && ((uintptr_t)d_src & 15) == 0;
    const size_t n = (size_t)H * W;
    const size_t work = flat ? n / VEC / kSelThreads + 1 : (size_t)H * (((size_t)W + kSelThreads - 1) / kSelThreads);
    const unsigned blocks = (unsigned)std::min<size_t>(std::max<size_t>(work, 1), kSelMaxBlocks);
    select_pass_kernel<T, 1, PLAIN><<<blocks, kSelThreads, 0, c->stream>>>(d_src, ss, H, W, flat, exclude, st);
    KM_LAUNCH_CHECK(c);
    select_pick_kernel<1><<<1, 256, 0, c->stream>>>(st, q, n_q);
    KM_LAUNCH_CHECK(c);
    select_pass_kernel<T, 2, PLAIN><<<blocks, kSelThreads, 0, c->stream>>>(d_src, ss, H, W, flat, exclude, st);
    KM_LAUNCH_CHECK(c);
    select_pick_kernel<2><<<1, 256, 0, c->stream>>>(st, q, n_q);
    KM_LAUNCH_CHECK(c);
    select_pass_kernel<T, 3, PLAIN><<<blocks, kSelThreads, 0, c->stream>>>(d_src, ss, H, W, flat, exclude, st);
    KM_LAUNCH_CHECK(c);
    select_pick_kernel<3><<<1, 256, 0, c->stream>>>(st, q, n_q);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

// _to_uint8's stretch in float64, every operation rounded on its own; NaN -> 0 (project choice), +inf -> 255, -inf -> 0
template <typename T>
__global__ __launch_bounds__(256) void stretch_kernel(const T *__restrict__ src, ptrdiff_t ss, int H, int W, double lo, double range,
                                                      uint8_t *__restrict__ dst, ptrdiff_t ds)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const double v = (double)(float)src[(ptrdiff_t)y * ss + x];
    double t = v - lo;
    t = t / range;
    t = t * 255.0;
    uint8_t out = 0;                      // NaN fails both comparisons below
    if (t >= 255.0) out = 255;
    else if (t > 0.0) out = (uint8_t)(int)t;
    dst[(ptrdiff_t)y * ds + x] = out;
}

__global__ __launch_bounds__(256) void fill_u8_kernel(uint8_t *__restrict__ dst, ptrdiff_t ds, int H, int W, uint8_t v)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x < W && y < H) dst[(ptrdiff_t)y * ds + x] = v;
}

dim3 grid64x4(int H, int W) { return dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)); }

// ---- CLAHE (OpenCV 4.8 CLAHE_Impl::apply on CV_8UC1) ----------------------------------------------------------------------------------
// Histograms: blockIdx.x = tile, blockIdx.y = slab of the tile's rows; a wave takes a row, its lanes walk along it.  The extended image
// (BORDER_REFLECT_101 on the right and at the bottom) is read through index arithmetic.
__global__ __launch_bounds__(256) void clahe_hist_kernel(const uint8_t *__restrict__ src, ptrdiff_t ss, int H, int W, int tiles_x, int tile_w,
                                                         int tile_h, int rows_per_slab, unsigned *__restrict__ d_hist)
{
    __shared__ unsigned h[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    h[tid] = 0;
    __syncthreads();
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int r0 = blockIdx.y * rows_per_slab, r1 = min(r0 + rows_per_slab, tile_h);
    for (int r = r0 + wave; r < r1; r += 4) {
        const uint8_t *row = src + (ptrdiff_t)km_reflect101(ty * tile_h + r, H) * ss;
        for (int xb = 0; xb < tile_w; xb += 64) {
            const int x = xb + lane;
            const bool inb = x < tile_w;
            const unsigned v = inb ? row[km_reflect101(tx * tile_w + x, W)] : kNone;
            lds_add_runs(h, v);
        }
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&d_hist[(size_t)tile * 256 + tid], h[tid]);
}

// One workgroup per tile: clip, redistribute, cumulative sum, scale (thread i owns bin i)
__global__ __launch_bounds__(256) void clahe_lut_kernel(const unsigned *__restrict__ d_hist, uint8_t *__restrict__ d_lut, int clip, float lut_scale)
{
    __shared__ int s[256];
    __shared__ int s_wave[4];
    const int t = threadIdx.x;
    int v = (int)d_hist[(size_t)blockIdx.x * 256 + t];
    if (clip > 0) {
        int ex = 0;
        if (v > clip) { ex = v - clip; v = clip; }
        for (int o = 32; o > 0; o >>= 1) ex += __shfl_xor(ex, o);
        if ((t & 63) == 0) s_wave[t >> 6] = ex;
        __syncthreads();
        const int clipped = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        const int batch = clipped / 256, residual = clipped - batch * 256;
        v += batch;
        if (residual != 0) {
            const int step = max(256 / residual, 1);   // for (i = 0; i < 256 && residual > 0; i += step, residual--) hist[i]++
            if (t % step == 0 && t / step < residual) v++;
        }
    }
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int add = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const float f = (float)s[t] * lut_scale;          // saturate_cast<uchar>(float): cvRound (half to even), then saturate
    const int iv = (int)rintf(f);
    d_lut[(size_t)blockIdx.x * 256 + t] = (uint8_t)(iv < 0 ? 0 : iv > 255 ? 255 : iv);
}

constexpr int kApplyThreads = 512, kApplyPx = 4;

// Bilinear blend of the four neighbouring tiles' LUTs over the original H x W; all LUTs staged in LDS, byte gathers from there.
// OpenCV's expression, every operation a float32 rounding of its own, in this order.
__global__ __launch_bounds__(kApplyThreads) void clahe_apply_kernel(const uint8_t *__restrict__ src, ptrdiff_t ss, int H, int W,
                                                                    const uint8_t *__restrict__ d_lut, int tiles_x, int tiles_y, float inv_tw,
                                                                    float inv_th, uint8_t *__restrict__ dst, ptrdiff_t ds)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_lut[];
    const int tid = threadIdx.x;
    {
        const int words = tiles_x * tiles_y * 64;   // 256 bytes per tile
        const unsigned *g = reinterpret_cast<const unsigned *>(d_lut);
        unsigned *l = reinterpret_cast<unsigned *>(s_lut);
        for (int i = tid; i < words; i += kApplyThreads) l[i] = g[i];
    }
    __syncthreads();
    constexpr int SEG = kApplyThreads * kApplyPx;
    const size_t segs = ((size_t)W + SEG - 1) / SEG, items = (size_t)H * segs;
    for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int y = (int)(item / segs);
        const int x0 = (int)(item - (size_t)y * segs) * SEG + tid * kApplyPx;
        if (x0 >= W) continue;
        const float tyf = (float)y * inv_th - 0.5f;
        int ty1 = (int)floorf(tyf);
        int ty2 = ty1 + 1;
        const float ya = tyf - (float)ty1, ya1 = 1.0f - ya;
        ty1 = max(ty1, 0);
        ty2 = min(ty2, tiles_y - 1);
        const uint8_t *p1 = s_lut + (size_t)ty1 * tiles_x * 256, *p2 = s_lut + (size_t)ty2 * tiles_x * 256;
        const uint8_t *sp = src + (ptrdiff_t)y * ss + x0;
        uint8_t *dp = dst + (ptrdiff_t)y * ds + x0;
        const int nv = min(kApplyPx, W - x0);
        uint8_t in[kApplyPx], out[kApplyPx];
        if (nv == kApplyPx && ((uintptr_t)sp & 3) == 0) {
            const unsigned w = *reinterpret_cast<const unsigned *>(sp);
            for (int k = 0; k < kApplyPx; k++) in[k] = (uint8_t)(w >> (8 * k));
        } else {
            for (int k = 0; k < kApplyPx; k++) in[k] = k < nv ? sp[k] : 0;
        }
#pragma unroll
        for (int k = 0; k < kApplyPx; k++) {
            const int x = x0 + k;
            const float txf = (float)x * inv_tw - 0.5f;
            int tx1 = (int)floorf(txf);
            int tx2 = tx1 + 1;
            const float xa = txf - (float)tx1, xa1 = 1.0f - xa;
            tx1 = max(tx1, 0);
            tx2 = min(tx2, tiles_x - 1);
            const int i1 = tx1 * 256 + in[k], i2 = tx2 * 256 + in[k];
            const float a = (float)p1[i1] * xa1, b = (float)p1[i2] * xa;
            const float cc = (float)p2[i1] * xa1, d = (float)p2[i2] * xa;
            const float top = (a + b) * ya1, bot = (cc + d) * ya;
            const float res = top + bot;
            const int iv = (int)rintf(res);
            out[k] = (uint8_t)(iv < 0 ? 0 : iv > 255 ? 255 : iv);
        }
        if (nv == kApplyPx && ((uintptr_t)dp & 3) == 0) {
            *reinterpret_cast<unsigned *>(dp) = (unsigned)out[0] | ((unsigned)out[1] << 8) | ((unsigned)out[2] << 16) | ((unsigned)out[3] << 24);
        } else {
            for (int k = 0; k < nv; k++) dp[k] = out[k];
        }
    }
}

}  // namespace

int kp_order_statistics(km_ctx *c, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, int exclude, int n_q, const double *q, kp_state *st,
                        bool plain)
{
    kp_q4 q4;
    for (int j = 0; j < KP_MAX_Q; j++) q4.q[j] = j < n_q ? q[j] : 0.0;
    KM_HIP(c, hipMemsetAsync(st, 0, sizeof(kp_state), c->stream));
    return km_with_pixel_type(c, dtype, "order_statistics: dtype %d (uint8, uint16, int16 and float32 only)", [&](auto t) {
        using T = decltype(t);
#ifdef KM_DEV   // the per-pixel-atomic form exists in the development build only (the A/B of DESIGN 12.1)
        if (plain) return select_run<T, true>(c, (const T *)d_src, H, W, ss, exclude, q4, n_q, st);
#else
        (void)plain;
#endif
        return select_run<T, false>(c, (const T *)d_src, H, W, ss, exclude, q4, n_q, st);
    });
}

int kp_stretch(km_ctx *c, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, double lo, double hi, uint8_t *d_dst, ptrdiff_t ds)
{
    const dim3 g = grid64x4(H, W);
    if (!(hi > lo)) {   // the reference's `if hi > lo ... else zeros` (a NaN percentile lands here too)
        fill_u8_kernel<<<g, 256, 0, c->stream>>>(d_dst, ds, H, W, 0);
        KM_LAUNCH_CHECK(c);
        return KM_OK;
    }
    const double range = hi - lo;
    if (int rc = km_with_pixel_type(c, dtype, "stretch_percentile_u8: dtype %d (uint8, uint16, int16 and float32 only)", [&](auto t) {
            using T = decltype(t);
            stretch_kernel<T><<<g, 256, 0, c->stream>>>((const T *)d_src, ss, H, W, lo, range, d_dst, ds);
            return KM_OK;
        })) return rc;
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kp_clahe_geometry(km_ctx *c, int H, int W, double clip_limit, int tiles_x, int tiles_y, kp_clahe_geom *g)
{
    if (tiles_x < 1 || tiles_y < 1) return km_fail(c, KM_E_ARG, "clahe: tile grid %d x %d", tiles_x, tiles_y);
    if ((long long)tiles_x * tiles_y * 256 > KP_CLAHE_MAX_LUT_BYTES)
        return km_fail(c, KM_E_ARG, "clahe: tile grid %d x %d needs more than %d bytes of LUTs", tiles_x, tiles_y, KP_CLAHE_MAX_LUT_BYTES);
    long long ew = W, eh = H;
    if (W % tiles_x != 0 || H % tiles_y != 0) {   // OpenCV extends BOTH dimensions then: a divisible one by a whole tiles_x / tiles_y
        ew = (long long)W + (tiles_x - W % tiles_x);
        eh = (long long)H + (tiles_y - H % tiles_y);
    }
    if (ew - W > W - 1 || eh - H > H - 1)
        return km_fail(c, KM_E_ARG, "clahe: %d x %d on a %d x %d grid needs a reflected border of %lld x %lld, more than the image holds", H, W,
                       tiles_y, tiles_x, eh - H, ew - W);
    const long long tw = ew / tiles_x, th = eh / tiles_y;
    if (tw < 1 || th < 1) return km_fail(c, KM_E_ARG, "clahe: fewer than one pixel per tile");
    if (tw * th > INT_MAX) return km_fail(c, KM_E_ARG, "clahe: tile of %lld x %lld pixels", th, tw);
    const int area = (int)(tw * th);
    g->tiles_x = tiles_x; g->tiles_y = tiles_y; g->tile_w = (int)tw; g->tile_h = (int)th;
    g->clip = 0;
    if (clip_limit > 0.0) {
        const double cl = clip_limit * area / 256;
        g->clip = cl >= 2147483647.0 ? INT_MAX : std::max((int)cl, 1);
    }
    g->lut_scale = 255.0f / (float)area;
    return KM_OK;
}

int kp_clahe(km_ctx *c, const uint8_t *d_src, int H, int W, ptrdiff_t ss, const kp_clahe_geom &g, unsigned *d_hist, uint8_t *d_lut, uint8_t *d_dst,
             ptrdiff_t ds)
{
    const int tiles = g.tiles_x * g.tiles_y;
    KM_HIP(c, hipMemsetAsync(d_hist, 0, (size_t)tiles * 256 * sizeof(unsigned), c->stream));
    // every tile split by rows over enough workgroups to fill the chip (64 tiles alone would leave three quarters of it idle)
    const int slabs = std::min(std::max((2048 + tiles - 1) / tiles, 1), (g.tile_h + 3) / 4);
    const int rows_per_slab = (g.tile_h + slabs - 1) / slabs;
    const dim3 hg((unsigned)tiles, (unsigned)((g.tile_h + rows_per_slab - 1) / rows_per_slab));
    clahe_hist_kernel<<<hg, 256, 0, c->stream>>>(d_src, ss, H, W, g.tiles_x, g.tile_w, g.tile_h, rows_per_slab, d_hist);
    KM_LAUNCH_CHECK(c);
    clahe_lut_kernel<<<tiles, 256, 0, c->stream>>>(d_hist, d_lut, g.clip, g.lut_scale);
    KM_LAUNCH_CHECK(c);
    const size_t segs = ((size_t)W + kApplyThreads * kApplyPx - 1) / (kApplyThreads * kApplyPx), items = (size_t)H * segs;
    const unsigned blocks = (unsigned)std::min<size_t>(items, 1024);
    clahe_apply_kernel<<<blocks, kApplyThreads, (size_t)tiles * 256, c->stream>>>(d_src, ss, H, W, d_lut, g.tiles_x, g.tiles_y,
                                                                                 1.0f / (float)g.tile_w, 1.0f / (float)g.tile_h, d_dst, ds);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
