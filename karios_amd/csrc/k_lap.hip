// K2 of the KARIOS matching path (gfx950): uint8 stretch -> Laplacian -> auto mask (klt.py:42-49, 268-273, 433-434) in two forms - the
// LDS-tiled general form and the marching form (one wavefront per column strip; the only inline assembly of the dense stages) - and
// the launch plan that chooses between them.  Integer-exact arithmetic, no MFMA.  The marching kernel - like the fused K3+K4
// (k_eig3.hip) and the integer ZNCC / MI kernels (k_zncc.hip, k_mi.hip) - is written for a batch of units (km_units, api_units.hip);
// a single tile or pair runs as a batch of one unit.
#include "k_pixel.hpp"
#include "lap_coef.hpp"
#include "lap_items.hpp"

#include <algorithm>

// occupancy target of the marching Laplacian kernel (waves per SIMD; 0 = leave it to the register allocator)
#ifndef KM_LAPM_WAVES
#define KM_LAPM_WAVES 0
#endif
#if KM_LAPM_WAVES
#define KM_LAPM_OCC __attribute__((amdgpu_waves_per_eu(KM_LAPM_WAVES, KM_LAPM_WAVES)))
#else
#define KM_LAPM_OCC
#endif

// ------------------------------------------------------------------ K2 stretch + Laplacian (+mask)
// Output tile 128x16 per 256-thread workgroup.  The Laplacian of odd ksize k is written as
//   sum_j ks[j] * (kd *x u8)[y+j] + kd[j] * (ks *x u8)[y+j]
// (ksize 1 and 3 fit the same form with kd=[1,-2,1] and ks=[0,1,0] / [1,2,1]); both images use
// radius R = max of the two, the shorter kernel zero-padded, so one launch serves mixed sizes.
//
// uint8 stretch of 16-bit integer images without a per-pixel fp64 division: numpy computes
// trunc(fl(fl(d/r)*255)) with d = v - min, r = max - min (integers).  When 255*d is not a multiple of r the exact
// quotient 255*d/r lies >= 1/r from any integer, far more than the fp64 rounding error, so the result is
// floor(255*d/r).  When 255*d == k*r the real quotient d/r equals k/255, the correctly rounded division gives
// fl(k/255) whatever d and r are, and fl(fl(k/255)*255) >= k holds for every k in 0..255 (256 cases, checked by
// tests/test_host_logic.py::test_stretch_exact_multiples) - again floor(255*d/r).  The kernels evaluate that floor as
//   (int) fma((double)d, 255/r, 0.5/r)
// : (255*d + 0.5)/r is never an integer, has the same floor, and stays >= 0.5/r >= 7.6e-6 away from the integers,
// eleven orders of magnitude above the fma's rounding error - three full-rate instructions, no branch, no table.
#define LAP_TW 128
#define LAP_TH 16

template <typename T> struct stretcher {
    // generic (f32 / u8): arithmetic path
    double mn, range;
    bool deg;
    __device__ void init(const double *mm, int img, const uint8_t *) {
        if constexpr (sizeof(T) == 1) { mn = 0; range = 1; deg = false; }
        else { mn = mm[2 * img]; const double mx = mm[2 * img + 1]; range = mx - mn; deg = !(mx > mn); }
    }
    __device__ __forceinline__ unsigned operator()(T v, const uint8_t *) const { return stretch_u8<T>(v, mn, range, deg); }
};
template <typename T> struct stretcher_i16 {
    int mn_i;
    double c1, c0;
    __device__ void init(const double *mm, int img, const uint8_t *) {
        const double mn = mm[2 * img], mx = mm[2 * img + 1];
        mn_i = (int)mn;
        if (mx > mn) { const double r = mx - mn; c1 = 255.0 / r; c0 = 0.5 / r; }
        else { c1 = 0.0; c0 = 0.0; }                     // degenerate range: every pixel maps to 0
    }
    __device__ __forceinline__ unsigned operator()(T v, const uint8_t *) const {
        return (unsigned)(int)__fma_rn((double)((int)v - mn_i), c1, c0);
    }
};
template <> struct stretcher<uint16_t> : stretcher_i16<uint16_t> {};
template <> struct stretcher<int16_t> : stretcher_i16<int16_t> {};

template <int R, typename T, int NIMG, bool MASK>
__global__ __launch_bounds__(256) void lap_kernel(const T *__restrict__ img0, const T *__restrict__ img1, int H, int W,
                                                  ptrdiff_t stride0, ptrdiff_t stride1, const double *__restrict__ mm,
                                                  lap_coef cf, int invert1, nodata_t nd,
                                                  uint8_t *__restrict__ out0, uint8_t *__restrict__ out1,
                                                  uint8_t *__restrict__ mask_out, unsigned *__restrict__ valid_partial)
{
    using HT = typename std::conditional<(R <= 3), short, int>::type;  // |kd*x| <= 3060, ks*x <= 16320 for k <= 7
    constexpr int HX = (R + 3) & ~3;          // x halo rounded to 4 for packed LDS words
    constexpr int TWH = LAP_TW + 2 * HX;      // LDS tile row length (bytes)
    constexpr int THH = LAP_TH + 2 * R;
    constexpr int CPR = TWH / 4;              // 4-pixel chunks per row
    constexpr int NQ = LAP_TW / 4;            // output quads per row
    constexpr int NIT = (THH * CPR + 255) / 256;
    __shared__ uint32_t tile[NIMG][THH][CPR];
    __shared__ __attribute__((aligned(16))) HT hbuf[2][NIMG][THH][LAP_TW];  // [0] = kd pass, [1] = ks pass
    auto &hd = hbuf[0];
    auto &hs = hbuf[1];
    const int X0 = blockIdx.x * LAP_TW, Y0 = blockIdx.y * LAP_TH;
    const int tid = threadIdx.x;
    stretcher<T> st[NIMG];
#pragma unroll
    for (int i = 0; i < NIMG; i++) st[i].init(mm, i, nullptr);
    const T *imgs[2] = {img0, img1};
    const ptrdiff_t strides[2] = {stride0, stride1};

    // ---- phase 1a: issue every global load of this thread (raw tile + halo, REFLECT_101)
    T v[NIT][NIMG][4];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int ci = it * 256 + tid;
        if (ci < THH * CPR) {
            const int row = ci / CPR, cx = ci - row * CPR;
            const int gy = km_reflect101(Y0 - R + row, H);
            const int gx0 = X0 - HX + cx * 4;
            const bool inside = gx0 >= 0 && gx0 + 3 < W;
#pragma unroll
            for (int i = 0; i < NIMG; i++) {
                const T *rowp = imgs[i] + (size_t)gy * strides[i];
                if (inside && ((((uintptr_t)(rowp + gx0)) & (4 * sizeof(T) - 1)) == 0)) {
                    if constexpr (sizeof(T) == 1) { uint32_t q = *(const uint32_t *)(rowp + gx0); __builtin_memcpy(v[it][i], &q, 4); }
                    else if constexpr (sizeof(T) == 2) { uint2 q = *(const uint2 *)(rowp + gx0); __builtin_memcpy(v[it][i], &q, 8); }
                    else { uint4 q = *(const uint4 *)(rowp + gx0); __builtin_memcpy(v[it][i], &q, 16); }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) v[it][i][k] = rowp[km_reflect101(gx0 + k, W)];
                }
            }
        }
    }
    // ---- phase 1b: stretch to u8, pack into LDS, emit the auto mask
    unsigned cnt = 0;
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int ci = it * 256 + tid;
        if (ci < THH * CPR) {
            const int row = ci / CPR, cx = ci - row * CPR;
            const int gx0 = X0 - HX + cx * 4;
#pragma unroll
            for (int i = 0; i < NIMG; i++) {
                uint32_t packed = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    unsigned u = st[i](v[it][i][k], nullptr);
                    if (i == 1 && invert1) u = 255u - u;
                    packed |= u << (8 * k);
                }
                tile[i][row][cx] = packed;
            }
            if constexpr (MASK) {
                // auto mask for interior pixels: v[.][0] = ref, v[.][1] = mon
                const int oy = Y0 - R + row;
                if (row >= R && row < R + LAP_TH && oy < H && gx0 >= X0 && gx0 < X0 + LAP_TW && gx0 < W) {
                    uint32_t mp = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const bool ok = (gx0 + k < W) && px_valid<T>(v[it][1][k], v[it][0][k], nd);
                        mp |= (ok ? 1u : 0u) << (8 * k);
                        cnt += ok;
                    }
                    const size_t o = (size_t)oy * W + gx0;
                    if (gx0 + 3 < W && (o & 3) == 0) *(uint32_t *)(mask_out + o) = mp;
                    else {
                        for (int k = 0; k < 4 && gx0 + k < W; k++) mask_out[o + k] = (uint8_t)((mp >> (8 * k)) & 1u);
                    }
                }
            }
        }
    }
    if constexpr (MASK) {
        // one partial per workgroup (a single-address atomic per wave would serialise ~10^5 updates)
        __shared__ unsigned s_cnt[4];
        const unsigned c64 = (unsigned)wave_sum_u64((unsigned long long)cnt);
        if ((tid & 63) == 0) s_cnt[tid >> 6] = c64;
        __syncthreads();
        if (tid == 0) valid_partial[blockIdx.y * gridDim.x + blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    } else {
        __syncthreads();
    }

    uint8_t *outs[2] = {out0, out1};
    if constexpr (R <= 3) {
        // ================= packed path (ksize <= 7): v_dot4 horizontally, v_dot2 vertically =================
        // pixels are stored biased (p - 128, bit 7 flipped) so that signed 8-bit dot products apply;
        // sum(kd) = 0 and sum(ks) = 4^R remove / restore the bias exactly.
        typedef short short2v __attribute__((ext_vector_type(2)));
        int *hds = (int *)&hd[0][0][0];  // [NIMG][THH][LAP_TW] packed (hd | hs << 16); hd+hs storage is contiguous
        int kdp[NIMG][2], ksp[NIMG][2], bias[NIMG], vk[NIMG][2 * R + 1];
#pragma unroll
        for (int i = 0; i < NIMG; i++) {
            int sum = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                unsigned a = 0, b = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int t = 4 * h + k;
                    const int d = t <= 2 * R ? cf.kd[i][t] : 0, sm = t <= 2 * R ? cf.ks[i][t] : 0;
                    a |= ((unsigned)d & 0xffu) << (8 * k);
                    b |= ((unsigned)sm & 0xffu) << (8 * k);
                    sum += sm;
                }
                kdp[i][h] = (int)a; ksp[i][h] = (int)b;
            }
            bias[i] = R == 4 ? 0 : 128 * sum;
#pragma unroll
            for (int t = 0; t <= 2 * R; t++) vk[i][t] = (cf.ks[i][t] & 0xffff) | (cf.kd[i][t] << 16);
        }
        // ---- phase 2: horizontal kd / ks passes, 4 outputs per item
        for (int it = tid; it < NIMG * THH * NQ; it += 256) {
            const int i = it / (THH * NQ);
            const int rem = it - i * (THH * NQ);
            const int row = rem / NQ, q = rem - row * NQ;
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = ((q + k < CPR) ? tile[i][row][q + k] : 0u) ^ 0x80808080u;
            int o4[4];
#pragma unroll
            for (int o = 0; o < 4; o++) {
                constexpr int base = HX - R;
                const int sft = (o + base) & 3, wi = (o + base) >> 2;
                const int g0 = (int)__builtin_amdgcn_alignbyte(w[wi + 1], w[wi], sft);
                const int g1 = (int)__builtin_amdgcn_alignbyte(wi + 2 < 4 ? w[wi + 2] : 0u, w[wi + 1], sft);
                const int vd = __builtin_amdgcn_sdot4(g0, kdp[i][0], __builtin_amdgcn_sdot4(g1, kdp[i][1], 0, false), false);
                const int vs = __builtin_amdgcn_sdot4(g0, ksp[i][0], __builtin_amdgcn_sdot4(g1, ksp[i][1], bias[i], false), false);
                o4[o] = (vd & 0xffff) | (vs << 16);
            }
            *(int4 *)&hds[((size_t)i * THH + row) * LAP_TW + 4 * q] = make_int4(o4[0], o4[1], o4[2], o4[3]);
        }
        __syncthreads();
        // ---- phase 3: vertical combine on 4x4 micro-tiles: one v_dot2 per tap and pixel
        for (int it = tid; it < NIMG * (LAP_TH / 4) * NQ; it += 256) {
            const int i = it / ((LAP_TH / 4) * NQ);
            const int rem = it - i * ((LAP_TH / 4) * NQ);
            const int rg = rem / NQ, q = rem - rg * NQ;
            const int ox = X0 + 4 * q;
            if (ox >= W || Y0 + 4 * rg >= H) continue;
            int acc[4][4];
#pragma unroll
            for (int o = 0; o < 4; o++)
#pragma unroll
                for (int c2 = 0; c2 < 4; c2++) acc[o][c2] = 0;
#pragma unroll
            for (int j = 0; j < 2 * R + 4; j++) {
                const int4 a = *(const int4 *)&hds[((size_t)i * THH + 4 * rg + j) * LAP_TW + 4 * q];
                const int av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    const int tap = j - o;
                    if (tap >= 0 && tap <= 2 * R) {
#pragma unroll
                        for (int c2 = 0; c2 < 4; c2++)
                            acc[o][c2] = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, av[c2]), __builtin_bit_cast(short2v, vk[i][tap]),
                                                                acc[o][c2], false);
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < 4; o++) {
                const int oy = Y0 + 4 * rg + o;
                if (oy >= H) break;
                uint32_t packed = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) packed |= (uint32_t)min(max(acc[o][k], 0), 255) << (8 * k);
                const size_t off = (size_t)oy * W + ox;
                if (ox + 3 < W && (off & 3) == 0) *(uint32_t *)(outs[i] + off) = packed;
                else {
                    for (int k = 0; k < 4 && ox + k < W; k++) outs[i][off + k] = (uint8_t)(packed >> (8 * k));
                }
            }
        }
    } else {
        // ================= generic path (ksize 9, 11): 24-bit multiply-adds on int32 planes =================
        // ---- phase 2: horizontal passes (kd and ks) for 4 consecutive outputs per item
        constexpr int NW = (2 * R + 4 + (HX - R) + 3) / 4;  // words covering [x+HX-R, x+HX+R+4)
        for (int it = tid; it < NIMG * THH * NQ; it += 256) {
            const int i = it / (THH * NQ);
            const int rem = it - i * (THH * NQ);
            const int row = rem / NQ, q = rem - row * NQ;
            uint32_t w[NW + 1];
#pragma unroll
            for (int k = 0; k < NW + 1; k++) w[k] = (q + k < CPR) ? tile[i][row][q + k] : 0u;
            int ad[4] = {0, 0, 0, 0}, as[4] = {0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < 2 * R + 4; t++) {
                const int b = t + (HX - R);
                const int pv = (int)((w[b >> 2] >> (8 * (b & 3))) & 0xffu);
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    const int k = t - o;  // tap index for output o
                    if (k >= 0 && k <= 2 * R) {
                        ad[o] = mad24(cf.kd[i][k], pv, ad[o]);
                        as[o] = mad24(cf.ks[i][k], pv, as[o]);
                    }
                }
            }
            HT *pd = &hd[i][row][4 * q], *ps = &hs[i][row][4 * q];
#pragma unroll
            for (int o = 0; o < 4; o++) { pd[o] = (HT)ad[o]; ps[o] = (HT)as[o]; }
        }
        __syncthreads();
        // ---- phase 3: vertical combine on 4x4 micro-tiles, clip to [0,255], packed stores
        for (int it = tid; it < NIMG * (LAP_TH / 4) * NQ; it += 256) {
            const int i = it / ((LAP_TH / 4) * NQ);
            const int rem = it - i * ((LAP_TH / 4) * NQ);
            const int rg = rem / NQ, q = rem - rg * NQ;
            const int ox = X0 + 4 * q;
            if (ox >= W || Y0 + 4 * rg >= H) continue;
            int acc[4][4];
#pragma unroll
            for (int o = 0; o < 4; o++)
#pragma unroll
                for (int c2 = 0; c2 < 4; c2++) acc[o][c2] = 0;
#pragma unroll
            for (int j = 0; j < 2 * R + 4; j++) {
                const HT *pa = &hd[i][4 * rg + j][4 * q], *pb = &hs[i][4 * rg + j][4 * q];
                int a[4], b[4];
#pragma unroll
                for (int c2 = 0; c2 < 4; c2++) { a[c2] = pa[c2]; b[c2] = pb[c2]; }
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    const int tap = j - o;
                    if (tap >= 0 && tap <= 2 * R) {
                        const int ksj = cf.ks[i][tap], kdj = cf.kd[i][tap];
#pragma unroll
                        for (int c2 = 0; c2 < 4; c2++) acc[o][c2] = mad24(ksj, a[c2], mad24(kdj, b[c2], acc[o][c2]));
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < 4; o++) {
                const int oy = Y0 + 4 * rg + o;
                if (oy >= H) break;
                uint32_t packed = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) packed |= (uint32_t)min(max(acc[o][k], 0), 255) << (8 * k);
                const size_t off = (size_t)oy * W + ox;
                if (ox + 3 < W && (off & 3) == 0) *(uint32_t *)(outs[i] + off) = packed;
                else {
                    for (int k = 0; k < 4 && ox + k < W; k++) outs[i][off + k] = (uint8_t)(packed >> (8 * k));
                }
            }
        }
    }
}

template <typename T, int NIMG, bool MASK>
static int launch_lap(km_ctx *c, int R, const T *a, const T *b, int H, int W, ptrdiff_t sa, ptrdiff_t sb, const double *mm,
                      const lap_coef &cf, int invert1, const nodata_t &nd, uint8_t *oa, uint8_t *ob, uint8_t *mask,
                      unsigned long long *valid_out)
{
    dim3 grid((W + LAP_TW - 1) / LAP_TW, (H + LAP_TH - 1) / LAP_TH);
    unsigned *valid = nullptr;
    if (MASK) {
        valid = (unsigned *)km_ws(c, WS_PARTIAL, (size_t)grid.x * grid.y * sizeof(unsigned));
        if (!valid) return KM_E_NOMEM;
    }
#define KM_LAP_CASE(RR)                                                                                         \
    case RR:                                                                                                    \
        lap_kernel<RR, T, NIMG, MASK><<<grid, 256, 0, c->stream>>>(a, b, H, W, sa, sb, mm, cf, invert1, nd, oa, ob, \
                                                                   mask, valid);                               \
        break;
    switch (R) {
        KM_LAP_CASE(1)
        KM_LAP_CASE(2)
        KM_LAP_CASE(3)
        KM_LAP_CASE(4)
        KM_LAP_CASE(5)
    default: return km_fail(c, KM_E_UNSUPPORTED, "laplacian radius %d", R);
    }
#undef KM_LAP_CASE
    KM_LAUNCH_CHECK(c);
    return MASK ? kd_sum_u32(c, valid, grid.x * grid.y, valid_out) : KM_OK;
}

// ---- K2, fast path (both images, ksize <= 7): one wavefront marches down a 256-column strip, 4 columns per
// lane (62 of the 64 lanes produce output, the outer two only feed their neighbours).  Per source row: raw
// pixels -> exact uint8 stretch -> horizontal kd / ks passes with v_dot4 on bytes assembled from the two
// neighbour lanes (DPP wave shifts + v_alignbyte) -> (hd | hs) pairs pushed into a (2R+1)-row register ring;
// per output row: one v_dot2 per tap and pixel over the ring.  No LDS tiles, no barriers, no index arithmetic.
// First link of a dot-product chain in the three-address VOP3P form (accumulator = inline 0 or a VGPR): the
// two-address v_dot4c / v_dot2c the compiler prefers needs a v_mov to seed every chain.  Coefficients are
// wave-uniform (SGPR operand; gfx9 allows one scalar source per VALU instruction, so the bias sits in a VGPR).
__device__ __forceinline__ int dot4_seed0(int bytes, int coef_uniform)
{
    int r;
    asm("v_dot4_i32_i8 %0, %1, %2, 0" : "=v"(r) : "v"(bytes), "s"(coef_uniform));
    return r;
}
__device__ __forceinline__ int dot4_seed(int bytes, int coef_uniform, int acc)
{
    int r;
    asm("v_dot4_i32_i8 %0, %1, %2, %3" : "=v"(r) : "v"(bytes), "s"(coef_uniform), "v"(acc));
    return r;
}
__device__ __forceinline__ int dot2_seed0(int pair, int coef_uniform)
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(pair), "s"(coef_uniform));
    return r;
}
// An empty asm makes a lane offset opaque at the point of use: the compiler then cannot fold it into a hoisted
// per-lane 64-bit pointer and addresses memory as scalar row base + 32-bit vector offset (no per-lane 64-bit arithmetic).
__device__ __forceinline__ unsigned opaque_lane_offset(unsigned x)
{
    asm volatile("" : "+v"(x));
    return x;
}
// The same in place, for a loop: the old value dies in the asm, so no copy of the offset is made per use (the by-value form keeps its
// argument alive and costs a v_mov each time).
__device__ __forceinline__ void reopaque_lane_offset(unsigned &x) { asm volatile("" : "+v"(x)); }
// f(0_c) .. f((N-1)_c): a fully unrolled loop whose index is a compile-time constant
template <class F, int... I> __device__ __forceinline__ void lapm_for_impl(F &&f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F> __device__ __forceinline__ void lapm_for(F &&f) { lapm_for_impl(f, std::make_integer_sequence<int, N>{}); }

// (LAPM_VALID_OF(R), the output columns of a strip, and the pixels an item counts: lap_items.hpp)
#ifndef LAPM_PF
#define LAPM_PF 3      // source rows in flight per wave (interior trips: really so; 2, 3 and 4 measure the same - profiles/lap_march_rows_kernel_stats.md)
#endif

template <int R, typename T, bool MASK>
__device__ __forceinline__ void lap_march_item(const T *__restrict__ img0, const T *__restrict__ img1, int H, int W,
                                               ptrdiff_t stride0, ptrdiff_t stride1, const double *__restrict__ mm,
                                               const lap_coef &cf, int invert1, const nodata_t &nd,
                                               uint8_t *__restrict__ out0, uint8_t *__restrict__ out1,
                                               uint8_t *__restrict__ mask_out, unsigned *__restrict__ valid_partial, int nstrips,
                                               int rows_per_item, int wave_id /* wave-uniform: this wavefront's work item */)
{
    typedef short short2v __attribute__((ext_vector_type(2)));
    // R = 5 (kernel 11; sum ks = 1024: a horizontal smoothing sum needs 18 bits, the ring holds 16-bit pairs): the kernels of size 11 are
    // those of size 9 convolved with [1 2 1] (OpenCV's getSobelKernels recurrence), so
    //     Laplacian_11 = ([1 2 1] x [1 2 1]) * (kd9 x ks9 + ks9 x kd9)          (before the saturation)
    // - the 9-tap pass (radius RH = 4) of this kernel, its 32-bit row kept unsaturated, then a 3 x 3 binomial on those integers.  REFLECT_101
    // commutes with it: a symmetric filter maps the whole-sample-symmetric extension of the image onto the extension of its own output.
    // Two halo lanes either side (the binomial needs the 9-tap value one column outside the strip), one row more either end of an item.
    constexpr int RH = R == 5 ? 4 : R;
    constexpr int NR = 2 * RH + 1;
    constexpr int HALO = R == 5 ? 8 : 4, VALID = 256 - 2 * HALO;
    static_assert(VALID == LAPM_VALID_OF(R), "strip geometry");
    const int lane = threadIdx.x & 63;
    const int rowblock = wave_id / nstrips, strip = wave_id - rowblock * nstrips;   // (row arithmetic, loop control and row bases stay scalar)
    stretcher<T> st[2];
    st[0].init(mm, 0, nullptr); st[1].init(mm, 1, nullptr);
    // A width that is no multiple of 4 would leave the last strip's border lane straddling the right edge (the per-lane general path:
    // 1 strip in 23 of a 5490-column unit, and + 22 % on the launch).  That strip is SHIFTED left instead so that its lane 63 starts
    // exactly at column W: it recomputes - and rewrites, byte for byte the same - columns of its left neighbour and counts valid
    // pixels only from `cnt_from` on.
    // (which strip, and which pixels an item counts: lap_items.hpp - the fused eigenvalue pass reads valid_partial[] by the same rule)
    const lap_item_grid grid = {H, W, rows_per_item, VALID, nstrips};
    const bool shifted = lapi_shifted(W, strip, nstrips);                       // (its lane 0 at column W - 252 lies inside the image)
    const int gx0 = (shifted ? W - (256 - HALO) : strip * VALID - HALO) + 4 * lane;           // first of this lane's 4 columns
    const int cnt_from = lapi_count_from(grid, strip);
    const uint32_t cnt_mask = gx0 >= cnt_from ? 0xffffffffu : gx0 + 4 <= cnt_from ? 0u : (0xffffffffu << (8 * (cnt_from - gx0)));
    const unsigned ugx = (unsigned)gx0;                           // used by output lanes only (gx0 >= 0 there)
    // FAST path (W % 4 == 0, aligned rows): a lane left of the image or right of it loads the 4 columns of its
    // in-image neighbour (clamped address) and mirrors the stretched bytes (REFLECT_101) with one byte permute:
    //   left  [c0 c1 c2 c3] -> [ . c3 c2 c1]   (columns -4..-1; -4 is never a tap for R <= 3; R = 4: below)
    //   right [c0 c1 c2 c3] -> [c2 c1 c0  . ]  (columns W..W+3)
    // R = 4 (ksize 9): column -4 / W + 3 IS a tap - the border lane loads the four columns ONE further inside (1..4 / W-5..W-2) and
    // reverses them: [c1 c2 c3 c4] -> [c4 c3 c2 c1] = columns -4..-1, [W-5 .. W-2] -> [W-2 .. W-5] = columns W..W+3
    // (RH = 4 in general: the lane at columns g .. g + 3 outside the image holds the reversed columns -g - 3 .. -g / 2W - 5 - g .. 2W - 2 - g;
    //  lanes further out than the halo hold columns nobody reads - clamped into the image)
    const unsigned ugx_load = RH == 4 ? (unsigned)min(max(gx0 < 0 ? -gx0 - 3 : gx0 >= W ? 2 * W - 5 - gx0 : gx0, 0), W - 4) : (unsigned)min(max(gx0, 0), W - 4);
    const unsigned edge_sel = RH == 4 ? ((gx0 < 0 || gx0 >= W) ? 0x00010203u : 0x03020100u)
                                      : (gx0 < 0 ? 0x01020300u : gx0 >= W ? 0x03000102u : 0x03020100u);
    const bool col_inside = gx0 >= 0 && gx0 + 3 < W;
    const bool vec0 = col_inside && (stride0 % 4 == 0) && ((uintptr_t)img0 % (4 * sizeof(T)) == 0);
    const bool vec1 = col_inside && (stride1 % 4 == 0) && ((uintptr_t)img1 % (4 * sizeof(T)) == 0);
    int rc[4];                                                    // REFLECT_101 columns for lanes on the border
#pragma unroll
    for (int k = 0; k < 4; k++) rc[k] = km_reflect101(gx0 + k, W);
    const bool out_lane = lane >= HALO / 4 && lane <= 63 - HALO / 4 && gx0 < W;
    const int y0 = lapi_row0(grid, rowblock), y1 = lapi_row1(grid, rowblock);

    // packed coefficients
    // (R = 4: nine taps = three dwords; the smoothing sum stays SIGNED there - sum ks (u - 128) spans [-32768, 32512], exactly an int16 -
    //  and needs no bias: the vertical derivative taps sum to zero, so a constant added to every smoothed row cancels in kd * hs)
    constexpr int NH = RH == 4 ? 3 : 2;
    int kdp[2][NH], ksp[2][NH], bias[2], vk[2][NR];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        int sum = 0;
#pragma unroll
        for (int h = 0; h < NH; h++) {
            unsigned a = 0, b = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int t = 4 * h + k;
                const int d = t < NR ? cf.kd[i][t] : 0, sm = t < NR ? cf.ks[i][t] : 0;
                a |= ((unsigned)d & 0xffu) << (8 * k);
                b |= ((unsigned)sm & 0xffu) << (8 * k);
                sum += sm;
            }
            kdp[i][h] = (int)a; ksp[i][h] = (int)b;
        }
        bias[i] = 128 * sum;
#pragma unroll
        for (int t = 0; t < NR; t++) vk[i][t] = (cf.ks[i][t] & 0xffff) | (cf.kd[i][t] << 16);
    }

    // 16-bit dtypes: nodata as a packed pixel pair (0 = "no further condition": absent, non-integral or out of range)
    typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));
    auto nodata16 = [](int has, double v) -> uint32_t {
        if (!has || v != floor(v)) return 0u;
        if constexpr (std::is_signed<T>::value) { if (v < -32768.0 || v > 32767.0) return 0u; }
        else { if (v < 0.0 || v > 65535.0) return 0u; }
        const uint32_t x = (uint32_t)(uint16_t)(int)v;
        return x | (x << 16);
    };
    const uint32_t nd16_mon = nodata16(nd.has_mon, nd.mon), nd16_ref = nodata16(nd.has_ref, nd.ref);
    (void)nd16_mon; (void)nd16_ref;
    int vbias[2];   // bias as vector operands (see dot4_seed); the asm keeps them out of the scalar file
    asm volatile("v_mov_b32 %0, %1" : "=v"(vbias[0]) : "s"(bias[0]));
    asm volatile("v_mov_b32 %0, %1" : "=v"(vbias[1]) : "s"(bias[1]));
    unsigned cnt = 0;
    uint8_t *outs[2] = {out0, out1};
    // FAST: every lane of the strip is an interior, aligned lane (wave-uniform) -> no per-lane fallbacks in the loop
    auto march = [&](auto fast_tag) {
    constexpr bool FAST = decltype(fast_tag)::value;
    auto load_raw = [&](int m, T (&v)[2][4]) {
        const int r = km_reflect101(m, H);
        const T *r0 = img0 + (size_t)r * stride0, *r1 = img1 + (size_t)r * stride1;
        const unsigned lx = opaque_lane_offset(ugx_load * (unsigned)sizeof(T));   // byte offset of the lane's first column
        if (FAST) {   // uniform row base + unsigned 32-bit lane offset: no per-lane 64-bit address arithmetic; any row alignment
            __builtin_memcpy(v[0], (const char *)r0 + lx, 4 * sizeof(T));
        } else if (vec0) {
            if constexpr (sizeof(T) == 1) { uint32_t q = *(const uint32_t *)(r0 + gx0); __builtin_memcpy(v[0], &q, 4); }
            else if constexpr (sizeof(T) == 2) { uint2 q = *(const uint2 *)(r0 + gx0); __builtin_memcpy(v[0], &q, 8); }
            else { uint4 q = *(const uint4 *)(r0 + gx0); __builtin_memcpy(v[0], &q, 16); }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) v[0][k] = r0[rc[k]];
        }
        if (FAST) {
            __builtin_memcpy(v[1], (const char *)r1 + lx, 4 * sizeof(T));
        } else if (vec1) {
            if constexpr (sizeof(T) == 1) { uint32_t q = *(const uint32_t *)(r1 + gx0); __builtin_memcpy(v[1], &q, 4); }
            else if constexpr (sizeof(T) == 2) { uint2 q = *(const uint2 *)(r1 + gx0); __builtin_memcpy(v[1], &q, 8); }
            else { uint4 q = *(const uint4 *)(r1 + gx0); __builtin_memcpy(v[1], &q, 16); }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) v[1][k] = r1[rc[k]];
        }
    };

    int hp[2][2][4];                                  // (R = 5) the binomial's two previous rows of horizontal sums
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int j = 0; j < 4; j++) hp[i][r][j] = 0;
    (void)hp;
    int ring[2][NR][4];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int k = 0; k < NR; k++)
#pragma unroll
            for (int j = 0; j < 4; j++) ring[i][k][j] = 0;
    // The stores of an interior trip (below) go through buffer descriptors: one per plane, its base the plane's row of the trip's
    // first step (mask: source row m; outputs: row m - R, at radius 5 the binomial's row m - RH - 1, the same), its size the rows
    // these trips write, the row a scalar offset that advances by W per step.  Every lane stores, unconditionally - a lane that
    // produces no output (halo lanes, lanes right of the image) carries an offset beyond any size (2^31) and the hardware drops its
    // store.  No exec mask, no branch round a store: the compiler's wait-count bookkeeping merges the two sides of such a branch to
    // "no store issued" and then waits for more than the row a step consumes.
    __amdgpu_buffer_rsrc_t rs_m = __builtin_amdgcn_make_buffer_rsrc((void *)nullptr, 0, 0, 0x00020000), rs_o0 = rs_m, rs_o1 = rs_m;
    unsigned srow = 0;                                                    // byte offset of the current step's row behind the bases
    const unsigned ux = out_lane ? ugx : 0x80000000u;
    const uint32_t cnt_mask_in = out_lane ? cnt_mask : 0u;
    (void)srow; (void)ux; (void)cnt_mask_in;
    // ---- one row step: source row m (ring slot k, a compile-time constant), raw pixels v.  IN: a step of an interior trip.  What IN
    // replaces, everywhere below:
    //   the tests on m (mask row: y0 <= m < y1; output row: m - R >= y0)  ->  nothing, they hold for every row of an interior trip
    //   `out_lane` round a store                                           ->  every lane stores, `ux` is out of range where !out_lane
    //   `out_lane` round the count of valid pixels, `cnt_mask`             ->  `cnt_mask_in`, zero where !out_lane
    //   row pointers computed from m, global stores                        ->  descriptor + `srow`
    // (IN implies FAST; the general step keeps the parent's text, its per-lane fallbacks included)
    auto row_step = [&](auto k_tag, auto in_tag, int m, const T (&v)[2][4]) {
            constexpr int k = decltype(k_tag)::value;
            constexpr bool IN = decltype(in_tag)::value;
            // ---- auto mask of source row m (it is an output row when y0 <= m < y1)
            if constexpr (MASK && FAST && sizeof(T) == 2) {
                // packed form: a pixel pair is valid iff min(mon, ref, mon ^ nodata_mon, ref ^ nodata_ref) != 0 (unsigned)
                if (IN || (m >= y0 && m < y1 && out_lane)) {
                    uint2 qm, qr;
                    __builtin_memcpy(&qm, v[1], 8); __builtin_memcpy(&qr, v[0], 8);
                    auto nz2 = [&](uint32_t a, uint32_t b) {
                        ushort2v mn2 = __builtin_elementwise_min(
                            __builtin_elementwise_min(__builtin_bit_cast(ushort2v, a), __builtin_bit_cast(ushort2v, b)),
                            __builtin_elementwise_min(__builtin_bit_cast(ushort2v, a ^ nd16_mon), __builtin_bit_cast(ushort2v, b ^ nd16_ref)));
                        mn2 = __builtin_elementwise_min(mn2, (ushort2v)(1));
                        return __builtin_bit_cast(uint32_t, mn2);
                    };
                    const uint32_t mp = __builtin_amdgcn_perm(nz2(qm.y, qr.y), nz2(qm.x, qr.x), 0x06040200u);
                    if constexpr (IN) {
                        cnt += (unsigned)__popc(mp & cnt_mask_in);
                        __builtin_amdgcn_raw_buffer_store_b32(mp, rs_m, ux, srow, 0);
                    } else {
                        cnt += (unsigned)__popc(mp & cnt_mask);
                        __builtin_memcpy((mask_out + (size_t)m * W) + opaque_lane_offset(ugx), &mp, 4);
                    }
                }
            } else if constexpr (MASK) {
                if (IN || (m >= y0 && m < y1 && out_lane)) {
                    uint32_t mp = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const bool ok = (gx0 + j < W) && px_valid<T>(v[1][j], v[0][j], nd);
                        mp |= (ok ? 1u : 0u) << (8 * j);
                        if constexpr (!IN) cnt += ok && gx0 + j >= cnt_from;
                    }
                    const size_t o = (size_t)m * W + gx0;
                    (void)o;
                    if constexpr (IN) {
                        cnt += (unsigned)__popc(mp & cnt_mask_in);       // (cnt_mask keeps the bytes of the columns from cnt_from on)
                        __builtin_amdgcn_raw_buffer_store_b32(mp, rs_m, ux, srow, 0);
                    } else if (FAST) __builtin_memcpy(mask_out + o, &mp, 4);
                    else if (gx0 + 3 < W && (o & 3) == 0) *(uint32_t *)(mask_out + o) = mp;
                    else {
                        for (int j = 0; j < 4 && gx0 + j < W; j++) mask_out[o + j] = (uint8_t)((mp >> (8 * j)) & 1u);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 2; i++) {
                // ---- stretch to uint8 (biased by -128 for the signed dot products)
                uint32_t cw = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) cw |= st[i](v[i][j], nullptr) << (8 * j);
                cw ^= (i == 1 && invert1) ? 0x7f7f7f7fu : 0x80808080u;   // (255 - u) - 128 == u ^ 0x7f
                if constexpr (FAST) cw = __builtin_amdgcn_perm(cw, cw, edge_sel);                    // border lanes: mirrored columns
                // (bound_ctrl: the lane without a neighbour reads 0, and the move needs no `old` value - an update_dpp(0, ..) costs a
                //  v_mov_b32 v, 0 to seed each of the two)
                const uint32_t lw = (uint32_t)__builtin_amdgcn_mov_dpp((int)cw, 0x138, 0xf, 0xf, true);   // lane-1
                const uint32_t rw = (uint32_t)__builtin_amdgcn_mov_dpp((int)cw, 0x130, 0xf, 0xf, true);   // lane+1
                // ---- horizontal kd / ks passes: bytes [4+o-R, 4+o-R+8) of (lw | cw | rw)
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    constexpr int dummy = 0; (void)dummy;
                    if constexpr (RH == 4) {
                        // nine taps: bytes [o, o + 9) of (lw | cw | rw)
                        const int g0 = (int)__builtin_amdgcn_alignbyte(cw, lw, o), g1 = (int)__builtin_amdgcn_alignbyte(rw, cw, o),
                                  g2 = (int)__builtin_amdgcn_alignbyte(0u, rw, o);
                        const int vd = __builtin_amdgcn_sdot4(g0, kdp[i][0], __builtin_amdgcn_sdot4(g1, kdp[i][1], dot4_seed0(g2, kdp[i][2]), false), false);
                        const int vs = __builtin_amdgcn_sdot4(g0, ksp[i][0], __builtin_amdgcn_sdot4(g1, ksp[i][1], dot4_seed0(g2, ksp[i][2]), false), false);
                        ring[i][k][o] = (int)__builtin_amdgcn_perm((uint32_t)vs, (uint32_t)vd, 0x05040100u);
                        continue;
                    }
                    const int sft = 4 + o - R;                 // 1..4 for R = 3, 3..6 for R = 1
                    int g0, g1;
                    if (sft < 4) {
                        g0 = (int)__builtin_amdgcn_alignbyte(cw, lw, sft & 3);
                        g1 = (int)__builtin_amdgcn_alignbyte(rw, cw, sft & 3);
                    } else if (sft == 4) {
                        g0 = (int)cw; g1 = (int)rw;
                    } else {
                        g0 = (int)__builtin_amdgcn_alignbyte(rw, cw, (sft - 4) & 3);
                        g1 = (int)__builtin_amdgcn_alignbyte(0u, rw, (sft - 4) & 3);   // taps beyond 2R are zero
                    }
                    const int vd = __builtin_amdgcn_sdot4(g0, kdp[i][0], dot4_seed0(g1, kdp[i][1]), false);
                    const int vs = __builtin_amdgcn_sdot4(g0, ksp[i][0], dot4_seed(g1, ksp[i][1], vbias[i]), false);
                    ring[i][k][o] = (int)__builtin_amdgcn_perm((uint32_t)vs, (uint32_t)vd, 0x05040100u);   // (vd & 0xffff) | (vs << 16)
                }
            }
            // ---- vertical combine for output row y = m - R (ring slot of source row y - R + j is (k + 1 + j) mod NR)
            if constexpr (R == 5) {
                // kernel 11: the 9-tap row yy = m - 4 unsaturated (every lane: the binomial reads the neighbour lanes' values through DPP), its
                // horizontal [1 2 1], then the vertical [1 2 1] over the rows yy - 2 .. yy: output row yo = yy - 1.  An image whose kernel is
                // smaller (b3 = 0) passes its 9-tap-padded row through unchanged, one row late like the other.
                const int yy = m - RH, yo = yy - 1;
                if (IN || yy >= y0 - 1) {
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        int a[4], h[4];
#pragma unroll
                        for (int o = 0; o < 4; o++) {
                            int acc = dot2_seed0(ring[i][(k + 1) % NR][o], vk[i][0]);
#pragma unroll
                            for (int j = 1; j < NR; j++)
                                acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, ring[i][(k + 1 + j) % NR][o]),
                                                             __builtin_bit_cast(short2v, vk[i][j]), acc, false);
                            a[o] = acc;
                        }
                        uint32_t packed = 0;
                        if (cf.b3[i]) {
                            const int al = __builtin_amdgcn_mov_dpp(a[3], 0x138, 0xf, 0xf, true);      // lane - 1: the column left of this lane's
                            const int ar = __builtin_amdgcn_mov_dpp(a[0], 0x130, 0xf, 0xf, true);      // lane + 1
#pragma unroll
                            for (int o = 0; o < 4; o++) h[o] = (o == 0 ? al : a[o - 1]) + 2 * a[o] + (o == 3 ? ar : a[o + 1]);
#pragma unroll
                            for (int o = 0; o < 4; o++) packed |= (uint32_t)min(max(hp[i][1][o] + 2 * hp[i][0][o] + h[o], 0), 255) << (8 * o);
                        } else {
#pragma unroll
                            for (int o = 0; o < 4; o++) { h[o] = a[o]; packed |= (uint32_t)min(max(hp[i][0][o], 0), 255) << (8 * o); }
                        }
#pragma unroll
                        for (int o = 0; o < 4; o++) { hp[i][1][o] = hp[i][0][o]; hp[i][0][o] = h[o]; }
                        if (IN || (yo >= y0 && out_lane)) {
                            const size_t off = (size_t)yo * W + gx0;
                            (void)off;
                            if constexpr (IN) __builtin_amdgcn_raw_buffer_store_b32(packed, i == 0 ? rs_o0 : rs_o1, ux, srow, 0);
                            else if (FAST) __builtin_memcpy((outs[i] + (size_t)yo * W) + opaque_lane_offset(ugx), &packed, 4);
                            else if (gx0 + 3 < W && (off & 3) == 0) *(uint32_t *)(outs[i] + off) = packed;
                            else {
                                for (int j = 0; j < 4 && gx0 + j < W; j++) outs[i][off + j] = (uint8_t)(packed >> (8 * j));
                            }
                        }
                    }
                }
            } else {
            const int y = m - R;
            if (IN || (y >= y0 && out_lane)) {
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    uint32_t packed = 0;
#pragma unroll
                    for (int o = 0; o < 4; o++) {
                        int acc = dot2_seed0(ring[i][(k + 1) % NR][o], vk[i][0]);
#pragma unroll
                        for (int j = 1; j < NR; j++)
                            acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, ring[i][(k + 1 + j) % NR][o]),
                                                         __builtin_bit_cast(short2v, vk[i][j]), acc, false);
                        packed |= (uint32_t)min(max(acc, 0), 255) << (8 * o);
                    }
                    const size_t off = (size_t)y * W + gx0;
                    (void)off;
                    if constexpr (IN) __builtin_amdgcn_raw_buffer_store_b32(packed, i == 0 ? rs_o0 : rs_o1, ux, srow, 0);
                    else if (FAST) __builtin_memcpy((outs[i] + (size_t)y * W) + opaque_lane_offset(ugx), &packed, 4);
                    else if (gx0 + 3 < W && (off & 3) == 0) *(uint32_t *)(outs[i] + off) = packed;
                    else {
                        for (int j = 0; j < 4 && gx0 + j < W; j++) outs[i][off + j] = (uint8_t)(packed >> (8 * j));
                    }
                }
            }
            }
    };  // row_step

    // An item's march: GENERAL trips (the warm-up that fills the ring, the rows that mirror at the top or bottom of the image, the tail
    // of the item) and INTERIOR trips in between.  Both run whole trips of NR row steps from the item's first source row y0 - R on, so
    // the ring slot of a row stays the compile-time constant k of its step.
    //  general:  the guarded form - every condition on m tested, rows mirrored, the row in flight LAPM_PF steps ahead kept in a short
    //            register FIFO that is SHIFTED every step: the shift reads the newest slot, so a general step waits for the loads of
    //            the step before (and, vmcnt counting stores in order with loads, for that step's stores)
    //  interior: trips whose NR rows m all are mask rows and output rows (y0 + R <= m < y1) with the rows m .. m + PF inside the image
    //            and inside [y0 - R, y1 + R).  No guard, no conditional load, no mirror; row bases advance by the stride.  The raw rows
    //            sit in NR STATIC slots - step k consumes slot k and loads the row of step k + PF into slot (k + PF) % NR - of which
    //            the live ranges keep PF + 1 in registers; nothing is copied, and a step waits only for the row it consumes.
    // A switch between the two forms hands no row in flight over: the last general steps of the warm-up still fill their FIFO, the
    // interior trips load those rows again into their slots, and the tail's FIFO reloads what the last trip prefetched - 2 PF row
    // loads per item that hit the cache (of the 40 - 170 rows of an item), for two forms that share no register state.
    // rows in flight: LAPM_PF, but two for float32 at radius 5 - a raw row is 8 registers there, and the third row ahead takes that
    // kernel from 165 to 174 registers: past 168, from three waves per SIMD to two (in the general steps' FIFO as in the slots)
    constexpr int DEPTH = (R == 5 && sizeof(T) == 4 && LAPM_PF > 2) ? 2 : LAPM_PF;
    constexpr int PF = DEPTH < NR ? DEPTH : NR - 1;         // (radius 1: three slots, so at most two rows ahead)
    constexpr int WARM = (2 * R + NR - 1) / NR * NR;        // whole trips until every step writes an output row: NR (radius 5: 2 NR)
    const int m_end = y1 + R;                               // one past the item's last source row
    int mbase = y0 - R;
    int n_in = 0;                                           // interior trips
    if constexpr (FAST) n_in = (min(y1, min(H, m_end) - PF) - (mbase + WARM)) / NR;
    int m_stop = n_in > 0 ? mbase + WARM : m_end;
    for (;;) {
        {
            T nxt[DEPTH][2][4];
#pragma unroll
            for (int f = 0; f < DEPTH; f++) load_raw(min(mbase + f, m_end - 1), nxt[f]);
            for (; mbase < m_stop; mbase += NR) {
                lapm_for<NR>([&](auto k_tag) {
                    const int m = mbase + decltype(k_tag)::value;      // source row of this step (may lie outside: mirrored)
                    if (m >= m_end) return;                  // (no break: ring indices must stay compile-time constants)
                    T v[2][4];
#pragma unroll
                    for (int i = 0; i < 2; i++)
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            v[i][j] = nxt[0][i][j];
#pragma unroll
                            for (int f = 0; f + 1 < DEPTH; f++) nxt[f][i][j] = nxt[f + 1][i][j];
                        }
                    if (m + DEPTH < m_end) load_raw(m + DEPTH, nxt[DEPTH - 1]);
                    row_step(k_tag, std::false_type{}, m, v);
                });
            }
        }
        if (mbase >= m_end) break;
        if constexpr (FAST) {
            const ptrdiff_t sb0 = stride0 * (ptrdiff_t)sizeof(T), sb1 = stride1 * (ptrdiff_t)sizeof(T);
            const char *p0 = (const char *)img0 + (ptrdiff_t)mbase * sb0, *p1 = (const char *)img1 + (ptrdiff_t)mbase * sb1;   // the next row to load
            unsigned lx = ugx_load * (unsigned)sizeof(T);    // byte offset of the lane's first column, opaque in place (see opaque_lane_offset)
            auto load_next = [&](T (&v)[2][4]) {
                reopaque_lane_offset(lx);
                __builtin_memcpy(v[0], p0 + lx, 4 * sizeof(T));
                __builtin_memcpy(v[1], p1 + lx, 4 * sizeof(T));
                p0 += sb0; p1 += sb1;
            };
            T slot[NR][2][4];
#pragma unroll
            for (int f = 0; f < PF; f++) load_next(slot[f]);
            const int span = n_in * NR * W;                  // the rows these trips write (an item has at most 4096 rows: far below 2^31 bytes)
            if constexpr (MASK) rs_m = __builtin_amdgcn_make_buffer_rsrc((void *)(mask_out + (size_t)mbase * W), 0, span, 0x00020000);
            rs_o0 = __builtin_amdgcn_make_buffer_rsrc((void *)(out0 + (size_t)(mbase - R) * W), 0, span, 0x00020000);
            rs_o1 = __builtin_amdgcn_make_buffer_rsrc((void *)(out1 + (size_t)(mbase - R) * W), 0, span, 0x00020000);
            srow = 0;
            for (int t = 0; t < n_in; t++) {
                lapm_for<NR>([&](auto k_tag) {
                    constexpr int k = decltype(k_tag)::value;
                    load_next(slot[(k + PF) % NR]);
                    row_step(k_tag, std::true_type{}, mbase + k, slot[k]);
                    srow += (unsigned)W;
                    // (a trip is one basic block: without a fence between the steps the scheduler interleaves the seven rows - a
                    //  fifth more registers, a wave per SIMD less - and moves the loads away from the step that issues them)
                    __builtin_amdgcn_sched_barrier(0);
                });
                mbase += NR;
            }
        }
        m_stop = m_end;
    }
    };  // march
    // FAST: every lane of the item either lies inside the image with its 4 columns or is a whole-lane mirror of its in-image neighbour
    // (wave-uniform).  Rows need no alignment - loads and stores are 4-column accesses at whatever address the row has (a 5490-column
    // tile: every other row sits off the dword grid; the per-pixel path there cost 1.75x).  The last strip of a width that is no multiple
    // of 4 is shifted (above); only a last strip of fewer than 4 columns (its left neighbour's border lane straddles the edge) and images of
    // a single strip still take the general path.
    const bool fast = (W % 4 == 0) || shifted || (strip * VALID - HALO + 4 * 64 <= W);
    if (fast) march(std::true_type{});
    else march(std::false_type{});
    if constexpr (MASK) {
        const unsigned c64 = (unsigned)wave_sum_u64((unsigned long long)cnt);
        if (lane == 0) valid_partial[wave_id] = c64;
    }
}

// The units' work items form ONE linear item space (unit u owns [item0[u], item0[u + 1])), a unit's items are (row block, column
// strip), strips fastest: the 4 waves of a workgroup take 4 consecutive items.  A wavefront finds its unit with a scalar scan of <= 16
// bounds and runs the item on that unit's rasters.  A single pair is a batch of one unit.
struct lapm_units_args {
    const void *img0[KM_UNITS_MAX], *img1[KM_UNITS_MAX];
    ptrdiff_t s0[KM_UNITS_MAX], s1[KM_UNITS_MAX];
    const double *mm[KM_UNITS_MAX];
    uint8_t *out0[KM_UNITS_MAX], *out1[KM_UNITS_MAX], *mask[KM_UNITS_MAX];
    unsigned *valid[KM_UNITS_MAX];
    int H[KM_UNITS_MAX], W[KM_UNITS_MAX], nstrips[KM_UNITS_MAX];
    int item0[KM_UNITS_MAX + 1];
    int n, rows;
};
template <int R, typename T, bool MASK>
__global__ __launch_bounds__(256) KM_LAPM_OCC void lap_march_units_kernel(lapm_units_args U, lap_coef cf, int invert1, nodata_t nd)
{
    const int total = U.item0[U.n];
    unsigned tile;
    if (!km_xcd_tile((unsigned)(total + 3) / 4u, tile)) return;
    const int wave_lin = (int)tile * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave_lin >= total) return;
    int u = 0;
    while (u + 1 < U.n && wave_lin >= U.item0[u + 1]) u++;
    lap_march_item<R, T, MASK>((const T *)U.img0[u], (const T *)U.img1[u], U.H[u], U.W[u], U.s0[u], U.s1[u], U.mm[u], cf, invert1, nd, U.out0[u], U.out1[u],
                               U.mask[u], U.valid[u], U.nstrips[u], U.rows, wave_lin - U.item0[u]);
}

// the instantiation of radius R (1..5, lap_make_plan): the one place that enumerates the radii - the occupancy query and the launch
// both go through this pointer
template <typename T, bool MASK>
static const void *lapm_kernel(int R)
{
    return R == 1 ? (const void *)lap_march_units_kernel<1, T, MASK> : R == 2 ? (const void *)lap_march_units_kernel<2, T, MASK>
         : R == 3 ? (const void *)lap_march_units_kernel<3, T, MASK> : R == 4 ? (const void *)lap_march_units_kernel<4, T, MASK>
         : (const void *)lap_march_units_kernel<5, T, MASK>;
}

// Rows per item and the units' item ranges: the value in [32, 160] that minimises whole rounds of resident waves x the work of one
// item over ALL units' strips (km_pick_rows_units); the resident waves are 4 SIMDs per CU x the waves per SIMD the register budget of
// the instantiation `fn` allows
static void lapm_items(km_ctx *c, int R, const void *fn, lapm_units_args &A)
{
    int wg_per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg_per_cu, fn, 256, 0) != hipSuccess || wg_per_cu < 1) wg_per_cu = 4;
    int rows = km_pick_rows_units(A.H, A.nstrips, A.n, 2 * R, (long)c->n_cu * 4 * wg_per_cu, 32, 160);
    if (const char *e = km_dev_env("KARIOS_HIP_LAP_ROWS")) { const int v = atoi(e); if (v >= 8 && v <= 4096) rows = v; }   // tuning override
    A.rows = rows;
    A.item0[0] = 0;
    for (int u = 0; u < A.n; u++) A.item0[u + 1] = A.item0[u] + A.nstrips[u] * ((A.H[u] + rows - 1) / rows);
}

static int lapm_launch(km_ctx *c, const void *fn, const lapm_units_args &A, const lap_coef &cf, int invert1, const nodata_t &nd)
{
    void *args[] = {(void *)&A, (void *)&cf, (void *)&invert1, (void *)&nd};       // (the kernel takes all four by value)
    KM_HIP(c, hipLaunchKernel(fn, dim3(km_xcd_grid((unsigned)(A.item0[A.n] + 3) / 4u)), dim3(256), args, 0, c->stream));
    return KM_OK;
}

// one pair (kd_stretch_laplacian_pair): a batch of one unit
template <typename T, bool MASK>
static int launch_lap_march(km_ctx *c, int R, const T *a, const T *b, int H, int W, ptrdiff_t sa, ptrdiff_t sb, const double *mm,
                            const lap_coef &cf, int invert1, const nodata_t &nd, uint8_t *oa, uint8_t *ob,
                            uint8_t *mask, unsigned long long *valid_out, km_valid_job *defer)
{
    lapm_units_args A;
    A.n = 1;
    A.img0[0] = a; A.img1[0] = b; A.s0[0] = sa; A.s1[0] = sb; A.mm[0] = mm;
    A.out0[0] = oa; A.out1[0] = ob; A.mask[0] = mask; A.valid[0] = nullptr;
    A.H[0] = H; A.W[0] = W; A.nstrips[0] = lapi_nstrips(W, LAPM_VALID_OF(R));
    const void *fn = lapm_kernel<T, MASK>(R);
    lapm_items(c, R, fn, A);                          // (the occupancy of the instantiation that runs)
    const unsigned nitems = (unsigned)A.item0[1];
    if (MASK) {
        // (a slot of its own: with the sum deferred to the second stream - below - the eigenvalue pass, which owns WS_PARTIAL, runs first)
        A.valid[0] = (unsigned *)km_ws(c, WS_LAP_VALID, ((size_t)nitems + 4) * sizeof(unsigned));
        if (!A.valid[0]) return KM_E_NOMEM;
    }
    if (int rc = lapm_launch(c, fn, A, cf, invert1, nd)) return rc;
    if (MASK) {
        if (defer) {
            // the count of valid pixels is only read at the end of the unit (frame header, statistics): its sum leaves the critical
            // path - klt_track_dev launches it on the second stream in front of the pyramids (kd_run_valid_sum)
            defer->partial = A.valid[0]; defer->n = nitems; defer->out = valid_out;
        } else if (int rc = kd_sum_u32(c, A.valid[0], nitems, valid_out)) return rc;
    }
    return KM_OK;
}

// the deferred sum of launch_lap_march, on whatever stream c->stream is at the moment (one workgroup of 1024 threads: the single
// wavefront of kd_valid_sum_units took 35 instead of 5 us over the ~3000 counts of a 10980^2 tile)
int kd_run_valid_sum(km_ctx *c, km_valid_job *job)
{
    if (!job->partial) return KM_OK;
    const km_valid_job j = *job;
    *job = km_valid_job();
    return kd_sum_u32(c, j.partial, j.n, j.out);
}

// ---- batched units: stretch + Laplacians + automatic mask of every unit in ONE launch; the per-item counts of valid pixels are summed
// per unit by kd_valid_sum_units (one workgroup per unit, on whatever stream c->stream is: the caller puts it beside the pyramids)
// (ONE wavefront per unit: the kernel runs beside the previous submission's LK, whose single-wave workgroups refill every slot a
// retiring wave leaves - a 1024-thread workgroup waited there for the whole launch, 2.6 ms with the pyramids queued behind it, and a
// 256-thread one still 2.4 ms: profiles/timeline_r06_c4.txt)
__global__ __launch_bounds__(64) void valid_sum_units_kernel(km_valid_units J)
{
    const unsigned *partial = J.partial[blockIdx.x];
    const unsigned n = J.n_partial[blockIdx.x];
    unsigned long long s = 0;
    for (unsigned i = threadIdx.x; i < n; i += 64) s += partial[i];
    s = wave_sum_u64(s);
    if (threadIdx.x == 0) *J.out[blockIdx.x] = s;
}

int kd_valid_sum_units(km_ctx *c, const km_valid_units &J)
{
    if (J.n <= 0) return KM_OK;
    valid_sum_units_kernel<<<J.n, 64, 0, c->stream>>>(J);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

// User masks of a batch (klt.py:258-266: the caller's raster instead of the automatic mask): every unit's box of its mask raster is
// packed into the unit's dense mask plane (the eigenvalue pass indexes masks with the image width) and its non-zero pixels are counted
// - what hipMemcpy2DAsync + kd_count_nonzero do for a single unit, for all units in one launch.  blockIdx.y = unit; a workgroup takes
// every gridDim.x-th group of rows; 16 bytes per thread at whatever address a row has.
struct mask_units_args {
    const uint8_t *src[KM_UNITS_MAX];
    uint8_t *dst[KM_UNITS_MAX];
    ptrdiff_t stride[KM_UNITS_MAX];
    unsigned *partial[KM_UNITS_MAX];
    int H[KM_UNITS_MAX], W[KM_UNITS_MAX];
};
__global__ __launch_bounds__(256) void mask_pack_units_kernel(mask_units_args A)
{
    const int u = blockIdx.y, H = A.H[u], W = A.W[u];
    const uint8_t *__restrict__ src = A.src[u];
    uint8_t *__restrict__ dst = A.dst[u];
    const ptrdiff_t stride = A.stride[u];
    unsigned cnt = 0;
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const uint8_t *r = src + (size_t)y * stride;
        uint8_t *w = dst + (size_t)y * W;
        for (int x = 16 * threadIdx.x; x < W; x += 16 * 256) {
            if (x + 16 <= W) {
                uint4 q;
                __builtin_memcpy(&q, r + x, 16);
                __builtin_memcpy(w + x, &q, 16);
                const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 4; k++) cnt += (unsigned)__popc(((d[k] | ((d[k] & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u));   // bytes != 0
            } else {
                for (int k = x; k < W; k++) { const uint8_t b = r[k]; w[k] = b; cnt += b != 0; }
            }
        }
    }
    const unsigned long long s = wave_sum_u64((unsigned long long)cnt);
    __shared__ unsigned sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (unsigned)s;
    __syncthreads();
    if (threadIdx.x == 0) A.partial[u][blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

template <typename T>
static int launch_lap_march_units(km_ctx *c, int R, const km_units &U, const lap_coef &cf, int invert1, const nodata_t &nd, km_valid_units *job)
{
    lapm_units_args A;
    A.n = U.n;
    for (int u = 0; u < U.n; u++) {
        A.img0[u] = U.ref[u]; A.img1[u] = U.mon[u]; A.s0[u] = U.sref[u]; A.s1[u] = U.smon[u]; A.mm[u] = U.mm[u];
        A.out0[u] = U.lap_ref[u]; A.out1[u] = U.lap_mon[u]; A.mask[u] = U.mask[u];
        A.H[u] = U.H[u]; A.W[u] = U.W[u]; A.nstrips[u] = lapi_nstrips(U.W[u], LAPM_VALID_OF(R));
    }
    lapm_items(c, R, lapm_kernel<T, true>(R), A);     // (the rows choice follows the MASK = true instantiation, with a user mask too)
    const int total = A.item0[U.n];
    const int mask_wgs = 256;                         // workgroups per unit of the user-mask pack
    const size_t n_partial = U.has_user_mask ? (size_t)mask_wgs * U.n : (size_t)total + 4 * KM_UNITS_MAX;
    unsigned *valid = (unsigned *)km_ws(c, WS_LAP_VALID, n_partial * sizeof(unsigned));
    if (!valid) return KM_E_NOMEM;
    job->n = U.n;
    if (U.has_user_mask) {
        // the caller's mask: packed + counted here, the Laplacian pass derives none (MASK = false: it neither reads nor writes a mask)
        mask_units_args M;
        for (int u = 0; u < U.n; u++) {
            M.src[u] = U.user_mask[u]; M.dst[u] = U.mask[u]; M.stride[u] = U.user_smask[u]; M.H[u] = U.H[u]; M.W[u] = U.W[u];
            M.partial[u] = valid + (size_t)mask_wgs * u;
            A.valid[u] = nullptr;
            job->partial[u] = M.partial[u]; job->n_partial[u] = (unsigned)mask_wgs; job->out[u] = &U.sc[u]->valid;
        }
        mask_pack_units_kernel<<<dim3(mask_wgs, U.n), 256, 0, c->stream>>>(M);
        KM_LAUNCH_CHECK(c);
        return lapm_launch(c, lapm_kernel<T, false>(R), A, cf, invert1, nd);
    }
    for (int u = 0; u < U.n; u++) {
        A.valid[u] = valid + A.item0[u];
        job->partial[u] = A.valid[u]; job->n_partial[u] = (unsigned)(A.item0[u + 1] - A.item0[u]); job->out[u] = &U.sc[u]->valid;
        // the counts item by item, for the eigenvalue pass of the same submission (lap_items.hpp says which pixels an entry counts)
        job->item_counts[u] = A.valid[u]; job->item_nstrips[u] = A.nstrips[u];
    }
    job->item_rows = A.rows; job->item_strip_w = LAPM_VALID_OF(R);
    return lapm_launch(c, lapm_kernel<T, true>(R), A, cf, invert1, nd);
}

// ---- the plan of one stretch + Laplacian pass: radius, coefficients and the form that runs, from the two kernel sizes and the
// smallest width and height involved (a pair: its own; a batch: over its units).  The marching form takes images of at least 8 x 8
// (16 x 16 at radius 5: two halo lanes either side), the general form everything else.  At radius 5 the marching kernel takes every
// image's kernel as a 9-tap pass, kernel 11 as the 9-tap pass of kernel 9 + the 3 x 3 binomial (lap_march_item, b3): coefficients
// centred at radius 4 there.
enum lap_form { LAP_NOT_COVERED = 0, LAP_GENERAL, LAP_MARCH };       // LAP_NOT_COVERED: a kernel size outside 1, 3 .. 11
struct lap_plan {
    int R = 0;
    lap_coef cf;
    lap_form form = LAP_NOT_COVERED;
};
static lap_plan lap_make_plan(int ksize_ref, int ksize_mon, int min_W, int min_H)
{
    lap_plan p;
    if (!km_lap_ksize_ok(ksize_ref) || !km_lap_ksize_ok(ksize_mon)) return p;
    const int ks[2] = {ksize_ref, ksize_mon};
    p.R = std::max(std::max(ksize_ref, ksize_mon) / 2, 1);
    const int edge = p.R == 5 ? 16 : 8;
    const bool march = min_W >= edge && min_H >= edge, march5 = march && p.R == 5;
    for (int i = 0; i < 2; i++) {
        p.cf.b3[i] = march5 && ks[i] == 11;
        if (!fill_coef(p.cf.b3[i] ? 9 : ks[i], march5 ? 4 : p.R, p.cf.kd[i], p.cf.ks[i])) return p;
    }
    p.form = march ? LAP_MARCH : LAP_GENERAL;
    return p;
}

// KM_E_UNSUPPORTED (no message) when the batch form does not cover the case (tiny units): the caller submits the units one by one instead
int kd_stretch_laplacian_units(km_ctx *c, const km_units &U, int ksize_ref, int ksize_mon, int invert_mon, const double *nodata_ref,
                               const double *nodata_mon, km_valid_units *job)
{
    const lap_plan p = lap_make_plan(ksize_ref, ksize_mon, *std::min_element(U.W, U.W + U.n), *std::min_element(U.H, U.H + U.n));
    if (p.form == LAP_NOT_COVERED) return km_fail(c, KM_E_UNSUPPORTED, "Laplacian ksize ref=%d mon=%d (supported: 1,3,5,7,9,11)", ksize_ref, ksize_mon);
    if (p.form != LAP_MARCH) return KM_E_UNSUPPORTED;
    const nodata_t nd = make_nodata(nodata_mon, nodata_ref);
    return km_with_pixel_type(c, U.dtype, "stretch_laplacian: bad dtype %d",
                              [&](auto t) { return launch_lap_march_units<decltype(t)>(c, p.R, U, p.cf, invert_mon, nd, job); });
}

// one uint8 image, no stretch: the general form (the plan of a pair of equal kernels on no extent at all)
int kd_laplacian_u8(km_ctx *c, const uint8_t *d_src, int H, int W, int ksize, uint8_t *d_dst)
{
    const lap_plan p = lap_make_plan(ksize, ksize, 0, 0);
    if (p.form == LAP_NOT_COVERED) return km_fail(c, KM_E_UNSUPPORTED, "Laplacian ksize %d (supported: 1,3,5,7,9,11)", ksize);
    return launch_lap<uint8_t, 1, false>(c, p.R, d_src, d_src, H, W, W, W, nullptr, p.cf, 0, make_nodata(nullptr, nullptr), d_dst, nullptr, nullptr,
                                         nullptr);
}

int kd_stretch_laplacian_pair(km_ctx *c, const void *d_ref, const void *d_mon, int dtype, int H, int W, ptrdiff_t sref,
                              ptrdiff_t smon, const double *d_mm, int ksize_ref, int ksize_mon, int invert_mon,
                              const double *nodata_ref, const double *nodata_mon, uint8_t *d_lap_ref, uint8_t *d_lap_mon,
                              uint8_t *d_mask_out, unsigned long long *d_valid, km_valid_job *defer)
{
    const lap_plan p = lap_make_plan(ksize_ref, ksize_mon, W, H);
    if (p.form == LAP_NOT_COVERED) return km_fail(c, KM_E_UNSUPPORTED, "Laplacian ksize ref=%d mon=%d (supported: 1,3,5,7,9,11)", ksize_ref, ksize_mon);
    const nodata_t nd = make_nodata(nodata_mon, nodata_ref);
    // (without a mask to write, the pass neither counts valid pixels nor defers their sum)
    return km_with_pixel_type(c, dtype, "stretch_laplacian: bad dtype %d", [&](auto t) {
        using T = decltype(t);
        const T *ref = (const T *)d_ref, *mon = (const T *)d_mon;
        if (p.form == LAP_MARCH)
            return d_mask_out ? launch_lap_march<T, true>(c, p.R, ref, mon, H, W, sref, smon, d_mm, p.cf, invert_mon, nd, d_lap_ref, d_lap_mon, d_mask_out, d_valid, defer)
                              : launch_lap_march<T, false>(c, p.R, ref, mon, H, W, sref, smon, d_mm, p.cf, invert_mon, nd, d_lap_ref, d_lap_mon, nullptr, nullptr, nullptr);
        return d_mask_out ? launch_lap<T, 2, true>(c, p.R, ref, mon, H, W, sref, smon, d_mm, p.cf, invert_mon, nd, d_lap_ref, d_lap_mon, d_mask_out, d_valid)
                          : launch_lap<T, 2, false>(c, p.R, ref, mon, H, W, sref, smon, d_mm, p.cf, invert_mon, nd, d_lap_ref, d_lap_mon, nullptr, nullptr);
    });
}
