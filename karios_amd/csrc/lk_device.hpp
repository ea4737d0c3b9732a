// K7, what both forms of the tracker (k_lk.hip, k_lk2.hip) are made of: arguments, patch staging, LDS reads, exact wave sums, weights, runs
#pragma once
#include "common.hpp"

#ifndef KM_LK_WAVES
#define KM_LK_WAVES 0   // occupancy target (waves per SIMD); 0 = leave it to the register allocator
#endif
#if KM_LK_WAVES
#define KM_LK_OCC __attribute__((amdgpu_waves_per_eu(KM_LK_WAVES, KM_LK_WAVES)))
#else
#define KM_LK_OCC
#endif

#include <float.h>
#include <type_traits>

struct lk_args {
    km_pyr A, B;
    const float *pts_in;
    const int *d_n;
    int n_max, win, max_count, backward;
    int general_templates;   // (development build, KARIOS_HIP_LK_GENERAL: every template through the general two-row form - A/B of the degenerate-weight forms)
    int lk_reuse;            // "lk_reuse" option: 1 = the second form keeps a run's byte pairs while the integer position stands, 0 = cuts them every iteration
    double epsilon;
    float *p1, *p0r;
    int *left_band;   // row-band mode: raised when a point's window needs rows outside the resident band
};

// rows [gy0, gy0 + rows) of level `level`, clipped to the image (REFLECT_101 only folds rows back INTO that range), resident?
__device__ __forceinline__ bool lk_rows_resident(const km_pyr &P, int level, int gy0, int rows)
{
    if (P.Hres[level] == 0) return true;
    const int lo = max(gy0, 0), hi = min(gy0 + rows, P.H[level]);
    // a window that overhangs the top / bottom of the image mirrors rows within `rows` of that border
    const int need_lo = gy0 < 0 ? 0 : lo, need_hi = gy0 + rows > P.H[level] ? P.H[level] : hi;
    return need_lo >= P.oy[level] && need_hi <= P.oy[level] + P.Hres[level] && (gy0 >= 0 || P.oy[level] == 0) &&
           (gy0 + rows <= P.H[level] || P.oy[level] + P.Hres[level] == P.H[level]);
}

__device__ __forceinline__ void lk_weights(float a, float b, int &w00, int &w01, int &w10, int &w11)
{
    const float oma = 1.f - a, omb = 1.f - b;
    const float t00 = oma * omb, t01 = a * omb, t10 = oma * b;
    w00 = __float2int_rn(t00 * 16384.f);
    w01 = __float2int_rn(t01 * 16384.f);
    w10 = __float2int_rn(t10 * 16384.f);
    w11 = 16384 - w00 - w01 - w10;
}

// Stage a rows x cols byte patch whose top-left pixel is (gx0, gy0) into LDS (row pitch `pitch`, multiple of 4).
// Inside the image: (unaligned) dword loads, ALL issued before the first one is consumed - a loop that loads and stores
// per trip exposes the memory latency once per trip (9 trips per level and pass at winSize 25).  Addresses are a uniform
// base + 32-bit lane offset, so a slot in flight costs one register.  Otherwise byte loads with REFLECT_101 (OpenCV pads
// every pyramid level by winSize with that border).
template <int MAXIT> struct lk_patch_regs {
    uint32_t v[MAXIT];
};

// (the half of the test that depends on the sizes alone: lk_launch.hpp proves it at compile time for every window the kernels serve)
constexpr bool lk_patch_fits(int rows, int cols, int maxit) { return rows * ((cols + 3) >> 2) <= 64 * maxit && rows * ((cols + 3) >> 2) < 1024 && cols <= 64; }
__device__ __forceinline__ bool lk_patch_inside(int IW, int IH, int gx0, int gy0, int rows, int cols, int maxit)
{
    return gx0 >= 0 && gy0 >= 0 && gx0 + cols + 4 <= IW && gy0 + rows <= IH && lk_patch_fits(rows, cols, maxit);
}

template <int MAXIT>
__device__ __forceinline__ void stage_patch_issue(const uint8_t *__restrict__ img, int IW, int gx0, int gy0, int rows, int cols, lk_patch_regs<MAXIT> &rg)
{
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));   // opaque: keeps the per-slot index arithmetic local (hoisted out of the level loop it costs ~30 VGPRs)
    const int nw = (cols + 3) >> 2, total = rows * nw;
    const unsigned inv_nw = 65536u / (unsigned)nw + 1u;   // i / nw == (i * inv_nw) >> 16 for i < 1024, nw <= 16 (a runtime division costs ~25 instructions)
    const unsigned base = (unsigned)gy0 * (unsigned)IW + (unsigned)gx0;
#pragma unroll
    for (int it = 0; it < MAXIT; it++) {
        const int i = min(lane + 64 * it, total - 1);     // surplus trips re-read the last word (never stored)
        const int r = (int)(((unsigned)i * inv_nw) >> 16), d = i - r * nw;
        const unsigned off = base + (unsigned)r * (unsigned)IW + 4u * (unsigned)d;
        __builtin_memcpy(&rg.v[it], img + off, 4);
    }
}

template <int MAXIT>
__device__ __forceinline__ void stage_patch_commit(int rows, int cols, uint8_t *lds, int pitch, const lk_patch_regs<MAXIT> &rg)
{
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    const int nw = (cols + 3) >> 2, total = rows * nw;
    const unsigned inv_nw = 65536u / (unsigned)nw + 1u;
#pragma unroll
    for (int it = 0; it < MAXIT; it++) {
        const int i = lane + 64 * it;
        if (i < total) {
            const int r = (int)(((unsigned)i * inv_nw) >> 16), d = i - r * nw;
            *(uint32_t *)(lds + r * pitch + 4 * d) = rg.v[it];
        }
    }
}

__device__ __forceinline__ void stage_patch_border(const uint8_t *__restrict__ img, int IW, int IH, int gx0, int gy0, int rows, int cols,
                                                   uint8_t *lds, int pitch)
{
    for (int i = threadIdx.x & 63; i < rows * cols; i += 64) {
        const int r = i / cols, cx = i - r * cols;
        lds[r * pitch + cx] = img[(size_t)km_reflect101(gy0 + r, IH) * IW + km_reflect101(gx0 + cx, IW)];
    }
}

template <int MAXIT>
__device__ __forceinline__ void stage_patch(const uint8_t *__restrict__ img, int IW, int IH, int gx0, int gy0, int rows, int cols,
                                            uint8_t *lds, int pitch)
{
    if (lk_patch_inside(IW, IH, gx0, gy0, rows, cols, MAXIT)) {
        lk_patch_regs<MAXIT> rg;
        stage_patch_issue<MAXIT>(img, IW, gx0, gy0, rows, cols, rg);
        stage_patch_commit<MAXIT>(rows, cols, lds, pitch, rg);
    } else {
        stage_patch_border(img, IW, IH, gx0, gy0, rows, cols, lds, pitch);
    }
}

// exact wave sum of an int64 whose per-lane magnitude is < 2^31: two int32 DPP reductions (low 16 bits / rest)
__device__ __forceinline__ int wave_sum_i32_dpp(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ long long wave_sum_split(int v)
{
    const int lo = v & 0xffff, hi = v >> 16;
    return ((long long)wave_sum_i32_dpp(hi) << 16) + (long long)wave_sum_i32_dpp(lo);
}
// the same when the sum over FOUR NEIGHBOURING LANES (4 i .. 4 i + 3) has a magnitude < 2^31: the first two steps of the scan add at
// most four lanes - still an int32 - so they run once, unsplit; only the remaining four steps need the two 16-bit halves.  A bound on
// the single lane is not enough: the four lanes of a group hold runs of the same window rows and reach their largest values together
// (0 / 255 stripes, tests/lk_cases.py).  Callers: lk_mismatch_sum below.
__device__ __forceinline__ long long wave_sum_split4(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    int lo = v & 0xffff, hi = v >> 16;
    lo += __builtin_amdgcn_update_dpp(0, lo, 0x114, 0xf, 0xf, false);
    hi += __builtin_amdgcn_update_dpp(0, hi, 0x114, 0xf, 0xf, false);
    lo += __builtin_amdgcn_update_dpp(0, lo, 0x118, 0xf, 0xf, false);
    hi += __builtin_amdgcn_update_dpp(0, hi, 0x118, 0xf, 0xf, false);
    lo += __builtin_amdgcn_update_dpp(0, lo, 0x142, 0xa, 0xf, false);
    hi += __builtin_amdgcn_update_dpp(0, hi, 0x142, 0xa, 0xf, false);
    lo += __builtin_amdgcn_update_dpp(0, lo, 0x143, 0xc, 0xf, false);
    hi += __builtin_amdgcn_update_dpp(0, hi, 0x143, 0xc, 0xf, false);
    return ((long long)__builtin_amdgcn_readlane(hi, 63) << 16) + (long long)__builtin_amdgcn_readlane(lo, 63);
}

// Eight patch bytes from a byte-aligned LDS address as three ALIGNED dwords + two v_alignbyte.  A ds_read_b64 whose address is
// not a multiple of 8 takes the LDS unit's unaligned path: ~55 cycles per wave instruction against ~4 aligned (PMC, round 5:
// SQ_LDS_UNALIGNED_STALL = 96 % of SQ_LDS_IDX_ACTIVE, the LDS unit busy 83 % of the kernel - the tracker was LDS-bound on it).
// Reads up to 3 bytes in front of p (same patch: its base is 16-byte aligned) and 4 behind p + 8 (the pitch / tail slack of lk2_geo).
__device__ __forceinline__ uint2 lk_lds_read8(const uint8_t *p, unsigned sh)
{
    const uint32_t *q = (const uint32_t *)(p - sh);
    const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
    uint2 r;
    r.x = __builtin_amdgcn_alignbyte(d1, d0, sh);
    r.y = __builtin_amdgcn_alignbyte(d2, d1, sh);
    return r;
}
__device__ __forceinline__ unsigned lk_lds_shift(const uint8_t *p) { return (unsigned)(size_t)p & 3u; }

// Window pixels are dealt to the lanes as horizontal RUNS of LK_RUN pixels (run r = t * 64 + lane covers columns
// [x0, x0 + n) of window row y).  A run needs LK_RUN + 1 consecutive bytes from each of two rows of the search patch:
// two (unaligned) 8-byte LDS reads per run and iteration instead of four byte reads per pixel, the byte pairs are cut out
// with v_perm and the bilinear interpolation is two v_dot2_i32_i16 per pixel; the mismatch vector is accumulated with
// v_dot2_i32_i16 over pixel pairs as well.  All arithmetic is the exact integer arithmetic of cv::calcOpticalFlowPyrLK.
#define LK_RUN 5
// every wavefront works on its own LDS region: only the compiler must be kept from reordering LDS traffic across the phases
#define LK_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
typedef short lk_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ lk_s2 lk_as_s2(uint32_t v) { return __builtin_bit_cast(lk_s2, v); }
__device__ __forceinline__ uint32_t lk_pack16(int lo, int hi) { return __builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x05040100u); }

// Wave sum of a mismatch component of the resident-patch form.  A pixel contributes at most 8160 x 4080 (Q5 difference of two uint8
// x Scharr value), a lane holds 5 NR pixels, so four lanes stay below 2^31 for NR <= 3 (4 x 15 x 8160 x 4080 = 2.0e9: winSize <= 30,
// the win-25 kernels among them) and wave_sum_split4 is exact.  NR = 4 (winSize 31 .. 35) reaches 2.66e9 and NR = 5 (36 .. 40) 3.33e9
// on saturated stripes - the unsplit steps wrapped and b was off by a multiple of 2^32 x 2^-20 - so those split before the first step.
template <int NR>
__device__ __forceinline__ long long lk_mismatch_sum(int v)
{
    if constexpr (4ll * LK_RUN * NR * 8160 * 4080 < (1ll << 31)) return wave_sum_split4(v);
    else return wave_sum_split(v);
}

// OpenCV's oscillation stop (lkpyramid.cpp, LKTrackerInvoker): `std::abs(delta.x + prevDelta.x) < 0.01 && std::abs(delta.y +
// prevDelta.y) < 0.01` - the float32 sum, its float32 magnitude, promoted to double against the DOUBLE literal 0.01.  0.01f is
// 0.00999999977...: a sum of exactly 0.01f passes OpenCV's test and would fail `< 0.01f` (tests/test_gpu_parity.py::test_lk_oscillation_literal).
__device__ __host__ __forceinline__ bool lk_oscillates(float ddx, float pdx, float ddy, float pdy)
{
    return (double)fabsf(ddx + pdx) < 0.01 && (double)fabsf(ddy + pdy) < 0.01;
}

// (a value every lane holds, said so: it and every test on it stay in scalar registers)
__device__ __forceinline__ float lk_uniform(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

// the lane's t-th run: y | x0 << 8 | n << 16 (n = 0: the lane has no t-th run).  By value, one run per call: a kernel's array filled
// through a reference compiles to other code than the loop written in the kernel, this form to the same.
__device__ __forceinline__ int lk_run_desc(int win, int t)
{
    const int rpr = (win + LK_RUN - 1) / LK_RUN, total = win * rpr;
    const int r = t * 64 + (int)(threadIdx.x & 63);
    const int y = r / rpr, x0 = (r - y * rpr) * LK_RUN;
    return r < total ? (y | (x0 << 8) | (min(LK_RUN, win - x0) << 16)) : 0;
}
