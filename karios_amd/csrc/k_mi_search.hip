// The mutual-information search around each key point (k_mi_search.hpp; arithmetic: mi_search_math.hpp).  One wavefront per key point
// and per workgroup, no workgroup barrier, key points dealt to the XCDs in contiguous eighths (neighbouring regions overlap in one L2).
//
// Integer pixels: the wave stages the (57 + 2R)^2 region of the monitored raster around the centre compute_mutual_info scores in its LDS
// once, as 16-bit values (int16 biased by 2^15), and every one of the (2R+1)^2 chips is then cut from LDS - the region is read from L2
// once.  Lane = chip column (57 of 64 lanes work), one chip row per step.  The reference chip is binned ONCE: its 57 bins per lane stay
// in registers (premultiplied by 32), the sum over its marginal is taken once.  Per offset: the chip's 57 pixels per lane -> registers,
// minimum / maximum by a wave reduction, mi::magic's constants, 3249 LDS atomics into the 1024-cell histogram, the column marginal
// (lane b < 32: column b), and the two table sums - T[count] from mi_clogc_q36.inc, 64-bit integers - as integer wave reductions; the
// cells are cleared as they are read.  float32 pixels take the plainer form: no staged region (a chip's pixels come from global memory,
// through L1 / L2, at every offset), numpy's 33 edges per chip in LDS as mi_kernel (k_mi.hip) keeps them, a search per pixel; counts and
// value rule are the same.
//
// The table lives in global memory (26 KB, read through L1): most cells hold 0 or a small count, so the loads fall into its first lines.
// LDS per workgroup (dynamic, by R): 16 S^2 (two surfaces) + 4096 (histogram) + 2 (57 + 2R)^2 (region) bytes = 11.9 / 13.8 / 19.4 KB at
// R = 2 / 4 / 8 for integer pixels, 16 S^2 + 4096 + 264 for float32: see DESIGN.md section 23 for the occupancy that gives.
#include "common.hpp"
#include "k_mi_search.hpp"

#include <type_traits>

#define MS_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

namespace {

__device__ const long long ms_table[ms::TABLE] = {
#include "mi_clogc_q36.inc"
};

__device__ __forceinline__ long long ms_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <typename T>
__device__ __forceinline__ unsigned ms_biased(T v)
{
    if constexpr (std::is_signed<T>::value) return ((unsigned)(int)v + 32768u) & 0xffffu;
    else return (unsigned)v;
}

// The bin rule of the chip whose column `lane` is pv[0 .. 57) (lanes >= 57: not part of the chip).  Integer pixels: the magic constants of
// the chip's range.  float32: numpy's edges -> `edges` (LDS, 33 values; the caller synchronises the wave before it reads them); *finite
// false: the chip holds a NaN or an infinity.
template <bool F, typename P, typename Rule>
__device__ __forceinline__ Rule ms_rule(const P (&pv)[ms::CHIP], bool on, int lane, double *edges, bool *finite)
{
    *finite = true;
    if constexpr (F) {
        float mn = INFINITY, mx = -INFINITY;
        bool good = true;
#pragma unroll
        for (int r = 0; r < ms::CHIP; r++) { mn = fminf(mn, pv[r]); mx = fmaxf(mx, pv[r]); good = good && fabsf(pv[r]) <= 3.4028234663852886e38f; }
        if (!on) { mn = INFINITY; mx = -INFINITY; good = true; }
        *finite = __all(good);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
        const ms::float_rule rule = ms::float_bins((double)mn, (double)mx);
        if (lane <= ms::BINS) edges[lane] = ms::float_edge(lane, rule);
        return rule;
    } else {
        unsigned mn = 0xffffu, mx = 0u;
#pragma unroll
        for (int r = 0; r < ms::CHIP; r++) { mn = min(mn, pv[r]); mx = max(mx, pv[r]); }
        if (!on) { mn = 0xffffu; mx = 0u; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn = min(mn, (unsigned)__shfl_xor((int)mn, o)); mx = max(mx, (unsigned)__shfl_xor((int)mx, o)); }
        return ms::int_bins(mn, mx);
    }
}

template <bool F, typename P, typename Rule>
__device__ __forceinline__ int ms_bin(P v, const Rule &rule, const double *edges)
{
    if constexpr (F) return ms::float_bin((double)v, rule, edges);
    else return ms::int_bin(v, rule);
}

// the wave's surfaces z, zmi (LDS, complete and visible) -> the row's outputs; the surface itself where the caller asked for it
__device__ __forceinline__ void ms_outputs(const kms_args &a, const double *z, const double *zmi, int lane, int k, int X0, int Y0, int X1, int Y1)
{
    const int R = a.radius, S = 2 * R + 1;
    int bi = -1;
    double bv = 0.0;
    for (int i = lane; i < S * S; i += 64) {
        const double v = z[i];
        if (a.surface) a.surface[(size_t)k * S * S + i] = v;
        if (zs::better(v, i, bv, bi)) { bv = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {     // (value, raster index): the first of equal values wins
        const double ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (zs::better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0)
        ms::finish(z, zmi, R, bi, X0, Y0, X1, Y1, a.offset + 2 * (size_t)k, a.peak + k, a.peak_mi + k, a.shift + 2 * (size_t)k, a.status + k);
}

template <typename T>
__global__ __launch_bounds__(64) void mi_search_kernel(const kms_args a)
{
    extern __shared__ __attribute__((aligned(16))) char ms_lds[];
    constexpr bool F = std::is_same<T, float>::value;
    using P = typename std::conditional<F, float, unsigned>::type;
    using Rule = typename std::conditional<F, ms::float_rule, ms::int_rule>::type;
    const int lane = threadIdx.x;
    // the key point of this wave: contiguous eighths of the rows per XCD
    const unsigned per = ((unsigned)a.n + KM_XCDS - 1) / KM_XCDS, row = (blockIdx.x % KM_XCDS) * per + blockIdx.x / KM_XCDS;
    if (blockIdx.x / KM_XCDS >= per || row >= (unsigned)a.n) return;
    const int k = (int)row, R = a.radius, S = 2 * R + 1, SS = S * S, RW = ms::CHIP + 2 * R;
    int X0, Y0, X1, Y1;
    if (!zs::centres(a.x0[k], a.y0[k], a.dx[k], a.dy[k], a.Href, a.Wref, a.Hmon, a.Wmon, X0, Y0, X1, Y1)) {
        if (a.surface)
            for (int i = lane; i < SS; i += 64) a.surface[(size_t)k * SS + i] = zs::quiet_nan();
        if (lane == 0) ms::skipped(a.offset + 2 * (size_t)k, a.peak + k, a.peak_mi + k, a.shift + 2 * (size_t)k, a.status + k);
        return;
    }
    double *z = (double *)ms_lds, *zmi = z + SS;
    unsigned *hist = (unsigned *)(zmi + SS);
    double *edges = (double *)(hist + ms::CELLS);               // float32 only: 33 values
    uint16_t *reg = (uint16_t *)(hist + ms::CELLS);             // integer types only: RW x RW
    const bool on = lane < ms::CHIP;
    const int col = on ? lane : 0;
#pragma unroll
    for (int i = 0; i < ms::CELLS / 64; i++) hist[i * 64 + lane] = 0;
    for (int i = lane; i < SS; i += 64) z[i] = zmi[i] = zs::quiet_nan();
    if constexpr (!F) {
        // the region whose first pixel is (X1 - R - 28, Y1 - R - 28), row by row; pixels outside the raster (only chips that are not
        // scored hold any): 0
        const T *mon = (const T *)a.mon;
        const int bx = X1 - R - ms::MARGIN, by = Y1 - R - ms::MARGIN;
        for (int r = 0; r < RW; r++) {
            const int gy = by + r;                                  // (wave-uniform)
            for (int cx = lane; cx < RW; cx += 64) {
                const int gx = bx + cx;
                unsigned v = 0;
                if (gy >= 0 && gy < a.Hmon && gx >= 0 && gx < a.Wmon) v = ms_biased<T>(mon[(ptrdiff_t)gy * a.smon + gx]);
                reg[r * RW + cx] = (uint16_t)v;
            }
        }
    }
    // the reference chip: binned once, bins x 32 in registers; the sum over its marginal
    P pv[ms::CHIP];
    unsigned rb[ms::CHIP];
    {
        const T *pr = (const T *)a.ref + (ptrdiff_t)(Y0 - ms::MARGIN) * a.sref + (X0 - ms::MARGIN) + col;
#pragma unroll
        for (int r = 0; r < ms::CHIP; r++) {
            if constexpr (F) pv[r] = pr[(ptrdiff_t)r * a.sref];
            else pv[r] = ms_biased<T>(pr[(ptrdiff_t)r * a.sref]);
        }
    }
    bool ref_ok;
    const Rule ref_rule = ms_rule<F, P, Rule>(pv, on, lane, edges, &ref_ok);
    MS_WAVE_SYNC();
    long long Sx = 0;
    if (ref_ok) {                                                   // (wave-uniform)
        if (on) {
#pragma unroll
            for (int r = 0; r < ms::CHIP; r++) {
                const int b = ms_bin<F, P, Rule>(pv[r], ref_rule, edges);
                rb[r] = (unsigned)b * ms::BINS;
                atomicAdd(&hist[b], 1u);
            }
        }
        MS_WAVE_SYNC();
        if (lane < ms::BINS) { Sx = ms_table[hist[lane]]; hist[lane] = 0; }
        Sx = ms_wave_sum(Sx);
        MS_WAVE_SYNC();
        const long long L = ms_table[ms::NPX];
        for (int oy = 0; oy < S; oy++)
            for (int ox = 0; ox < S; ox++) {
                const int x = X1 + ox - R, y = Y1 + oy - R;
                if (!ms::chip_inside(x, y, a.Wmon, a.Hmon)) continue;     // (wave-uniform; the value stays NaN)
                if constexpr (F) {
                    const T *pm = (const T *)a.mon + (ptrdiff_t)(y - ms::MARGIN) * a.smon + (x - ms::MARGIN) + col;
#pragma unroll
                    for (int r = 0; r < ms::CHIP; r++) pv[r] = pm[(ptrdiff_t)r * a.smon];
                } else {
                    const uint16_t *pm = reg + oy * RW + ox + col;
#pragma unroll
                    for (int r = 0; r < ms::CHIP; r++) pv[r] = pm[r * RW];
                }
                bool mon_ok;
                const Rule rule = ms_rule<F, P, Rule>(pv, on, lane, edges, &mon_ok);
                MS_WAVE_SYNC();
                if (mon_ok) {                                           // (wave-uniform)
                    if (on) {
#pragma unroll
                        for (int r = 0; r < ms::CHIP; r++) atomicAdd(&hist[rb[r] + (unsigned)ms_bin<F, P, Rule>(pv[r], rule, edges)], 1u);
                    }
                    MS_WAVE_SYNC();
                    long long Sy = 0, Sxy = 0;
                    if (lane < ms::BINS) {
                        unsigned ry = 0;
#pragma unroll 8
                        for (int j = 0; j < ms::BINS; j++) ry += hist[j * ms::BINS + lane];
                        Sy = ms_table[ry];
                    }
                    MS_WAVE_SYNC();
#pragma unroll
                    for (int i = 0; i < ms::CELLS / 64; i++) {
                        const unsigned c = hist[i * 64 + lane];
                        hist[i * 64 + lane] = 0;
                        Sxy += ms_table[c];
                    }
                    Sy = ms_wave_sum(Sy); Sxy = ms_wave_sum(Sxy);
                    if (lane == 0) {
                        const int64_t num = ms::numerator(L, Sx, Sy), den = ms::denominator(L, Sxy);
                        z[oy * S + ox] = ms::studholme(num, den);
                        zmi[oy * S + ox] = ms::mi_score(num, den);
                    }
                }
                MS_WAVE_SYNC();
            }
    }
    MS_WAVE_SYNC();
    ms_outputs(a, z, zmi, lane, k, X0, Y0, X1, Y1);
}

template <typename T>
int ms_launch(km_ctx *c, const kms_args &a)
{
    const int S = 2 * a.radius + 1, RW = ms::CHIP + 2 * a.radius;
    const size_t tail = std::is_same<T, float>::value ? (size_t)(ms::BINS + 1) * sizeof(double) : (((size_t)RW * RW * sizeof(uint16_t) + 15) & ~(size_t)15);
    const size_t lds = (size_t)2 * S * S * sizeof(double) + (size_t)ms::CELLS * sizeof(unsigned) + tail;
    mi_search_kernel<T><<<km_xcd_grid((unsigned)a.n), 64, lds, c->stream>>>(a);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

}  // namespace

int kms_search(km_ctx *c, const kms_args &a)
{
    if (a.n <= 0) return KM_OK;
    switch (a.dtype) {
    case KM_U8: return ms_launch<uint8_t>(c, a);
    case KM_U16: return ms_launch<uint16_t>(c, a);
    case KM_I16: return ms_launch<int16_t>(c, a);
    case KM_F32: return ms_launch<float>(c, a);
    default: return KM_E_ARG;
    }
}
