// The ZNCC search around each key point (k_zncc_search.hpp; arithmetic: zncc_math.hpp).  One wavefront per key point, four per workgroup,
// no workgroup barrier: a wave stages the (43 + 2R)^2 region of the monitored raster around the centre compute_zncc scores and the 43^2
// template of the reference raster in its own LDS, once, and every one of the (2R+1)^2 offsets is then evaluated from LDS - the region
// is read (2R+1)^2 times without touching L2 again.
//
// Integer pixels: lane = (group g, column offset ox), 64 / S groups of S lanes; a group owns one row offset oy at a time.  Per template
// pixel a lane reads the template value (one address for the whole wave: a broadcast) and its own region pixel (the lanes of a group
// read neighbouring halfwords) and updates S_b, S_bb, S_ab; the template's S_a, S_aa are summed once.  All moments are exact integers
// (uint8: 32 bits, < 2^27; 16-bit types: 64 bits, < 2^43), so the value is zncc_math.hpp's int_value of the same integers on every
// device and on the host.  float32 pixels take the plainer form of zncc_kernel (k_zncc.hip): the centred template in registers, lane =
// pixel, two float64 passes per offset over the staged region, three wave reductions.
#include "common.hpp"
#include "k_zncc_search.hpp"

#include <type_traits>

#define ZS_MAX_S (2 * zs::MAX_RADIUS + 1)
#define ZS_MAX_RW (zs::SIDE + 2 * zs::MAX_RADIUS)
#define ZS_PER_LANE ((zs::NPX + 63) / 64)
#define ZS_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

namespace {

__device__ __forceinline__ double zs_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The key point of this wave (contiguous eighths of the rows per XCD, as zncc_kernel deals them) and its centres.
// false: no row for this wave.  *ok false: the row is skipped, and its outputs are written here.
__device__ __forceinline__ bool zs_row(const kzs_args &a, int lane, int &k, int &X0, int &Y0, int &X1, int &Y1, bool &ok)
{
    const unsigned per = ((unsigned)(a.n + 3) / 4 + KM_XCDS - 1) / KM_XCDS, blk = (blockIdx.x % KM_XCDS) * per + blockIdx.x / KM_XCDS;
    k = (int)blk * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (blockIdx.x / KM_XCDS >= per || k >= a.n) return false;
    ok = zs::centres(a.x0[k], a.y0[k], a.dx[k], a.dy[k], a.Href, a.Wref, a.Hmon, a.Wmon, X0, Y0, X1, Y1);
    if (!ok) {
        const int S = 2 * a.radius + 1;
        if (a.surface)
            for (int i = lane; i < S * S; i += 64) a.surface[(size_t)k * S * S + i] = zs::quiet_nan();
        if (lane == 0) zs::skipped(a.offset + 2 * (size_t)k, a.peak + k, a.shift + 2 * (size_t)k, a.status + k);
    }
    return true;
}

// the wave's surface z (LDS, complete and visible) -> the row's outputs; the surface itself where the caller asked for it
__device__ __forceinline__ void zs_outputs(const kzs_args &a, const double *z, int lane, int k, int X0, int Y0, int X1, int Y1)
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
    if (lane == 0) zs::finish(z, R, bi, X0, Y0, X1, Y1, a.offset + 2 * (size_t)k, a.peak + k, a.shift + 2 * (size_t)k, a.status + k);
}

template <typename T>
__device__ __forceinline__ unsigned zs_biased(T v)
{
    if constexpr (std::is_signed<T>::value) return ((unsigned)(int)v + 32768u) & 0xffffu;
    else return (unsigned)v;
}

// the RW x RW region of `mon` whose first pixel is (bx, by) -> dst, row by row (lane = column, RW <= 59); pixels outside the raster: 0
template <typename T, typename D, typename F>
__device__ __forceinline__ void zs_stage(const T *__restrict__ img, int H, int W, ptrdiff_t stride, int bx, int by, int RW, int lane, D *dst, F convert)
{
    const int gx = bx + lane;
    const bool col = lane < RW && gx >= 0 && gx < W;
#pragma unroll 4
    for (int r = 0; r < RW; r++) {
        const int gy = by + r;                                  // (wave-uniform)
        D v = 0;
        if (col && gy >= 0 && gy < H) v = convert(img[(ptrdiff_t)gy * stride + gx]);
        if (lane < RW) dst[r * RW + lane] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void zncc_search_int_kernel(const kzs_args a)
{
    __shared__ uint16_t s_reg[4][ZS_MAX_RW * ZS_MAX_RW + 1];
    __shared__ uint16_t s_tpl[4][zs::NPX + 1];
    __shared__ double s_z[4][ZS_MAX_S * ZS_MAX_S];
    using acc_t = typename std::conditional<sizeof(T) == 1, unsigned, unsigned long long>::type;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int k, X0, Y0, X1, Y1;
    bool ok;
    if (!zs_row(a, lane, k, X0, Y0, X1, Y1, ok) || !ok) return;
    const int R = a.radius, S = 2 * R + 1, RW = zs::SIDE + 2 * R;
    uint16_t *reg = s_reg[w], *tpl = s_tpl[w];
    double *z = s_z[w];
    auto conv = [](T v) { return (uint16_t)zs_biased<T>(v); };
    zs_stage<T, uint16_t>((const T *)a.mon, a.Hmon, a.Wmon, a.smon, X1 - R - zs::HW, Y1 - R - zs::HW, RW, lane, reg, conv);
    zs_stage<T, uint16_t>((const T *)a.ref, a.Href, a.Wref, a.sref, X0 - zs::HW, Y0 - zs::HW, zs::SIDE, lane, tpl, conv);
    ZS_WAVE_SYNC();
    // the template's moments, once
    unsigned sa = 0;
    unsigned long long saa = 0;
    for (int i = lane; i < zs::NPX; i += 64) { const unsigned t = tpl[i]; sa += t; saa += (unsigned long long)t * t; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sa += (unsigned)__shfl_xor((int)sa, o); saa += (unsigned long long)__shfl_xor((long long)saa, o); }
    const long long v1 = zs::variance_n2((long long)sa, (long long)saa);
    const int G = 64 / S, g = lane / S, ox = lane - g * S;
    for (int oy0 = 0; oy0 < S; oy0 += G) {
        const int oy = oy0 + g;
        if (g < G && oy < S) {
            const uint16_t *pr = reg + oy * RW + ox;
            unsigned sb = 0;
            acc_t sbb = 0, sab = 0;
#pragma unroll 1
            for (int r = 0; r < zs::SIDE; r++) {
                const uint16_t *prr = pr + r * RW, *ptr = tpl + r * zs::SIDE;
#pragma unroll
                for (int cx = 0; cx < zs::SIDE; cx++) {
                    const unsigned t = ptr[cx], p = prr[cx];
                    sb += p;
                    sbb += (acc_t)p * p;
                    sab += (acc_t)t * p;
                }
            }
            double v = zs::quiet_nan();
            if (zs::window_inside(X1 + ox - R, Y1 + oy - R, a.Wmon, a.Hmon))
                v = zs::int_value(zs::covariance_n2((long long)sa, (long long)sb, (long long)sab), v1, zs::variance_n2((long long)sb, (long long)sbb));
            z[oy * S + ox] = v;
        }
    }
    ZS_WAVE_SYNC();
    zs_outputs(a, z, lane, k, X0, Y0, X1, Y1);
}

__global__ __launch_bounds__(256) void zncc_search_f32_kernel(const kzs_args a)
{
    __shared__ float s_reg[4][ZS_MAX_RW * ZS_MAX_RW];
    __shared__ double s_z[4][ZS_MAX_S * ZS_MAX_S];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int k, X0, Y0, X1, Y1;
    bool ok;
    if (!zs_row(a, lane, k, X0, Y0, X1, Y1, ok) || !ok) return;
    const int R = a.radius, S = 2 * R + 1, RW = zs::SIDE + 2 * R;
    float *reg = s_reg[w];
    double *z = s_z[w];
    zs_stage<float, float>((const float *)a.mon, a.Hmon, a.Wmon, a.smon, X1 - R - zs::HW, Y1 - R - zs::HW, RW, lane, reg, [](float v) { return v; });
    // the template: read once, centred, in registers; off[i] = where pixel i of a window sits in the region, relative to the window's origin
    const float *pa = (const float *)a.ref + (ptrdiff_t)(Y0 - zs::HW) * a.sref + (X0 - zs::HW);
    double va[ZS_PER_LANE];
    int off[ZS_PER_LANE];
    double s1 = 0.0;
#pragma unroll
    for (int i = 0; i < ZS_PER_LANE; i++) {
        const int idx = i * 64 + lane;
        va[i] = 0.0; off[i] = 0;
        if (idx < zs::NPX) {
            const int r = idx / zs::SIDE, cx = idx - r * zs::SIDE;
            va[i] = (double)pa[(ptrdiff_t)r * a.sref + cx];
            off[i] = r * RW + cx;
            s1 += va[i];
        }
    }
    const double m1 = zs_wave_sum(s1) / (double)zs::NPX;
    double q1 = 0.0;
#pragma unroll
    for (int i = 0; i < ZS_PER_LANE; i++) {
        va[i] = i * 64 + lane < zs::NPX ? va[i] - m1 : 0.0;
        q1 += va[i] * va[i];
    }
    const double sd1 = sqrt(zs_wave_sum(q1) / (double)zs::NPX);
    ZS_WAVE_SYNC();
    for (int oy = 0; oy < S; oy++)
        for (int ox = 0; ox < S; ox++) {
            const float *pw = reg + oy * RW + ox;
            double s2 = 0.0;
#pragma unroll
            for (int i = 0; i < ZS_PER_LANE; i++)
                if (i * 64 + lane < zs::NPX) s2 += (double)pw[off[i]];
            const double m2 = zs_wave_sum(s2) / (double)zs::NPX;
            double q2 = 0.0, cc = 0.0;
#pragma unroll
            for (int i = 0; i < ZS_PER_LANE; i++)
                if (i * 64 + lane < zs::NPX) {
                    const double b = (double)pw[off[i]] - m2;
                    q2 += b * b; cc += va[i] * b;
                }
            q2 = zs_wave_sum(q2); cc = zs_wave_sum(cc);
            const double sd2 = sqrt(q2 / (double)zs::NPX);
            if (lane == 0)
                z[oy * S + ox] = (!zs::window_inside(X1 + ox - R, Y1 + oy - R, a.Wmon, a.Hmon) || sd1 == 0.0 || sd2 == 0.0)
                                     ? zs::quiet_nan() : cc / (sd1 * sd2) / (double)zs::NPX;
        }
    ZS_WAVE_SYNC();
    zs_outputs(a, z, lane, k, X0, Y0, X1, Y1);
}

}  // namespace

int kzs_search(km_ctx *c, const kzs_args &a)
{
    if (a.n <= 0) return KM_OK;
    const unsigned nb = km_xcd_grid((unsigned)((a.n + 3) / 4));
    switch (a.dtype) {
    case KM_U8: zncc_search_int_kernel<uint8_t><<<nb, 256, 0, c->stream>>>(a); break;
    case KM_U16: zncc_search_int_kernel<uint16_t><<<nb, 256, 0, c->stream>>>(a); break;
    case KM_I16: zncc_search_int_kernel<int16_t><<<nb, 256, 0, c->stream>>>(a); break;
    case KM_F32: zncc_search_f32_kernel<<<nb, 256, 0, c->stream>>>(a); break;
    default: return KM_E_ARG;
    }
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
