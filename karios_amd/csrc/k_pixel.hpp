// Device-side pixel helpers shared by the dense kernel files that came out of one (k_raster.hip, k_lap.hip) and by the key-point chips
// (k_chips.hip): pixel-type traits, wave reductions, the exact uint8 stretch and the valid-pixel rule of the automatic mask.  Device
// inline code only; included by those files and nothing else.
#pragma once
#include "common.hpp"

#include <type_traits>

// ------------------------------------------------------------------ helpers
// 24-bit multiply-add: full-rate v_mad_i32_i24 (a plain int multiply is a quarter-rate v_mul_lo_u32);
// every use below has both factors within +-2^23 and a product within int32.
__device__ __forceinline__ int mad24(int a, int b, int c) { return __mul24(a, b) + c; }

template <typename T> struct px_traits;
template <> struct px_traits<uint8_t> { using acc = int; static constexpr int code = KM_U8; };
template <> struct px_traits<uint16_t> { using acc = int; static constexpr int code = KM_U16; };
template <> struct px_traits<int16_t> { using acc = int; static constexpr int code = KM_I16; };
template <> struct px_traits<float> { using acc = float; static constexpr int code = KM_F32; };

__device__ __forceinline__ double wave_min(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// stretch one raw value to uint8 exactly like numpy does in _to_uint8 (klt.py:48):
// integer dtypes in fp64, float32 in fp32; truncating cast; NaN -> 0.
template <typename T>
__device__ __forceinline__ unsigned stretch_u8(T v, double mn, double range, bool degenerate)
{
    if constexpr (sizeof(T) == 1) {
        return (unsigned)v;
    } else if constexpr (px_traits<T>::code == KM_F32) {
        if (degenerate) return 0u;
        float t = __fmul_rn(__fdiv_rn(__fsub_rn(v, (float)mn), (float)range), 255.0f);
        return (t != t) ? 0u : (unsigned)(int)t;
    } else {
        if (degenerate) return 0u;
        double t = __dmul_rn(__ddiv_rn(__dsub_rn((double)v, mn), range), 255.0);
        return (unsigned)(int)t;
    }
}

struct nodata_t {
    double mon, ref;
    int has_mon, has_ref;
};

template <typename T>
__device__ __forceinline__ bool px_valid(T a /*mon*/, T b /*ref*/, const nodata_t &nd)
{
    bool ok = (a != (T)0) && (b != (T)0);
    if constexpr (px_traits<T>::code == KM_F32) ok = ok && isfinite(a) && isfinite(b);
    if (nd.has_mon) ok = ok && ((double)a != nd.mon);
    if (nd.has_ref) ok = ok && ((double)b != nd.ref);
    return ok;
}

static nodata_t make_nodata(const double *nodata_mon, const double *nodata_ref)
{
    nodata_t nd;
    nd.has_mon = nodata_mon != nullptr; nd.mon = nodata_mon ? *nodata_mon : 0.0;
    nd.has_ref = nodata_ref != nullptr; nd.ref = nodata_ref ? *nodata_ref : 0.0;
    return nd;
}
