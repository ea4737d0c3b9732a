// report_math.hpp: the arithmetic of the report's mean profiles (karios/report/commons.py:49-71) and the display range's pixel test
// (karios/report/overview_plot.py:134-194) as plain C++, shared by the kernels (k_report.hip), the host build of the launchers
// (k_report.hpp) and the CPU test (tests/test_report_host.py compiles this file with g++).
// tests/report_restatement.py is the definition; every function here is held to it bit for bit, which needs -ffp-contract=off and
// correctly rounded division / square root on every compiler that reads this text.
#pragma once
#include <math.h>
#include <stdint.h>

#include "accuracy_math.hpp"

// one rounding per operation: the device intrinsics, plain operators on the host.  The float64 square root is sqrt() on both sides (IEEE
// on the device as on the host; chips_math.hpp has the note on HIP's __fsqrt_rn, whose float64 kin this file avoids alike)
#if defined(__HIP_DEVICE_COMPILE__)
#define RP_FSUB(a, b) __fsub_rn((a), (b))
#define RP_FADD(a, b) __fadd_rn((a), (b))
#define RP_FMUL(a, b) __fmul_rn((a), (b))
#define RP_FDIV(a, b) __fdiv_rn((a), (b))
#define RP_DSUB(a, b) __dsub_rn((a), (b))
#define RP_DADD(a, b) __dadd_rn((a), (b))
#define RP_DMUL(a, b) __dmul_rn((a), (b))
#define RP_DDIV(a, b) __ddiv_rn((a), (b))
#else
#define RP_FSUB(a, b) ((a) - (b))
#define RP_FADD(a, b) ((a) + (b))
#define RP_FMUL(a, b) ((a) * (b))
#define RP_FDIV(a, b) ((a) / (b))
#define RP_DSUB(a, b) ((a) - (b))
#define RP_DADD(a, b) ((a) + (b))
#define RP_DMUL(a, b) ((a) * (b))
#define RP_DDIV(a, b) ((a) / (b))
#endif

namespace rp {

enum {
    MAX_NO_VALUES = 16,            // KM_DISPLAY_MAX_NO_VALUES
    MAX_TESTS = MAX_NO_VALUES + 1, // ... and the no-data value
    MAX_PROFILES = 8,              // KM_PROFILE_MAX
    MAX_ROWS = 1 << 20,
    MAX_BIN = 1 << 24,
};
constexpr uint32_t DROPPED = 0xFFFFFFFFu;   // order key of a row without a group (no finite key maps there)

// ---- display range: the values a pixel is compared with, in the pixel's own type (api_prep.hip fills it: a DN value the type cannot
// hold, or a NaN, matches no pixel and is left out)
struct tests {
    int n;
    union { int32_t i[MAX_TESTS]; float f[MAX_TESTS]; };
};
// (double)v as a pixel of the type, where one can equal it
AC_HD inline bool as_integer_pixel(double v, double lo, double hi, int32_t &out)
{
    if (!(v >= lo && v <= hi) || v != floor(v)) return false;
    out = (int32_t)v;
    return true;
}
AC_HD inline bool as_float_pixel(double v, float &out)
{
    if (v != v) return false;
    const float f = (float)v;
    if ((double)f != v) return false;
    out = f;
    return true;
}
template <typename T> AC_HD inline bool listed(T raw, const tests &t)
{
    bool hit = false;
    for (int k = 0; k < t.n; k++) hit = hit || (int32_t)raw == t.i[k];
    return hit;
}
template <> AC_HD inline bool listed<float>(float raw, const tests &t)
{
    bool hit = false;
    for (int k = 0; k < t.n; k++) hit = hit || raw == t.f[k];      // (0 in the list matches -0.0; a NaN pixel matches nothing)
    return hit;
}
// finite and not zero (-0.0 is a zero)
template <typename T> AC_HD inline bool countable(T raw) { return raw != (T)0; }
template <> AC_HD inline bool countable<float>(float raw) { return (ac::f32_bits(raw) & 0x7FFFFFFFu) < 0x7F800000u && raw != 0.0f; }
template <typename T> AC_HD inline bool is_nan(T) { return false; }
template <> AC_HD inline bool is_nan<float>(float raw) { return raw != raw; }

// float32 -> uint32 whose unsigned order is the numeric order (-0.0 directly below +0.0), and back
AC_HD inline uint32_t order_key(float f)
{
    const uint32_t u = ac::f32_bits(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
AC_HD inline float key_value(uint32_t k) { return ac::bits_f32((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// ---- mean profiles
// np.floor_divide(a, b) of float32 by float32, b >= 1: numpy's npy_divmodf
AC_HD inline float floor_divide(float a, float b)
{
    const float mod = fmodf(a, b);
    float div = RP_FDIV(RP_FSUB(a, mod), b);
    if (mod != 0.0f && (mod < 0.0f)) div = RP_FSUB(div, 1.0f);      // (b > 0: a remainder of the other sign lowers the quotient; NaN: neither)
    if (div != 0.0f) {
        float fl = floorf(div);
        if (RP_FSUB(div, fl) > 0.5f) fl = RP_FADD(fl, 1.0f);
        return fl;
    }
    return copysignf(0.0f, RP_FDIV(a, b));
}
// the order key of a row's group: -0.0 folded onto 0.0, DROPPED for a NaN key
AC_HD inline uint32_t group_key(float position, float bin)
{
    float k = floor_divide(position, bin);
    if (k != k) return DROPPED;
    if (k == 0.0f) k = 0.0f;
    return order_key(k);
}
// int32(float32(float32(key * bin) + float32(bin // 2))); false where numpy's cast is not defined
AC_HD inline bool group_position(float key, int bin, int32_t &out)
{
    const float p = RP_FADD(RP_FMUL(key, (float)bin), (float)(bin / 2));
    if (!(p >= -2147483648.0f && p < 2147483648.0f)) { out = 0; return false; }
    out = (int32_t)p;
    return true;
}
// pandas' group_mean (Kahan, float32) and group_var (Welford, float64) over the rows of one group, in row order
struct accum {
    float s, c;
    double m, m2;
    int32_t n;
};
AC_HD inline accum accum_zero() { accum a; a.s = 0.0f; a.c = 0.0f; a.m = 0.0; a.m2 = 0.0; a.n = 0; return a; }
AC_HD inline void accum_add(accum &a, float x)
{
    if (x != x) return;
    const float y = RP_FSUB(x, a.c);
    const float t = RP_FADD(a.s, y);
    a.c = RP_FSUB(RP_FSUB(t, a.s), y);
    if (a.c != a.c) a.c = 0.0f;
    a.s = t;
    a.n++;
    const double xd = (double)x, old = a.m;
    a.m = RP_DADD(old, RP_DDIV(RP_DSUB(xd, old), (double)a.n));
    a.m2 = RP_DADD(a.m2, RP_DMUL(RP_DSUB(xd, a.m), RP_DSUB(xd, old)));
}
AC_HD inline float accum_mean(const accum &a) { return a.n ? RP_FDIV(a.s, (float)a.n) : ac::bits_f32(0x7FC00000u); }
AC_HD inline float accum_std(const accum &a) { return a.n >= 2 ? (float)sqrt(RP_DDIV(a.m2, (double)(a.n - 1))) : ac::bits_f32(0x7FC00000u); }

}  // namespace rp
