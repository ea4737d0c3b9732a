// SIFT of the global align step, the part that is per candidate / per key point, and the scalars the dense part needs: the C++ form of
// tests/sift_restatement.py (the definition; its header lists what is OpenCV knowledge and what is a choice of this project).
// Compiled by hipcc for the kernels (k_sift.hip), for the library's host side (api_sift.hip), and by g++ alone under the sanitizers
// (tests/test_sift_host.py), which holds it to the restatement bit for bit.  Needs -ffp-contract=off: every product and sum rounds
// on its own.  No libm call reaches a value: exp, sin, cos and atan2 are written out; sqrt and division are correctly rounded.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SF_HD __host__ __device__ inline
#else
#define SF_HD inline
#endif

namespace sf {

enum { BORDER = 5, MAX_STEPS = 5, ORI_BINS = 36, D_WIDTH = 4, D_BINS = 8, D_LEN = 128, D_HIST = 6 * 6 * 10, MAX_OCTAVES = 16, MAX_RADIUS = 32 };

SF_HD float absf(float v) { return __builtin_fabsf(v); }
SF_HD int round_i(float v) { return (int)__builtin_rintf(v); }          // cvRound: to nearest, ties to even (exact, no rounding of its own)
SF_HD int floor_i(float v) { const int i = (int)v; return i - (v < (float)i); }

// ---- transcendentals
SF_HD double exp64(double x)
{
    if (x < -700.0) return 0.0;
    const double t = x * 0x1.71547652b82fep+0;
    const long long n = (long long)(t >= 0 ? t + 0.5 : t - 0.5);
    const double nf = (double)n;
    const double r = (x - nf * 0x1.62e42fee00000p-1) - nf * 0x1.a39ef35793c76p-33;
    const double C[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0,
                          1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
    double p = C[13];
    for (int k = 12; k >= 0; k--) p = p * r + C[k];
    const uint64_t bits = (uint64_t)(n + 1023) << 52;
    double scale;
    memcpy(&scale, &bits, sizeof scale);
    return p * scale;
}
SF_HD float exp32(float x) { return (float)exp64((double)x); }
#define SF_LN2 0x1.62e42fefa39efp-1

// (cos, sin) of a float32 angle in degrees, 0 <= a <= 360
SF_HD void sincos_deg(float af, float &cos_out, float &sin_out)
{
    const double a = (double)af;
    const long long q = (long long)(a / 90.0 + 0.5);
    const double x = (a - 90.0 * (double)q) * 0x1.1df46a2529d39p-6;
    const double x2 = x * x;
    const double S[8] = {1.0, -1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0, -1.0 / 1307674368000.0};
    const double Cc[9] = {1.0, -1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0, 1.0 / 479001600.0, -1.0 / 87178291200.0,
                          1.0 / 20922789888000.0};
    double s = S[7];
    for (int k = 6; k >= 0; k--) s = s * x2 + S[k];
    s = s * x;
    double c = Cc[8];
    for (int k = 7; k >= 0; k--) c = c * x2 + Cc[k];
    switch (q & 3) {
    case 0: cos_out = (float)c; sin_out = (float)s; break;
    case 1: cos_out = (float)-s; sin_out = (float)c; break;
    case 2: cos_out = (float)-c; sin_out = (float)-s; break;
    default: cos_out = (float)s; sin_out = (float)-c; break;
    }
}

// fastAtan2: degrees in [0, 360]
SF_HD float atan2_deg(float y, float x)
{
    const float r2d = 57.29577951308232f;
    const float p1 = 0.9997878412794807f * r2d, p3 = -0.3258083974640975f * r2d, p5 = 0.1555786518463281f * r2d, p7 = -0.04432655554792128f * r2d;
    const float eps = 2.220446049250313e-16f;
    const float ax = absf(x), ay = absf(y);
    float a;
    if (ax >= ay) {
        const float c = ay / (ax + eps), c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        const float c = ax / (ay + eps), c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// ---- scalars of the dense part (host)
// taps of the Gaussian kernel of `sigma` -> its size n (odd), or 0 when n exceeds max_taps; taps[n / 2] is the centre
SF_HD int gaussian_kernel(double sigma, float *taps, int max_taps)
{
    const int n = (int)__builtin_rint(sigma * 8 + 1) | 1;
    if (n > max_taps) return 0;
    const double scale2 = -0.5 / (sigma * sigma);
    double t[2 * MAX_RADIUS + 1];
    double s = 0.0;
    for (int i = 0; i < n; i++) {
        const double x = (double)i - (n - 1) * 0.5;
        t[i] = exp64(scale2 * (x * x));
        s += t[i];
    }
    const double inv = 1.0 / s;
    for (int i = 0; i < n; i++) taps[i] = (float)(t[i] * inv);
    return n;
}

SF_HD float base_sigma(double sigma)
{
    const float s = (float)sigma;
    const float d = s * s - 0.5f * 0.5f * 4.f;
    return __builtin_sqrtf(d > 0.01f ? d : 0.01f);
}

// sigma of the blur that takes level i - 1 to level i (i >= 1)
SF_HD double level_sigma(double sigma, int n_layers, int i)
{
    const double prev = exp64((double)(i - 1) * SF_LN2 / (double)n_layers) * sigma;
    const double total = exp64((double)i * SF_LN2 / (double)n_layers) * sigma;
    return __builtin_sqrt(total * total - prev * prev);
}

SF_HD int n_octaves(int h2, int w2)
{
    const long long m = h2 < w2 ? h2 : w2;
    if (m <= 0) return 0;
    int fl = 63 - __builtin_clzll((unsigned long long)(m * m));
    int n = ((fl - 3) >> 1) + 1;
    return n < 0 ? 0 : n > MAX_OCTAVES ? MAX_OCTAVES : n;
}

// ---- the refinement of one candidate
struct Refined {
    int layer, r, c, octave;
    float x, y, size, response;
};

struct Derivs { float dx, dy, ds, dxx, dyy, dss, dxy, dxs, dys; };

// dog: the octave's DoG planes, `plane` floats apart, rows `stride` floats apart
SF_HD Derivs derivs(const float *dog, size_t plane, ptrdiff_t stride, int layer, int r, int c)
{
    const float img_scale = 1.f / 255.f;
    const float deriv_scale = img_scale * 0.5f, second_scale = img_scale, cross_scale = img_scale * 0.25f;
    const float *img = dog + (size_t)layer * plane + (ptrdiff_t)r * stride + c, *prev = img - plane, *next = img + plane;
    Derivs d;
    d.dx = (img[1] - img[-1]) * deriv_scale;
    d.dy = (img[stride] - img[-stride]) * deriv_scale;
    d.ds = (next[0] - prev[0]) * deriv_scale;
    const float v2 = img[0] * 2.f;
    d.dxx = (img[1] + img[-1] - v2) * second_scale;
    d.dyy = (img[stride] + img[-stride] - v2) * second_scale;
    d.dss = (next[0] + prev[0] - v2) * second_scale;
    d.dxy = (img[stride + 1] - img[stride - 1] - img[-stride + 1] + img[-stride - 1]) * cross_scale;
    d.dxs = (next[1] - next[-1] - prev[1] + prev[-1]) * cross_scale;
    d.dys = (next[stride] - next[-stride] - prev[stride] + prev[-stride]) * cross_scale;
    return d;
}

// Cramer's rule of the symmetric 3 x 3 system; a zero determinant gives the zero vector
SF_HD void solve3(const Derivs &d, float X[3])
{
    const float a00 = d.dxx, a01 = d.dxy, a02 = d.dxs, a10 = d.dxy, a11 = d.dyy, a12 = d.dys, a20 = d.dxs, a21 = d.dys, a22 = d.dss;
    const float b0 = d.dx, b1 = d.dy, b2 = d.ds;
    const float det = a00 * (a11 * a22 - a21 * a12) - a01 * (a10 * a22 - a20 * a12) + a02 * (a10 * a21 - a20 * a11);
    if (det == 0) { X[0] = X[1] = X[2] = 0.f; return; }
    const float inv = 1.f / det;
    X[0] = inv * (b0 * (a11 * a22 - a12 * a21) - a01 * (b1 * a22 - a12 * b2) + a02 * (b1 * a21 - a11 * b2));
    X[1] = inv * (a00 * (b1 * a22 - a12 * b2) - b0 * (a10 * a22 - a12 * a20) + a02 * (a10 * b2 - b1 * a20));
    X[2] = inv * (a00 * (a11 * b2 - b1 * a21) - a01 * (a10 * b2 - b1 * a20) + b0 * (a10 * a21 - a11 * a20));
}

SF_HD bool refine(const float *dog, size_t plane, ptrdiff_t stride, int rows, int cols, int octv, int layer, int r, int c, int n_layers,
                  double contrast_threshold, double edge_threshold, double sigma, Refined &out)
{
    float xc = 0, xr = 0, xi = 0;
    int step = 0;
    for (; step < MAX_STEPS; step++) {
        const Derivs d = derivs(dog, plane, stride, layer, r, c);
        float X[3];
        solve3(d, X);
        xc = -X[0]; xr = -X[1]; xi = -X[2];
        if (absf(xi) < 0.5f && absf(xr) < 0.5f && absf(xc) < 0.5f) break;
        const float big = (float)(2147483647 / 3);
        if (!(absf(xi) <= big && absf(xr) <= big && absf(xc) <= big)) return false;   // a NaN offset counts as huge
        c += round_i(xc); r += round_i(xr); layer += round_i(xi);
        if (layer < 1 || layer > n_layers || c < BORDER || c >= cols - BORDER || r < BORDER || r >= rows - BORDER) return false;
    }
    if (step >= MAX_STEPS) return false;
    const Derivs d = derivs(dog, plane, stride, layer, r, c);
    const float t = d.dx * xc + d.dy * xr + d.ds * xi;
    const float contr = dog[(size_t)layer * plane + (ptrdiff_t)r * stride + c] * (1.f / 255.f) + t * 0.5f;
    if ((double)(absf(contr) * (float)n_layers) < contrast_threshold) return false;
    const float tr = d.dxx + d.dyy, det = d.dxx * d.dyy - d.dxy * d.dxy;
    if (det <= 0 || (double)(tr * tr) * edge_threshold >= (edge_threshold + 1.0) * (edge_threshold + 1.0) * (double)det) return false;
    const float sc = (float)(1 << octv);
    out.layer = layer; out.r = r; out.c = c;
    out.x = ((float)c + xc) * sc;
    out.y = ((float)r + xr) * sc;
    out.octave = octv + (layer << 8) + (int)((unsigned)round_i((xi + 0.5f) * 255.f) << 16);
    const float p = (float)exp64((double)(((float)layer + xi) / (float)n_layers) * SF_LN2);
    out.size = (float)(sigma * (double)p * (double)(1 << octv) * 2.0);
    out.response = absf(contr);
    return true;
}

// ---- orientations of one refined key point on its Gaussian level -> number of angles (at most ORI_BINS / 2), in bin order
SF_HD int orientations(const float *img, ptrdiff_t stride, int rows, int cols, int r0, int c0, float size, int octv, float *angles)
{
    const int n = ORI_BINS;
    const float scl_octv = size * 0.5f / (float)(1 << octv);
    const int radius = round_i(4.5f * scl_octv);
    const float sigma = 1.5f * scl_octv;
    const float expf_scale = -1.f / (2.f * sigma * sigma);
    const float bins_per_deg = (float)n / 360.f;
    float tmp[ORI_BINS + 4];
    for (int k = 0; k < n + 4; k++) tmp[k] = 0.f;
    for (int i = -radius; i <= radius; i++) {
        const int y = r0 + i;
        if (y <= 0 || y >= rows - 1) continue;
        for (int j = -radius; j <= radius; j++) {
            const int x = c0 + j;
            if (x <= 0 || x >= cols - 1) continue;
            const float *p = img + (ptrdiff_t)y * stride + x;
            const float dx = p[1] - p[-1], dy = p[-stride] - p[stride];
            const float w = exp32((float)(i * i + j * j) * expf_scale);
            const float ori = atan2_deg(dy, dx);
            const float mag = __builtin_sqrtf(dx * dx + dy * dy);
            int bin = round_i(bins_per_deg * ori);
            if (bin >= n) bin -= n;
            if (bin < 0) bin += n;
            tmp[bin + 2] += w * mag;
        }
    }
    tmp[0] = tmp[n]; tmp[1] = tmp[n + 1]; tmp[n + 2] = tmp[2]; tmp[n + 3] = tmp[3];
    float hist[ORI_BINS];
    float omax = 0.f;
    for (int k = 0; k < n; k++) {
        hist[k] = (tmp[k] + tmp[k + 4]) * (1.f / 16.f) + (tmp[k + 1] + tmp[k + 3]) * (4.f / 16.f) + tmp[k + 2] * (6.f / 16.f);
        if (k == 0 || hist[k] > omax) omax = hist[k];
    }
    const float thr = omax * 0.8f;
    int count = 0;
    for (int j = 0; j < n; j++) {
        const int l = j > 0 ? j - 1 : n - 1, r2 = j < n - 1 ? j + 1 : 0;
        if (hist[j] > hist[l] && hist[j] > hist[r2] && hist[j] >= thr) {
            float b = (float)j + 0.5f * (hist[l] - hist[r2]) / (hist[l] - 2.f * hist[j] + hist[r2]);
            b = b < 0 ? (float)n + b : b >= (float)n ? b - (float)n : b;
            float a = 360.f - 360.f / (float)n * b;
            if (absf(a - 360.f) < 1.1920929e-07f) a = 0.f;
            angles[count++] = a;
        }
    }
    return count;
}

// ---- descriptor of one key point on its Gaussian level.  px, py: the point on this level; scl: size / 2 on this level.
// hist: D_HIST floats of working room, HS floats apart (a lane's column of an LDS array on the device).
template <int HS>
SF_HD void descriptor(const float *img, ptrdiff_t stride, int rows, int cols, float px, float py, float angle, float scl, float *hist, uint8_t *out)
{
    const int d = D_WIDTH, n = D_BINS;
    float ori = 360.f - angle;
    if (absf(ori - 360.f) < 1.1920929e-07f) ori = 0.f;
    const int ptx = round_i(px), pty = round_i(py);
    float cos_t, sin_t;
    sincos_deg(ori, cos_t, sin_t);
    const float bins_per_deg = (float)n / 360.f;
    const float exp_scale = -1.f / ((float)(d * d) * 0.5f);
    const float hist_width = 3.f * scl;
    int radius = round_i(hist_width * 1.4142135623730951f * (float)(d + 1) * 0.5f);
    const int diag = (int)__builtin_sqrt((double)cols * cols + (double)rows * rows);
    if (radius > diag) radius = diag;
    cos_t = cos_t / hist_width;
    sin_t = sin_t / hist_width;
    for (int k = 0; k < D_HIST; k++) hist[k * HS] = 0.f;
    const int s_c = n + 2, s_r = (d + 2) * (n + 2);
    for (int i = -radius; i <= radius; i++)
        for (int j = -radius; j <= radius; j++) {
            const float c_rot = (float)j * cos_t - (float)i * sin_t;
            const float r_rot = (float)j * sin_t + (float)i * cos_t;
            float rbin = r_rot + (float)(d / 2) - 0.5f;
            float cbin = c_rot + (float)(d / 2) - 0.5f;
            const int r = pty + i, c = ptx + j;
            if (!(rbin > -1 && rbin < d && cbin > -1 && cbin < d && r > 0 && r < rows - 1 && c > 0 && c < cols - 1)) continue;
            const float *p = img + (ptrdiff_t)r * stride + c;
            const float dx = p[1] - p[-1], dy = p[-stride] - p[stride];
            const float w = exp32((c_rot * c_rot + r_rot * r_rot) * exp_scale);
            const float o = atan2_deg(dy, dx);
            const float mag = __builtin_sqrtf(dx * dx + dy * dy) * w;
            float obin = (o - ori) * bins_per_deg;
            const int r0 = floor_i(rbin), c0 = floor_i(cbin);
            int o0 = floor_i(obin);
            rbin -= (float)r0; cbin -= (float)c0; obin -= (float)o0;
            if (o0 < 0) o0 += n;
            if (o0 >= n) o0 -= n;
            const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
            const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11;
            const float v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
            const float v111 = v_rc11 * obin, v110 = v_rc11 - v111;
            const float v101 = v_rc10 * obin, v100 = v_rc10 - v101;
            const float v011 = v_rc01 * obin, v010 = v_rc01 - v011;
            const float v001 = v_rc00 * obin, v000 = v_rc00 - v001;
            const int idx = ((r0 + 1) * (d + 2) + c0 + 1) * (n + 2) + o0;
            hist[idx * HS] += v000;
            hist[(idx + 1) * HS] += v001;
            hist[(idx + s_c) * HS] += v010;
            hist[(idx + s_c + 1) * HS] += v011;
            hist[(idx + s_r) * HS] += v100;
            hist[(idx + s_r + 1) * HS] += v101;
            hist[(idx + s_r + s_c) * HS] += v110;
            hist[(idx + s_r + s_c + 1) * HS] += v111;
        }
    // fold the circular orientation bins of every cell (all 36 cells, as the restatement does; only the inner 16 are read)
    for (int cell = 0; cell < (d + 2) * (d + 2); cell++) {
        hist[(cell * (n + 2)) * HS] += hist[(cell * (n + 2) + n) * HS];
        hist[(cell * (n + 2) + 1) * HS] += hist[(cell * (n + 2) + n + 1) * HS];
    }
    float nrm2 = 0.f;
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++)
            for (int k = 0; k < n; k++) {
                const float v = hist[(((i + 1) * (d + 2) + (j + 1)) * (n + 2) + k) * HS];
                nrm2 += v * v;
            }
    const float thr = __builtin_sqrtf(nrm2) * 0.2f;
    nrm2 = 0.f;
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++)
            for (int k = 0; k < n; k++) {
                float &v = hist[(((i + 1) * (d + 2) + (j + 1)) * (n + 2) + k) * HS];
                v = v < thr ? v : thr;
                nrm2 += v * v;
            }
    const float root = __builtin_sqrtf(nrm2);
    const float scale = 512.f / (root > 1.1920929e-07f ? root : 1.1920929e-07f);
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++)
            for (int k = 0; k < n; k++) {
                const int v = round_i(hist[(((i + 1) * (d + 2) + (j + 1)) * (n + 2) + k) * HS] * scale);
                out[(i * d + j) * n + k] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
            }
}

// ---- the final order: x, y ascending; size descending; angle ascending; response, octave descending
struct Key {
    float x, y, size, angle, response;
    int octave;
};
SF_HD bool key_less(const Key &a, const Key &b)
{
    if (a.x != b.x) return a.x < b.x;
    if (a.y != b.y) return a.y < b.y;
    if (a.size != b.size) return a.size > b.size;
    if (a.angle != b.angle) return a.angle < b.angle;
    if (a.response != b.response) return a.response > b.response;
    return a.octave > b.octave;
}
SF_HD bool key_duplicate(const Key &a, const Key &b) { return a.x == b.x && a.y == b.y && a.size == b.size && a.angle == b.angle; }

}  // namespace sf
