// Global align step (karios/matcher/global_align.py): cv2.warpPerspective, the Sobel gradient magnitude (_sobel_magnitude) and
// cv2.findTransformECC(MOTION_HOMOGRAPHY).  The arithmetic is restated in numpy in tests/align_restatement.py, which is the
// definition these kernels are held to bit for bit (warps, Sobel) or to fp64 summation order
// (the 66 sums of an ECC iteration; every per-pixel product is exact in fp64, only the order of the additions differs).  The
// Gaussian, gradient and pre-mask kernels follow the restatement's operation order too and are held to it bit for bit through
// km_ecc_stages (tests/test_gpu_align_stages.py).
#include "k_align.hpp"

#include <math.h>

namespace {

constexpr int kWarpBX = 64, kWarpBY = 4;
constexpr int kEccThreads = 256;

// std::max(INT_MIN, std::min(INT_MAX, v)) with std::min(a, b) = b < a ? b : a: NaN -> INT_MAX (imgwarp.cpp)
__device__ __forceinline__ double clamp_int(double v)
{
    v = v < 2147483647.0 ? v : 2147483647.0;
    return -2147483648.0 < v ? v : -2147483648.0;
}
__device__ __forceinline__ int sat_short(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

// WarpPerspectiveInvoker: X0 / Y0 / W0 in fp64 at the first column of the bw0-wide block, then + M * x1 inside the block.
// num = 32 (linear: positions on the 1/32 grid) or 1 (nearest).  Returns the rounded fixed-point positions.
__device__ __forceinline__ void warp_pos(const ka_m9 &M, int x, int y, int bw0, double num, int &X, int &Y)
{
    const int x1i = x % bw0;
    const double xb = (double)(x - x1i), x1 = (double)x1i, yd = (double)y;
    const double X0 = M.m[0] * xb + M.m[1] * yd + M.m[2];
    const double Y0 = M.m[3] * xb + M.m[4] * yd + M.m[5];
    const double W0 = M.m[6] * xb + M.m[7] * yd + M.m[8];
    double W = W0 + M.m[6] * x1;
    W = W != 0.0 ? num / W : 0.0;
    X = (int)rint(clamp_int((X0 + M.m[0] * x1) * W));
    Y = (int)rint(clamp_int((Y0 + M.m[3] * x1) * W));
}

template <typename T>
__device__ __forceinline__ T tap(const T *__restrict__ s, ptrdiff_t ss, int sH, int sW, int x, int y, T cval)
{
    return ((unsigned)x < (unsigned)sW && (unsigned)y < (unsigned)sH) ? s[(ptrdiff_t)y * ss + x] : cval;
}

template <typename T, bool LINEAR>
__global__ __launch_bounds__(kWarpBX *kWarpBY) void warp_kernel(const T *__restrict__ src, ptrdiff_t ss, int sH, int sW, T *__restrict__ dst,
                                                                 ptrdiff_t ds, int dH, int dW, ka_m9 M, int bw0, T cval)
{
    const int x = blockIdx.x * kWarpBX + threadIdx.x, y = blockIdx.y * kWarpBY + threadIdx.y;
    if (x >= dW || y >= dH) return;
    int X, Y;
    T out;
    if (!LINEAR) {
        warp_pos(M, x, y, bw0, 1.0, X, Y);
        out = tap(src, ss, sH, sW, sat_short(X), sat_short(Y), cval);
    } else {
        warp_pos(M, x, y, bw0, 32.0, X, Y);
        const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5), fx = X & 31, fy = Y & 31;
        if (sx >= sW || sx + 1 < 0 || sy >= sH || sy + 1 < 0) {
            out = cval;
        } else {
            const T v0 = tap(src, ss, sH, sW, sx, sy, cval), v1 = tap(src, ss, sH, sW, sx + 1, sy, cval);
            const T v2 = tap(src, ss, sH, sW, sx, sy + 1, cval), v3 = tap(src, ss, sH, sW, sx + 1, sy + 1, cval);
            if constexpr (sizeof(T) == 1) {
                // BilinearTab_i (the saturated (0, 0) entry of OpenCV's table gives the same 8-bit result: align_restatement.py)
                const int wx0 = 32 - fx, wy0 = 32 - fy;
                const int s = (int)v0 * (wy0 * wx0 * 32) + (int)v1 * (wy0 * fx * 32) + (int)v2 * (fy * wx0 * 32) + (int)v3 * (fy * fx * 32);
                const int r = (s + (1 << 14)) >> 15;
                out = (T)(r < 0 ? 0 : r > 255 ? 255 : r);
            } else {
                const float tx = (float)fx * (1.0f / 32), ty = (float)fy * (1.0f / 32), ax = 1.0f - tx, ay = 1.0f - ty;
                float s = v0 * (ay * ax);
                s = s + v1 * (ay * tx);
                s = s + v2 * (ty * ax);
                s = s + v3 * (ty * tx);
                out = s;
            }
        }
    }
    dst[(ptrdiff_t)y * ds + x] = out;
}

// cv2.Sobel(u8, CV_32F, 1, 0 / 0, 1, ksize=3) (REFLECT_101, exact integers) + cv2.magnitude; the maximum through an unsigned atomic max
// on the bit pattern (non-negative floats order like their bits: the result does not depend on the order)
__global__ __launch_bounds__(256) void sobel_mag_kernel(const uint8_t *__restrict__ src, ptrdiff_t ss, int H, int W, float *__restrict__ out,
                                                        unsigned *__restrict__ d_max)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    float mag = 0.0f;
    if (x < W && y < H) {
        const int xm = km_reflect101(x - 1, W), xp = km_reflect101(x + 1, W);
        const uint8_t *r0 = src + (ptrdiff_t)km_reflect101(y - 1, H) * ss, *r1 = src + (ptrdiff_t)y * ss, *r2 = src + (ptrdiff_t)km_reflect101(y + 1, H) * ss;
        const int gx = ((int)r0[xp] - r0[xm]) + 2 * ((int)r1[xp] - r1[xm]) + ((int)r2[xp] - r2[xm]);
        const int gy = ((int)r2[xm] - r0[xm]) + 2 * ((int)r2[x] - r0[x]) + ((int)r2[xp] - r0[xp]);
        mag = sqrtf((float)(gx * gx + gy * gy));
        out[(size_t)y * W + x] = mag;
    }
    float m = mag;
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __shared__ float wmax[4];
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        // one address takes only ~90 atomics / us: a workgroup only raises the maximum when it can (the value only grows)
        if (m > 0.0f && __float_as_uint(m) > __hip_atomic_load(d_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(d_max, __float_as_uint(m));
    }
}

__global__ __launch_bounds__(256) void div_max_kernel(float *__restrict__ a, size_t n, const unsigned *__restrict__ d_max)
{
    const float m = __uint_as_float(*d_max);
    if (!(m > 0.0f)) return;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) a[i] = a[i] / m;
}

// GaussianBlur 5 x 5 on float32, row pass: k0 c + k1 (l1 + r1) + k2 (l2 + r2).  MODE 0: float input, 1: uint8 input, 2: uint8 mask
// thresholded at > 0 (the pre-mask)
template <typename T, int MODE>
__global__ __launch_bounds__(256) void gauss_row_kernel(const T *__restrict__ src, ptrdiff_t ss, int H, int W, float *__restrict__ dst)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const T *r = src + (ptrdiff_t)y * ss;
    auto ld = [&](int xx) -> float {
        const T v = r[km_reflect101(xx, W)];
        return MODE == 2 ? (v > 0 ? 1.0f : 0.0f) : (float)v;
    };
    float s = 0.375f * ld(x);
    s = s + 0.25f * (ld(x - 1) + ld(x + 1));
    s = s + 0.0625f * (ld(x - 2) + ld(x + 2));
    dst[(size_t)y * W + x] = s;
}

__global__ __launch_bounds__(256) void gauss_col_kernel(const float *__restrict__ src, int H, int W, float *__restrict__ dst)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    auto ld = [&](int yy) { return src[(size_t)km_reflect101(yy, H) * W + x]; };
    float s = 0.375f * ld(y);
    s = s + 0.25f * (ld(y - 1) + ld(y + 1));
    s = s + 0.0625f * (ld(y - 2) + ld(y + 2));
    dst[(size_t)y * W + x] = s;
}

// pre-mask (blurred 0 / 1 mask * (float)(0.5 / 0.95), rounded half to even) and the central-difference gradients of the blurred
// image times it: plane = {image, gx, gy, pre-mask}, one 16-byte load per bilinear tap of the iteration
__global__ __launch_bounds__(256) void ecc_plane_kernel(const float *__restrict__ img, const float *__restrict__ pm_blur, int H, int W,
                                                        float4 *__restrict__ plane)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float pm = pm_blur ? rintf(pm_blur[p] * (float)(0.5 / 0.95)) : 1.0f;
    const float *r = img + (size_t)y * W;
    float gx = 0.0f;
    gx = gx + -0.5f * r[km_reflect101(x - 1, W)];
    gx = gx + 0.5f * r[km_reflect101(x + 1, W)];
    float gy = 0.0f;
    gy = gy + -0.5f * img[(size_t)km_reflect101(y - 1, H) * W + x];
    gy = gy + 0.5f * img[(size_t)km_reflect101(y + 1, H) * W + x];
    plane[p] = make_float4(r[x], gx * pm, gy * pm, pm);
}

__device__ __forceinline__ float4 tap4(const float4 *__restrict__ pl, int H, int W, int x, int y)
{
    return ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) ? pl[(size_t)y * W + x] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// One ECC iteration: every template pixel warps image / gx / gy (linear, WARP_INVERSE_MAP, border 0) and the pre-mask (nearest),
// builds the 8 Jacobian terms (image_jacobian_homo_ECC, float32) and adds its share of the KA_NSUM fp64 sums.  Per-workgroup
// partials, reduced in a fixed order by ecc_reduce_kernel: bitwise identical run to run.
__global__ __launch_bounds__(kEccThreads) void ecc_iter_kernel(const float *__restrict__ tmpl, int hs, int ws, const float4 *__restrict__ plane,
                                                               int hd, int wd, ka_m9 M, ka_h8 h, int bw0, double *__restrict__ partials)
{
    double acc[KA_NSUM];
#pragma unroll
    for (int k = 0; k < KA_NSUM; k++) acc[k] = 0.0;
    const size_t n = (size_t)hs * ws;
    for (size_t p = (size_t)blockIdx.x * kEccThreads + threadIdx.x; p < n; p += (size_t)gridDim.x * kEccThreads) {
        const int y = (int)(p / ws), x = (int)(p - (size_t)y * ws);
        int X, Y;
        warp_pos(M, x, y, bw0, 32.0, X, Y);
        const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5), fx = X & 31, fy = Y & 31;
        float I = 0.0f, gxw = 0.0f, gyw = 0.0f;
        if (!(sx >= wd || sx + 1 < 0 || sy >= hd || sy + 1 < 0)) {
            const float4 v0 = tap4(plane, hd, wd, sx, sy), v1 = tap4(plane, hd, wd, sx + 1, sy);
            const float4 v2 = tap4(plane, hd, wd, sx, sy + 1), v3 = tap4(plane, hd, wd, sx + 1, sy + 1);
            const float tx = (float)fx * (1.0f / 32), ty = (float)fy * (1.0f / 32), ax = 1.0f - tx, ay = 1.0f - ty;
            const float w0 = ay * ax, w1 = ay * tx, w2 = ty * ax, w3 = ty * tx;
            I = v0.x * w0; I = I + v1.x * w1; I = I + v2.x * w2; I = I + v3.x * w3;
            gxw = v0.y * w0; gxw = gxw + v1.y * w1; gxw = gxw + v2.y * w2; gxw = gxw + v3.y * w3;
            gyw = v0.z * w0; gyw = gyw + v1.z * w1; gyw = gyw + v2.z * w2; gyw = gyw + v3.z * w3;
        }
        warp_pos(M, x, y, bw0, 1.0, X, Y);
        const float mf = tap4(plane, hd, wd, sat_short(X), sat_short(Y)).w;
        const float T = tmpl[p];
        const float xf = (float)x, yf = (float)y;
        const float den = (xf * h.h[2] + yf * h.h[5]) + 1.0f;
        const float hatX = ((-(xf * h.h[0])) - yf * h.h[3] - h.h[6]) / den;
        const float hatY = ((-(xf * h.h[1])) - yf * h.h[4] - h.h[7]) / den;
        const float g1 = gxw / den, g2 = gyw / den;
        const float temp = hatX * g1 + hatY * g2;
        const float J[8] = {g1 * xf, g2 * xf, temp * xf, g1 * yf, g2 * yf, temp * yf, g1, g2};
        const double m = (double)mf, Id = (double)I, Td = (double)T;
        acc[0] += m;
        acc[1] += m * Id;
        acc[2] += m * Id * Id;
        acc[3] += m * Td;
        acc[4] += m * Td * Td;
        acc[5] += m * Td * Id;
        int q = 6;
#pragma unroll
        for (int k = 0; k < 8; k++)
#pragma unroll
            for (int l = k; l < 8; l++) acc[q++] += (double)J[k] * (double)J[l];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double j = (double)J[k];
            acc[42 + k] += j * Id;
            acc[50 + k] += j * m;
            acc[58 + k] += j * m * Td;
        }
    }
    __shared__ double red[kEccThreads / 64][KA_NSUM];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KA_NSUM; k++) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < KA_NSUM) {
        double s = red[0][threadIdx.x];
        for (int w = 1; w < kEccThreads / 64; w++) s += red[w][threadIdx.x];
        partials[(size_t)blockIdx.x * KA_NSUM + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(128) void ecc_reduce_kernel(const double *__restrict__ partials, int nblk, double *__restrict__ out)
{
    const int t = threadIdx.x;
    if (t >= KA_NSUM) return;
    double s = 0.0;
    for (int b = 0; b < nblk; b++) s += partials[(size_t)b * KA_NSUM + t];
    out[t] = s;
}

__global__ __launch_bounds__(256) void count_nonzero_kernel(const uint8_t *__restrict__ a, size_t n, unsigned long long *__restrict__ out)
{
    unsigned c = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) c += a[i] != 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

inline dim3 grid64x4(int H, int W) { return dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)); }

}  // namespace

int ka_warp_block_width(int dH, int dW)
{
    const int bh0 = dH < 16 ? dH : 16;
    const int bw0 = 1024 / bh0;
    return bw0 < dW ? bw0 : dW;
}

int ka_warp(km_ctx *c, const void *d_src, int dtype, int sH, int sW, ptrdiff_t ss, void *d_dst, int dH, int dW, ptrdiff_t ds, int linear,
            const double Minv[9], double border)
{
    ka_m9 M;
    for (int i = 0; i < 9; i++) M.m[i] = Minv[i];
    const int bw0 = ka_warp_block_width(dH, dW);
    const dim3 grid((unsigned)((dW + kWarpBX - 1) / kWarpBX), (unsigned)((dH + kWarpBY - 1) / kWarpBY)), block(kWarpBX, kWarpBY);
    if (dtype == KM_U8) {
        // saturate_cast<uchar>(double): round half to even, saturate, NaN -> 0
        const double r = border != border ? 0.0 : rint(border);
        const uint8_t cv = (uint8_t)(r < 0.0 ? 0.0 : r > 255.0 ? 255.0 : r);
        const uint8_t *s = (const uint8_t *)d_src;
        uint8_t *d = (uint8_t *)d_dst;
        if (linear) warp_kernel<uint8_t, true><<<grid, block, 0, c->stream>>>(s, ss, sH, sW, d, ds, dH, dW, M, bw0, cv);
        else warp_kernel<uint8_t, false><<<grid, block, 0, c->stream>>>(s, ss, sH, sW, d, ds, dH, dW, M, bw0, cv);
    } else if (dtype == KM_F32) {
        const float *s = (const float *)d_src;
        float *d = (float *)d_dst;
        if (linear) warp_kernel<float, true><<<grid, block, 0, c->stream>>>(s, ss, sH, sW, d, ds, dH, dW, M, bw0, (float)border);
        else warp_kernel<float, false><<<grid, block, 0, c->stream>>>(s, ss, sH, sW, d, ds, dH, dW, M, bw0, (float)border);
    } else {
        return km_fail(c, KM_E_UNSUPPORTED, "warp_perspective: dtype %d (uint8 and float32 only)", dtype);
    }
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ka_sobel_magnitude(km_ctx *c, const uint8_t *d_src, int H, int W, ptrdiff_t ss, float *d_out, unsigned *d_max)
{
    KM_HIP(c, hipMemsetAsync(d_max, 0, sizeof(unsigned), c->stream));
    sobel_mag_kernel<<<grid64x4(H, W), 256, 0, c->stream>>>(d_src, ss, H, W, d_out, d_max);
    KM_LAUNCH_CHECK(c);
    const size_t n = (size_t)H * W;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    div_max_kernel<<<blocks, 256, 0, c->stream>>>(d_out, n, d_max);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ka_gauss5(km_ctx *c, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, float *d_tmp, float *d_out)
{
    const dim3 g = grid64x4(H, W);
    if (dtype == KM_F32) gauss_row_kernel<float, 0><<<g, 256, 0, c->stream>>>((const float *)d_src, ss, H, W, d_tmp);
    else if (dtype == KM_U8) gauss_row_kernel<uint8_t, 1><<<g, 256, 0, c->stream>>>((const uint8_t *)d_src, ss, H, W, d_tmp);
    else if (dtype == KA_MASK) gauss_row_kernel<uint8_t, 2><<<g, 256, 0, c->stream>>>((const uint8_t *)d_src, ss, H, W, d_tmp);
    else return km_fail(c, KM_E_UNSUPPORTED, "find_transform_ecc: dtype %d (uint8 and float32 only)", dtype);
    KM_LAUNCH_CHECK(c);
    gauss_col_kernel<<<g, 256, 0, c->stream>>>(d_tmp, H, W, d_out);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ka_ecc_plane(km_ctx *c, const float *d_blur, const float *d_pm_blur, int H, int W, float4 *d_plane)
{
    ecc_plane_kernel<<<grid64x4(H, W), 256, 0, c->stream>>>(d_blur, d_pm_blur, H, W, d_plane);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ka_ecc_blocks(int hs, int ws)
{
    const size_t n = (size_t)hs * ws, b = (n + kEccThreads - 1) / kEccThreads;
    return (int)(b < KA_ECC_MAX_BLOCKS ? b : KA_ECC_MAX_BLOCKS);
}

int ka_ecc_sums(km_ctx *c, const float *d_tmpl, int hs, int ws, const float4 *d_plane, int hd, int wd, const float map[9], double *d_partials,
                double *d_sums)
{
    ka_m9 M;
    for (int i = 0; i < 9; i++) M.m[i] = (double)map[i];
    // image_jacobian_homo_ECC's h0_ .. h7_ = map[0], map[3], map[6], map[1], map[4], map[7], map[2], map[5]
    ka_h8 h;
    const int order[8] = {0, 3, 6, 1, 4, 7, 2, 5};
    for (int i = 0; i < 8; i++) h.h[i] = map[order[i]];
    const int nb = ka_ecc_blocks(hs, ws);
    ecc_iter_kernel<<<nb, kEccThreads, 0, c->stream>>>(d_tmpl, hs, ws, d_plane, hd, wd, M, h, ka_warp_block_width(hs, ws), d_partials);
    KM_LAUNCH_CHECK(c);
    ecc_reduce_kernel<<<1, 128, 0, c->stream>>>(d_partials, nb, d_sums);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ka_count_nonzero(km_ctx *c, const uint8_t *d_a, size_t n, unsigned long long *d_out)
{
    KM_HIP(c, hipMemsetAsync(d_out, 0, sizeof(unsigned long long), c->stream));
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
    count_nonzero_kernel<<<blocks, 256, 0, c->stream>>>(d_a, n, d_out);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
