// Kernels of SIFT detectAndCompute (k_sift.hpp).  The dense stages (base, blur + DoG, decimation, extrema scan) are one lane per
// sample and bound by memory; the sparse stages (refinement, orientation, descriptor) are one lane per candidate / key point and
// run sift_math.hpp as it stands, so their sums are the restatement's by construction.
#include "k_sift.hpp"

namespace {

// BORDER_REFLECT_101, reflected until the index lands inside (a kernel may be wider than a small octave)
__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// the doubled image: dst(2i) = src(i), dst(2i + 1) = (src(i) + src(i + 1)) / 2 with the last sample replicated, rows the same way
__global__ __launch_bounds__(256) void base_kernel(const uint8_t *__restrict__ img, int H, int W, ptrdiff_t stride, float *__restrict__ out)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= 2 * W) return;
    const int x0 = x >> 1, x1 = (x & 1) ? (x0 + 1 < W ? x0 + 1 : W - 1) : x0;
    const int y0 = y >> 1, y1 = (y & 1) ? (y0 + 1 < H ? y0 + 1 : H - 1) : y0;
    const uint8_t *r0 = img + (ptrdiff_t)y0 * stride, *r1 = img + (ptrdiff_t)y1 * stride;
    const float a = ((float)r0[x0] + (float)r0[x1]) * 0.5f, b = ((float)r1[x0] + (float)r1[x1]) * 0.5f;
    out[(size_t)y * (2 * W) + x] = (a + b) * 0.5f;
}

// row pass: s = k0 x0; s += kj (x[-j] + x[+j]), j = 1 .. radius.  Only the workgroups at the two ends of a row reflect.
__global__ __launch_bounds__(256) void blur_rows_kernel(const float *__restrict__ src, int h, int w, ksf_taps taps, float *__restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int R = taps.radius;
    const bool interior = (int)(blockIdx.x * 256) - R >= 0 && (int)(blockIdx.x * 256) + 255 + R < w;
    if (x >= w) return;
    const float *row = src + (size_t)y * w;
    float s = taps.k[0] * row[x];
    if (interior) {
        for (int j = 1; j <= R; j++) s += taps.k[j] * (row[x - j] + row[x + j]);
    } else {
        for (int j = 1; j <= R; j++) s += taps.k[j] * (row[reflect101(x - j, w)] + row[reflect101(x + j, w)]);
    }
    dst[(size_t)y * w + x] = s;
}

// column pass of the same sum; stores the level and, fused, the DoG level against the level it was blurred from
__global__ __launch_bounds__(256) void blur_cols_kernel(const float *__restrict__ tmp, const float *__restrict__ prev, int h, int w, ksf_taps taps,
                                                        float *__restrict__ dst, float *__restrict__ dog)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int R = taps.radius;
    if (x >= w) return;
    float s = taps.k[0] * tmp[(size_t)y * w + x];
    if (y - R >= 0 && y + R < h) {
        for (int j = 1; j <= R; j++) s += taps.k[j] * (tmp[(size_t)(y - j) * w + x] + tmp[(size_t)(y + j) * w + x]);
    } else {
        for (int j = 1; j <= R; j++) s += taps.k[j] * (tmp[(size_t)reflect101(y - j, h) * w + x] + tmp[(size_t)reflect101(y + j, h) * w + x]);
    }
    dst[(size_t)y * w + x] = s;
    if (dog) dog[(size_t)y * w + x] = s - prev[(size_t)y * w + x];
}

__global__ __launch_bounds__(256) void decimate_kernel(const float *__restrict__ src, int w, int h2, int w2, float *__restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w2 || y >= h2) return;
    dst[(size_t)y * w2 + x] = src[(size_t)(2 * y) * w + 2 * x];
}

// extrema of DoG layer blockIdx.z + 1 inside the border: |v| > threshold and v >= (v > 0) or <= (v < 0) all 26 neighbours.
// The candidates of a workgroup take their places with one LDS counter and one global atomic; the list's order is arbitrary.
__global__ __launch_bounds__(256) void scan_kernel(const float *__restrict__ dog, size_t plane, int h, int w, float threshold,
                                                   ksf_cand *__restrict__ cand, unsigned cap, unsigned *__restrict__ counter)
{
    __shared__ unsigned s_count, s_base;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const int x = sf::BORDER + blockIdx.x * 256 + threadIdx.x, y = sf::BORDER + blockIdx.y, layer = blockIdx.z + 1;
    bool hit = false;
    if (x < w - sf::BORDER && y < h - sf::BORDER) {
        const float *p = dog + (size_t)layer * plane + (size_t)y * w + x;
        const float v = p[0];
        if (sf::absf(v) > threshold) {
            bool ge = true, le = true;
            for (int dl = -1; dl <= 1; dl++)
                for (int dr = -1; dr <= 1; dr++) {
                    const float *q = p + (ptrdiff_t)dl * (ptrdiff_t)plane + (ptrdiff_t)dr * w;
#pragma unroll
                    for (int dc = -1; dc <= 1; dc++) { ge = ge && v >= q[dc]; le = le && v <= q[dc]; }
                }
            hit = (v > 0 && ge) || (v < 0 && le);
        }
    }
    unsigned mine = 0;
    if (hit) mine = atomicAdd(&s_count, 1u);
    __syncthreads();
    if (threadIdx.x == 0 && s_count) s_base = atomicAdd(counter, s_count);
    __syncthreads();
    if (hit && (unsigned long long)s_base + mine < cap) cand[s_base + mine] = ksf_cand{layer, y, x};
}

// the place of a lane's record in a list: one atomic per wave
__device__ __forceinline__ unsigned wave_append(bool flag, unsigned *counter)
{
    const unsigned long long ballot = __ballot(flag);
    const int lane = threadIdx.x & 63;
    unsigned base = 0;
    if (lane == 0 && ballot) base = atomicAdd(counter, (unsigned)__popcll(ballot));
    base = __shfl(base, 0);
    return base + (unsigned)__popcll(ballot & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(256) void refine_kernel(const float *__restrict__ dog, size_t plane, int h, int w, int octv, const ksf_cand *__restrict__ cand,
                                                     unsigned n_cand, int n_layers, double contrast, double edge, double sigma,
                                                     sf::Refined *__restrict__ out, unsigned *__restrict__ counter)
{
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    sf::Refined r;
    bool ok = false;
    if (i < n_cand) {
        const ksf_cand cd = cand[i];
        ok = sf::refine(dog, plane, w, h, w, octv, cd.layer, cd.r, cd.c, n_layers, contrast, edge, sigma, r);
    }
    const unsigned at = wave_append(ok, counter);     // at most n_cand records: the list has room for all of them
    if (ok) out[at] = r;
}

__global__ __launch_bounds__(64) void orient_kernel(const float *__restrict__ gauss, size_t plane, int h, int w, int octv,
                                                    const sf::Refined *__restrict__ refined, unsigned n_refined, sf::Key *__restrict__ kp, unsigned cap,
                                                    unsigned *__restrict__ counter)
{
    const unsigned i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_refined) return;
    const sf::Refined r = refined[i];
    float angles[sf::ORI_BINS / 2];
    const int n = sf::orientations(gauss + (size_t)r.layer * plane, w, h, w, r.r, r.c, r.size, octv, angles);
    if (n == 0) return;
    const unsigned at = atomicAdd(counter, (unsigned)n);
    for (int k = 0; k < n; k++)
        if ((unsigned long long)at + k < cap) kp[at + k] = sf::Key{r.x, r.y, r.size, angles[k], r.response, r.octave};
}

// one wave per workgroup: a lane's 6 x 6 x 10 histogram is its column of the LDS array (word k * 64 + lane)
__global__ __launch_bounds__(64) void describe_kernel(const float *__restrict__ gauss, size_t plane, int h, int w, int octv, const sf::Key *__restrict__ kp,
                                                      unsigned n, uint8_t *__restrict__ desc)
{
    __shared__ float hist[sf::D_HIST * 64];
    const unsigned i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const sf::Key q = kp[i];
    const int layer = (q.octave >> 8) & 255;
    const float inv = 1.f / (float)(1 << octv);
    uint8_t row[sf::D_LEN];
    sf::descriptor<64>(gauss + (size_t)layer * plane, w, h, w, q.x * inv, q.y * inv, q.angle, q.size * inv * 0.5f, hist + threadIdx.x, row);
    uint32_t *dst = (uint32_t *)(desc + (size_t)i * sf::D_LEN);
    for (int k = 0; k < sf::D_LEN / 4; k++)
        dst[k] = (uint32_t)row[4 * k] | ((uint32_t)row[4 * k + 1] << 8) | ((uint32_t)row[4 * k + 2] << 16) | ((uint32_t)row[4 * k + 3] << 24);
}

__global__ __launch_bounds__(128) void gather_kernel(const sf::Key *__restrict__ kp, const uint8_t *__restrict__ desc, const int *__restrict__ perm, int n,
                                                     float *__restrict__ x, float *__restrict__ y, float *__restrict__ size, float *__restrict__ angle,
                                                     float *__restrict__ response, int *__restrict__ octave, void *__restrict__ out_desc, int as_f32,
                                                     ptrdiff_t desc_stride)
{
    const int i = blockIdx.x;
    if (i >= n) return;
    const int src = perm[i];
    if (threadIdx.x == 0) {
        const sf::Key q = kp[src];
        x[i] = q.x * 0.5f; y[i] = q.y * 0.5f; size[i] = q.size * 0.5f; angle[i] = q.angle; response[i] = q.response;
        octave[i] = (q.octave & ~255) | ((q.octave - 1) & 255);      // firstOctave = -1
    }
    const uint8_t v = desc[(size_t)src * sf::D_LEN + threadIdx.x];
    if (as_f32) ((float *)out_desc)[(ptrdiff_t)i * desc_stride + threadIdx.x] = (float)v;
    else ((uint8_t *)out_desc)[(ptrdiff_t)i * desc_stride + threadIdx.x] = v;
}

inline dim3 grid2(int w, int h) { return dim3((unsigned)((w + 255) / 256), (unsigned)h); }

}  // namespace

int ksf_base(km_ctx *c, const uint8_t *d_img, int H, int W, ptrdiff_t stride, float *d_out)
{
    base_kernel<<<grid2(2 * W, 2 * H), 256, 0, c->stream>>>(d_img, H, W, stride, d_out);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ksf_blur(km_ctx *c, const float *src, int h, int w, const ksf_taps &taps, float *tmp, float *dst, float *dog)
{
    blur_rows_kernel<<<grid2(w, h), 256, 0, c->stream>>>(src, h, w, taps, tmp);
    KM_LAUNCH_CHECK(c);
    blur_cols_kernel<<<grid2(w, h), 256, 0, c->stream>>>(tmp, src, h, w, taps, dst, dog);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ksf_decimate(km_ctx *c, const float *src, int h, int w, float *dst)
{
    const int h2 = h / 2, w2 = w / 2;
    if (h2 <= 0 || w2 <= 0) return KM_OK;
    decimate_kernel<<<grid2(w2, h2), 256, 0, c->stream>>>(src, w, h2, w2, dst);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ksf_scan(km_ctx *c, const float *dog, size_t plane, int h, int w, int n_layers, float threshold, ksf_cand *cand, unsigned cap, unsigned *counter)
{
    if (h <= 2 * sf::BORDER || w <= 2 * sf::BORDER) return KM_OK;
    const dim3 grid((unsigned)((w - 2 * sf::BORDER + 255) / 256), (unsigned)(h - 2 * sf::BORDER), (unsigned)n_layers);
    scan_kernel<<<grid, 256, 0, c->stream>>>(dog, plane, h, w, threshold, cand, cap, counter);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ksf_refine(km_ctx *c, const float *dog, size_t plane, int h, int w, int octv, const ksf_cand *cand, unsigned n_cand, int n_layers,
               double contrast_threshold, double edge_threshold, double sigma, sf::Refined *out, unsigned *counter)
{
    refine_kernel<<<(n_cand + 255) / 256, 256, 0, c->stream>>>(dog, plane, h, w, octv, cand, n_cand, n_layers, contrast_threshold, edge_threshold, sigma, out,
                                                               counter);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ksf_orient(km_ctx *c, const float *gauss, size_t plane, int h, int w, int octv, const sf::Refined *refined, unsigned n_refined, sf::Key *kp,
               unsigned cap, unsigned *counter)
{
    orient_kernel<<<(n_refined + 63) / 64, 64, 0, c->stream>>>(gauss, plane, h, w, octv, refined, n_refined, kp, cap, counter);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ksf_describe(km_ctx *c, const float *gauss, size_t plane, int h, int w, int octv, const sf::Key *kp, unsigned n, uint8_t *desc)
{
    describe_kernel<<<(n + 63) / 64, 64, 0, c->stream>>>(gauss, plane, h, w, octv, kp, n, desc);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int ksf_gather(km_ctx *c, const sf::Key *kp, const uint8_t *desc, const int *perm, int n, float *x, float *y, float *size, float *angle,
               float *response, int *octave, void *out_desc, int desc_dtype, ptrdiff_t desc_stride)
{
    gather_kernel<<<(unsigned)n, 128, 0, c->stream>>>(kp, desc, perm, n, x, y, size, angle, response, octave, out_desc, desc_dtype == KM_F32, desc_stride);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
