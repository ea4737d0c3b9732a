// Whole-raster passes of the KARIOS matching path (gfx950) - HBM-bound reductions, copies and one small stencil, integer-exact, no MFMA:
//   K1  NaN-aware min/max reduction            (reference klt.py:46)
//       stand-alone uint8 stretch, automatic mask, non-zero count of a user mask (klt.py:42-49, 268-276)
//       final reductions of per-workgroup partials (kd_sum_u32 / kd_max_u32: the dense stages' one-workgroup sums and maxima)
//   K6  pyrDown 5x5, both images of a pair - of every unit of a batch (km_units, api_units.hip) - in one launch
//   K11 integer image shift                     (core/image.py:70-101)
// K1 keeps a single-tile kernel of its own beside the batched one: the batched one carries the `deep` path of background launches
// (58 instead of 20 VGPRs at 16 bits) and measured 85 instead of 75 us on a blocking 10980^2 tile.
// K6 is here, not in a file of its own, for its instructions' sake: alone in a translation unit its one call of the runtime header's
// static min(int, int) is the last call of a static function, the inliner prices that differently and pyrdown_units_kernel comes out
// with another schedule (same results).  Beside K1's calls of the same function it compiles to what it always was.
#include "k_pixel.hpp"

// ------------------------------------------------------------------ K1 min/max
// One image (or one box of a larger raster: stride > W) reduced by the `nth` threads of a launch that share it: 16-byte vector loads
// over the aligned body of every contiguous span - the whole image when its rows are dense, else row by row (a box of a larger
// raster: the tiles of `KLT.match` on a resident pair; byte loads there cost 0.27 ms per 30-Mpx tile) - packed 16-bit min / max.
template <typename T>
__device__ __forceinline__ void minmax_image(const T *__restrict__ img, int H, int W, ptrdiff_t stride, unsigned blk, unsigned nblk, double *partial_out,
                                             bool deep = false)
{
    using A = typename px_traits<T>::acc;
    A mn, mx;
    if constexpr (px_traits<T>::code == KM_F32) { mn = INFINITY; mx = -INFINITY; }
    else { mn = 0x7fffffff; mx = -0x7fffffff - 1; }
    auto upd = [&](T v) {
        if constexpr (px_traits<T>::code == KM_F32) { mn = fminf(mn, v); mx = fmaxf(mx, v); }
        else { mn = min(mn, (A)v); mx = max(mx, (A)v); }
    };
    constexpr int V = 16 / sizeof(T);
    // 16-bit pixels: packed minimum / maximum of the dwords as loaded (v_pk_min/max_u16|i16: 2 instructions per pixel pair
    // where widening each pixel took 6), folded into mn / mx after the loop
    typedef typename std::conditional<std::is_signed<T>::value, short, unsigned short>::type P16;
    typedef P16 pk2 __attribute__((ext_vector_type(2)));
    constexpr bool PACKED = sizeof(T) == 2 && px_traits<T>::code != KM_F32;
    pk2 pmn, pmx;
    pmn.x = pmn.y = std::is_signed<T>::value ? (P16)0x7fff : (P16)0xffff;
    pmx.x = pmx.y = std::is_signed<T>::value ? (P16)0x8000 : (P16)0;
    bool packed_used = false;
    auto take = [&](const uint4 &q) {
        if constexpr (PACKED) {
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                pk2 v;
                __builtin_memcpy(&v, &w[k], 4);
                pmn = __builtin_elementwise_min(pmn, v);
                pmx = __builtin_elementwise_max(pmx, v);
            }
            packed_used = true;
        } else {
            T e[V];
            __builtin_memcpy(e, &q, 16);
#pragma unroll
            for (int k = 0; k < V; k++) upd(e[k]);
        }
    };
    // span of n contiguous pixels, shared by threads tid of nth
    auto span = [&](const T *p, size_t n, size_t tid, size_t nth) {
        const uintptr_t base = (uintptr_t)p;
        size_t head = ((16 - (base & 15)) & 15) / sizeof(T);
        if (head > n) head = n;
        const size_t nvec = (n - head) / V;
        const uint4 *vp = (const uint4 *)(p + head);
        // `deep` - eight independent 16-byte loads in flight per thread: beside instruction-bound kernels (the next submission's min / max beside
        // LK .. ZNCC) the kernel runs as ONE workgroup per compute unit - it must reach its bandwidth with four waves per CU, and must
        // not occupy more: spread over every wave slot LK's retiring waves left, its long-lived workgroups kept the 1024-thread workgroups
        // of the frame stage waiting for whole CUs until it had drained (fb_compact 5 -> 189 us per submission)
        size_t i = tid;
        if (deep)
        for (; i + 7 * nth < nvec; i += 8 * nth) {
            uint4 q[8];
#pragma unroll
            for (int k = 0; k < 8; k++) q[k] = vp[i + k * nth];
#pragma unroll
            for (int k = 0; k < 8; k++) take(q[k]);
        }
        for (; i < nvec; i += nth) take(vp[i]);
        if (tid < head) upd(p[tid]);
        const size_t tail0 = head + nvec * V;
        if (tail0 + tid < n && tid < (size_t)V) upd(p[tail0 + tid]);
    };
    if (stride == W) {
        span(img, (size_t)H * W, (size_t)blk * blockDim.x + threadIdx.x, (size_t)nblk * blockDim.x);
    } else {
        for (int y = (int)blk; y < H; y += (int)nblk) span(img + (size_t)y * stride, (size_t)W, threadIdx.x, blockDim.x);
    }
    if constexpr (PACKED) {
        if (packed_used) {      // (the packed accumulators hold real pixels or their neutral start values)
            mn = min(mn, min((A)pmn.x, (A)pmn.y));
            mx = max(mx, max((A)pmx.x, (A)pmx.y));
        }
    }
    double dmn = wave_min((double)mn), dmx = wave_max((double)mx);
    __shared__ double s[2][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s[0][w] = dmn; s[1][w] = dmx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial_out[0] = fmin(fmin(s[0][0], s[0][1]), fmin(s[0][2], s[0][3]));
        partial_out[1] = fmax(fmax(s[1][0], s[1][1]), fmax(s[1][2], s[1][3]));
    }
}

// blockIdx.y selects the image (kd_minmax with a second image: both rasters of a pair in one launch); partials of image y start at 2 * gridDim.x * y
template <typename T>
__global__ __launch_bounds__(256) void minmax_partial_kernel(const T *__restrict__ img0, const T *__restrict__ img1, int H, int W,
                                                             ptrdiff_t stride0, ptrdiff_t stride1, double *partial)
{
    minmax_image<T>(blockIdx.y ? img1 : img0, H, W, blockIdx.y ? stride1 : stride0, blockIdx.x, gridDim.x,
                    partial + (size_t)2 * gridDim.x * blockIdx.y + 2 * blockIdx.x);
}

// batched units: blockIdx.z = unit, blockIdx.y = raster (0 ref, 1 mon)
struct mm_units_args {
    const void *img[2][KM_UNITS_MAX];
    ptrdiff_t stride[2][KM_UNITS_MAX];
    int H[KM_UNITS_MAX], W[KM_UNITS_MAX];
    double *out[KM_UNITS_MAX];
};
template <typename T>
__global__ __launch_bounds__(256) void minmax_partial_units_kernel(mm_units_args U, double *partial, int deep)
{
    const unsigned u = blockIdx.z, im = blockIdx.y;
    minmax_image<T>((const T *)U.img[im][u], U.H[u], U.W[u], U.stride[im][u], blockIdx.x, gridDim.x,
                    partial + (size_t)2 * gridDim.x * (2 * u + im) + 2 * blockIdx.x, deep != 0);
}

__device__ __forceinline__ void minmax_final(const double *partial, int nb, double *out)
{
    double mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) {
        mn = fmin(mn, partial[2 * i]);
        mx = fmax(mx, partial[2 * i + 1]);
    }
    mn = wave_min(mn); mx = wave_max(mx);
    __shared__ double s[2][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s[0][w] = mn; s[1][w] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = fmin(fmin(s[0][0], s[0][1]), fmin(s[0][2], s[0][3]));
        out[1] = fmax(fmax(s[1][0], s[1][1]), fmax(s[1][2], s[1][3]));
    }
}
__global__ __launch_bounds__(256) void minmax_final_kernel(const double *partial, int nb, double *out)
{
    minmax_final(partial + (size_t)2 * nb * blockIdx.x, nb, out + 2 * blockIdx.x);     // (one block per image)
}
__global__ __launch_bounds__(256) void minmax_final_units_kernel(const double *partial, int nb, mm_units_args U)
{
    minmax_final(partial + (size_t)2 * nb * (2 * blockIdx.y + blockIdx.x), nb, U.out[blockIdx.y] + 2 * blockIdx.x);   // grid (2, units)
}

// min / max of one image (d_b == nullptr) or of the two rasters of a pair in one launch: d_mm[0..1] (and d_mm[2..3])
int kd_minmax(km_ctx *c, const void *d_a, int dtype, int H, int W, ptrdiff_t sa, double *d_mm, const void *d_b, ptrdiff_t sb, int ws_slot)
{
    // workgroups per image.  Beside LK (early min / max: ws_slot != WS_PARTIAL) the kernel is off the critical path and takes
    // fewer wave slots from the kernel it shares the GPU with
    static const int nb_early = [] { const char *e = km_dev_env("KARIOS_HIP_MM_EARLY_NB"); const int v = e ? atoi(e) : 0; return v >= 64 && v <= 2048 ? v : 2048; }();
    // (one pair at a time: the early min / max has only LK .. ZNCC of ONE pair, 0.27 ms, to hide behind - it needs the bandwidth of many
    // workgroups; a batched submission's runs as one workgroup per CU, kd_minmax_units)
    const int nb = ws_slot == WS_PARTIAL ? 2048 : nb_early, ni = d_b ? 2 : 1;
    double *partial = (double *)km_ws(c, ws_slot, (size_t)2 * nb * ni * sizeof(double));
    if (!partial) return KM_E_NOMEM;
    const dim3 grid(nb, ni);
    if (int rc = km_with_pixel_type(c, dtype, "minmax: bad dtype %d", [&](auto t) {
            using T = decltype(t);
            minmax_partial_kernel<T><<<grid, 256, 0, c->stream>>>((const T *)d_a, (const T *)d_b, H, W, sa, sb, partial);
            return KM_OK;
        })) return rc;
    KM_LAUNCH_CHECK(c);
    minmax_final_kernel<<<ni, 256, 0, c->stream>>>(partial, nb, d_mm);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

// both rasters of every unit of a batch in ONE launch (+ one final launch): out[u] = {min_ref, max_ref, min_mon, max_mon}
int kd_minmax_units(km_ctx *c, const km_units &U, double *const *d_out, int ws_slot)
{
    mm_units_args A;
    for (int u = 0; u < U.n; u++) {
        A.img[0][u] = U.ref[u]; A.img[1][u] = U.mon[u]; A.stride[0][u] = U.sref[u]; A.stride[1][u] = U.smon[u];
        A.H[u] = U.H[u]; A.W[u] = U.W[u]; A.out[u] = d_out[u];
    }
    // workgroups per raster: ~4096 - 8192 over the batch on the critical path.  Beside other kernels (ws_slot != WS_PARTIAL: the early
    // min / max of a submission behind another one) whole rasters run as ONE workgroup per compute unit over the batch with eight
    // loads in flight per thread (`deep`); boxes of larger rasters go row by row - too few vectors per thread and row for that
    int nb = U.n >= 8 ? 256 : U.n >= 4 ? 512 : 1024, deep = 0;
    if (ws_slot != WS_PARTIAL) {
        bool flat = true;
        for (int u = 0; u < U.n; u++) flat = flat && U.sref[u] == U.W[u] && U.smon[u] == U.W[u];
        if (flat) { nb = std::max(8, c->n_cu / (2 * U.n)); deep = 1; }
    }
    double *partial = (double *)km_ws(c, ws_slot, (size_t)2 * nb * 2 * U.n * sizeof(double));
    if (!partial) return KM_E_NOMEM;
    const dim3 grid(nb, 2, U.n);
    if (int rc = km_with_pixel_type(c, U.dtype, "minmax: bad dtype %d", [&](auto t) {
            minmax_partial_units_kernel<decltype(t)><<<grid, 256, 0, c->stream>>>(A, partial, deep);
            return KM_OK;
        })) return rc;
    KM_LAUNCH_CHECK(c);
    minmax_final_units_kernel<<<dim3(2, U.n), 256, 0, c->stream>>>(partial, nb, A);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

// ------------------------------------------------------------------ standalone stretch / mask
template <typename T>
__global__ __launch_bounds__(256) void to_uint8_kernel(const T *__restrict__ img, int H, int W, ptrdiff_t stride,
                                                       const double *mm, int invert, uint8_t *out)
{
    const double mn = mm[0], mx = mm[1], range = mx - mn;
    const bool deg = !(mx > mn);
    const size_t n = (size_t)H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        int y = (int)(i / W), x = (int)(i - (size_t)y * W);
        unsigned r = stretch_u8<T>(img[(size_t)y * stride + x], mn, range, deg);
        out[i] = (uint8_t)(invert ? 255u - r : r);
    }
}

int kd_to_uint8(km_ctx *c, const void *d_img, int dtype, int H, int W, ptrdiff_t stride, const double *d_mm,
                int invert, uint8_t *d_out)
{
    const int nb = 4096;
    if (int rc = km_with_pixel_type(c, dtype, "to_uint8: bad dtype %d", [&](auto t) {
            using T = decltype(t);
            to_uint8_kernel<T><<<nb, 256, 0, c->stream>>>((const T *)d_img, H, W, stride, d_mm, invert, d_out);
            return KM_OK;
        })) return rc;
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void auto_mask_kernel(const T *__restrict__ mon, const T *__restrict__ ref, int H, int W,
                                                        ptrdiff_t smon, ptrdiff_t sref, nodata_t nd, uint8_t *mask,
                                                        unsigned long long *valid)
{
    const size_t n = (size_t)H * W;
    unsigned long long cnt = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        int y = (int)(i / W), x = (int)(i - (size_t)y * W);
        bool ok = px_valid<T>(mon[(size_t)y * smon + x], ref[(size_t)y * sref + x], nd);
        mask[i] = ok ? 1 : 0;
        cnt += ok;
    }
    cnt = wave_sum_u64(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(valid, cnt);
}

int kd_auto_mask(km_ctx *c, const void *d_mon, const void *d_ref, int dtype, int H, int W, ptrdiff_t smon,
                 ptrdiff_t sref, const double *nodata_mon, const double *nodata_ref, uint8_t *d_mask,
                 unsigned long long *d_valid)
{
    nodata_t nd = make_nodata(nodata_mon, nodata_ref);
    KM_HIP(c, hipMemsetAsync(d_valid, 0, sizeof(unsigned long long), c->stream));
    const int nb = 4096;
    if (int rc = km_with_pixel_type(c, dtype, "auto_mask: bad dtype %d", [&](auto t) {
            using T = decltype(t);
            auto_mask_kernel<T><<<nb, 256, 0, c->stream>>>((const T *)d_mon, (const T *)d_ref, H, W, smon, sref, nd, d_mask, d_valid);
            return KM_OK;
        })) return rc;
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

// non-zero bytes of a user mask (the valid-pixel count of klt.py:276): 16-byte loads over the aligned body, the non-zero bytes of a
// dword counted with three logic operations and a population count (a byte load per pixel made this 0.2 ms at 10980^2 - as long as
// the whole stretch + Laplacian kernel it precedes)
__device__ __forceinline__ unsigned nonzero_bytes(uint32_t w)
{
    const uint32_t t = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;   // bit 7 of every byte that is not 0
    return (unsigned)__popc(t);
}
__global__ __launch_bounds__(256) void count_nonzero_kernel(const uint8_t *__restrict__ m, size_t n, unsigned *__restrict__ partial)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    size_t head = (16 - ((uintptr_t)m & 15)) & 15;
    if (head > n) head = n;
    const size_t nvec = (n - head) / 16;
    const uint4 *vp = (const uint4 *)(m + head);
    unsigned cnt32 = 0;
    for (size_t i = tid; i < nvec; i += nth) {
        const uint4 q = vp[i];
        cnt32 += nonzero_bytes(q.x) + nonzero_bytes(q.y) + nonzero_bytes(q.z) + nonzero_bytes(q.w);     // (< 2^32: a lane sees < 2^28 bytes)
    }
    unsigned long long cnt = cnt32;
    if (tid < head) cnt += m[tid] != 0;
    const size_t tail0 = head + nvec * 16;
    if (tid < 16 && tail0 + tid < n) cnt += m[tail0 + tid] != 0;
    // one partial per workgroup, summed by sum_u32_kernel: 8192 device-scope atomics on ONE word serialise (~10 ns each: 80 of the
    // kernel's 115 us were that)
    cnt = wave_sum_u64(cnt);
    __shared__ unsigned sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (unsigned)cnt;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

int kd_count_nonzero(km_ctx *c, const uint8_t *d_mask, size_t n, unsigned long long *d_valid)
{
    const unsigned nb = 4096;
    unsigned *partial = (unsigned *)km_ws(c, WS_PARTIAL, nb * sizeof(unsigned));
    if (!partial) return KM_E_NOMEM;
    count_nonzero_kernel<<<nb, 256, 0, c->stream>>>(d_mask, n, partial);
    KM_LAUNCH_CHECK(c);
    return kd_sum_u32(c, partial, nb, d_valid);
}

// final reductions of per-workgroup partials (one workgroup; the partial arrays are tens of KB)
__global__ __launch_bounds__(1024) void sum_u32_kernel(const unsigned *__restrict__ partial, unsigned n, unsigned long long *out)
{
    // ONE workgroup: writes (not accumulates) the total, so the launcher needs no memset
    unsigned long long s = 0;
    for (unsigned i = threadIdx.x; i < n; i += 1024) s += partial[i];
    s = wave_sum_u64(s);
    __shared__ unsigned long long sh[16];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int i = 0; i < 16; i++) t += sh[i];
        *out = t;
    }
}
__global__ __launch_bounds__(1024) void max_u32_kernel(const unsigned *__restrict__ partial, unsigned n, unsigned *out)
{
    unsigned m = 0;
    for (unsigned i = threadIdx.x; i < n; i += 1024) m = max(m, partial[i]);
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    __shared__ unsigned sh[16];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int i = 0; i < 16; i++) t = max(t, sh[i]);
        *out = t;
    }
}
int kd_sum_u32(km_ctx *c, const unsigned *d_partial, unsigned n, unsigned long long *d_out)
{
    sum_u32_kernel<<<1, 1024, 0, c->stream>>>(d_partial, n, d_out);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
int kd_max_u32(km_ctx *c, const unsigned *d_partial, unsigned n, unsigned *d_out)
{
    max_u32_kernel<<<1, 1024, 0, c->stream>>>(d_partial, n, d_out);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

// ------------------------------------------------------------------ K6 pyrDown
// cv::pyrDown u8: separable [1 4 6 4 1], (sum + 128) >> 8, REFLECT_101, dst = ((W+1)/2, (H+1)/2).
// Each thread owns 4 adjacent output columns and marches down PYR_RS output rows with a 5-deep register ring
// of horizontal sums (two new source rows per output row, loaded one step ahead as 4 aligned dwords each).
// Both images of a pair - of every unit of a batch - are processed by one launch (blockIdx.z).
#ifndef PYR_RS
#define PYR_RS 8    // output rows per thread: short items = more waves in different phases (0.14 ms at 32 rows, 0.098 at 8, 0.18 at 64; 10980^2 pair)
#endif

// horizontal [1 4 6 4 1] sums of 4 outputs from 16 source bytes starting at source column 8q-4: output j covers the
// bytes 2j+2 .. 2j+6 - four of them through one v_dot4_u32_u8 with the coefficients (1,4,6,4), the fifth added on top
__device__ __forceinline__ void pyr_hsum(const uint32_t (&w)[4], int (&h)[4])
{
    const unsigned coef = 0x04060401u;                                   // bytes (1, 4, 6, 4)
    const uint32_t q0 = __builtin_amdgcn_alignbyte(w[1], w[0], 2);       // bytes 2..5
    const uint32_t q2 = __builtin_amdgcn_alignbyte(w[2], w[1], 2);       // bytes 6..9
    h[0] = (int)__builtin_amdgcn_udot4(q0, coef, (w[1] >> 16) & 0xffu, false);    // + byte 6
    h[1] = (int)__builtin_amdgcn_udot4(w[1], coef, w[2] & 0xffu, false);          // bytes 4..7 + byte 8
    h[2] = (int)__builtin_amdgcn_udot4(q2, coef, (w[2] >> 16) & 0xffu, false);    // + byte 10
    h[3] = (int)__builtin_amdgcn_udot4(w[2], coef, w[3] & 0xffu, false);          // bytes 8..11 + byte 12
}

// One thread: output columns 4q .. 4q+3 of rows [y0, y1).  FAST (block-uniform): one 16-byte load per source row at whatever alignment
// the row has (a level of odd width - 5490 -> 2745 - puts three rows in four off the dword grid; the hardware reads unaligned just as
// well); otherwise byte by byte with REFLECT_101 columns.
template <bool FAST>
__device__ __forceinline__ void pyrdown_quad(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int H, int W, int dw, int q, int y0, int y1)
{
    const int sx0 = 8 * q - 4;                                  // first source byte loaded
    auto load_row = [&](int sy, uint32_t (&w)[4]) {
        const uint8_t *row = src + (size_t)km_reflect101(sy, H) * W;
        if (FAST) {
            __builtin_memcpy(w, row + sx0, 16);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t v = 0;
#pragma unroll 1
                for (int b = 0; b < 4; b++) v |= (uint32_t)row[km_reflect101(sx0 + 4 * k + b, W)] << (8 * b);     // (one byte at a time: these
                w[k] = v;                                                                                              // few lanes must not set the kernel's register count)
            }
        }
    };
    // ring of horizontal sums for source rows 2y-2 .. 2y+2, two outputs per dword (a sum is at most 16 x 255 = 4080, the vertical
    // [1 4 6 4 1] of five of them at most 65 280, + 128 for the rounding: everything stays inside 16 bits - packed arithmetic)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    auto hsum2 = [&](const uint32_t (&w)[4], u16x2 (&h)[2]) {
        int t[4];
        pyr_hsum(w, t);
        h[0] = __builtin_bit_cast(u16x2, (uint32_t)t[0] | ((uint32_t)t[1] << 16));
        h[1] = __builtin_bit_cast(u16x2, (uint32_t)t[2] | ((uint32_t)t[3] << 16));
    };
    u16x2 h0[2], h1[2], h2[2], h3[2], h4[2];
    uint32_t wa[4], wb[4];
    load_row(2 * y0 - 2, wa); hsum2(wa, h0);
    load_row(2 * y0 - 1, wa); hsum2(wa, h1);
    load_row(2 * y0, wa); hsum2(wa, h2);
    load_row(2 * y0 + 1, wa);
    load_row(2 * y0 + 2, wb);
    auto step = [&](int y) {
        hsum2(wa, h3);
        hsum2(wb, h4);
        if (y + 1 < y1) { load_row(2 * y + 3, wa); load_row(2 * y + 4, wb); }   // next step's rows, in flight during the math
        uint32_t r[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u16x2 s = (h0[j] + h4[j]) + (h1[j] + h3[j]) * (u16x2)(4) + h2[j] * (u16x2)(6) + (u16x2)(128);
            r[j] = __builtin_bit_cast(uint32_t, s >> (u16x2)(8));
        }
        const uint32_t packed = __builtin_amdgcn_perm(r[1], r[0], 0x06040200u);
        const int ox = 4 * q;
        const size_t o = (size_t)y * dw + ox;
        if (FAST || ox + 3 < dw) __builtin_memcpy(dst + o, &packed, 4);  // (one dword store, aligned or not)
        else {
            for (int j = 0; j < 4 && ox + j < dw; j++) dst[o + j] = (uint8_t)(packed >> (8 * j));
        }
#pragma unroll
        for (int j = 0; j < 2; j++) { h0[j] = h2[j]; h1[j] = h3[j]; h2[j] = h4[j]; }
    };
    if constexpr (FAST) {
#pragma unroll
        for (int t = 0; t < PYR_RS; t++) {                       // (unrolled: the ring rotates by renaming)
            if (y0 + t >= y1) break;
            step(y0 + t);
        }
    } else {
#pragma unroll 1
        for (int y = y0; y < y1; y++) step(y);
    }
}

// Work split of one image (blockIdx.x, blockIdx.y): the x-blocks [0, gx_fast) hold the INTERIOR quads 1 .. q_hi - every lane on the
// 16-byte path, no per-lane border code in those waves; the quads that touch the left / right border (quad 0 and the one or two behind
// q_hi) of ALL rows are gathered into the x-block gx_fast, 256 (output row, border quad) items per workgroup.  (With the border
// code behind a per-lane test, the first and the last wave of every row of workgroups ran the byte-by-byte path for one or two live
// lanes - 2 waves in 22 of a 5490-column level, and 40 % of the launch's vector instructions.)
__device__ __forceinline__ void pyrdown_item(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int H, int W, int dh, int dw, int nquads)
{
    const int q_hi = W >= 28 ? (W - 12) / 8 : 0;                // interior quads: 1 <= q <= q_hi  (8q - 4 >= 0, 8q + 12 <= W; 4q + 3 < dw follows)
    const int gx_fast = (q_hi + 255) / 256;
    if ((int)blockIdx.x < gx_fast) {
        const int q = 1 + blockIdx.x * 256 + threadIdx.x;
        const int y0 = blockIdx.y * PYR_RS, y1 = min(dh, y0 + PYR_RS);
        if (q > q_hi || y0 >= dh) return;
        pyrdown_quad<true>(src, dst, H, W, dw, q, y0, y1);
        return;
    }
    if ((int)blockIdx.x > gx_fast) return;
    // (ONE output row per border thread: its byte loads are issued one at a time - a thread marching 8 rows that way was the launch's
    //  tail: 124 us alone where the interior needs 80)
    const int nb = nquads - q_hi;                               // border quads: 0, q_hi + 1 .. nquads - 1
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (i >= nb * dh) return;
    const int y = i / nb, b = i - y * nb;
    const int q = b == 0 ? 0 : q_hi + b;
    pyrdown_quad<false>(src, dst, H, W, dw, q, y, y + 1);
}

// blockIdx.z = 2 * unit + image (kd_pyrdown_u8: one image); the grid covers the largest unit, the others leave their surplus workgroups
// at once
struct pyr_units_args {
    const uint8_t *src[2 * KM_UNITS_MAX];
    uint8_t *dst[2 * KM_UNITS_MAX];
    int H[KM_UNITS_MAX], W[KM_UNITS_MAX];
};
__global__ __launch_bounds__(256) void pyrdown_units_kernel(pyr_units_args P)
{
    const int u = blockIdx.z >> 1, H = P.H[u], W = P.W[u], dh = (H + 1) / 2, dw = (W + 1) / 2;
    pyrdown_item(P.src[blockIdx.z], P.dst[blockIdx.z], H, W, dh, dw, (dw + 3) / 4);
}

// grid.x of pyrdown_item's work split for a level of width W: the interior x-blocks + the one that gathers the border quads
static inline int pyr_grid_x(int W)
{
    const int q_hi = W >= 28 ? (W - 12) / 8 : 0;
    return (q_hi + 255) / 256 + 1;
}

// nimg images: grid.x for the widest level (pyr_grid_x), dh = the largest output height
static int pyrdown_launch(km_ctx *c, const pyr_units_args &P, int gx, int dh, int nimg)
{
    pyrdown_units_kernel<<<dim3(gx, (dh + PYR_RS - 1) / PYR_RS, nimg), 256, 0, c->stream>>>(P);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

// level l of both pyramids of every unit from level l - 1 (units whose pyramid ends below l are skipped by the caller: H = 0)
int kd_pyrdown_units(km_ctx *c, const km_units &U, int level)
{
    pyr_units_args P;
    int max_dh = 0, max_q = 0, n = 0;
    for (int u = 0; u < U.n; u++) {
        if (U.A[u].levels < level) continue;
        P.src[2 * n] = U.A[u].img[level - 1]; P.src[2 * n + 1] = U.B[u].img[level - 1];
        P.dst[2 * n] = (uint8_t *)U.A[u].img[level]; P.dst[2 * n + 1] = (uint8_t *)U.B[u].img[level];
        P.H[n] = U.A[u].H[level - 1]; P.W[n] = U.A[u].W[level - 1];
        const int dh = (P.H[n] + 1) / 2;
        max_dh = dh > max_dh ? dh : max_dh;
        max_q = pyr_grid_x(P.W[n]) > max_q ? pyr_grid_x(P.W[n]) : max_q;       // (x-blocks, not quads)
        n++;
    }
    if (n == 0) return KM_OK;
    return pyrdown_launch(c, P, max_q, max_dh, 2 * n);
}

int kd_pyrdown_u8(km_ctx *c, const uint8_t *d_src, int H, int W, uint8_t *d_dst)
{
    pyr_units_args P;
    P.src[0] = d_src; P.dst[0] = d_dst; P.H[0] = H; P.W[0] = W;
    return pyrdown_launch(c, P, pyr_grid_x(W), (H + 1) / 2, 1);
}

int kd_pyrdown_u8_pair(km_ctx *c, const uint8_t *d_src_a, const uint8_t *d_src_b, int H, int W, uint8_t *d_dst_a, uint8_t *d_dst_b)
{
    pyr_units_args P;
    P.src[0] = d_src_a; P.src[1] = d_src_b; P.dst[0] = d_dst_a; P.dst[1] = d_dst_b; P.H[0] = H; P.W[0] = W;
    return pyrdown_launch(c, P, pyr_grid_x(W), (H + 1) / 2, 2);
}

// ------------------------------------------------------------------ K11 integer shift
// out(y, x) = img(y + y_off, x + x_off), zero outside (reference large_offset.py `_shift_image`): a row is a byte copy at an offset -
// 16 bytes per lane with unaligned loads and stores, whatever the element size (one element per lane with a 64-bit division each
// ran at 2.5 TB/s; sub-dword global accesses pass the address unit a lane at a time).  Chunks that touch an edge go byte by byte.
__global__ __launch_bounds__(256) void shift_rows_kernel(const uint8_t *__restrict__ img, int H, long long rowbytes, long long stride_bytes, int y_off,
                                                         long long xoff_bytes, uint8_t *__restrict__ out)
{
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const long long sy = (long long)y + y_off;
        const bool row_in = sy >= 0 && sy < H;
        const uint8_t *src = img + (size_t)(row_in ? sy : 0) * (size_t)stride_bytes;
        uint8_t *o = out + (size_t)y * (size_t)rowbytes;
        for (long long b = ((long long)blockIdx.x * 256 + threadIdx.x) * 16; b < rowbytes; b += (long long)gridDim.x * 256 * 16) {
            const long long sb = b + xoff_bytes;
            if (row_in && sb >= 0 && sb + 16 <= rowbytes && b + 16 <= rowbytes) {
                uint4 v;
                __builtin_memcpy(&v, src + sb, 16);
                __builtin_memcpy(o + b, &v, 16);
            } else {
                for (int k = 0; k < 16 && b + k < rowbytes; k++) {
                    const long long sx = sb + k;
                    o[b + k] = row_in && sx >= 0 && sx < rowbytes ? src[sx] : (uint8_t)0;
                }
            }
        }
    }
}

int kd_shift_image(km_ctx *c, const void *d_img, int elem_size, int H, int W, ptrdiff_t stride, int y_off, int x_off, void *d_out)
{
    if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) return km_fail(c, KM_E_ARG, "shift_image: elem_size %d", elem_size);
    if (H <= 0 || W <= 0) return KM_OK;
    const long long rowbytes = (long long)W * elem_size;
    const dim3 grid((unsigned)std::min<long long>((rowbytes + 16 * 256 - 1) / (16 * 256), 64), (unsigned)std::min(H, 65535));
    shift_rows_kernel<<<grid, 256, 0, c->stream>>>((const uint8_t *)d_img, H, rowbytes, (long long)stride * elem_size, y_off, (long long)x_off * elem_size, (uint8_t *)d_out);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
