// The corner mask under a geometric prior (k_prior.hpp, prior_math.hpp; DESIGN.md section 21, rule 4).  One thread per pixel: a wave
// reads 64 consecutive pixels of a reference row (or of the user mask) and writes 64 consecutive mask bytes; the monitored read is a
// gather at the rounded mapped position - for a shift that is a row-wise copy, for a homography neighbouring lanes still meet
// neighbouring pixels.  The mask is one byte per pixel and the pass is bound by the two raster reads.
#include "common.hpp"
#include "k_prior.hpp"

template <typename T>
__global__ __launch_bounds__(256) void prior_mask_kernel(kp_mask_args a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const T *ref = (const T *)a.ref, *mon = (const T *)a.mon;
    bool ok = a.base ? a.base[(ptrdiff_t)y * a.sbase + x] != 0 : pm::valid<T>(ref[(ptrdiff_t)y * a.sref + x], a.has_nd_ref, a.nd_ref);
    int rx, ry;
    // (pm::target: 0 <= rx < W and 0 <= ry < H, or no read)
    ok = ok && pm::target(a.P, a.x_off, a.y_off, x, y, a.W, a.H, rx, ry) && pm::valid<T>(mon[(ptrdiff_t)ry * a.smon + rx], a.has_nd_mon, a.nd_mon);
    a.mask[(size_t)y * a.W + x] = ok ? 1 : 0;
}

// Batched units: the same item for the pixel (x, y) of unit blockIdx.z, whose arguments are entry blockIdx.z of the table (kernel
// arguments: the entry is read with scalar loads, the index is the same in every lane).  The grid spans the widest and the tallest
// unit; a workgroup outside its unit's box leaves at once.
static_assert(KP_MASK_UNITS_MAX == KM_UNITS_MAX, "one table entry per unit of a batched submission");
template <typename T>
__global__ __launch_bounds__(256) void prior_mask_units_kernel(kp_mask_units A)
{
    const kp_mask_args &a = A.a[blockIdx.z];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const T *ref = (const T *)a.ref, *mon = (const T *)a.mon;
    bool ok = a.base ? a.base[(ptrdiff_t)y * a.sbase + x] != 0 : pm::valid<T>(ref[(ptrdiff_t)y * a.sref + x], a.has_nd_ref, a.nd_ref);
    int rx, ry;
    // (pm::target: 0 <= rx < W and 0 <= ry < H, or no read)
    ok = ok && pm::target(a.P, a.x_off, a.y_off, x, y, a.W, a.H, rx, ry) && pm::valid<T>(mon[(ptrdiff_t)ry * a.smon + rx], a.has_nd_mon, a.nd_mon);
    a.mask[(size_t)y * a.W + x] = ok ? 1 : 0;
}

int kp_prior_mask_units(km_ctx *c, const kp_mask_units &A)
{
    if (A.n <= 0) return KM_OK;
    if (A.n > KP_MASK_UNITS_MAX) return km_fail(c, KM_E_ARG, "prior_mask: %d units (at most %d)", A.n, KP_MASK_UNITS_MAX);
    int W = 0, H = 0;
    for (int u = 0; u < A.n; u++) {
        if (A.a[u].dtype != A.a[0].dtype) return km_fail(c, KM_E_ARG, "prior_mask: the units of a batch share one pixel type");
        W = A.a[u].W > W ? A.a[u].W : W; H = A.a[u].H > H ? A.a[u].H : H;
    }
    if (H <= 0 || W <= 0) return KM_OK;
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4), (unsigned)A.n);
    if (grid.y > 65535u) return km_fail(c, KM_E_UNSUPPORTED, "prior_mask: %d rows (at most 262140)", H);
    if (int rc = km_with_pixel_type(c, A.a[0].dtype, "prior_mask: bad dtype %d", [&](auto t) {
            using T = decltype(t);
            prior_mask_units_kernel<T><<<grid, 256, 0, c->stream>>>(A);
            return KM_OK;
        })) return rc;
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kp_prior_mask(km_ctx *c, const kp_mask_args &a)
{
    if (a.H <= 0 || a.W <= 0) return KM_OK;
    const dim3 grid((unsigned)((a.W + 63) / 64), (unsigned)((a.H + 3) / 4));
    if (grid.y > 65535u) return km_fail(c, KM_E_UNSUPPORTED, "prior_mask: %d rows (at most 262140)", a.H);
    if (int rc = km_with_pixel_type(c, a.dtype, "prior_mask: bad dtype %d", [&](auto t) {
            using T = decltype(t);
            prior_mask_kernel<T><<<grid, 256, 0, c->stream>>>(a);
            return KM_OK;
        })) return rc;
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
