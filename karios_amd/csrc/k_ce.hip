// Device half of the circular-error figure's numbers (karios/report/circular_error_plot.py), see k_ce.hpp.  Every operation that decides a
// bit is ce_math.hpp's or accuracy_math.hpp's; the library's -ffp-contract=off and correctly rounded division / square root apply.  Counts
// and orders come from integer counters and the radix sort only, so two runs of a call give the same bits.
//   kce_scale          one lane per row of the sample: x, y, the radial error; minimum and maximum of dx, +-dy, x, y as order keys -
//                      a xor-butterfly per wavefront, one integer atomic per wavefront and extreme
//   kce_axis_hist      blockIdx.y = axis.  Up to ce::LDS_BINS bins: the edges and the counters of the axis in LDS, LDS integer atomics,
//                      the non-zero counters added to the global ones at the end; above: global integer atomics, the edges from memory
//   kce_grid_hist      100 LDS counters per workgroup
//   kce_density_keys   one lane per row: knots and coefficients from a device table into LDS, bispeu in float64; the sort keys
//   kce_sort_gather    km_sort_u64 over the keys of both columns, then one lane per rank
#include "k_ce.hpp"
#include "common.hpp"

namespace {

constexpr int CE_T = 256;

__global__ __launch_bounds__(CE_T) void kce_scale_kernel(const float *__restrict__ cols, int n_max, float res, float *__restrict__ scaled, kce_state *s)
{
    const int i = blockIdx.x * CE_T + threadIdx.x, n = s->st.n;
    if (i == 0) {
        ka_state z = ka_state();
        z.n = n; z.n_nan = s->st.n_nan;
        s->scaled = z;
    }
    uint32_t k[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};       // (no row: below every key of a row - min keys are inverted, zero is ~(+NaN))
    if (i < n) {
        const float dx = cols[i], dy = cols[(size_t)n_max + i];
        const float v[4] = {dx, dy, dx * res, dy * res};
        scaled[i] = v[2];
        scaled[(size_t)n_max + i] = v[3];
        scaled[2 * (size_t)n_max + i] = ac::radial(dx, dy, res);
#pragma unroll
        for (int j = 0; j < 4; j++) { k[2 * j] = kce_min_key(v[j]); k[2 * j + 1] = ac::order_key(v[j]); }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t m = k[j];
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = (uint32_t)__shfl_xor((int)m, o);
            m = u > m ? u : m;
        }
        if ((threadIdx.x & 63) == 0 && m) atomicMax(&s->ext[j], m);
    }
}

__global__ void kce_block_kernel(kce_state *s) { kce_fill_block(s); }

__global__ __launch_bounds__(CE_T) void kce_axis_hist_kernel(const float *__restrict__ scaled, int n_max, const kce_state *__restrict__ s, kce_axis ax0,
                                                             kce_axis ax1)
{
    __shared__ float s_edges[ce::LDS_BINS + 1];
    __shared__ unsigned s_count[ce::LDS_BINS];
    const kce_axis ax = blockIdx.y ? ax1 : ax0;
    const int nb = ax.bins, n = s->st.n;
    if (nb <= 0) return;
    const float *v = scaled + (size_t)blockIdx.y * n_max;
    const float first = ax.edges[0], denom = ax.edges[nb] - first;
    const int step = gridDim.x * CE_T;
    if (nb <= ce::LDS_BINS) {
        for (int j = threadIdx.x; j <= nb; j += CE_T) s_edges[j] = ax.edges[j];
        for (int j = threadIdx.x; j < nb; j += CE_T) s_count[j] = 0u;
        __syncthreads();
        for (int i = blockIdx.x * CE_T + threadIdx.x; i < n; i += step) atomicAdd(&s_count[ce::axis_bin(v[i], first, denom, nb, s_edges)], 1u);
        __syncthreads();
        for (int j = threadIdx.x; j < nb; j += CE_T)
            if (s_count[j]) atomicAdd(&ax.count[j], s_count[j]);
    } else {
        for (int i = blockIdx.x * CE_T + threadIdx.x; i < n; i += step) atomicAdd(&ax.count[ce::axis_bin(v[i], first, denom, nb, ax.edges)], 1u);
    }
}

__global__ __launch_bounds__(CE_T) void kce_grid_hist_kernel(const float *__restrict__ scaled, int n_max, const kce_state *__restrict__ s,
                                                             const float *__restrict__ edges, unsigned *__restrict__ count)
{
    __shared__ float s_edges[2 * (ce::GRID + 1)];
    __shared__ unsigned s_count[ce::GRID * ce::GRID];
    const int n = s->st.n;
    if (threadIdx.x < 2 * (ce::GRID + 1)) s_edges[threadIdx.x] = edges[threadIdx.x];
    if (threadIdx.x < ce::GRID * ce::GRID) s_count[threadIdx.x] = 0u;
    __syncthreads();
    for (int i = blockIdx.x * CE_T + threadIdx.x; i < n; i += gridDim.x * CE_T) {
        const int bx = ce::grid_bin(scaled[i], s_edges), by = ce::grid_bin(scaled[(size_t)n_max + i], s_edges + ce::GRID + 1);
        if (bx >= 0 && bx < ce::GRID && by >= 0 && by < ce::GRID) atomicAdd(&s_count[bx * ce::GRID + by], 1u);
    }
    __syncthreads();
    if (threadIdx.x < ce::GRID * ce::GRID && s_count[threadIdx.x]) atomicAdd(&count[threadIdx.x], s_count[threadIdx.x]);
}

__global__ __launch_bounds__(CE_T) void kce_density_keys_kernel(const float *__restrict__ scaled, int n_max, const kce_state *__restrict__ s,
                                                                const kce_spline *__restrict__ sp, float *__restrict__ z,
                                                                unsigned long long *__restrict__ keys)
{
    __shared__ double s_t[2 * ce::KNOTS + ce::GRID * ce::GRID];
    for (int j = threadIdx.x; j < 2 * ce::KNOTS + ce::GRID * ce::GRID; j += CE_T)
        s_t[j] = j < ce::KNOTS ? sp->tx[j] : j < 2 * ce::KNOTS ? sp->ty[j - ce::KNOTS] : sp->c[j - 2 * ce::KNOTS];
    const float box[4] = {sp->box[0], sp->box[1], sp->box[2], sp->box[3]};
    __syncthreads();
    const int i = blockIdx.x * CE_T + threadIdx.x;
    if (i >= n_max) return;
    if (i >= s->st.n) {
        keys[i] = ce::pad_key(0, (uint32_t)i);
        keys[(size_t)n_max + i] = ce::pad_key(1, (uint32_t)i);
        return;
    }
    const float zi = ce::density(s_t, s_t + ce::KNOTS, s_t + 2 * ce::KNOTS, box, scaled[i], scaled[(size_t)n_max + i]);
    z[i] = zi;
    keys[i] = ce::sort_key(0, ce::z_key(zi), (uint32_t)i);
    keys[(size_t)n_max + i] = ce::sort_key(1, ac::order_key(scaled[2 * (size_t)n_max + i]), (uint32_t)i);
}

__global__ __launch_bounds__(CE_T) void kce_gather_kernel(const float *__restrict__ scaled, const float *__restrict__ z, const unsigned long long *__restrict__ keys,
                                                          int n_max, kce_state *s, float *__restrict__ sx, float *__restrict__ sy, float *__restrict__ sz,
                                                          float *__restrict__ radial, unsigned *outside)
{
    const int j = blockIdx.x * CE_T + threadIdx.x, n = s->st.n;
    bool nan = false;
    if (j < n) {
        const uint32_t row = ce::key_row(keys[j]);
        const float zr = z[row];
        sx[j] = scaled[row]; sy[j] = scaled[(size_t)n_max + row]; sz[j] = zr;
        nan = ac::is_nan(zr);
        radial[j] = ac::order_value(ce::key_value(keys[(size_t)n_max + j]));
    }
    const unsigned long long nans = __ballot(nan);
    if ((threadIdx.x & 63) == 0 && nans) atomicAdd(outside, (unsigned)__popcll(nans));
}

__global__ void kce_tail_kernel(kce_state *s, const unsigned long long *radial_keys, const unsigned *outside) { kce_fill_tail(s, radial_keys, (int)*outside); }

unsigned rows_grid(int n_max) { return (unsigned)((n_max + CE_T - 1) / CE_T); }
// grid of a kernel that strides over the rows and ends with one atomic per counter: enough workgroups to fill the device, no more
unsigned strided_grid(km_ctx *c, int n_max)
{
    const unsigned all = rows_grid(n_max), want = (unsigned)c->n_cu * 4u;
    return all < want ? all : want;
}

}  // namespace

int kce_scale(km_ctx *c, const float *d_cols, int n_max, float res, float *d_scaled, kce_state *s)
{
    KM_HIP(c, hipMemsetAsync(s->ext, 0, sizeof s->ext, c->stream));
    kce_scale_kernel<<<rows_grid(n_max), CE_T, 0, c->stream>>>(d_cols, n_max, res, d_scaled, s);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kce_block(km_ctx *c, kce_state *s)
{
    kce_block_kernel<<<1, 1, 0, c->stream>>>(s);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kce_axis_hist(km_ctx *c, const float *d_scaled, int n_max, const kce_state *s, kce_axis x, kce_axis y)
{
    if (!x.bins && !y.bins) return KM_OK;
    kce_axis_hist_kernel<<<dim3(strided_grid(c, n_max), 2), CE_T, 0, c->stream>>>(d_scaled, n_max, s, x, y);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kce_grid_hist(km_ctx *c, const float *d_scaled, int n_max, const kce_state *s, const float *d_edges, unsigned *d_count)
{
    kce_grid_hist_kernel<<<strided_grid(c, n_max), CE_T, 0, c->stream>>>(d_scaled, n_max, s, d_edges, d_count);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kce_density_keys(km_ctx *c, const float *d_scaled, int n_max, const kce_state *s, const kce_spline *d_sp, float *d_z, unsigned long long *d_keys)
{
    kce_density_keys_kernel<<<rows_grid(n_max), CE_T, 0, c->stream>>>(d_scaled, n_max, s, d_sp, d_z, d_keys);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kce_sort_gather(km_ctx *c, const float *d_scaled, const float *d_z, unsigned long long *d_keys, unsigned long long *d_keys_b, int n_max, kce_state *s,
                    float *d_sx, float *d_sy, float *d_sz, float *d_radial)
{
    const int rc = km_sort_u64(c, d_keys, d_keys_b, nullptr, nullptr, 2 * (size_t)n_max, false);
    if (rc) return rc;
    unsigned *outside = (unsigned *)&s->tail.n_outside;
    KM_HIP(c, hipMemsetAsync(outside, 0, sizeof(unsigned), c->stream));
    kce_gather_kernel<<<rows_grid(n_max), CE_T, 0, c->stream>>>(d_scaled, d_z, d_keys, n_max, s, d_sx, d_sy, d_sz, d_radial, outside);
    KM_LAUNCH_CHECK(c);
    kce_tail_kernel<<<1, 1, 0, c->stream>>>(s, d_keys + n_max, outside);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
