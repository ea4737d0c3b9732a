// Device half of ChipService.generate_chips (karios/report/chip_service.py), see k_chips.hpp.  Every operation that decides a pick
// or a pixel is chips_math.hpp's (the selection, the windows), k_pixel.hpp's stretch_u8 or integer arithmetic.
//   kch_select   one workgroup per cell, seven strided scans of the columns: the centre by a block argmin of the lexicographic pick;
//                the quarters' sizes; a radix select of the order keys of the distances, eight bits a scan, with LDS histograms for
//                the two middle ranks of the four quarters at once (integer atomics: the counts do not depend on their order); a
//                block argmin of |distance - median| per quarter.  One thread then packs the slots in cell order.
//   kch_chips    one workgroup per (row, image): the 57 x 57 window from the raster at its own pitch into registers (13 pixels a
//                thread), the raw chip out, minimum / maximum by wave reductions (NaN skipped), stretch_u8 into LDS, the row pass of
//                both separable kernels into LDS, the column pass, saturation.  29 KB of LDS a workgroup.
#include "k_chips.hpp"
#include "k_pixel.hpp"

namespace {

constexpr int SEL_T = 256;
constexpr int SEL_W = SEL_T / 64;

__device__ __forceinline__ ch::pick wave_best(ch::pick p)
{
    for (int o = 32; o > 0; o >>= 1) {
        ch::pick q;
        q.hi = __shfl_xor(p.hi, o);
        q.row = __shfl_xor(p.row, o);
        if (ch::better(q, p)) p = q;
    }
    return p;
}
// every thread leaves with the workgroup's best pick; `tmp` holds SEL_W picks
__device__ __forceinline__ ch::pick block_best(ch::pick p, ch::pick *tmp)
{
    p = wave_best(p);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = p;
    __syncthreads();
    ch::pick best = tmp[0];
    for (int w = 1; w < SEL_W; w++)
        if (ch::better(tmp[w], best)) best = tmp[w];
    return best;
}

__global__ __launch_bounds__(SEL_T) void kch_select_kernel(const float *__restrict__ x0, const float *__restrict__ y0, const float *__restrict__ score,
                                                           int n, ch::grid g, int32_t *__restrict__ slots)
{
    __shared__ ch::pick tmp[SEL_W];
    __shared__ unsigned hist[4][2][256];       // [quarter][lower / upper middle rank][digit]
    __shared__ unsigned count[4];
    __shared__ unsigned prefix[4][2], rank[4][2];
    const int cell = blockIdx.x, tid = threadIdx.x;
    const ch::cell_box b = ch::make_box(g, cell);

    // the centre: the nearest row, then the larger score, then the first row
    ch::pick mine = ch::no_pick();
    for (int i = tid; i < n; i += SEL_T) {
        const float s = score[i], x = x0[i], y = y0[i];
        if (!ch::passes(s, g.thr) || ch::cell_of(x, y, g) != cell) continue;
        const ch::pick p = ch::make_pick(ch::dist(x, y, b), s, (uint32_t)i);
        if (ch::better(p, mine)) mine = p;
    }
    const ch::pick centre = block_best(mine, tmp);
    int32_t *slot = slots + (size_t)cell * ch::PICKS;
    if (centre.row == 0xffffffffu) {
        if (tid < ch::PICKS) slot[tid] = -1;
        return;
    }
    if (tid == 0) slot[0] = (int32_t)centre.row;

    // rows of the quarters: the cell's rows without the centre row
    if (tid < 4) count[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += SEL_T) {
        const float s = score[i], x = x0[i], y = y0[i];
        if ((uint32_t)i == centre.row || !ch::passes(s, g.thr) || ch::cell_of(x, y, g) != cell) continue;
        const unsigned qm = ch::quarters(x, y, b);
        for (int q = 0; q < 4; q++)
            if (qm >> q & 1u) atomicAdd(&count[q], 1u);
    }
    __syncthreads();
    if (tid < 8) {
        const int q = tid >> 1, t = tid & 1;
        const unsigned m = count[q];
        prefix[q][t] = 0;
        rank[q][t] = m ? (t ? m / 2 : (m - 1) / 2) : 0;
    }
    // radix select of the two middle order statistics of every quarter's distances
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int k = tid; k < 4 * 2 * 256; k += SEL_T) (&hist[0][0][0])[k] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += SEL_T) {
            const float s = score[i], x = x0[i], y = y0[i];
            if ((uint32_t)i == centre.row || !ch::passes(s, g.thr) || ch::cell_of(x, y, g) != cell) continue;
            const unsigned qm = ch::quarters(x, y, b);
            if (!qm) continue;
            const uint32_t key = ac::order_key(ch::dist(x, y, b));
            const uint32_t head = (uint32_t)((unsigned long long)key >> (shift + 8));
            for (int q = 0; q < 4; q++) {
                if (!(qm >> q & 1u)) continue;
                for (int t = 0; t < 2; t++)
                    if (head == prefix[q][t]) atomicAdd(&hist[q][t][(key >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        if (tid < 8) {
            const int q = tid >> 1, t = tid & 1;
            if (count[q]) {
                unsigned r = rank[q][t], d = 0;
                while (d < 255 && r >= hist[q][t][d]) { r -= hist[q][t][d]; d++; }
                rank[q][t] = r;
                prefix[q][t] = (prefix[q][t] << 8) | d;
            }
        }
        __syncthreads();
    }
    float med[4];
    for (int q = 0; q < 4; q++) med[q] = count[q] ? ch::median_of(prefix[q][0], prefix[q][1], (int)count[q]) : 0.0f;

    // the quarters' picks: the distance nearest to the median
    ch::pick best[4];
    for (int q = 0; q < 4; q++) best[q] = ch::no_pick();
    for (int i = tid; i < n; i += SEL_T) {
        const float s = score[i], x = x0[i], y = y0[i];
        if ((uint32_t)i == centre.row || !ch::passes(s, g.thr) || ch::cell_of(x, y, g) != cell) continue;
        const unsigned qm = ch::quarters(x, y, b);
        if (!qm) continue;
        const float d = ch::dist(x, y, b);
        for (int q = 0; q < 4; q++) {
            if (!(qm >> q & 1u)) continue;
            const ch::pick p = ch::make_pick(ch::dev(d, med[q]), s, (uint32_t)i);
            if (ch::better(p, best[q])) best[q] = p;
        }
    }
    for (int q = 0; q < 4; q++) {
        const ch::pick p = block_best(best[q], tmp);
        if (tid == 0) slot[1 + q] = count[q] ? (int32_t)p.row : -1;
    }
}

__global__ void kch_pack_kernel(const int32_t *__restrict__ slots, int n_slots, int32_t *__restrict__ index, int32_t *__restrict__ count)
{
    if (blockIdx.x || threadIdx.x) return;
    int m = 0;
    for (int k = 0; k < n_slots; k++)
        if (slots[k] >= 0) index[m++] = slots[k];
    *count = m;
}

// ---- chips
constexpr int CHIP_T = 256;
constexpr int CHIP_PER = (ch::PIXELS + CHIP_T - 1) / CHIP_T;      // 13 pixels a thread

struct kch_chip_args {
    kch_images I;
    kch_rows R;
    kch_taps taps;
    int lap[2];
    km_chip_outputs out;
};

template <typename T>
__global__ __launch_bounds__(CHIP_T) void kch_chips_kernel(kch_chip_args A)
{
    __shared__ uint8_t u8s[ch::PIXELS + 3];
    __shared__ int hd[ch::PIXELS], hs[ch::PIXELS];
    __shared__ double red[2][CHIP_T / 64];
    const int row = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const ch::window w = ch::make_window(A.R.x0[row], A.R.y0[row], A.R.dx[row], A.R.dy[row], A.I.Href, A.I.Wref, A.I.Hmon, A.I.Wmon);
    if (img == 0 && tid == 0) {
        A.out.ok[row] = (uint8_t)w.ok;
        int32_t *win = A.out.windows + 4 * (size_t)row;
        win[0] = w.X0; win[1] = w.Y0; win[2] = w.X1; win[3] = w.Y1;
    }
    const size_t at = (size_t)row * ch::PIXELS;
    T *raw = (T *)(img ? A.out.mon_raw : A.out.ref_raw) + at;
    uint8_t *u8 = (img ? A.out.mon_u8 : A.out.ref_u8) + at;
    uint8_t *lap = A.lap[img] ? (img ? A.out.mon_lap : A.out.ref_lap) + at : nullptr;
    if (!w.ok) {
        for (int p = tid; p < ch::PIXELS; p += CHIP_T) {
            raw[p] = (T)0; u8[p] = 0;
            if (lap) lap[p] = 0;
        }
        return;
    }
    const int X = img ? w.X1 : w.X0, Y = img ? w.Y1 : w.Y0;
    const ptrdiff_t stride = img ? A.I.smon : A.I.sref;
    const T *src = (const T *)(img ? A.I.mon : A.I.ref) + (ptrdiff_t)(Y - ch::MARGIN) * stride + (X - ch::MARGIN);
    T v[CHIP_PER];
    double mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < CHIP_PER; k++) {
        const int p = tid + k * CHIP_T;
        v[k] = (T)0;
        if (p < ch::PIXELS) {
            const int y = p / ch::CHIP, x = p - y * ch::CHIP;
            v[k] = src[(ptrdiff_t)y * stride + x];
            raw[p] = v[k];
            const double d = (double)v[k];
            if (d == d) { mn = fmin(mn, d); mx = fmax(mx, d); }
        }
    }
    mn = wave_min(mn); mx = wave_max(mx);
    if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; }
    __syncthreads();
    for (int k = 0; k < CHIP_T / 64; k++) { mn = fmin(mn, red[0][k]); mx = fmax(mx, red[1][k]); }
    const bool degenerate = !(mx > mn);
    const double range = mx - mn;
#pragma unroll
    for (int k = 0; k < CHIP_PER; k++) {
        const int p = tid + k * CHIP_T;
        if (p < ch::PIXELS) {
            const uint8_t u = (uint8_t)stretch_u8<T>(v[k], mn, range, degenerate);
            u8s[p] = u; u8[p] = u;
        }
    }
    if (!lap) return;
    __syncthreads();
    const int R = A.taps.R[img];
    const int *kd = A.taps.cf.kd[img], *ks = A.taps.cf.ks[img];
    for (int p = tid; p < ch::PIXELS; p += CHIP_T) {
        const int y = p / ch::CHIP, x = p - y * ch::CHIP;
        int d = 0, s = 0;
        for (int j = 0; j <= 2 * R; j++) {
            const int px = u8s[y * ch::CHIP + ch::reflect(x + j - R)];
            d += kd[j] * px; s += ks[j] * px;
        }
        hd[p] = d; hs[p] = s;
    }
    __syncthreads();
    for (int p = tid; p < ch::PIXELS; p += CHIP_T) {
        const int y = p / ch::CHIP, x = p - y * ch::CHIP;
        int acc = 0;
        for (int j = 0; j <= 2 * R; j++) {
            const int q = ch::reflect(y + j - R) * ch::CHIP + x;
            acc += ks[j] * hd[q] + kd[j] * hs[q];
        }
        lap[p] = (uint8_t)min(max(acc, 0), 255);
    }
}

}  // namespace

int kch_select(km_ctx *c, const float *d_x0, const float *d_y0, const float *d_score, int n, const ch::grid &g, int32_t *d_slots, int32_t *d_index,
               int32_t *d_count)
{
    kch_select_kernel<<<(unsigned)(g.rows * g.cols), SEL_T, 0, c->stream>>>(d_x0, d_y0, d_score, n, g, d_slots);
    KM_LAUNCH_CHECK(c);
    kch_pack_kernel<<<1, 1, 0, c->stream>>>(d_slots, (int)kch_slots(g), d_index, d_count);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kch_chips(km_ctx *c, const kch_images &I, const kch_rows &R, int ksize_ref, int ksize_mon, const km_chip_outputs &out)
{
    kch_chip_args A;
    A.I = I; A.R = R; A.out = out;
    A.lap[0] = ksize_ref != 0; A.lap[1] = ksize_mon != 0;
    if (!kch_make_taps(ksize_ref, ksize_mon, A.taps)) return km_fail(c, KM_E_ARG, "chips: Laplacian ksize ref=%d mon=%d (0, 1, 3, 5, 7, 9, 11)", ksize_ref, ksize_mon);
    if (R.n <= 0) return KM_OK;
    return km_with_pixel_type(c, I.dtype, "chips: bad dtype %d", [&](auto t) {
        kch_chips_kernel<decltype(t)><<<dim3((unsigned)R.n, 2), CHIP_T, 0, c->stream>>>(A);
        KM_LAUNCH_CHECK(c);
        return (int)KM_OK;
    });
}
