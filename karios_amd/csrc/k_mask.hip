// Vector masks on the device (karios/core/image.py:104-191, karios/api/core.py:593-612); tests/rasterize_restatement.py is the
// definition, mask_math.hpp the arithmetic.
//
// Fill: a work item is a band of KMK_BAND rows by a strip of at most KMK_STRIP columns, for ALL features, so that every output byte of
// the window is stored exactly once, zeros included: no memset, no read-modify-write of global memory.  Per feature whose row range
// meets the band, its edges pass through LDS in chunks of 32-byte records; the lanes stride over (row, edge) and toggle, with an LDS
// atomic XOR, the bit of the rounded crossing in the row's bitmap - clamped to the strip's first bit on the left, dropped beyond its
// last column.  The pairs rule of the definition burns pixel x iff the number of crossings <= x is odd (proof there), so the row's
// fill is the prefix parity of that bitmap: inside a word by shifts, across words by a ballot of the words' parities, one wavefront
// per row.  It is ORed into the row's accumulator; the spans of horizontal edges on a centre line go into the accumulator directly
// (LDS atomic OR).  After the last feature the accumulator's bits become bytes: 16-byte stores on the 16-byte grid of the output row,
// bytes for the head and the tail - rows have any stride, W is a multiple of nothing.
//
// Lines: stream-ordered behind the fill, one lane per edge.  The two axis-parallel cases are clamped ranges, stored by the wavefront
// together; the general case is a sequential walk by definition (x and y accumulate rounding: a segment cannot be split bit-exactly)
// under a hard cap of steps.  Every writer stores the same byte 1 with plain byte stores.
//
// AND: 16 pixels per lane where the three rows allow 16-byte accesses there, bytes elsewhere; the three counts per wavefront, one
// atomic each.
#include "k_mask.hpp"

#include "common.hpp"

#include <algorithm>

namespace {

constexpr int kT = 256;
constexpr int KMK_BAND = 8;
constexpr int KMK_STRIP = 16384;

__device__ __forceinline__ unsigned expand4(unsigned b)     // bits 0 .. 3 -> four bytes of 0 / 1
{
    return (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21);
}

__global__ __launch_bounds__(kT) void mask_fill_kernel(kmk_polygons p, int chunk, int words, unsigned nstrips, unsigned long long ntiles)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    mk::edge *s_edge = reinterpret_cast<mk::edge *>(lds);
    unsigned *acc = reinterpret_cast<unsigned *>(lds + (size_t)chunk * sizeof(mk::edge));      // KMK_BAND rows of `words`
    unsigned *cur = acc + KMK_BAND * words;                                                    // the same for the feature at hand
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (unsigned long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned strip = (unsigned)(tile % nstrips);
        const long long r0 = (long long)(tile / nstrips) * KMK_BAND, c0 = (long long)strip * KMK_STRIP;
        const int rows = (int)std::min<long long>(KMK_BAND, p.H - r0), width = (int)std::min<long long>(KMK_STRIP, p.W - c0);
        for (int i = tid; i < 2 * KMK_BAND * words; i += kT) acc[i] = 0u;
        __syncthreads();

        for (int f = 0; f < p.n_features; f++) {
            const kmk_feature F = p.features[f];                          // (uniform: every branch on it is the workgroup's)
            if (F.miny > F.maxy || F.maxy < r0 || F.miny >= r0 + rows) continue;
            const int ya = (int)std::max<long long>(F.miny, r0), yb = (int)std::min<long long>(F.maxy, r0 + rows - 1), nrow = yb - ya + 1;
            const int base = (int)(ya - r0);
            for (int e0 = F.e0; e0 < F.e1; e0 += chunk) {
                const int n = std::min(chunk, F.e1 - e0);
                for (int i = tid; i < n; i += kT) s_edge[i] = p.edges[e0 + i];
                __syncthreads();
                for (int t = tid; t < n * nrow; t += kT) {
                    const int r = t / n, e = t - r * n;
                    int a, b;
                    const int kind = mk::crossing(s_edge[e], (double)(ya + r) + 0.5, a, b);
                    if (kind == mk::CROSS) {
                        long long v = (long long)a - c0;
                        if (v < width) {
                            if (v < 0) v = 0;
                            atomicXor(&cur[(base + r) * words + (int)(v >> 5)], 1u << (v & 31));
                        }
                    } else if (kind == mk::SPAN) {
                        const long long first = std::max<long long>((long long)a - c0, 0), last = std::min<long long>((long long)b - c0, width - 1);
                        for (long long w = first >> 5; first <= last && w <= (last >> 5); w++) {
                            unsigned m = 0xFFFFFFFFu;
                            if (w == (first >> 5)) m &= 0xFFFFFFFFu << (first & 31);
                            if (w == (last >> 5)) m &= 0xFFFFFFFFu >> (31 - (last & 31));
                            atomicOr(&acc[(base + r) * words + (int)w], m);
                        }
                    }
                }
                __syncthreads();
            }
            // prefix parity of the feature's rows into the accumulator; the feature's bitmap back to zero
            for (int r = wave; r < nrow; r += kT / 64) {
                unsigned *crow = cur + (base + r) * words, *arow = acc + (base + r) * words;
                unsigned carry = 0;
                for (int w0 = 0; w0 < words; w0 += 64) {
                    const int w = w0 + lane;
                    unsigned v = w < words ? crow[w] : 0u;
                    v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16;       // bit i: parity of the word's bits 0 .. i
                    const unsigned long long odd = __ballot((int)(v >> 31));
                    if ((carry ^ (unsigned)__popcll(odd & ((1ull << lane) - 1ull))) & 1u) v = ~v;
                    if (w < words) { arow[w] |= v; crow[w] = 0u; }
                    carry ^= (unsigned)__popcll(odd) & 1u;
                }
            }
            __syncthreads();
        }

        // bits -> bytes.  Bits at and beyond `width` of a row's last word hold prefix residue: they are never read as pixels
        for (int r = 0; r < rows; r++) {
            uint8_t *dst = p.out + (ptrdiff_t)(r0 + r) * p.stride + (ptrdiff_t)c0;
            const unsigned *arow = acc + r * words;
            int head = (int)(-(uintptr_t)dst & 15u);
            if (head > width) head = width;
            const int nvec = (width - head) >> 4, tail0 = head + (nvec << 4);
            for (int v = tid; v < nvec; v += kT) {
                const int bit = head + (v << 4), w = bit >> 5, sh = bit & 31;
                unsigned bits = arow[w] >> sh;
                if (sh > 16) bits |= arow[w + 1] << (32 - sh);            // (w + 1 < words: 16 pixels start at `bit`)
                reinterpret_cast<uint4 *>(dst + head)[v] = make_uint4(expand4(bits), expand4(bits >> 4), expand4(bits >> 8), expand4(bits >> 12));
            }
            if (tid < head) dst[tid] = (uint8_t)((arow[tid >> 5] >> (tid & 31)) & 1u);
            const int t = tail0 + tid;
            if (t < width) dst[t] = (uint8_t)((arow[t >> 5] >> (t & 31)) & 1u);      // (fewer than 16 of them)
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void mask_lines_kernel(kmk_polygons p, int32_t *__restrict__ flag)
{
    const int lane = threadIdx.x;
    const long long e = (long long)blockIdx.x * 64 + lane;
    mk::line_plan L;
    L.kind = mk::L_SKIP; L.fixed = L.lo = L.hi = 0;
    if (e < p.n_edges) mk::plan_line(p.edges[e], p.H, p.W, L);
    unsigned long long ranges = __ballot(L.kind == mk::L_COLUMN || L.kind == mk::L_ROW);
    while (ranges) {                                 // (wave-uniform: one range after the other, all lanes store)
        const int src = __ffsll((long long)ranges) - 1;
        ranges &= ranges - 1;
        const int kind = __shfl(L.kind, src), fixed = __shfl(L.fixed, src), hi = __shfl(L.hi, src);
        const long long lo = __shfl(L.lo, src);
        if (kind == mk::L_COLUMN)
            for (long long y = lo + lane; y <= hi; y += 64) p.out[(ptrdiff_t)y * p.stride + fixed] = 1;
        else
            for (long long x = lo + lane; x <= hi; x += 64) p.out[(ptrdiff_t)fixed * p.stride + (ptrdiff_t)x] = 1;
    }
    if (L.kind != mk::L_WALK) return;
    const long long cap = mk::walk_cap(p.H, p.W);
    long long steps = 0;
    int ix, iy;
    bool burn;
    while (mk::walk_step(L, p.H, p.W, ix, iy, burn)) {
        if (++steps > cap) { atomicOr(flag, 1); break; }
        if (burn) p.out[(ptrdiff_t)iy * p.stride + ix] = 1;
    }
}

__device__ __forceinline__ unsigned nonzero_bytes(unsigned w)     // 0x01 in every byte of w that is not zero
{
    return ((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u) >> 7;
}

__global__ __launch_bounds__(kT) void mask_and_kernel(const uint8_t *__restrict__ a, ptrdiff_t sa, const uint8_t *__restrict__ b, ptrdiff_t sb, int H, int W,
                                                     uint8_t *__restrict__ out, ptrdiff_t so, unsigned long long *__restrict__ counts, unsigned per_row,
                                                     unsigned long long items)
{
    unsigned na = 0, nb = 0, nab = 0;
    for (unsigned long long item = (unsigned long long)blockIdx.x * kT + threadIdx.x; item < items; item += (unsigned long long)gridDim.x * kT) {
        const ptrdiff_t y = (ptrdiff_t)(item / per_row), x0 = (ptrdiff_t)(item % per_row) * 16;
        const int n = (int)std::min<ptrdiff_t>(16, W - x0);
        const uint8_t *pa = a + y * sa + x0, *pb = b + y * sb + x0;
        uint8_t *po = out + y * so + x0;
        if (n == 16 && (((uintptr_t)pa | (uintptr_t)pb | (uintptr_t)po) & 15u) == 0) {
            const uint4 va = *reinterpret_cast<const uint4 *>(pa), vb = *reinterpret_cast<const uint4 *>(pb);
            const unsigned wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
            unsigned wo[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned za = nonzero_bytes(wa[k]), zb = nonzero_bytes(wb[k]);
                wo[k] = za & zb;
                na += __popc(za); nb += __popc(zb); nab += __popc(wo[k]);
            }
            *reinterpret_cast<uint4 *>(po) = make_uint4(wo[0], wo[1], wo[2], wo[3]);
        } else {
            for (int k = 0; k < n; k++) {
                const unsigned za = pa[k] > 0, zb = pb[k] > 0;
                po[k] = (uint8_t)(za & zb);
                na += za; nb += zb; nab += za & zb;
            }
        }
    }
    // (a lane holds at most 16 pixels per item and fewer than 2^28 items: the 32-bit sums of a wavefront cannot wrap below 2^32 pixels)
    unsigned long long s[3] = {na, nb, nab};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
        if ((threadIdx.x & 63) == 0 && s[k]) atomicAdd(&counts[k], s[k]);
    }
}

}  // namespace

int kmk_fill(km_ctx *c, const kmk_polygons &p, int edge_chunk)
{
    const int chunk = edge_chunk >= 1 && edge_chunk <= KMK_EDGE_CHUNK ? edge_chunk : KMK_EDGE_CHUNK;
    const int words = (std::min(p.W, KMK_STRIP) + 31) / 32;
    const unsigned nstrips = (unsigned)(((long long)p.W + KMK_STRIP - 1) / KMK_STRIP);
    const unsigned long long ntiles = (unsigned long long)(((long long)p.H + KMK_BAND - 1) / KMK_BAND) * nstrips;
    const size_t lds = (size_t)chunk * sizeof(mk::edge) + (size_t)2 * KMK_BAND * words * sizeof(unsigned);      // at most 28 + 32 KiB
    mask_fill_kernel<<<(unsigned)std::min<unsigned long long>(ntiles, 1ull << 16), kT, lds, c->stream>>>(p, chunk, words, nstrips, ntiles);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kmk_lines(km_ctx *c, const kmk_polygons &p, int32_t *d_flag)
{
    if (p.n_edges == 0) return KM_OK;
    mask_lines_kernel<<<(unsigned)((p.n_edges + 63) / 64), 64, 0, c->stream>>>(p, d_flag);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

int kmk_mask_and(km_ctx *c, const uint8_t *d_a, ptrdiff_t sa, const uint8_t *d_b, ptrdiff_t sb, int H, int W, uint8_t *d_out, ptrdiff_t so,
                 unsigned long long *d_counts)
{
    KM_HIP(c, hipMemsetAsync(d_counts, 0, 3 * sizeof(unsigned long long), c->stream));
    const unsigned per_row = (unsigned)(((long long)W + 15) / 16);
    const unsigned long long items = (unsigned long long)per_row * (unsigned long long)H;
    const unsigned blocks = (unsigned)std::min<unsigned long long>((items + kT - 1) / kT, (unsigned long long)c->n_cu * 16);
    mask_and_kernel<<<blocks, kT, 0, c->stream>>>(d_a, sa, d_b, sb, H, W, d_out, so, d_counts, per_row, items);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
