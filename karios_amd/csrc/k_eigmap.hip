// The two-kernel fallback of the fused eigenvalue + candidate passes (k_eig2.hip, k_eig3.hip), gfx950:
//   K3  Sobel -> structure tensor -> box sum -> min eigenvalue (+ masked max): the LDS-tiled general form, any block size 1..31
//   K4  threshold + 3x3 local maxima + mask -> candidate keys
// Integer-exact sums, individually rounded float32 formulas, no MFMA.
#include "common.hpp"

// ------------------------------------------------------------------ K3 min-eigenvalue map
// Output tile 64x32.  Exact-integer Sobel products and box sums (<= 31x31 window fits int32),
// one conversion to f32, then OpenCV's calcMinEigenVal formula with every f32 op rounded
// separately.  cov's own REFLECT_101 border (boxFilter) is honoured by evaluating the Sobel
// at the reflected position, NOT by reflecting the image under the window.
#define EIG_TW 64
#define EIG_TH 32
#define EIG_SEG 16

__device__ __forceinline__ unsigned eig_key(float f)
{
    unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float eig_unkey(unsigned k)
{
    unsigned b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(b);
#else
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
#endif
}

__global__ __launch_bounds__(256) void eig_kernel(const uint8_t *__restrict__ src, const uint8_t *__restrict__ mask, int H,
                                                  int W, int block, double scale2, float *__restrict__ eig,
                                                  unsigned int *__restrict__ max_partial)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int L = block / 2, Rr = block - 1 - L;
    const int PW = EIG_TW + L + Rr, PH = EIG_TH + L + Rr;  // product region
    const int LW = (PW + 2 + 3) & ~3, LH = PH + 2;          // lap tile (1-px Sobel halo), row padded to 4
    uint8_t *lap = smem;                                    // [LH][LW]
    int *dxy = (int *)(smem + (((size_t)LH * LW + 15) & ~(size_t)15));  // [PH][PW] packed (dx | dy<<16)
    int *hsum = dxy + (size_t)PH * PW;                      // [3][PH][EIG_TW]
    const int X0 = blockIdx.x * EIG_TW, Y0 = blockIdx.y * EIG_TH;
    const int tid = threadIdx.x;
    const int lx0 = X0 - L - 1, ly0 = Y0 - L - 1;           // global coords of lap[0][0]

    for (int i = tid; i < LH * LW; i += 256) {
        const int r = i / LW, cx = i - r * LW;
        lap[i] = src[(size_t)km_reflect101(ly0 + r, H) * W + km_reflect101(lx0 + cx, W)];
    }
    __syncthreads();

    const int xlim = min(X0 + EIG_TW, W) - 1 + Rr, ylim = min(Y0 + EIG_TH, H) - 1 + Rr;
    for (int i = tid; i < PH * PW; i += 256) {
        const int r = i / PW, cx = i - r * PW;
        const int gx = X0 - L + cx, gy = Y0 - L + r;
        int packed = 0;
        if (gx <= xlim && gy <= ylim) {
            const int qx = km_reflect101(gx, W) - lx0, qy = km_reflect101(gy, H) - ly0;
            const uint8_t *p = lap + (size_t)qy * LW + qx;
            const int a00 = p[-LW - 1], a01 = p[-LW], a02 = p[-LW + 1];
            const int a10 = p[-1], a12 = p[1];
            const int a20 = p[LW - 1], a21 = p[LW], a22 = p[LW + 1];
            const int dx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
            const int dy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
            packed = (dx & 0xffff) | (dy << 16);
        }
        dxy[i] = packed;
    }
    __syncthreads();

    // horizontal box sums: one row segment of EIG_SEG outputs per work item (sliding window)
    const int nseg = EIG_TW / EIG_SEG;
    for (int it = tid; it < PH * nseg; it += 256) {
        const int r = it / nseg, sg = it - r * nseg;
        const int *row = dxy + (size_t)r * PW + sg * EIG_SEG;
        int sxx = 0, sxy = 0, syy = 0;
        for (int k = 0; k < block; k++) {
            const int v = row[k];
            const int dx = (int)(short)(v & 0xffff), dy = v >> 16;
            sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
        }
        int *o0 = hsum + (size_t)r * EIG_TW + sg * EIG_SEG;
        int *o1 = o0 + (size_t)PH * EIG_TW, *o2 = o1 + (size_t)PH * EIG_TW;
        o0[0] = sxx; o1[0] = sxy; o2[0] = syy;
        for (int x = 1; x < EIG_SEG; x++) {
            const int vo = row[x - 1], vn = row[x - 1 + block];
            const int dxo = (int)(short)(vo & 0xffff), dyo = vo >> 16;
            const int dxn = (int)(short)(vn & 0xffff), dyn = vn >> 16;
            sxx += dxn * dxn - dxo * dxo; sxy += dxn * dyn - dxo * dyo; syy += dyn * dyn - dyo * dyo;
            o0[x] = sxx; o1[x] = sxy; o2[x] = syy;
        }
    }
    __syncthreads();

    // vertical box sums + eigenvalue: thread = column x, 8 consecutive rows
    const int x = tid & 63, yc = (tid >> 6) * (EIG_TH / 4);
    const int gx = X0 + x;
    float best = -INFINITY;
    bool have = false;
    if (gx < W) {
        const int *h0 = hsum + x, *h1 = h0 + (size_t)PH * EIG_TW, *h2 = h1 + (size_t)PH * EIG_TW;
        int sa = 0, sb = 0, sc = 0;
        for (int k = 0; k < block; k++) {
            sa += h0[(size_t)(yc + k) * EIG_TW]; sb += h1[(size_t)(yc + k) * EIG_TW]; sc += h2[(size_t)(yc + k) * EIG_TW];
        }
        for (int r = 0; r < EIG_TH / 4; r++) {
            const int gy = Y0 + yc + r;
            if (gy >= H) break;
            if (r > 0) {
                const size_t o = (size_t)(yc + r - 1) * EIG_TW, n = (size_t)(yc + r - 1 + block) * EIG_TW;
                sa += h0[n] - h0[o]; sb += h1[n] - h1[o]; sc += h2[n] - h2[o];
            }
            const float cxx = (float)__dmul_rn((double)sa, scale2);
            const float cxy = (float)__dmul_rn((double)sb, scale2);
            const float cyy = (float)__dmul_rn((double)sc, scale2);
            const float a = __fmul_rn(cxx, 0.5f), b = cxy, cc = __fmul_rn(cyy, 0.5f);
            const float t = __fsub_rn(a, cc);
            const float s = __fadd_rn(__fmul_rn(t, t), __fmul_rn(b, b));
            const float e = __fsub_rn(__fadd_rn(a, cc), sqrtf(s));
            const size_t o = (size_t)gy * W + gx;
            eig[o] = e;
            if (!mask || mask[o]) { best = have ? fmaxf(best, e) : e; have = true; }
        }
    }
    unsigned key = have ? eig_key(best) : 0u;
    for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, o));
    __shared__ unsigned s_key[4];
    if ((tid & 63) == 0) s_key[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) max_partial[blockIdx.y * gridDim.x + blockIdx.x] = max(max(s_key[0], s_key[1]), max(s_key[2], s_key[3]));
}

__device__ __forceinline__ float dpp_shr1(float v)  // value of lane-1 (0 for lane 0)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_shl1(float v)  // value of lane+1 (0 for lane 63)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, false));
}

int kd_min_eigen(km_ctx *c, const uint8_t *d_src, const uint8_t *d_mask, int H, int W, int block, float *d_eig,
                 unsigned int *d_max_key)
{
    if (block < 1 || block > 31) return km_fail(c, KM_E_UNSUPPORTED, "blockSize %d (supported 1..31)", block);
    const int rc2 = k2_min_eigen(c, d_src, d_mask, H, W, block, d_eig, d_max_key);
    if (rc2 != KM_E_UNSUPPORTED) return rc2;
    const double scale = 1.0 / (4.0 * (double)block * 255.0);
    // generic LDS-tiled kernel: any block size 1..31, any image size
    const int L = block / 2, Rr = block - 1 - L;
    const int PW = EIG_TW + L + Rr, PH = EIG_TH + L + Rr, LW = (PW + 2 + 3) & ~3, LH = PH + 2;
    const size_t sm = (((size_t)LH * LW + 15) & ~(size_t)15) + (size_t)PH * PW * 4 + (size_t)3 * PH * EIG_TW * 4;
    if (sm > 160 * 1024 - 256) return km_fail(c, KM_E_UNSUPPORTED, "blockSize %d needs %zu B LDS", block, sm);
    static unsigned long long opted = 0;  // dynamic-LDS opt-in, per DEVICE (hipFuncSetAttribute applies to the current one); the kernel also holds a few static words
    if (sm > 48 * 1024 && !(opted & (1ull << (c->device & 63)))) {
        KM_HIP(c, hipFuncSetAttribute((const void *)eig_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
        opted |= 1ull << (c->device & 63);
    }
    dim3 grid((W + EIG_TW - 1) / EIG_TW, (H + EIG_TH - 1) / EIG_TH);
    unsigned *partial = (unsigned *)km_ws(c, WS_PARTIAL, (size_t)grid.x * grid.y * sizeof(unsigned));
    if (!partial) return KM_E_NOMEM;
    eig_kernel<<<grid, 256, sm, c->stream>>>(d_src, d_mask, H, W, block, scale * scale, d_eig, partial);
    KM_LAUNCH_CHECK(c);
    return kd_max_u32(c, partial, grid.x * grid.y, d_max_key);
}

// ------------------------------------------------------------------ K4 candidates
// goodFeaturesToTrack steps 4-5: thr = (float)(maxVal*q); TOZERO threshold;
// pixel is a candidate iff it is non-zero, equals the 3x3 max of the thresholded map, lies off
// the 1-px border and passes the mask.  Key = (f32 bits << 32) | raster index, so a single
// descending u64 sort reproduces greaterThanPtr (value desc, address desc).
// One wavefront marches down a 256-column strip (one float4 per lane and row), keeping the thresholded
// rows y-1, y, y+1 in registers; the 3x3 max uses the two neighbour lanes through DPP wave shifts.
// Candidates are compacted into a per-wave LDS stage and flushed with ONE global atomic per flush.
#define CAND_RS 32     // output rows per wave
#define CAND_STAGE 512 // keys per wave stage (a row step adds at most 256)

struct cand_row {
    float v[4];
    float lft, rgt;  // thresholded neighbours x-1 (lane 0 only) and x+4 (lane 63 only) from the adjacent strips
};


__global__ __launch_bounds__(256) void cand_kernel(const float *__restrict__ eig, const uint8_t *__restrict__ mask, int H, int W,
                                                   double quality, km_scalars *sc, unsigned long long *__restrict__ keys,
                                                   size_t cap, int nstrips, int gyw)
{
    __shared__ unsigned long long stage[4][CAND_STAGE];
    const unsigned mk = sc->max_eig_key;
    const float maxv = mk ? eig_unkey(mk) : 0.f;
    const float thr = (float)__dmul_rn((double)maxv, quality);
    if (blockIdx.x == 0 && threadIdx.x == 0) { sc->thr = thr; sc->max_eig = maxv; }
    const int gxw = (nstrips + 3) / 4;                  // logical grid gxw x gyw, XCD-swizzled
    unsigned tile;
    if (!km_xcd_tile((unsigned)(gxw * gyw), tile)) return;
    const int bx = (int)tile % gxw, by = (int)tile / gxw;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strip = bx * 4 + wv;
    if (strip >= nstrips) return;
    unsigned long long *st = stage[wv];
    const int x0 = strip * 256 + lane * 4;               // first of this lane's 4 columns
    const int y0 = by * CAND_RS, y1 = min(H, y0 + CAND_RS);
    const bool vec = (W % 4 == 0) && x0 + 3 < W;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;

    // raw loads are issued a group of rows ahead (load_raw), thresholding happens when the row is consumed
    auto load_raw = [&](int y, cand_row &r) {
        r.v[0] = r.v[1] = r.v[2] = r.v[3] = 0.f; r.lft = 0.f; r.rgt = 0.f;
        if (y < 0 || y >= H) return;                      // outside rows never matter (border rows are excluded)
        const float *row = eig + (size_t)y * W;
        if (vec) {
            const float4 q = *(const float4 *)(row + x0);
            r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) if (x0 + j < W) r.v[j] = row[x0 + j];
        }
        if (lane == 0 && x0 - 1 >= 0) r.lft = row[x0 - 1];
        if (lane == 63 && x0 + 4 < W) r.rgt = row[x0 + 4];
    };
    auto threshold = [&](cand_row &r) {
#pragma unroll
        for (int j = 0; j < 4; j++) r.v[j] = r.v[j] > thr ? r.v[j] : 0.f;   // THRESH_TOZERO
        r.lft = r.lft > thr ? r.lft : 0.f;
        r.rgt = r.rgt > thr ? r.rgt : 0.f;
    };

    unsigned cnt = 0;  // keys in the stage (wave-uniform)
    const int wave_id = by * (gxw * 4) + strip;
    const unsigned shard = (unsigned)wave_id % KM_NSHARD;
    const size_t cap_s = cap / KM_NSHARD;
    auto flush = [&]() {
        if (cnt == 0) return;
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&sc->shard_cnt[shard], cnt);
        base = __shfl(base, 0);
        for (unsigned i = lane; i < cnt; i += 64)
            if ((size_t)base + i < cap_s) keys[shard * cap_s + base + i] = st[i];
        cnt = 0;
    };

    constexpr int PF = 4;  // rows in flight
    cand_row up, mid, dn, pre[PF];
    uint32_t pmask[PF];    // mask bytes of the 4 pixels of row yb+k (all-ones without a mask)
    auto load_mask = [&](int y) -> uint32_t {
        if (!mask || y < 0 || y >= H) return 0x01010101u;
        const uint8_t *row = mask + (size_t)y * W;
        if (vec) return *(const uint32_t *)(row + x0);
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) if (x0 + j < W) m |= (uint32_t)row[x0 + j] << (8 * j);
        return m;
    };
    load_raw(y0 - 1, up); threshold(up);
    load_raw(y0, mid); threshold(mid);
    for (int yb = y0; yb < y1; yb += PF) {
#pragma unroll
        for (int k = 0; k < PF; k++) { load_raw(yb + k + 1, pre[k]); pmask[k] = load_mask(yb + k); }
#pragma unroll
        for (int k = 0; k < PF; k++) {
            const int y = yb + k;
            if (y >= y1) continue;
            dn = pre[k]; threshold(dn);
            if (y >= 1 && y < H - 1) {
                bool any = false;
#pragma unroll
                for (int j = 0; j < 4; j++) any = any || (mid.v[j] != 0.f);
                if (__ballot(any)) {
                    // column-wise max of the three rows, then the horizontal neighbours
                    float m3[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) m3[j] = fmaxf(fmaxf(up.v[j], mid.v[j]), dn.v[j]);
                    float mL = dpp_shr1(m3[3]), mR = dpp_shl1(m3[0]);
                    if (lane == 0) mL = fmaxf(fmaxf(up.lft, mid.lft), dn.lft);
                    if (lane == 63) mR = fmaxf(fmaxf(up.rgt, mid.rgt), dn.rgt);
                    if (cnt + 256 > CAND_STAGE) flush();
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const float left = j == 0 ? mL : m3[j - 1], right = j == 3 ? mR : m3[j + 1];
                        const float nb = fmaxf(fmaxf(left, right), fmaxf(up.v[j], dn.v[j]));
                        const float v = mid.v[j];
                        const int x = x0 + j;
                        const bool is = v != 0.f && v >= nb && x >= 1 && x < W - 1 && ((pmask[k] >> (8 * j)) & 0xffu) != 0;
                        const unsigned long long bal = __ballot(is);
                        if (is) st[cnt + __popcll(bal & lt_mask)] =
                            ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)((unsigned)y * (unsigned)W + (unsigned)x);
                        cnt += (unsigned)__popcll(bal);
                    }
                }
            }
            up = mid; mid = dn;
        }
    }
    flush();
}

int kd_candidates(km_ctx *c, const float *d_eig, const uint8_t *d_mask, int H, int W, double quality, km_scalars *d_sc,
                  unsigned long long *d_keys, size_t cap, bool rezero)
{
    if (rezero) KM_HIP(c, hipMemsetAsync(d_sc->shard_cnt, 0, KM_NSHARD * sizeof(unsigned int), c->stream));
    if (H < 3 || W < 3) {
        return KM_OK;
    }
    const int nstrips = (W + 255) / 256;
    dim3 grid((nstrips + 3) / 4, (H + CAND_RS - 1) / CAND_RS);
    cand_kernel<<<km_xcd_grid(grid.x * grid.y), 256, 0, c->stream>>>(d_eig, d_mask, H, W, quality, d_sc, d_keys, cap, nstrips, (int)grid.y);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

