// K7: pyramidal Lucas-Kanade tracker, forward and backward pass fused
// (cv2.calcOpticalFlowPyrLK x2, reference klt.py:134-140; algorithm SURVEY App. A.3).
//
// One 64-lane wavefront per keypoint.  Per pyramid level the (w+3)^2 neighbourhood of the
// template image is staged in LDS, the Scharr derivative is evaluated there (no dense
// derivative image is ever written to HBM), and every lane keeps its <= NPL window pixels
// (Q5 intensity, Ix, Iy) in registers for all iterations.  The normal matrix and mismatch
// vector are exact integer sums (per-lane int32, wave-reduced in int64) converted once to
// f32, so the result does not depend on the reduction order; all f32 steps of the 2x2
// solve are rounded individually (this file is compiled with -ffp-contract=off).
// The backward pass starts from the forward result of the same keypoint, so both passes run
// back to back in the same wavefront.
// This file: the FIRST form (any pyramid, row bands), kl_track - which chooses the form - and the oscillation probe.  The second form
// (two-level pyramids, whole levels: the default path) is k_lk2.hip; what both are made of, lk_device.hpp; the launch rules, lk_launch.hpp.
#include "lk_launch.hpp"

#define LK_M 3  // margin (px) of the cached search-image patch around the current window
#define LK_WPB 1   // key points (= wavefronts) per workgroup (4 measured slower: 0.363 vs 0.328 ms - a workgroup only retires with its slowest wave)

// Track one point from image pyramid I to J (all lanes hold identical scalars); run_desc: lk_run_desc, lk_device.hpp.
template <int NR>
__device__ void lk_track_point(const km_pyr &I, const km_pyr &J, float px, float py, int win, int max_count, double epsilon,
                               const int (&run_desc)[NR], uint8_t *raw, short *derx, uint8_t *jp, float &outx, float &outy, bool &left_band)
{
    const int lane = threadIdx.x & 63;
    const float half = (float)(win - 1) * 0.5f;
    const float FLT_SCALE = 1.f / (1 << 20);
    const int RW = win + 3, DW = win + 1;
    short *dery = derx + DW * DW + 8;                 // second derivative plane (8 shorts of slack behind each plane)
    const int RP = (RW + 3 + 3) & ~3;                 // raw patch pitch
    const int JS = win + 1 + 2 * LK_M, JP = (JS + 3 + 3) & ~3;
    float resx = px, resy = py;
    for (int level = I.levels; level >= 0; level--) {
        const uint8_t *Iimg = I.img[level], *Jimg = J.img[level];
        const int IW = I.W[level], IH = I.H[level], JW = J.W[level], JH = J.H[level];
        const float sc = (float)(1. / (1 << level));
        float prx = px * sc, pry = py * sc;
        float nx, ny;
        if (level == I.levels) { nx = prx; ny = pry; }
        else { nx = resx * 2.f; ny = resy * 2.f; }
        resx = nx; resy = ny;
        prx -= half; pry -= half;
        const int ipx = (int)floorf(prx), ipy = (int)floorf(pry);
        if (ipx < -win || ipx >= IW || ipy < -win || ipy >= IH) continue;
        float a = prx - (float)ipx, b = pry - (float)ipy;
        int w00, w01, w10, w11;
        lk_weights(a, b, w00, w01, w10, w11);

        // stage the template neighbourhood and (speculatively) the search neighbourhood around the start position
        LK_WAVE_SYNC();
        int jx0 = (int)floorf(nx - half) - LK_M, jy0 = (int)floorf(ny - half) - LK_M;
        if (!lk_rows_resident(I, level, ipy - 1, RW) || !lk_rows_resident(J, level, jy0, JS)) { left_band = true; break; }
        {
            constexpr int MAXIT = 2 * NR;                 // covers (win + 7)^2 / 4 words for every winSize served by NR runs per lane
            const bool in_i = lk_patch_inside(IW, IH, ipx - 1, ipy - 1, RW, RW, MAXIT), in_j = lk_patch_inside(JW, JH, jx0, jy0, JS, JS, MAXIT);
            if (in_i && in_j) {                           // template and search patch travel together
                lk_patch_regs<MAXIT> ri, rj;
                stage_patch_issue<MAXIT>(Iimg, IW, ipx - 1, ipy - 1, RW, RW, ri);
                stage_patch_issue<MAXIT>(Jimg, JW, jx0, jy0, JS, JS, rj);
                stage_patch_commit<MAXIT>(RW, RW, raw, RP, ri);
                stage_patch_commit<MAXIT>(JS, JS, jp, JP, rj);
            } else {
                stage_patch<MAXIT>(Iimg, IW, IH, ipx - 1, ipy - 1, RW, RW, raw, RP);
                stage_patch<MAXIT>(Jimg, JW, JH, jx0, jy0, JS, JS, jp, JP);
            }
        }
        LK_WAVE_SYNC();
        // Scharr derivative on the (w+1)^2 bilinear support; zero outside the image.  Four adjacent positions per lane
        // and step share their 3x6 neighbourhood (column sums s = 3*(a0+a2)+10*a1 and d = a2-a0 per column).
        {
            const int ngrp = (DW + 3) >> 2;
            const unsigned inv_ngrp = 65536u / (unsigned)ngrp + 1u;   // exact quotient for i < 1024, ngrp <= 16
            for (int i = lane; i < DW * ngrp; i += 64) {
                const int r = (int)(((unsigned)i * inv_ngrp) >> 16), g = i - r * ngrp;
                const int cx0 = 4 * g;
                const uint8_t *p = raw + (r + 1) * RP + cx0;      // column cx0-1 of the centre row is p[0]
                int sv[6], dv[6];
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    const int a0 = p[k - RP], a1 = p[k], a2 = p[k + RP];
                    sv[k] = (a0 + a2) * 3 + a1 * 10;   // vertical smoothing  [3 10 3]
                    dv[k] = a2 - a0;                   // vertical difference [-1 0 1]
                }
                const int gy = ipy + r;
                const bool row_in = (unsigned)gy < (unsigned)IH;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int cx = cx0 + k;
                    if (cx < DW) {
                        int ix = 0, iy = 0;
                        if (row_in && (unsigned)(ipx + cx) < (unsigned)IW) {
                            ix = sv[k + 2] - sv[k];
                            iy = (dv[k] + dv[k + 2]) * 3 + dv[k + 1] * 10;
                        }
                        derx[r * DW + cx] = (short)ix;      // two 16-bit planes: a run reads its 6 consecutive values per
                        dery[r * DW + cx] = (short)iy;      // row with one (unaligned) 16-byte LDS read
                    }
                }
            }
        }
        LK_WAVE_SYNC();
        // per-lane window pixels -> registers (16-bit pairs along the run: Q5 intensity, Ix, Iy); exact integer normal matrix
        uint32_t IvP[NR][3], IxP[NR][3], IyP[NR][3];
        int sA11 = 0, sA12 = 0, sA22 = 0;  // per-lane partial sums stay below 2^31 (<= 25 pixels per lane: 25 * 4080^2 = 4.2e8)
        {
            const lk_s2 wt0 = lk_as_s2(lk_pack16(w00, w01)), wt1 = lk_as_s2(lk_pack16(w10, w11));   // signed: w11 may be -1
#pragma unroll
            for (int t = 0; t < NR; t++) {
                int rd = run_desc[t];
                asm volatile("" : "+v"(rd));   // opaque: the LDS addresses of the run are recomputed here instead of living in registers across the kernel
                const int y = rd & 0xff, x0 = (rd >> 8) & 0xff, n = rd >> 16;
                // template intensity (Q5): bytes x0+1 .. x0+6 of raw rows y+1, y+2
                const uint8_t *pr = raw + (y + 1) * RP + (x0 + 1);
                uint2 r0, r1;
                __builtin_memcpy(&r0, pr, 8);
                __builtin_memcpy(&r1, pr + RP, 8);
                // derivatives: values x0 .. x0+5 of rows y, y+1 of both planes
                uint4 gx0, gx1, gy0, gy1;
                __builtin_memcpy(&gx0, derx + y * DW + x0, 16);
                __builtin_memcpy(&gx1, derx + (y + 1) * DW + x0, 16);
                __builtin_memcpy(&gy0, dery + y * DW + x0, 16);
                __builtin_memcpy(&gy1, dery + (y + 1) * DW + x0, 16);
                const uint32_t ax0[4] = {gx0.x, gx0.y, gx0.z, gx0.w}, ax1[4] = {gx1.x, gx1.y, gx1.z, gx1.w};
                const uint32_t ay0[4] = {gy0.x, gy0.y, gy0.z, gy0.w}, ay1[4] = {gy1.x, gy1.y, gy1.z, gy1.w};
                int iv[LK_RUN + 1], ixv[LK_RUN + 1], iyv[LK_RUN + 1];
                iv[LK_RUN] = 0; ixv[LK_RUN] = 0; iyv[LK_RUN] = 0;
#pragma unroll
                for (int k = 0; k < LK_RUN; k++) {
                    const uint32_t sel = 0x0c000c00u | (uint32_t)k | ((uint32_t)(k + 1) << 16);
                    const lk_s2 c0 = lk_as_s2(__builtin_amdgcn_perm(r0.y, r0.x, sel)), c1 = lk_as_s2(__builtin_amdgcn_perm(r1.y, r1.x, sel));
                    iv[k] = __builtin_amdgcn_sdot2(c0, wt0, __builtin_amdgcn_sdot2(c1, wt1, 1 << (14 - 5 - 1), false), false) >> (14 - 5);
                    // 16-bit pair (value k, value k+1) of a row held as 4 dwords
                    auto pair = [&](const uint32_t (&a)[4]) -> lk_s2 {
                        return lk_as_s2((k & 1) ? __builtin_amdgcn_alignbyte(a[(k + 1) / 2], a[k / 2], 2) : a[k / 2]);
                    };
                    ixv[k] = __builtin_amdgcn_sdot2(pair(ax0), wt0, __builtin_amdgcn_sdot2(pair(ax1), wt1, 1 << 13, false), false) >> 14;
                    iyv[k] = __builtin_amdgcn_sdot2(pair(ay0), wt0, __builtin_amdgcn_sdot2(pair(ay1), wt1, 1 << 13, false), false) >> 14;
                }
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    // pixels beyond the run's length (window edge, surplus lanes) contribute nothing
                    const uint32_t pm = n >= 2 * q + 2 ? 0xffffffffu : (n == 2 * q + 1 ? 0x0000ffffu : 0u);
                    IvP[t][q] = lk_pack16(iv[2 * q], iv[2 * q + 1]) & pm;
                    IxP[t][q] = lk_pack16(ixv[2 * q], ixv[2 * q + 1]) & pm;
                    IyP[t][q] = lk_pack16(iyv[2 * q], iyv[2 * q + 1]) & pm;
                    sA11 = __builtin_amdgcn_sdot2(lk_as_s2(IxP[t][q]), lk_as_s2(IxP[t][q]), sA11, false);
                    sA12 = __builtin_amdgcn_sdot2(lk_as_s2(IxP[t][q]), lk_as_s2(IyP[t][q]), sA12, false);
                    sA22 = __builtin_amdgcn_sdot2(lk_as_s2(IyP[t][q]), lk_as_s2(IyP[t][q]), sA22, false);
                }
            }
        }
        const long long iA11 = wave_sum_split(sA11), iA12 = wave_sum_split(sA12), iA22 = wave_sum_split(sA22);
        const float A11 = (float)iA11 * FLT_SCALE, A12 = (float)iA12 * FLT_SCALE, A22 = (float)iA22 * FLT_SCALE;
        float D = A11 * A22 - A12 * A12;
        const float dA = A11 - A22;
        const float q = dA * dA + 4.f * A12 * A12;
        const float minEig = (A22 + A11 - sqrtf(q)) / (float)(2 * win * win);
        if (minEig < 1e-4f || D < FLT_EPSILON) continue;
        D = 1.f / D;
        nx -= half; ny -= half;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < max_count; j++) {
            const int inx = (int)floorf(nx), iny = (int)floorf(ny);
            if (inx < -win || inx >= JW || iny < -win || iny >= JH) break;
            if (inx < jx0 || iny < jy0 || inx > jx0 + 2 * LK_M || iny > jy0 + 2 * LK_M) {
                // the window left the cached neighbourhood: re-centre it
                LK_WAVE_SYNC();
                jx0 = inx - LK_M; jy0 = iny - LK_M;
                if (!lk_rows_resident(J, level, jy0, JS)) { left_band = true; break; }
                stage_patch<2 * NR>(Jimg, JW, JH, jx0, jy0, JS, JS, jp, JP);
                LK_WAVE_SYNC();
            }
            a = nx - (float)inx; b = ny - (float)iny;
            lk_weights(a, b, w00, w01, w10, w11);
            const lk_s2 wr0 = lk_as_s2(lk_pack16(w00, w01)), wr1 = lk_as_s2(lk_pack16(w10, w11));   // signed: w11 may be -1
            const uint8_t *jb = jp + (iny - jy0) * JP + (inx - jx0);
            int sb1 = 0, sb2 = 0;
#pragma unroll
            for (int t = 0; t < NR; t++) {
                const int y = run_desc[t] & 0xff, x0 = (run_desc[t] >> 8) & 0xff;
                const uint8_t *p0 = jb + y * JP + x0;
                const unsigned jsh = lk_lds_shift(p0);
                const uint2 r0 = lk_lds_read8(p0, jsh), r1 = lk_lds_read8(p0 + JP, jsh);   // bytes x0 .. x0+7 of the two patch rows
                int val[LK_RUN + 1];
                val[LK_RUN] = 0;
#pragma unroll
                for (int k = 0; k < LK_RUN; k++) {
                    const uint32_t sel = 0x0c000c00u | (uint32_t)k | ((uint32_t)(k + 1) << 16);   // (byte k, byte k+1) as 16-bit values
                    const lk_s2 c0 = lk_as_s2(__builtin_amdgcn_perm(r0.y, r0.x, sel)), c1 = lk_as_s2(__builtin_amdgcn_perm(r1.y, r1.x, sel));
                    val[k] = __builtin_amdgcn_sdot2(c0, wr0, __builtin_amdgcn_sdot2(c1, wr1, 1 << (14 - 5 - 1), false), false) >> (14 - 5);
                }
#pragma unroll
                for (int q2 = 0; q2 < 3; q2++) {
                    const lk_s2 diff = lk_as_s2(lk_pack16(val[2 * q2], val[2 * q2 + 1])) - lk_as_s2(IvP[t][q2]);
                    sb1 = __builtin_amdgcn_sdot2(diff, lk_as_s2(IxP[t][q2]), sb1, false);
                    sb2 = __builtin_amdgcn_sdot2(diff, lk_as_s2(IyP[t][q2]), sb2, false);
                }
            }
            const long long ib1 = wave_sum_split(sb1), ib2 = wave_sum_split(sb2);
            const float b1 = (float)ib1 * FLT_SCALE, b2 = (float)ib2 * FLT_SCALE;
            const float ddx = (A12 * b2 - A22 * b1) * D;
            const float ddy = (A12 * b1 - A11 * b2) * D;
            nx += ddx; ny += ddy;
            resx = nx + half; resy = ny + half;
            if ((double)ddx * (double)ddx + (double)ddy * (double)ddy <= epsilon) break;
            if (j > 0 && lk_oscillates(ddx, pdx, ddy, pdy)) {
                resx -= ddx * 0.5f; resy -= ddy * 0.5f;
                break;
            }
            pdx = ddx; pdy = ddy;
        }
        if (left_band) break;
    }
    outx = resx; outy = resy;
}

template <int NR>
__global__ __launch_bounds__(64 * LK_WPB) KM_LK_OCC void lk_kernel(lk_args g, int sm_per_wave)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = blockIdx.x * LK_WPB + wv;
    const int n = __builtin_amdgcn_readfirstlane(g.d_n ? min(*g.d_n, g.n_max) : g.n_max);
    if (p >= n) return;                                  // (no workgroup barrier anywhere: waves are independent)
    unsigned char *smem = smem_all + (size_t)wv * sm_per_wave;
    const int win = g.win;
    const int RP = (win + 3 + 3 + 3) & ~3, JS = win + 1 + 2 * LK_M, JP = (JS + 3 + 3) & ~3;
    uint8_t *raw = smem;
    uint8_t *jp = smem + (((win + 3) * RP + 15) & ~15);
    short *derx = (short *)(jp + ((JS * JP + 15) & ~15));   // two int16 planes of (win+1)^2 values, 8 shorts of slack each
    int run_desc[NR];
#pragma unroll
    for (int t = 0; t < NR; t++) run_desc[t] = lk_run_desc(win, t);
    const float px = g.pts_in[2 * p], py = g.pts_in[2 * p + 1];
    float fx, fy;
    bool left_band = false;
    lk_track_point<NR>(g.A, g.B, px, py, win, g.max_count, g.epsilon, run_desc, raw, derx, jp, fx, fy, left_band);
    if ((threadIdx.x & 63) == 0) { g.p1[2 * p] = fx; g.p1[2 * p + 1] = fy; }
    if (g.backward) {
        float rx, ry;
        lk_track_point<NR>(g.B, g.A, fx, fy, win, g.max_count, g.epsilon, run_desc, raw, derx, jp, rx, ry, left_band);
        if ((threadIdx.x & 63) == 0) { g.p0r[2 * p] = rx; g.p0r[2 * p + 1] = ry; }
    }
    if (left_band && g.left_band && (threadIdx.x & 63) == 0) atomicOr(g.left_band, 1);
}

// the form is chosen here: the second where it serves the pyramids; the first for row bands (d_left_band), other pyramids and "lk2" off
int kl_track(km_ctx *c, const km_pyr &A, const km_pyr &B, const float *d_pts_in, const int *d_n, int n_max, int win, int max_count,
             double epsilon, bool backward_too, float *d_p1, float *d_p0r, int *d_left_band)
{
    if (n_max <= 0) return KM_OK;
    { const int rc = lk_check_window(c, win); if (rc) return rc; }
    const lk_args g = lk_fill_args(c, A, B, d_pts_in, d_n, n_max, win, max_count, epsilon, backward_too, d_p1, d_p0r, d_left_band);
    if (lk2_serves(c, A, B) && !d_left_band) return lk2_track(c, g);
    const int RP = (win + 3 + 3 + 3) & ~3, JS = win + 1 + 2 * LK_M, JP = (JS + 3 + 3) & ~3;
    const size_t sm = (((size_t)(win + 3) * RP + 15) & ~(size_t)15) + (((size_t)JS * JP + 15) & ~(size_t)15) + ((size_t)(win + 1) * (win + 1) + 8) * 2 * sizeof(short) + 16;
    const size_t smw = (sm + 15) & ~(size_t)15, sm_all = smw * LK_WPB;
    const int nblk = (n_max + LK_WPB - 1) / LK_WPB;
    switch (lk_shape_of(win).nr) {
    case 1: lk_kernel<1><<<nblk, 64 * LK_WPB, sm_all, c->stream>>>(g, (int)smw); break;
    case 2: lk_kernel<2><<<nblk, 64 * LK_WPB, sm_all, c->stream>>>(g, (int)smw); break;
    case 3: lk_kernel<3><<<nblk, 64 * LK_WPB, sm_all, c->stream>>>(g, (int)smw); break;
    case 4: lk_kernel<4><<<nblk, 64 * LK_WPB, sm_all, c->stream>>>(g, (int)smw); break;
    default: lk_kernel<5><<<nblk, 64 * LK_WPB, sm_all, c->stream>>>(g, (int)smw); break;
    }
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}

// test hook of lk_oscillates (km_lk_oscillation_probe): one thread per quadruple
__global__ void lk_oscillation_probe_kernel(const float *__restrict__ q, int n, uint8_t *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = lk_oscillates(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]) ? 1 : 0;
}
int kl_oscillation_probe(km_ctx *c, const float *d_q, int n, uint8_t *d_out)
{
    if (n <= 0) return KM_OK;
    lk_oscillation_probe_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(d_q, n, d_out);
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
