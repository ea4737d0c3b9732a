// K7, second form (two-level pyramids = the reference's maxLevel 1, klt.py:128-140; whole levels resident).
//
// What the first form pays per key point besides the window arithmetic: FOUR round trips to HBM (template + search
// neighbourhood per level and direction - the backward pass stages exactly the neighbourhoods the forward pass just had,
// with the roles of the two images swapped), a Scharr pass that writes two int16 planes to LDS through byte reads
// (two thirds of the kernel's LDS instructions) and reads them back, and index arithmetic on run-time sizes.
// Here every wavefront stages ONE (win + 7)^2 neighbourhood per image and level around its key point - four patches, all
// loads of the key point in flight together - and both directions work on them: the forward search patch of J is the
// backward template patch, the forward template patch of I is the backward search patch.  A lane evaluates the Scharr
// derivative of its own runs straight from the patch bytes in packed 16-bit arithmetic (4 unaligned 8-byte LDS reads per
// run, no derivative planes, no LDS write / barrier / read-back), so a patch is never modified and stays valid for the
// other direction.  A patch is re-centred (re-read from HBM) only when a window leaves its margin (displacements > 2 px
// per level; the reference's data is pre-aligned to less).  The arithmetic is the first form's, bit for bit.
//
// This file: the form's device code, its kernels and launchers.  kl_track (k_lk.hip) chooses between the forms.
#include "lk_launch.hpp"
#include "k_prior.hpp"

#include <cstddef>
#include <cstring>

#define LK2_M 3                       // margin (px) of a patch around the window it was centred on
#define LK2_INVALID (-(1 << 28))      // origin of a patch that holds nothing yet

template <int WIN> struct lk2_geo {
    int win;
    __device__ __host__ constexpr explicit lk2_geo(int w) : win(WIN ? WIN : w) {}
    __device__ __host__ constexpr int ps() const { return (WIN ? WIN : win) + 1 + 2 * LK2_M; }          // rows = columns of a patch
    __device__ __host__ constexpr int pp() const { return (ps() + 4 + 3) & ~3; }                       // row pitch (8-byte run reads end <= 4 bytes behind a row)
    __device__ __host__ constexpr int bytes() const { return (ps() * pp() + 16 + 15) & ~15; }          // + slack behind the last row
};
// the four patches of a key point stay within the 64 KB a workgroup may take without asking for more (9856 bytes at winSize 40); the
// patch side is the (win + 7) that lk_table_holds (lk_launch.hpp) proves the staging slots for
constexpr bool lk2_lds_holds()
{
    for (int win = LK_WIN_MIN; win <= LK_WIN_MAX; win++)
        if (4 * lk2_geo<0>(win).bytes() > 64 * 1024 || lk2_geo<0>(win).ps() != win + 7) return false;
    return true;
}
static_assert(lk2_lds_holds(), "the four patches of a key point exceed a workgroup's LDS");

typedef unsigned short lk_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ lk_us2 lk_as_us2(uint32_t v) { return __builtin_bit_cast(lk_us2, v); }
__device__ __forceinline__ uint32_t lk_us_as_u(lk_us2 v) { return __builtin_bit_cast(uint32_t, v); }

// (re)load the patch of image level (img, IW, IH) with origin (ox, oy); caller brackets with LK_WAVE_SYNC
template <int MAXIT, int WIN>
__device__ __forceinline__ void lk2_restage(const uint8_t *__restrict__ img, int IW, int IH, int ox, int oy, const lk2_geo<WIN> &geo, uint8_t *patch)
{
    stage_patch<MAXIT>(img, IW, IH, ox, oy, geo.ps(), geo.ps(), patch, geo.pp());
}

// a * b (two int16 products) + k with the addend in a register that stays live: VOP3P form, no copy of the constant.  The result
// is only ever the accumulator (src C) of the next dot of the same family, which the hardware forwards (tools/hazard_scan.py
// checks the generated code: the compiler cannot see a DOT behind inline assembly).
__device__ __forceinline__ int lk_dot2_k(lk_s2 a, lk_s2 b, int k)
{
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(k));
    return d;
}

// One direction of the tracker on the resident patches.  I = template image (patches pI[level 0, 1]), J = search image; oI / oJ: patch
// origins per level, updated when a patch is re-centred.
// SEEDED (a geometric prior): outx / outy carry the START position in - the search begins there at the top level,
// where the unseeded form begins at the key point (cv2's rule for OPTFLOW_USE_INITIAL_FLOW); everything else is the same text.
template <int NR, int WIN, int MAXIT, bool SEEDED = false>
__device__ void lk2_track_point(const km_pyr &I, const km_pyr &J, uint8_t *pI, uint8_t *pJ, int (&oI)[2][2], int (&oJ)[2][2], float px, float py,
                                const lk2_geo<WIN> &geo, int max_count, double epsilon, const int (&run_desc)[NR], float &outx, float &outy, int general_templates, int lk_reuse)
{
    const int win = geo.win;
    const int always_cut = lk_reuse ? 0 : 1;   // ("lk_reuse" 0: every iteration cuts its byte pairs out of LDS again)
    const float half = (float)(win - 1) * 0.5f;
    const float FLT_SCALE = 1.f / (1 << 20);
    const int PP = geo.pp(), PB = geo.bytes();
    float resx = px, resy = py;
    // rounding constants live in registers: the three-operand v_dot2_i32_i16 (lk_dot2_k) takes them as its addend, where the
    // compiler's accumulating v_dot2c needs a v_mov of the literal in front of every interpolated value
    int k_half9 = 1 << (14 - 5 - 1), k_half14 = 1 << 13;
    asm volatile("" : "+v"(k_half9), "+v"(k_half14));
#pragma unroll 1
    for (int level = 1; level >= 0; level--) {
        const int IW = I.W[level], IH = I.H[level], JW = J.W[level], JH = J.H[level];
        const float sc = level ? 0.5f : 1.f;
        float prx = px * sc, pry = py * sc;
        float nx, ny;
        if (level == 1) {
            if constexpr (SEEDED) { nx = outx * sc; ny = outy * sc; }
            else { nx = prx; ny = pry; }
        }
        else { nx = resx * 2.f; ny = resy * 2.f; }
        resx = nx; resy = ny;
        prx -= half; pry -= half;
        const int ipx = (int)floorf(prx), ipy = (int)floorf(pry);
        if (ipx < -win || ipx >= IW || ipy < -win || ipy >= IH) continue;
        float a = prx - (float)ipx, b = pry - (float)ipy;
        int w00, w01, w10, w11;
        lk_weights(a, b, w00, w01, w10, w11);
        uint8_t *X = pI + level * PB, *Y = pJ + level * PB;
        // the template needs patch rows / columns [t - 1, t + win + 1] with t = window origin - patch origin: 1 <= t <= 2 M - 1
        int tx = ipx - oI[level][0], ty = ipy - oI[level][1];
        if (tx < 1 || tx > 2 * LK2_M - 1 || ty < 1 || ty > 2 * LK2_M - 1) {
            LK_WAVE_SYNC();
            oI[level][0] = ipx - LK2_M; oI[level][1] = ipy - LK2_M;
            lk2_restage<MAXIT>(I.img[level], IW, IH, oI[level][0], oI[level][1], geo, X);
            LK_WAVE_SYNC();
            tx = ty = LK2_M;
        }
        // derivatives are zero outside the image (OpenCV pads the derivative image with zeros, the intensities with REFLECT_101)
        const bool need_mask = !(ipx >= 0 && ipy >= 0 && ipx + win <= IW - 1 && ipy + win <= IH - 1);
        uint32_t IvP[NR][3], IxP[NR][3], IyP[NR][3];
        int sA11 = 0, sA12 = 0, sA22 = 0;
        // The template's share of the mismatch vector does not change over the iterations: b = sum (J - I) (Ix, Iy) = sum J (Ix, Iy) - cI,
        // cI = sum I (Ix, Iy) per lane, once per pass (round 6: three packed subtractions per run and iteration less; exact integers either way)
        int cI1 = 0, cI2 = 0;
        // The bilinear weights of the TEMPLATE are often degenerate: a key point of the forward pass is an integer position (a corner
        // of goodFeaturesToTrack) and winSize is odd, so at level 0 the weights are exactly (16384, 0, 0, 0) and at level 1 multiples of
        // 4096 - I = 32 p, Ix / Iy = the Scharr values themselves, CV_DESCALE changes nothing.  MODE 2 (w01 = w10 =
        // w11 = 0): no interpolation at all, one bilinear row; MODE 1 (w10 = w11 = 0): one bilinear row, horizontal interpolation only;
        // MODE 0: the general two-row form (the backward pass, whose start positions are the forward pass's sub-pixel results).  The
        // values are the general form's bit for bit: a zero weight contributes a zero to an exact integer sum.
        auto build_templates = [&](auto mode_tag) {
            constexpr int MODE = decltype(mode_tag)::value;
            constexpr int ROWS = MODE == 0 ? 4 : 3, ND = MODE == 0 ? 2 : 1;
            const lk_s2 wt0 = lk_as_s2(lk_pack16(w00, w01)), wt1 = lk_as_s2(lk_pack16(w10, w11));   // signed: w11 may be -1
            const uint8_t *xb = X + (ty - 1) * PP + (tx - 1);
#pragma unroll
            for (int t = 0; t < NR; t++) {
                int rd = run_desc[t];
                asm volatile("" : "+v"(rd));
                const int y = rd & 0xff, x0 = (rd >> 8) & 0xff, n = rd >> 16;
                // patch rows y-1 .. y+2 (window coordinates), bytes x0-1 .. x0+6
                const uint8_t *pr = xb + y * PP + x0;
                uint2 R[4];
                const unsigned rsh = lk_lds_shift(pr);          // (the pitch is a multiple of 4: one shift for all rows)
#pragma unroll
                for (int k = 0; k < ROWS; k++) R[k] = lk_lds_read8(pr + k * PP, rsh);
                if constexpr (ROWS == 3) R[3] = R[2];
                // columns as 16-bit pairs (c0,c1) (c2,c3) (c4,c5) (c6,c7)
                lk_us2 E[4][4];
#pragma unroll
                for (int k = 0; k < ROWS; k++)
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        E[k][j] = lk_as_us2(__builtin_amdgcn_perm(R[k].y, R[k].x, 0x0c000c00u | (uint32_t)(2 * j) | ((uint32_t)(2 * j + 1) << 16)));
                uint32_t gx[2][3], gy[2][3];      // derivative pairs of the two bilinear rows: positions (0,1) (2,3) (4,5)
#pragma unroll
                for (int d = 0; d < ND; d++) {
                    lk_us2 S[4], V[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        S[j] = (E[d][j] + E[d + 2][j]) * (unsigned short)3 + E[d + 1][j] * (unsigned short)10;   // [3 10 3] down the column
                        V[j] = E[d + 2][j] - E[d][j];                                                               // [-1 0 1] down the column
                    }
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        gx[d][q] = lk_us_as_u(S[q + 1] - S[q]);                                                     // s(c+1) - s(c-1)
                        const lk_us2 vo = lk_as_us2(__builtin_amdgcn_alignbyte(lk_us_as_u(V[q + 1]), lk_us_as_u(V[q]), 2));   // (v(c), v(c+1)) of the odd columns
                        gy[d][q] = lk_us_as_u((V[q] + V[q + 1]) * (unsigned short)3 + vo * (unsigned short)10);     // 3 (v(c-1) + v(c+1)) + 10 v(c)
                    }
                }
                if (need_mask) {
                    const int gy0 = ipy + y, gx0 = ipx + x0;
#pragma unroll
                    for (int d = 0; d < ND; d++) {
                        const uint32_t mrow = (unsigned)(gy0 + d) < (unsigned)IH ? 0xffffffffu : 0u;
#pragma unroll
                        for (int q = 0; q < 3; q++) {
                            const uint32_t m = (((unsigned)(gx0 + 2 * q) < (unsigned)IW ? 0x0000ffffu : 0u) |
                                                ((unsigned)(gx0 + 2 * q + 1) < (unsigned)IW ? 0xffff0000u : 0u)) & mrow;
                            gx[d][q] &= m; gy[d][q] &= m;
                        }
                    }
                }
                if constexpr (MODE == 2) {
                    // weights (16384, 0, 0, 0): I = 32 p (bytes 1 .. 6 of patch row y), Ix / Iy = the Scharr pairs as they are
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        const uint32_t pm = n >= 2 * q + 2 ? 0xffffffffu : (n == 2 * q + 1 ? 0x0000ffffu : 0u);
                        const uint32_t pp2 = __builtin_amdgcn_perm(R[1].y, R[1].x, 0x0c000c00u | (uint32_t)(2 * q + 1) | ((uint32_t)(2 * q + 2) << 16));
                        IvP[t][q] = (pp2 << 5) & pm;                    // (two values <= 255: the shift does not cross the halves)
                        IxP[t][q] = gx[0][q] & pm;
                        IyP[t][q] = gy[0][q] & pm;
                        sA11 = __builtin_amdgcn_sdot2(lk_as_s2(IxP[t][q]), lk_as_s2(IxP[t][q]), sA11, false);
                        sA12 = __builtin_amdgcn_sdot2(lk_as_s2(IxP[t][q]), lk_as_s2(IyP[t][q]), sA12, false);
                        sA22 = __builtin_amdgcn_sdot2(lk_as_s2(IyP[t][q]), lk_as_s2(IyP[t][q]), sA22, false);
                        cI1 = __builtin_amdgcn_sdot2(lk_as_s2(IvP[t][q]), lk_as_s2(IxP[t][q]), cI1, false);
                        cI2 = __builtin_amdgcn_sdot2(lk_as_s2(IvP[t][q]), lk_as_s2(IyP[t][q]), cI2, false);
                    }
                } else {
                int iv[LK_RUN + 1], ixv[LK_RUN + 1], iyv[LK_RUN + 1];
                iv[LK_RUN] = 0; ixv[LK_RUN] = 0; iyv[LK_RUN] = 0;
#pragma unroll
                for (int k = 0; k < LK_RUN; k++) {
                    // intensities: bytes k+1, k+2 of patch rows y, y+1
                    const uint32_t sel = 0x0c000c00u | (uint32_t)(k + 1) | ((uint32_t)(k + 2) << 16);
                    const lk_s2 c0 = lk_as_s2(__builtin_amdgcn_perm(R[1].y, R[1].x, sel));
                    auto pair = [&](const uint32_t (&g)[3]) -> lk_s2 {
                        return lk_as_s2((k & 1) ? __builtin_amdgcn_alignbyte(g[(k + 1) / 2], g[k / 2], 2) : g[k / 2]);
                    };
                    if constexpr (MODE == 1) {
                        // (the compiler's own dot: its result is read by a shift, and a DOT result behind inline assembly gets no hazard padding)
                        iv[k] = __builtin_amdgcn_sdot2(c0, wt0, k_half9, false) >> (14 - 5);
                        ixv[k] = __builtin_amdgcn_sdot2(pair(gx[0]), wt0, k_half14, false) >> 14;
                        iyv[k] = __builtin_amdgcn_sdot2(pair(gy[0]), wt0, k_half14, false) >> 14;
                    } else {
                        const lk_s2 c1 = lk_as_s2(__builtin_amdgcn_perm(R[2].y, R[2].x, sel));
                        iv[k] = __builtin_amdgcn_sdot2(c0, wt0, lk_dot2_k(c1, wt1, k_half9), false) >> (14 - 5);
                        ixv[k] = __builtin_amdgcn_sdot2(pair(gx[0]), wt0, lk_dot2_k(pair(gx[1]), wt1, k_half14), false) >> 14;
                        iyv[k] = __builtin_amdgcn_sdot2(pair(gy[0]), wt0, lk_dot2_k(pair(gy[1]), wt1, k_half14), false) >> 14;
                    }
                }
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const uint32_t pm = n >= 2 * q + 2 ? 0xffffffffu : (n == 2 * q + 1 ? 0x0000ffffu : 0u);
                    IvP[t][q] = lk_pack16(iv[2 * q], iv[2 * q + 1]) & pm;
                    IxP[t][q] = lk_pack16(ixv[2 * q], ixv[2 * q + 1]) & pm;
                    IyP[t][q] = lk_pack16(iyv[2 * q], iyv[2 * q + 1]) & pm;
                    sA11 = __builtin_amdgcn_sdot2(lk_as_s2(IxP[t][q]), lk_as_s2(IxP[t][q]), sA11, false);
                    sA12 = __builtin_amdgcn_sdot2(lk_as_s2(IxP[t][q]), lk_as_s2(IyP[t][q]), sA12, false);
                    sA22 = __builtin_amdgcn_sdot2(lk_as_s2(IyP[t][q]), lk_as_s2(IyP[t][q]), sA22, false);
                    cI1 = __builtin_amdgcn_sdot2(lk_as_s2(IvP[t][q]), lk_as_s2(IxP[t][q]), cI1, false);
                    cI2 = __builtin_amdgcn_sdot2(lk_as_s2(IvP[t][q]), lk_as_s2(IyP[t][q]), cI2, false);
                }
                }
            }
        };
        {
            // (wave-uniform: every lane holds the key point's scalars; readfirstlane makes the branch a scalar one)
            const int z01 = __builtin_amdgcn_readfirstlane(w01), z1 = __builtin_amdgcn_readfirstlane(w10 | w11) | general_templates;
            if (z1 == 0 && z01 == 0) build_templates(std::integral_constant<int, 2>{});
            else if (z1 == 0) build_templates(std::integral_constant<int, 1>{});
            else build_templates(std::integral_constant<int, 0>{});
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
        int jx0 = oJ[level][0], jy0 = oJ[level][1];
        // The search patch's bytes under the window depend on the INTEGER position (inx, iny) and the patch origin only, and from the
        // second iteration on a step is a fraction of a pixel: the vertical byte pairs of every run stay in registers (KV) and are cut
        // out of LDS again only when the integer position moved (always on a pass's first iteration; a restage implies a move).  The
        // position is the same in every lane, so the test is a scalar branch.  The integers are the same either way.
        uint32_t KV[NR][LK_RUN + 1];
        int kinx = LK2_INVALID, kiny = LK2_INVALID;
        for (int j = 0; j < max_count; j++) {
            const int inx = (int)floorf(nx), iny = (int)floorf(ny);
            if (inx < -win || inx >= JW || iny < -win || iny >= JH) break;
            if (inx < jx0 || iny < jy0 || inx > jx0 + 2 * LK2_M || iny > jy0 + 2 * LK2_M) {
                // the window left the cached neighbourhood: re-centre it
                LK_WAVE_SYNC();
                jx0 = inx - LK2_M; jy0 = iny - LK2_M;
                lk2_restage<MAXIT>(J.img[level], JW, JH, jx0, jy0, geo, Y);
                LK_WAVE_SYNC();
                kinx = LK2_INVALID;
            }
            a = nx - (float)inx; b = ny - (float)iny;
            lk_weights(a, b, w00, w01, w10, w11);
            const lk_s2 wc0 = lk_as_s2(lk_pack16(w00, w10)), wc1 = lk_as_s2(lk_pack16(w01, w11));   // (column k, column k + 1); signed: w11 may be -1
            const int sinx = __builtin_amdgcn_readfirstlane(inx), siny = __builtin_amdgcn_readfirstlane(iny);
            if (((sinx ^ kinx) | (siny ^ kiny) | always_cut) != 0) {
                kinx = sinx; kiny = siny;
                const uint8_t *jb = Y + (iny - jy0) * PP + (inx - jx0);
#pragma unroll
                for (int t = 0; t < NR; t++) {
                    const int y = run_desc[t] & 0xff, x0 = (run_desc[t] >> 8) & 0xff;
                    const uint8_t *p0 = jb + y * PP + x0;
                    const unsigned jsh = lk_lds_shift(p0);
                    const uint2 r0 = lk_lds_read8(p0, jsh), r1 = lk_lds_read8(p0 + PP, jsh);   // bytes x0 .. x0+7 of the two patch rows
                    // VERTICAL byte pairs (row y, row y + 1) of columns 0 .. 5: six v_perm serve the five interpolated values (the horizontal
                    // pairs (k, k + 1) of either row took ten); the integer sum w00 p(k) + w10 q(k) + w01 p(k+1) + w11 q(k+1) is the same
#pragma unroll
                    for (int k = 0; k <= LK_RUN; k++) {
                        const uint32_t sel = 0x0c000c00u | (uint32_t)(k & 3) | ((uint32_t)(4 + (k & 3)) << 16);
                        KV[t][k] = k < 4 ? __builtin_amdgcn_perm(r1.x, r0.x, sel) : __builtin_amdgcn_perm(r1.y, r0.y, sel);
                    }
                }
            }
            int sb1 = -cI1, sb2 = -cI2;
#pragma unroll
            for (int t = 0; t < NR; t++) {
                int val[LK_RUN + 1];
                val[LK_RUN] = 0;
#pragma unroll
                for (int k = 0; k < LK_RUN; k++)
                    val[k] = __builtin_amdgcn_sdot2(lk_as_s2(KV[t][k]), wc0, lk_dot2_k(lk_as_s2(KV[t][k + 1]), wc1, k_half9), false) >> (14 - 5);
#pragma unroll
                for (int q2 = 0; q2 < 3; q2++) {
                    const lk_s2 jv = lk_as_s2(lk_pack16(val[2 * q2], val[2 * q2 + 1]));      // (positions beyond the run meet a zero Ix / Iy)
                    sb1 = __builtin_amdgcn_sdot2(jv, lk_as_s2(IxP[t][q2]), sb1, false);
                    sb2 = __builtin_amdgcn_sdot2(jv, lk_as_s2(IyP[t][q2]), sb2, false);
                }
            }
            const long long ib1 = lk_mismatch_sum<NR>(sb1), ib2 = lk_mismatch_sum<NR>(sb2);
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
        oJ[level][0] = jx0; oJ[level][1] = jy0;
    }
    outx = resx; outy = resy;
}

// ---- one key point per workgroup (= one wavefront): its four patches, both passes on them
// The patches [image][level] with origins oA / oB; one nobody wants (level skipped, search outside at once) is not staged.  `inside`: all
// four wanted and inside their images - all loads in flight together; otherwise level by level, each by its own path.  Ends with the wave sync.
template <int MAXIT, int WIN>
__device__ __forceinline__ void lk2_stage_all(const lk_args &g, const lk2_geo<WIN> &geo, const int (&oA)[2][2], const int (&oB)[2][2],
                                              const bool (&wantA)[2], const bool (&wantB)[2], bool inside, uint8_t *pA, uint8_t *pB)
{
    const int PS = geo.ps(), PP = geo.pp(), PB = geo.bytes();
    if (inside) {
        lk_patch_regs<MAXIT> r0, r1, r2, r3;
        stage_patch_issue<MAXIT>(g.A.img[1], g.A.W[1], oA[1][0], oA[1][1], PS, PS, r0);
        stage_patch_issue<MAXIT>(g.B.img[1], g.B.W[1], oB[1][0], oB[1][1], PS, PS, r1);
        stage_patch_issue<MAXIT>(g.A.img[0], g.A.W[0], oA[0][0], oA[0][1], PS, PS, r2);
        stage_patch_issue<MAXIT>(g.B.img[0], g.B.W[0], oB[0][0], oB[0][1], PS, PS, r3);
        stage_patch_commit<MAXIT>(PS, PS, pA + PB, PP, r0);
        stage_patch_commit<MAXIT>(PS, PS, pB + PB, PP, r1);
        stage_patch_commit<MAXIT>(PS, PS, pA, PP, r2);
        stage_patch_commit<MAXIT>(PS, PS, pB, PP, r3);
    } else {
#pragma unroll 1
        for (int l = 1; l >= 0; l--) {
            if (wantA[l]) lk2_restage<MAXIT>(g.A.img[l], g.A.W[l], g.A.H[l], oA[l][0], oA[l][1], geo, pA + l * PB);
            if (wantB[l]) lk2_restage<MAXIT>(g.B.img[l], g.B.W[l], g.B.H[l], oB[l][0], oB[l][1], geo, pB + l * PB);
        }
    }
    LK_WAVE_SYNC();
}

// Forward pass from (gx, gy) - the key point itself where nothing seeds the search -, p1 stored; backward pass from p1 - (g - p0), p0r
// stored.  The backward pass never reads p0 itself; its search patch is the forward template's, re-centred if p1 moved away.
// UNIFORM_SHIFT (the batched seeded kernels): g - p0, the same in every lane, is taken in front of the forward pass and waits for the
// backward pass in scalar registers - the unit's arguments come through the table pointer there, and the guess's two vector registers,
// live across the forward pass, were the ones the win-25 instance had to spill.
template <int NR, int WIN, int MAXIT, bool SEEDED, bool UNIFORM_SHIFT = false>
__device__ __forceinline__ void lk2_both_passes(const lk_args &g, int p, float px, float py, float gx, float gy, const lk2_geo<WIN> &geo,
                                                const int (&run_desc)[NR], uint8_t *pA, uint8_t *pB, int (&oA)[2][2], int (&oB)[2][2])
{
    float sx = 0.f, sy = 0.f;
    if constexpr (UNIFORM_SHIFT) {
        int isx = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, gx - px)), isy = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, gy - py));
        asm volatile("" : "+s"(isx), "+s"(isy));      // (HERE, in scalar registers: left alone the compiler sinks both behind the forward pass)
        sx = __builtin_bit_cast(float, isx); sy = __builtin_bit_cast(float, isy);
    }
    float fx = gx, fy = gy;
    lk2_track_point<NR, WIN, MAXIT, SEEDED>(g.A, g.B, pA, pB, oA, oB, px, py, geo, g.max_count, g.epsilon, run_desc, fx, fy, g.general_templates, g.lk_reuse);
    if ((threadIdx.x & 63) == 0) { g.p1[2 * p] = fx; g.p1[2 * p + 1] = fy; }
    if (g.backward) {
        if constexpr (!UNIFORM_SHIFT) { sx = gx - px; sy = gy - py; }
        float rx = fx - sx, ry = fy - sy;
        lk2_track_point<NR, WIN, MAXIT, SEEDED>(g.B, g.A, pB, pA, oB, oA, fx, fy, geo, g.max_count, g.epsilon, run_desc, rx, ry, g.general_templates, g.lk_reuse);
        if ((threadIdx.x & 63) == 0) { g.p0r[2 * p] = rx; g.p0r[2 * p + 1] = ry; }
    }
}

// Unseeded: one neighbourhood per image and level, centred on the key point's window in BOTH images (the second image's patch takes
// the first's origin and the first's verdict: no test of its own in the hot kernels).
template <int NR, int WIN, int MAXIT>
__device__ __forceinline__ void lk2_body(const lk_args &g, const int *__restrict__ order)
{
    // (what a wave reads through a pointer that itself came from the unit table arrives in vector registers: the corner count and the key
    // point are the same in every lane, and saying so keeps the per-level geometry and every test on it in scalar registers)
    const int n = __builtin_amdgcn_readfirstlane(g.d_n ? min(*g.d_n, g.n_max) : g.n_max);
    // workgroup w runs on XCD w % 8: every XCD takes one contiguous eighth of the (spatially ordered) point list
    const unsigned per = ((unsigned)n + KM_XCDS - 1) / KM_XCDS, slot = (blockIdx.x % KM_XCDS) * per + blockIdx.x / KM_XCDS;
    if (blockIdx.x / KM_XCDS >= per || slot >= (unsigned)n) return;
    const int p = order ? order[slot] : (int)slot;
    const lk2_geo<WIN> geo(g.win);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    const int win = geo.win, PS = geo.ps(), PB = geo.bytes();
    uint8_t *pA = smem_all, *pB = smem_all + 2 * PB;      // patches: [image][level]
    int run_desc[NR];
#pragma unroll
    for (int t = 0; t < NR; t++) run_desc[t] = lk_run_desc(win, t);
    const float px = lk_uniform(g.pts_in[2 * p]), py = lk_uniform(g.pts_in[2 * p + 1]);
    const float half = (float)(win - 1) * 0.5f;
    int oA[2][2], oB[2][2];
    bool want[2], inside = true;
#pragma unroll
    for (int l = 0; l < 2; l++) {
        const float sc = l ? 0.5f : 1.f;
        const int ipx = (int)floorf(px * sc - half), ipy = (int)floorf(py * sc - half);
        want[l] = !(ipx < -win || ipx >= g.A.W[l] || ipy < -win || ipy >= g.A.H[l]);      // (else the level is skipped: nothing to stage)
        oA[l][0] = oB[l][0] = want[l] ? ipx - LK2_M : LK2_INVALID;
        oA[l][1] = oB[l][1] = want[l] ? ipy - LK2_M : LK2_INVALID;
        inside = inside && want[l] && lk_patch_inside(g.A.W[l], g.A.H[l], oA[l][0], oA[l][1], PS, PS, MAXIT);
    }
    lk2_stage_all<MAXIT>(g, geo, oA, oB, want, want, inside, pA, pB);
    lk2_both_passes<NR, WIN, MAXIT, false>(g, p, px, py, px, py, geo, run_desc, pA, pB, oA, oB);
}

// Seeded (a geometric prior).  The guess of a key point is either given (seed.guess) or the prior evaluated on the key
// point - wave-uniform doubles, prior_math.hpp; a key point without a guess starts at itself, as the unseeded form does (the mask of
// k_prior.hip keeps such pixels from becoming corners).  The A patches are staged around the key point's window, the B patches around the
// GUESS's window - the search's first position.  A level whose template lies outside the first image is skipped by the tracker (nothing to
// stage in either image); a guess window the iteration loop would leave at once (inx < -win or >= W, likewise y) stages nothing in B.
template <int NR, int WIN, int MAXIT, bool UNITS = false>
__device__ __forceinline__ void lk2_seeded_body(const lk_args &g, const kl_seed &seed)
{
    const int n = __builtin_amdgcn_readfirstlane(g.d_n ? min(*g.d_n, g.n_max) : g.n_max);      // (as lk2_body)
    const unsigned per = ((unsigned)n + KM_XCDS - 1) / KM_XCDS, slot = (blockIdx.x % KM_XCDS) * per + blockIdx.x / KM_XCDS;
    if (blockIdx.x / KM_XCDS >= per || slot >= (unsigned)n) return;
    const int p = (int)slot;
    const lk2_geo<WIN> geo(g.win);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    const int win = geo.win, PS = geo.ps(), PB = geo.bytes();
    uint8_t *pA = smem_all, *pB = smem_all + 2 * PB;      // patches: [image][level]
    int run_desc[NR];
#pragma unroll
    for (int t = 0; t < NR; t++) run_desc[t] = lk_run_desc(win, t);
    const float px = lk_uniform(g.pts_in[2 * p]), py = lk_uniform(g.pts_in[2 * p + 1]);
    const float half = (float)(win - 1) * 0.5f;
    float gx = px, gy = py;
    if (!seed.guess) {
        float tx, ty;
        if (pm::guess(seed.P, seed.x_off, seed.y_off, px, py, tx, ty)) { gx = lk_uniform(tx); gy = lk_uniform(ty); }
    } else { gx = lk_uniform(seed.guess[2 * p]); gy = lk_uniform(seed.guess[2 * p + 1]); }
    int oA[2][2], oB[2][2];
    bool wantA[2], wantB[2], inside = true;
#pragma unroll
    for (int l = 0; l < 2; l++) {
        const float sc = l ? 0.5f : 1.f;
        const int ipx = (int)floorf(px * sc - half), ipy = (int)floorf(py * sc - half);
        const int jpx = (int)floorf(gx * sc - half), jpy = (int)floorf(gy * sc - half);
        wantA[l] = !(ipx < -win || ipx >= g.A.W[l] || ipy < -win || ipy >= g.A.H[l]);
        wantB[l] = wantA[l] && !(jpx < -win || jpx >= g.B.W[l] || jpy < -win || jpy >= g.B.H[l]);
        oA[l][0] = wantA[l] ? ipx - LK2_M : LK2_INVALID; oA[l][1] = wantA[l] ? ipy - LK2_M : LK2_INVALID;
        oB[l][0] = wantB[l] ? jpx - LK2_M : LK2_INVALID; oB[l][1] = wantB[l] ? jpy - LK2_M : LK2_INVALID;
        inside = inside && wantB[l] && lk_patch_inside(g.A.W[l], g.A.H[l], oA[l][0], oA[l][1], PS, PS, MAXIT) &&
                 lk_patch_inside(g.B.W[l], g.B.H[l], oB[l][0], oB[l][1], PS, PS, MAXIT);
    }
    lk2_stage_all<MAXIT>(g, geo, oA, oB, wantA, wantB, inside, pA, pB);
    lk2_both_passes<NR, WIN, MAXIT, true, UNITS>(g, p, px, py, gx, gy, geo, run_desc, pA, pB, oA, oB);
}

// ---- the kernels: four families (plain, seeded, batched units, batched units under priors), each with one instance per NR class and one for the reference's
// window (matching_winsize 25, processing_configuration.json:14) with every size a compile-time constant, pinned to 5 waves per SIMD
#ifndef LK2_25_WAVES
#define LK2_25_WAVES 5
#endif
#if LK2_25_WAVES
#define LK2_25_OCC __attribute__((amdgpu_waves_per_eu(LK2_25_WAVES, LK2_25_WAVES)))
#else
#define LK2_25_OCC
#endif
static_assert(lk_shape_of(25).nr == 2 && lk_shape_of(25).maxit == 4 && lk_shape_of(25).win == 25, "the win-25 kernels are lk2_*<2, 25, 4>");
template <int NR, int WIN, int MAXIT>
__global__ __launch_bounds__(64) KM_LK_OCC void lk2_kernel(lk_args g, const int *__restrict__ order) { lk2_body<NR, WIN, MAXIT>(g, order); }
__global__ __launch_bounds__(64) LK2_25_OCC void lk2_kernel_win25(lk_args g, const int *__restrict__ order) { lk2_body<2, 25, 4>(g, order); }
// seeded (kl_track_seeded below): kernels of their own - the arguments, the registers and the code of the unseeded ones do not know of them
template <int NR, int WIN, int MAXIT>
__global__ __launch_bounds__(64) KM_LK_OCC void lk2_seeded_kernel(lk_args g, kl_seed seed) { lk2_seeded_body<NR, WIN, MAXIT>(g, seed); }
__global__ __launch_bounds__(64) LK2_25_OCC void lk2_seeded_kernel_win25(lk_args g, kl_seed seed) { lk2_seeded_body<2, 25, 4>(g, seed); }
// batched units (api_units.hip): ONE launch tracks the corners of every unit (blockIdx.y = unit): a launch pays one wave lifetime of
// fill + drain (~30 us) whatever its size, and sixteen units' 320 000 corners keep the GPU in steady state throughout.
// The per-unit arguments are the single-unit kernel's own `lk_args`, in a table in device memory (sixteen of them exceed the 4 KB of
// kernel arguments): the tracker indexes the pyramids by level at run time, which wants them in addressable memory, not in registers.
template <int NR, int WIN, int MAXIT>
__global__ __launch_bounds__(64) KM_LK_OCC void lk2_units_kernel(const lk_args *__restrict__ table) { lk2_body<NR, WIN, MAXIT>(table[blockIdx.y], nullptr); }
__global__ __launch_bounds__(64) LK2_25_OCC void lk2_units_kernel_win25(const lk_args *__restrict__ table) { lk2_body<2, 25, 4>(table[blockIdx.y], nullptr); }
// batched units under a prior each (km_klt_units_frame_prior_submit): the seeded body on unit blockIdx.y's arguments and seed.  Both
// tables are read at an index that is the same in every lane, through pointers nothing else writes: scalar loads, and the seed stays in
// scalar registers as the prologue of lk2_seeded_body assumes
template <int NR, int WIN, int MAXIT>
__global__ __launch_bounds__(64) KM_LK_OCC void lk2_seeded_units_kernel(const lk_args *__restrict__ table, const kl_seed *__restrict__ seeds)
{
    lk2_seeded_body<NR, WIN, MAXIT, true>(table[blockIdx.y], seeds[blockIdx.y]);
}
__global__ __launch_bounds__(64) LK2_25_OCC void lk2_seeded_units_kernel_win25(const lk_args *__restrict__ table, const kl_seed *__restrict__ seeds)
{
    lk2_seeded_body<2, 25, 4, true>(table[blockIdx.y], seeds[blockIdx.y]);
}

// ---- launches.  A family names its instances; lk2_launch picks the one lk_shape_of(win) says.
struct lk2_plain { static constexpr auto win25 = lk2_kernel_win25; template <int NR, int MAXIT> static constexpr auto generic = lk2_kernel<NR, 0, MAXIT>; };
struct lk2_seeded { static constexpr auto win25 = lk2_seeded_kernel_win25; template <int NR, int MAXIT> static constexpr auto generic = lk2_seeded_kernel<NR, 0, MAXIT>; };
struct lk2_units { static constexpr auto win25 = lk2_units_kernel_win25; template <int NR, int MAXIT> static constexpr auto generic = lk2_units_kernel<NR, 0, MAXIT>; };
struct lk2_seeded_units { static constexpr auto win25 = lk2_seeded_units_kernel_win25; template <int NR, int MAXIT> static constexpr auto generic = lk2_seeded_units_kernel<NR, 0, MAXIT>; };

template <class F, class... Args>
static int lk2_launch(km_ctx *c, dim3 grid, int win, const Args &...args)
{
    const lk_shape s = lk_shape_of(win);
    const size_t sm = (size_t)4 * lk2_geo<0>(win).bytes();
#define LK2_INSTANCE(NR) case NR: F::template generic<NR, lk2_maxit(NR)><<<grid, 64, sm, c->stream>>>(args...); break
    if (s.win == 25) F::win25<<<grid, 64, sm, c->stream>>>(args...);
    else switch (s.nr) {
    LK2_INSTANCE(1); LK2_INSTANCE(2); LK2_INSTANCE(3); LK2_INSTANCE(4); LK2_INSTANCE(5);
    }
#undef LK2_INSTANCE
    KM_LAUNCH_CHECK(c);
    return KM_OK;
}
// the plain launch (kl_track, k_lk.hip, has checked the window and that this form serves the pyramids)
int lk2_track(km_ctx *c, const lk_args &g)
{
    const int *order = nullptr;          // (processing order of the points: a caller may pass a list)
    return lk2_launch<lk2_plain>(c, km_xcd_grid((unsigned)g.n_max), g.win, g, order);
}

// The second form from a start position per key point.  KM_E_UNSUPPORTED, nothing queued: what lk2_serves refuses (the first form stays unseeded).
int kl_track_seeded(km_ctx *c, const km_pyr &A, const km_pyr &B, const float *d_pts_in, const int *d_n, int n_max, int win, int max_count,
                    double epsilon, bool backward_too, float *d_p1, float *d_p0r, const kl_seed &seed)
{
    if (n_max <= 0) return KM_OK;
    { const int rc = lk_check_window(c, win); if (rc) return rc; }
    if (!lk2_serves(c, A, B))
        return km_fail(c, KM_E_UNSUPPORTED, "a prior needs the two-level tracker on whole images (pyramid levels %d / %d)", A.levels, B.levels);
    const lk_args g = lk_fill_args(c, A, B, d_pts_in, d_n, n_max, win, max_count, epsilon, backward_too, d_p1, d_p0r, nullptr);
    return lk2_launch<lk2_seeded>(c, km_xcd_grid((unsigned)n_max), win, g, seed);
}

// The argument table of n forward + backward runs (units of a batch, jobs of the kernel-size search): `entry(i, g)` sets pyramids, points
// and outputs of run i.  KM_E_UNSUPPORTED (no message): a run this form does not serve - kl_track run by run.
template <class Entry>
static int lk2_fill_table(km_ctx *c, lk_args *host, int n, int n_max, int win, int max_count, double epsilon, Entry entry)
{
    const lk_args shared = lk_fill_args(c, km_pyr(), km_pyr(), nullptr, nullptr, n_max, win, max_count, epsilon, true, nullptr, nullptr, nullptr);
    for (int i = 0; i < n; i++) {
        host[i] = shared;
        entry(i, host[i]);
        if (!lk2_serves(c, host[i].A, host[i].B)) return KM_E_UNSUPPORTED;
    }
    return KM_OK;
}
// ... uploaded into WS_UNITS_LK on c->stream
template <class Entry>
static int lk2_upload_table(km_ctx *c, int n, int capacity, int n_max, int win, int max_count, double epsilon, Entry entry)
{
    lk_args host[KM_LK_JOBS_MAX > KM_UNITS_MAX ? KM_LK_JOBS_MAX : KM_UNITS_MAX];
    if (const int rc = lk2_fill_table(c, host, n, n_max, win, max_count, epsilon, entry)) return rc;
    lk_args *table = (lk_args *)km_ws(c, WS_UNITS_LK, sizeof(lk_args) * (size_t)capacity);
    if (!table) return KM_E_NOMEM;
    return km_h2d_small(c, table, host, sizeof(lk_args) * (size_t)n);
}

// kl_units_prepare: validate + upload the table (early in the call: the small copy is then off the critical path); kl_units_launch: the launch
static void lk2_unit_entry(const km_units &U, int u, lk_args &g)
{
    g.A = U.A[u]; g.B = U.B[u]; g.pts_in = U.p0[u]; g.d_n = &U.sc[u]->n_corners; g.p1 = U.p1[u]; g.p0r = U.p0r[u];
}
int kl_units_prepare(km_ctx *c, const km_units &U, int n_max, int win, int max_count, double epsilon)
{
    if (n_max <= 0 || U.n <= 0) return KM_OK;
    { const int rc = lk_check_window(c, win); if (rc) return rc; }
    return lk2_upload_table(c, U.n, KM_UNITS_MAX, n_max, win, max_count, epsilon, [&](int u, lk_args &g) { lk2_unit_entry(U, u, g); });
}
int kl_units_launch(km_ctx *c, int n_units, int n_max, int win)
{
    if (n_max <= 0 || n_units <= 0) return KM_OK;
    const lk_args *table = (const lk_args *)km_ws_peek(c, WS_UNITS_LK);
    return lk2_launch<lk2_units>(c, dim3(km_xcd_grid((unsigned)n_max), n_units), win, table);
}

// ... under a prior per unit (`priors`: U.n x 9, unit order; the origin is the unit's).  The seeds lie behind the table's KM_UNITS_MAX
// entries in the same slot and travel in the SAME small copy: whatever orders the table for the launch orders the seeds
struct lk2_seeded_table {
    lk_args args[KM_UNITS_MAX];
    kl_seed seeds[KM_UNITS_MAX];
};
int kl_units_prepare_seeded(km_ctx *c, const km_units &U, const double *priors, int n_max, int win, int max_count, double epsilon)
{
    if (n_max <= 0 || U.n <= 0) return KM_OK;
    { const int rc = lk_check_window(c, win); if (rc) return rc; }
    lk2_seeded_table host = {};
    if (const int rc = lk2_fill_table(c, host.args, U.n, n_max, win, max_count, epsilon, [&](int u, lk_args &g) { lk2_unit_entry(U, u, g); })) return rc;
    for (int u = 0; u < U.n; u++) {
        kl_seed &s = host.seeds[u];
        s.guess = nullptr; memcpy(s.P, priors + 9 * u, sizeof s.P); s.x_off = (double)U.x_off[u]; s.y_off = (double)U.y_off[u];
    }
    lk2_seeded_table *table = (lk2_seeded_table *)km_ws(c, WS_UNITS_LK, sizeof(lk2_seeded_table));
    if (!table) return KM_E_NOMEM;
    return km_h2d_small(c, table, &host, offsetof(lk2_seeded_table, seeds) + sizeof(kl_seed) * (size_t)U.n);
}
int kl_units_launch_seeded(km_ctx *c, int n_units, int n_max, int win)
{
    if (n_max <= 0 || n_units <= 0) return KM_OK;
    const lk2_seeded_table *table = (const lk2_seeded_table *)km_ws_peek(c, WS_UNITS_LK);
    return lk2_launch<lk2_seeded_units>(c, dim3(km_xcd_grid((unsigned)n_max), n_units), win, table->args, table->seeds);
}

// Independent tracker runs in ONE launch (unit = blockIdx.y): the 25 (mon kernel, ref kernel) runs of the Laplacian kernel-size search (klt.py:465-545),
// every job its own pyramids, corner list and outputs.  Every refusal is silent: too many jobs, a window or pyramids the form does not hold, lk2 off.
int kl_jobs_launch(km_ctx *c, const km_lk_job *jobs, int n_jobs, int n_max, int win, int max_count, double epsilon)
{
    if (n_max <= 0 || n_jobs <= 0) return KM_OK;
    if (n_jobs > KM_LK_JOBS_MAX || !lk_window_served(win)) return KM_E_UNSUPPORTED;
    const int rc = lk2_upload_table(c, n_jobs, KM_LK_JOBS_MAX, n_max, win, max_count, epsilon, [&](int j, lk_args &g) {
        g.A = jobs[j].A; g.B = jobs[j].B; g.pts_in = jobs[j].pts_in; g.d_n = jobs[j].d_n; g.p1 = jobs[j].p1; g.p0r = jobs[j].p0r;
    });
    return rc ? rc : kl_units_launch(c, n_jobs, n_max, win);
}

