// TEST INFRASTRUCTURE (tests/test_host_asan.py): stand-ins of the launchers of the align step (k_align.hpp, k_prep.hpp, k_match.hpp,
// k_ransac.hpp, k_sift.hpp) for the host-only sanitizer build; the rule of stub_kernels.cpp holds - inputs are READ completely and
// outputs WRITTEN completely, at the sizes the launchers are entitled to.
//
// RANSAC and SIFT are not do-little: their stand-ins are loops over ransac_math.hpp / sift_math.hpp, the text the kernels compile,
// plus the dense SIFT stages in the operation order k_sift.hip states.  km_find_homography_ransac* and km_sift_detect_and_compute*
// therefore run end to end on the CPU and are held to tests/ransac_restatement.py / tests/sift_restatement.py bit for bit
// (driver_align.py).  Prep, match and align fill what the host reads back with simple arithmetic of their own; the exact formulas
// live only in the kernels and are the GPU tests' business.
//
// Stream order (stub_order.hpp): the stand-ins of THIS file declare no accesses.  An unannotated launcher claims nothing, so it can only
// hide a conflict from the checker, never invent one; the align step runs on the main stream alone.  The same holds for the clip stage's
// stand-in, which lives in csrc/k_clip.hpp.
#include "../../karios_amd/csrc/k_align.hpp"
#include "../../karios_amd/csrc/k_match.hpp"
#include "../../karios_amd/csrc/k_prep.hpp"
#include "../../karios_amd/csrc/k_ransac.hpp"
#include "../../karios_amd/csrc/k_sift.hpp"
#include "../../karios_amd/csrc/ransac_math.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

// ------------------------------------------------------------------ RANSAC (k_ransac.hpp): the arithmetic is ransac_math.hpp's
int krs_pack(km_ctx *, const float *d_src, ptrdiff_t ss, const float *d_dst, ptrdiff_t sd, int n, float *d_pairs)
{
    for (int i = 0; i < n; i++) {
        const float *s = d_src + (size_t)i * ss, *d = d_dst + (size_t)i * sd;
        float *p = d_pairs + 4 * (size_t)i;
        p[0] = s[0]; p[1] = s[1]; p[2] = d[0]; p[3] = d[1];
    }
    return KM_OK;
}
int krs_solve(km_ctx *, const float *d_pairs, int, const int *d_idx, int first, int count, double *d_H64, float *d_Hf, int *d_valid, int *d_count)
{
    for (size_t it = (size_t)first; it < (size_t)first + count; it++) {
        float M[8], m[8];
        for (int k = 0; k < 4; k++) {
            const float *p = d_pairs + 4 * (size_t)d_idx[4 * it + k];
            M[2 * k] = p[0]; M[2 * k + 1] = p[1]; m[2 * k] = p[2]; m[2 * k + 1] = p[3];
        }
        double H[9] = {0};
        const int ok = rs::dlt(M, m, 4, H);
        for (int k = 0; k < 9; k++) {
            d_H64[it * 9 + k] = ok ? H[k] : 0.;
            d_Hf[it * KRS_HSTRIDE + k] = ok ? (float)H[k] : __builtin_nanf("");
        }
        for (int k = 9; k < KRS_HSTRIDE; k++) d_Hf[it * KRS_HSTRIDE + k] = 0.f;
        d_valid[it] = ok;
        d_count[it] = 0;
    }
    return KM_OK;
}
int krs_score(km_ctx *, const float *d_pairs, int n, const float *d_Hf, int first, int count, float thr, int *d_count)
{
    for (size_t it = (size_t)first; it < (size_t)first + count; it++) {
        const float *H = d_Hf + it * KRS_HSTRIDE;
        int cnt = 0;
        for (int i = 0; i < n; i++) { const float *p = d_pairs + 4 * (size_t)i; cnt += rs::reproj_err(H, p[0], p[1], p[2], p[3]) <= thr; }
        d_count[it] += cnt;
    }
    return KM_OK;
}
int krs_mask(km_ctx *, const float *d_pairs, int n, const float *Hf, float thr, uint8_t *d_mask, int *d_total)
{
    int total = 0;
    for (int i = 0; i < n; i++) {
        const float *p = d_pairs + 4 * (size_t)i;
        d_mask[i] = rs::reproj_err(Hf, p[0], p[1], p[2], p[3]) <= thr ? 1 : 0;
        total += d_mask[i];
    }
    *d_total = total;
    return KM_OK;
}

// ------------------------------------------------------------------ SIFT (k_sift.hpp): dense stages in k_sift.hip's operation order
static int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}
int ksf_base(km_ctx *, const uint8_t *img, int H, int W, ptrdiff_t stride, float *out)
{
    for (int y = 0; y < 2 * H; y++)
        for (int x = 0; x < 2 * W; x++) {
            const int x0 = x >> 1, x1 = (x & 1) ? std::min(x0 + 1, W - 1) : x0;
            const int y0 = y >> 1, y1 = (y & 1) ? std::min(y0 + 1, H - 1) : y0;
            const uint8_t *r0 = img + (ptrdiff_t)y0 * stride, *r1 = img + (ptrdiff_t)y1 * stride;
            const float a = ((float)r0[x0] + (float)r0[x1]) * 0.5f, b = ((float)r1[x0] + (float)r1[x1]) * 0.5f;
            out[(size_t)y * (2 * W) + x] = (a + b) * 0.5f;
        }
    return KM_OK;
}
// centre tap first, then k[j] * (x[-j] + x[+j]); rows into tmp, columns into dst, the DoG level against src fused
int ksf_blur(km_ctx *, const float *src, int h, int w, const ksf_taps &taps, float *tmp, float *dst, float *dog)
{
    const int R = taps.radius;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const float *row = src + (size_t)y * w;
            float s = taps.k[0] * row[x];
            for (int j = 1; j <= R; j++) s += taps.k[j] * (row[reflect101(x - j, w)] + row[reflect101(x + j, w)]);
            tmp[(size_t)y * w + x] = s;
        }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float s = taps.k[0] * tmp[(size_t)y * w + x];
            for (int j = 1; j <= R; j++) s += taps.k[j] * (tmp[(size_t)reflect101(y - j, h) * w + x] + tmp[(size_t)reflect101(y + j, h) * w + x]);
            const float prev = src[(size_t)y * w + x];      // (dst never aliases src: read before the store all the same)
            dst[(size_t)y * w + x] = s;
            if (dog) dog[(size_t)y * w + x] = s - prev;
        }
    return KM_OK;
}
int ksf_decimate(km_ctx *, const float *src, int h, int w, float *dst)
{
    const int h2 = h / 2, w2 = w / 2;
    for (int y = 0; y < h2; y++)
        for (int x = 0; x < w2; x++) dst[(size_t)y * w2 + x] = src[(size_t)(2 * y) * w + 2 * x];
    return KM_OK;
}
// the kernels' list protocol, here and below: the counter counts every record, only records below `cap` are written
int ksf_scan(km_ctx *, const float *dog, size_t plane, int h, int w, int n_layers, float threshold, ksf_cand *cand, unsigned cap, unsigned *counter)
{
    for (int layer = 1; layer <= n_layers; layer++)
        for (int y = sf::BORDER; y < h - sf::BORDER; y++)
            for (int x = sf::BORDER; x < w - sf::BORDER; x++) {
                const float *p = dog + (size_t)layer * plane + (size_t)y * w + x;
                const float v = p[0];
                if (!(sf::absf(v) > threshold)) continue;
                bool ge = true, le = true;
                for (int dl = -1; dl <= 1; dl++)
                    for (int dr = -1; dr <= 1; dr++)
                        for (int dc = -1; dc <= 1; dc++) {
                            const float q = p[(ptrdiff_t)dl * (ptrdiff_t)plane + (ptrdiff_t)dr * w + dc];
                            ge = ge && v >= q; le = le && v <= q;
                        }
                if (!((v > 0 && ge) || (v < 0 && le))) continue;
                const unsigned at = (*counter)++;
                if (at < cap) cand[at] = ksf_cand{layer, y, x};
            }
    return KM_OK;
}
int ksf_refine(km_ctx *, const float *dog, size_t plane, int h, int w, int octv, const ksf_cand *cand, unsigned n_cand, int n_layers, double contrast_threshold,
               double edge_threshold, double sigma, sf::Refined *out, unsigned *counter)
{
    for (unsigned i = 0; i < n_cand; i++) {
        sf::Refined r;
        if (sf::refine(dog, plane, w, h, w, octv, cand[i].layer, cand[i].r, cand[i].c, n_layers, contrast_threshold, edge_threshold, sigma, r))
            out[(*counter)++] = r;           // at most n_cand records: the list has room for all of them
    }
    return KM_OK;
}
int ksf_orient(km_ctx *, const float *gauss, size_t plane, int h, int w, int octv, const sf::Refined *refined, unsigned n_refined, sf::Key *kp, unsigned cap,
               unsigned *counter)
{
    for (unsigned i = 0; i < n_refined; i++) {
        const sf::Refined r = refined[i];
        float angles[sf::ORI_BINS / 2];
        const int n = sf::orientations(gauss + (size_t)r.layer * plane, w, h, w, r.r, r.c, r.size, octv, angles);
        for (int k = 0; k < n; k++) {
            const unsigned at = (*counter)++;
            if (at < cap) kp[at] = sf::Key{r.x, r.y, r.size, angles[k], r.response, r.octave};
        }
    }
    return KM_OK;
}
int ksf_describe(km_ctx *, const float *gauss, size_t plane, int h, int w, int octv, const sf::Key *kp, unsigned n, uint8_t *desc)
{
    const float inv = 1.f / (float)(1 << octv);
    for (unsigned i = 0; i < n; i++) {
        const sf::Key q = kp[i];
        float hist[sf::D_HIST];
        sf::descriptor<1>(gauss + (size_t)((q.octave >> 8) & 255) * plane, w, h, w, q.x * inv, q.y * inv, q.angle, q.size * inv * 0.5f, hist,
                          desc + (size_t)i * sf::D_LEN);
    }
    return KM_OK;
}
int ksf_gather(km_ctx *, const sf::Key *kp, const uint8_t *desc, const int *perm, int n, float *x, float *y, float *size, float *angle, float *response,
               int *octave, void *out_desc, int desc_dtype, ptrdiff_t desc_stride)
{
    for (int i = 0; i < n; i++) {
        const sf::Key q = kp[perm[i]];
        x[i] = q.x * 0.5f; y[i] = q.y * 0.5f; size[i] = q.size * 0.5f; angle[i] = q.angle; response[i] = q.response;
        octave[i] = (q.octave & ~255) | ((q.octave - 1) & 255);      // firstOctave = -1
        for (int k = 0; k < sf::D_LEN; k++) {
            const uint8_t v = desc[(size_t)perm[i] * sf::D_LEN + k];
            if (desc_dtype == KM_F32) ((float *)out_desc)[(ptrdiff_t)i * desc_stride + k] = (float)v;
            else ((uint8_t *)out_desc)[(ptrdiff_t)i * desc_stride + k] = v;
        }
    }
    return KM_OK;
}

// ------------------------------------------------------------------ prep (k_prep.hpp): a sort instead of the radix select
static double prep_px(const void *img, int dtype, size_t i)
{
    switch (dtype) {
    case KM_U8: return ((const uint8_t *)img)[i];
    case KM_U16: return ((const uint16_t *)img)[i];
    case KM_I16: return ((const int16_t *)img)[i];
    default: return ((const float *)img)[i];
    }
}
int kp_order_statistics(km_ctx *, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, int exclude, int n_q, const double *q, kp_state *st, bool)
{
    memset(st, 0, sizeof *st);
    std::vector<double> v;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const double p = prep_px(d_src, dtype, (size_t)y * ss + x);
            if (exclude ? std::isfinite(p) : p == p) v.push_back(p);
        }
    std::sort(v.begin(), v.end());
    st->n = (long long)v.size();
    for (int j = 0; j < n_q && !v.empty(); j++) {
        st->vi[j] = q[j] * (double)(v.size() - 1);
        const size_t lo = (size_t)st->vi[j];
        st->v0[j] = v[lo]; st->v1[j] = v[std::min(lo + 1, v.size() - 1)];
    }
    return KM_OK;
}
int kp_stretch(km_ctx *, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, double lo, double hi, uint8_t *d_dst, ptrdiff_t ds)
{
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const double t = hi > lo ? (prep_px(d_src, dtype, (size_t)y * ss + x) - lo) / (hi - lo) * 255.0 : 0.0;
            d_dst[(size_t)y * ds + x] = (uint8_t)(t > 0 ? std::min(t, 255.0) : 0.0);      // (NaN lands on 0)
        }
    return KM_OK;
}
int kp_clahe_geometry(km_ctx *c, int H, int W, double clip_limit, int tiles_x, int tiles_y, kp_clahe_geom *g)
{
    if (tiles_x < 1 || tiles_y < 1 || (long long)tiles_x * tiles_y * 256 > KP_CLAHE_MAX_LUT_BYTES) return km_fail(c, KM_E_ARG, "clahe: tile grid %d x %d", tiles_x, tiles_y);
    g->tiles_x = tiles_x; g->tiles_y = tiles_y; g->tile_w = (W + tiles_x - 1) / tiles_x; g->tile_h = (H + tiles_y - 1) / tiles_y;
    g->clip = clip_limit > 0.0 ? 1 : 0;
    g->lut_scale = 255.0f / (float)(g->tile_w * g->tile_h);
    return KM_OK;
}
// the tiles' histograms of the input, identity LUTs, the input through the LUT of its tile
int kp_clahe(km_ctx *, const uint8_t *d_src, int H, int W, ptrdiff_t ss, const kp_clahe_geom &g, unsigned *d_hist, uint8_t *d_lut, uint8_t *d_dst, ptrdiff_t ds)
{
    const size_t tiles = (size_t)g.tiles_x * g.tiles_y;
    for (size_t i = 0; i < tiles * 256; i++) { d_hist[i] = 0; d_lut[i] = (uint8_t)i; }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t tile = (size_t)(y / g.tile_h) * g.tiles_x + x / g.tile_w;
            const uint8_t v = d_src[(size_t)y * ss + x];
            d_hist[tile * 256 + v]++;
            d_dst[(size_t)y * ds + x] = d_lut[tile * 256 + v];
        }
    return KM_OK;
}

// ------------------------------------------------------------------ match (k_match.hpp): brute force on the packed rows
int kmt_state_reset(km_ctx *, kmt_state *st)
{
    memset(st, 0, sizeof *st);
    st->first_bad[0] = st->first_bad[1] = ~0ull;
    return KM_OK;
}
int kmt_pack(km_ctx *, const void *d_src, int dtype, int n, ptrdiff_t stride, void *d_dst, kmt_state *st, int which, kmt_packed *out)
{
    int8_t *rows = (int8_t *)d_dst;
    int *norm = (int *)(rows + (size_t)n * KMT_DIM);
    memset(d_dst, 0, kmt_packed_bytes(n));
    for (int i = 0; i < n; i++) {
        int s = 0;
        for (int k = 0; k < KMT_DIM; k++) {
            const size_t at = (size_t)i * stride + k;
            int v;
            if (dtype == KM_U8) v = ((const uint8_t *)d_src)[at];
            else {
                const float f = ((const float *)d_src)[at];
                const bool good = f >= 0.f && f <= 255.f && f == (float)(int)f;
                v = good ? (int)f : 0;
                if (!good) { st->n_bad[which]++; st->first_bad[which] = std::min(st->first_bad[which], (unsigned long long)i * KMT_DIM + k); }
            }
            rows[(size_t)i * KMT_DIM + k] = (int8_t)(v - 128);
            s += (v - 128) * (v - 128);
        }
        norm[i] = s;
    }
    out->rows = rows; out->norm = norm; out->n = n;
    return KM_OK;
}
int kmt_chunks(const km_ctx *, int, int n_t) { return std::min((n_t + KMT_TILE - 1) / KMT_TILE, KMT_MAX_CHUNKS); }
int kmt_knn(km_ctx *c, const kmt_packed &q, const kmt_packed &t, int k, unsigned long long *d_part, int *d_idx, float *d_dist)
{
    const size_t n_part = (size_t)q.n * kmt_chunks(c, q.n, t.n) * k;
    for (size_t i = 0; i < n_part; i++) d_part[i] = ~0ull;
    for (int i = 0; i < q.n; i++) {
        int best[2] = {-1, -1};
        long long d2[2] = {-1, -1};
        for (int j = 0; j < t.n; j++) {
            long long s = (long long)q.norm[i] + t.norm[j];
            for (int e = 0; e < KMT_DIM; e++) s -= 2 * (int)q.rows[(size_t)i * KMT_DIM + e] * (int)t.rows[(size_t)j * KMT_DIM + e];
            if (best[0] < 0 || s < d2[0]) { best[1] = best[0]; d2[1] = d2[0]; best[0] = j; d2[0] = s; }
            else if (best[1] < 0 || s < d2[1]) { best[1] = j; d2[1] = s; }
        }
        for (int r = 0; r < k; r++) { d_idx[(size_t)i * k + r] = best[r]; d_dist[(size_t)i * k + r] = best[r] < 0 ? INFINITY : sqrtf((float)d2[r]); }
    }
    return KM_OK;
}
int kmt_filter(km_ctx *, const int *d_fwd_idx, const float *d_fwd_dist, const int *d_bwd_idx, int n_mon, int n_ref, double ratio, unsigned *d_flag, int cap, int *d_qi,
               int *d_ti, float *d_dist, kmt_state *st)
{
    int lowe = 0, mutual = 0;
    volatile int last = d_bwd_idx[n_ref - 1];      // (the loop reads the backward matches only where a forward match points)
    (void)last;
    for (int i = 0; i < n_mon; i++) {
        const int j = d_fwd_idx[2 * i];
        const bool pass = j >= 0 && j < n_ref && (double)d_fwd_dist[2 * i] < ratio * (double)d_fwd_dist[2 * i + 1];
        const bool both = pass && d_bwd_idx[j] == i;
        d_flag[i] = both; d_flag[n_mon + i] = (unsigned)mutual;
        if (both && mutual < cap) { d_qi[mutual] = i; d_ti[mutual] = j; d_dist[mutual] = d_fwd_dist[2 * i]; }
        lowe += pass; mutual += both;
    }
    st->counts[0] = n_mon; st->counts[1] = lowe; st->counts[2] = mutual;
    return KM_OK;
}

// ------------------------------------------------------------------ align (k_align.hpp)
// the source at (min(y, sH - 1), min(x, sW - 1)): the identity on equal shapes, whatever the map
int ka_warp(km_ctx *, const void *d_src, int dtype, int sH, int sW, ptrdiff_t ss, void *d_dst, int dH, int dW, ptrdiff_t ds, int, const double Minv[9], double)
{
    volatile double m = 0;
    for (int i = 0; i < 9; i++) m = m + Minv[i];
    const size_t es = dtype == KM_U8 ? 1 : 4;
    for (int y = 0; y < sH; y++) { volatile uint8_t t = ((const uint8_t *)d_src)[((size_t)y * ss + sW - 1) * es + es - 1]; (void)t; }
    for (int y = 0; y < dH; y++)
        for (int x = 0; x < dW; x++)
            memcpy((char *)d_dst + ((size_t)y * ds + x) * es, (const char *)d_src + ((size_t)std::min(y, sH - 1) * ss + std::min(x, sW - 1)) * es, es);
    return KM_OK;
}
int ka_sobel_magnitude(km_ctx *, const uint8_t *d_src, int H, int W, ptrdiff_t ss, float *d_out, unsigned *d_max)
{
    float mx = 0.f;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) { const float v = d_src[(size_t)y * ss + x]; d_out[(size_t)y * W + x] = v; mx = std::max(mx, v); }
    memcpy(d_max, &mx, sizeof mx);
    return KM_OK;
}
int ka_gauss5(km_ctx *, const void *d_src, int dtype, int H, int W, ptrdiff_t ss, float *d_tmp, float *d_out)
{
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t at = (size_t)y * ss + x;
            const float v = dtype == KM_F32 ? ((const float *)d_src)[at] : dtype == KA_MASK ? (float)(((const uint8_t *)d_src)[at] > 0) : (float)((const uint8_t *)d_src)[at];
            d_tmp[(size_t)y * W + x] = v; d_out[(size_t)y * W + x] = v;
        }
    return KM_OK;
}
int ka_ecc_plane(km_ctx *, const float *d_blur, const float *d_pm_blur, int H, int W, float4 *d_plane)
{
    for (size_t i = 0; i < (size_t)H * W; i++) d_plane[i] = float4{d_blur[i], 0.f, 0.f, d_pm_blur ? d_pm_blur[i] : 1.f};
    return KM_OK;
}
// Sums of a well-conditioned system: the true first and second moments of template and input over their common rectangle, a Hessian
// of v = N var(input) on the diagonal but for H11 = 4 v and H01 = H10 = 1.5 v (positive definite, and its first column has its largest
// element below the diagonal, so lu_inv_f32 swaps rows) and small projections that shrink with the map's distance from the identity,
// so every iteration moves the map.  An input without variance gives the singular Hessian and an undefined correlation.
int ka_ecc_sums(km_ctx *, const float *d_tmpl, int hs, int ws, const float4 *d_plane, int hd, int wd, const float map[9], double *d_partials, double *d_sums)
{
    for (size_t i = 0; i < (size_t)KA_ECC_MAX_BLOCKS * KA_NSUM; i++) d_partials[i] = 0.0;
    double s[KA_NSUM] = {0};
    for (int y = 0; y < hs; y++) { volatile float t = d_tmpl[(size_t)y * ws + ws - 1]; (void)t; }
    for (int y = 0; y < hd; y++) { volatile float t = d_plane[(size_t)y * wd + wd - 1].w; (void)t; }
    for (int y = 0; y < std::min(hs, hd); y++)
        for (int x = 0; x < std::min(ws, wd); x++) {
            const double T = d_tmpl[(size_t)y * ws + x], I = d_plane[(size_t)y * wd + x].x, m = d_plane[(size_t)y * wd + x].w;
            s[0] += m; s[1] += m * I; s[2] += m * I * I; s[3] += m * T; s[4] += m * T * T; s[5] += m * T * I;
        }
    const double off = fabs(map[0] - 1.0) + fabs(map[1]) + fabs(map[2]) + fabs(map[3]) + fabs(map[4] - 1.0) + fabs(map[5]) + fabs(map[6]) + fabs(map[7]);
    const double var_n = s[0] ? s[2] - s[1] * s[1] / s[0] : 0.0;
    int q = 6;
    for (int k = 0; k < 8; k++)
        for (int l = k; l < 8; l++) s[q++] = k == l ? (k == 1 ? 4.0 : 1.0) * var_n : k == 0 && l == 1 ? 1.5 * var_n : 0.0;
    for (int k = 0; k < 8; k++) { s[42 + k] = 1e-3 * (k + 1) / (1.0 + off); s[50 + k] = 0.0; s[58 + k] = 5e-4 * (k + 1) / (1.0 + off); }
    memcpy(d_sums, s, sizeof s);
    return KM_OK;
}
int ka_count_nonzero(km_ctx *, const uint8_t *d_a, size_t n, unsigned long long *d_out)
{
    unsigned long long k = 0;
    for (size_t i = 0; i < n; i++) k += d_a[i] != 0;
    *d_out = k;
    return KM_OK;
}
