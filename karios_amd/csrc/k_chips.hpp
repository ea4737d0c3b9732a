// k_chips.hip: the device half of ChipService.generate_chips (karios/report/chip_service.py): the key-point selection of
// CenterAndQuarterCellPointSelector (:46-306) and, per selected row, the 57 x 57 chips of both rasters, their uint8 stretch and their
// Laplacian (:544-648).  The arithmetic is chips_math.hpp's; tests/chips_restatement.py is the definition.
// A compiler that is not hipcc (the host sanitizer build of the API files, the stand-alone program of tests/test_chips_host.py) gets
// the launchers defined here, as plain loops over the same header: device memory is host memory there, `c` is not touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/karios_hip.h"
#include "chips_math.hpp"
#include "lap_coef.hpp"

struct kch_images {
    const void *ref, *mon;
    int dtype, Href, Wref, Hmon, Wmon;
    ptrdiff_t sref, smon;          // elements between rows
};
struct kch_rows {
    const float *x0, *y0, *dx, *dy;
    int n;
};
// the taps of both images' kernels, each centred at its own radius; ksize 0: no Laplacian of that image
struct kch_taps {
    int R[2];
    lap_coef cf;
};
static inline bool kch_make_taps(int ksize_ref, int ksize_mon, kch_taps &t)
{
    const int ks[2] = {ksize_ref, ksize_mon};
    for (int i = 0; i < 2; i++) {
        t.R[i] = ks[i] > 1 ? ks[i] / 2 : 1;
        if (!ch::ksize_ok(ks[i])) return false;
        if (ks[i] == 0) { for (int j = 0; j < 11; j++) t.cf.kd[i][j] = t.cf.ks[i][j] = 0; }
        else if (!fill_coef(ks[i], t.R[i], t.cf.kd[i], t.cf.ks[i])) return false;
    }
    return true;
}
static inline size_t kch_slots(const ch::grid &g) { return (size_t)g.rows * g.cols * ch::PICKS; }

// rows with score >= g.thr -> per cell the centre pick and the four quarter picks (row index or -1) in d_slots[kch_slots(g)], then in
// cell / pick order without the empty ones -> d_index[kch_slots(g)], *d_count
int kch_select(km_ctx *c, const float *d_x0, const float *d_y0, const float *d_score, int n, const ch::grid &g, int32_t *d_slots, int32_t *d_index,
               int32_t *d_count);
// per row: ok and the four window centres; the raw, uint8 and (ksize != 0) Laplacian chips of both images, zero where ok is 0
int kch_chips(km_ctx *c, const kch_images &I, const kch_rows &R, int ksize_ref, int ksize_mon, const km_chip_outputs &out);

#if !defined(__HIPCC__)
#include <algorithm>
#include <vector>

inline int kch_select(km_ctx *, const float *d_x0, const float *d_y0, const float *d_score, int n, const ch::grid &g, int32_t *d_slots,
                      int32_t *d_index, int32_t *d_count)
{
    const int cells = g.rows * g.cols;
    std::vector<std::vector<int>> members((size_t)cells);
    for (int i = 0; i < n; i++)
        if (ch::passes(d_score[i], g.thr)) members[(size_t)ch::cell_of(d_x0[i], d_y0[i], g)].push_back(i);
    for (int cell = 0; cell < cells; cell++) {
        int32_t *slot = d_slots + (size_t)cell * ch::PICKS;
        for (int k = 0; k < ch::PICKS; k++) slot[k] = -1;
        const std::vector<int> &rows = members[(size_t)cell];
        if (rows.empty()) continue;
        const ch::cell_box b = ch::make_box(g, cell);
        ch::pick best = ch::no_pick();
        for (int i : rows) {
            const ch::pick p = ch::make_pick(ch::dist(d_x0[i], d_y0[i], b), d_score[i], (uint32_t)i);
            if (ch::better(p, best)) best = p;
        }
        slot[0] = (int32_t)best.row;
        for (int q = 0; q < 4; q++) {
            std::vector<uint32_t> keys;
            for (int i : rows)
                if ((uint32_t)i != best.row && (ch::quarters(d_x0[i], d_y0[i], b) >> q & 1u)) keys.push_back(ac::order_key(ch::dist(d_x0[i], d_y0[i], b)));
            if (keys.empty()) continue;
            std::sort(keys.begin(), keys.end());
            const int m = (int)keys.size();
            const float med = ch::median_of(keys[(size_t)(m - 1) / 2], keys[(size_t)m / 2], m);
            ch::pick bq = ch::no_pick();
            for (int i : rows) {
                if ((uint32_t)i == best.row || !(ch::quarters(d_x0[i], d_y0[i], b) >> q & 1u)) continue;
                const ch::pick p = ch::make_pick(ch::dev(ch::dist(d_x0[i], d_y0[i], b), med), d_score[i], (uint32_t)i);
                if (ch::better(p, bq)) bq = p;
            }
            slot[1 + q] = (int32_t)bq.row;
        }
    }
    int count = 0;
    for (size_t k = 0; k < kch_slots(g); k++)
        if (d_slots[k] >= 0) d_index[count++] = d_slots[k];
    *d_count = count;
    return KM_OK;
}

// _to_uint8 of one value (k_pixel.hpp stretch_u8 in plain C++): integers in float64, float32 in float32, truncation, NaN -> 0
template <typename T> static inline unsigned kch_stretch(T v, double mn, double range, bool degenerate)
{
    if (sizeof(T) == 1) return (unsigned)v;
    if (degenerate) return 0u;
    const double t = (((double)v - mn) / range) * 255.0;
    return (unsigned)(int)t;
}
template <> inline unsigned kch_stretch<float>(float v, double mn, double range, bool degenerate)
{
    if (degenerate) return 0u;
    const float t = ((v - (float)mn) / (float)range) * 255.0f;
    return t != t ? 0u : (unsigned)(int)t;
}

template <typename T>
static inline void kch_chip_host(const T *img, ptrdiff_t stride, int X, int Y, int R, const int *kd, const int *ks, T *raw, uint8_t *u8, uint8_t *lap)
{
    const T *src = img + (ptrdiff_t)(Y - ch::MARGIN) * stride + (X - ch::MARGIN);
    double mn = INFINITY, mx = -INFINITY;
    for (int y = 0; y < ch::CHIP; y++)
        for (int x = 0; x < ch::CHIP; x++) {
            const T v = src[(ptrdiff_t)y * stride + x];
            raw[y * ch::CHIP + x] = v;
            const double d = (double)v;
            if (d != d) continue;
            mn = d < mn ? d : mn; mx = d > mx ? d : mx;
        }
    const bool degenerate = !(mx > mn);
    for (int p = 0; p < ch::PIXELS; p++) u8[p] = (uint8_t)kch_stretch<T>(raw[p], mn, mx - mn, degenerate);
    if (!lap) return;
    std::vector<int> hd(ch::PIXELS), hs(ch::PIXELS);
    for (int y = 0; y < ch::CHIP; y++)
        for (int x = 0; x < ch::CHIP; x++) {
            int d = 0, s = 0;
            for (int j = 0; j <= 2 * R; j++) { const int v = u8[y * ch::CHIP + ch::reflect(x + j - R)]; d += kd[j] * v; s += ks[j] * v; }
            hd[(size_t)(y * ch::CHIP + x)] = d; hs[(size_t)(y * ch::CHIP + x)] = s;
        }
    for (int y = 0; y < ch::CHIP; y++)
        for (int x = 0; x < ch::CHIP; x++) {
            int acc = 0;
            for (int j = 0; j <= 2 * R; j++) { const size_t at = (size_t)(ch::reflect(y + j - R) * ch::CHIP + x); acc += ks[j] * hd[at] + kd[j] * hs[at]; }
            lap[y * ch::CHIP + x] = (uint8_t)(acc < 0 ? 0 : acc > 255 ? 255 : acc);
        }
}

template <typename T>
static inline int kch_chips_host(const kch_images &I, const kch_rows &R, const kch_taps &t, bool lap_ref, bool lap_mon, const km_chip_outputs &out)
{
    for (int i = 0; i < R.n; i++) {
        const ch::window w = ch::make_window(R.x0[i], R.y0[i], R.dx[i], R.dy[i], I.Href, I.Wref, I.Hmon, I.Wmon);
        out.ok[i] = (uint8_t)w.ok;
        int32_t *win = out.windows + 4 * (size_t)i;
        win[0] = w.X0; win[1] = w.Y0; win[2] = w.X1; win[3] = w.Y1;
        const size_t at = (size_t)i * ch::PIXELS;
        T *raw[2] = {(T *)out.ref_raw + at, (T *)out.mon_raw + at};
        uint8_t *u8[2] = {out.ref_u8 + at, out.mon_u8 + at};
        uint8_t *lap[2] = {lap_ref ? out.ref_lap + at : nullptr, lap_mon ? out.mon_lap + at : nullptr};
        for (int k = 0; k < 2; k++) {
            if (!w.ok) {
                for (int p = 0; p < ch::PIXELS; p++) { raw[k][p] = (T)0; u8[k][p] = 0; if (lap[k]) lap[k][p] = 0; }
                continue;
            }
            kch_chip_host<T>((const T *)(k ? I.mon : I.ref), k ? I.smon : I.sref, k ? w.X1 : w.X0, k ? w.Y1 : w.Y0, t.R[k], t.cf.kd[k], t.cf.ks[k],
                             raw[k], u8[k], lap[k]);
        }
    }
    return KM_OK;
}

inline int kch_chips(km_ctx *, const kch_images &I, const kch_rows &R, int ksize_ref, int ksize_mon, const km_chip_outputs &out)
{
    kch_taps t;
    if (!kch_make_taps(ksize_ref, ksize_mon, t)) return KM_E_ARG;
    const bool lr = ksize_ref != 0, lm = ksize_mon != 0;
    switch (I.dtype) {
    case KM_U8: return kch_chips_host<uint8_t>(I, R, t, lr, lm, out);
    case KM_U16: return kch_chips_host<uint16_t>(I, R, t, lr, lm, out);
    case KM_I16: return kch_chips_host<int16_t>(I, R, t, lr, lm, out);
    case KM_F32: return kch_chips_host<float>(I, R, t, lr, lm, out);
    default: return KM_E_ARG;
    }
}
#endif
