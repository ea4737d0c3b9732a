// k_ce.hip: the numbers of the circular-error figure (karios/report/circular_error_plot.py) on resident columns - the scaled sample with
// its extremes, both axis histograms, the 10 x 10 density, the spline's value per point, the drawing order and the sorted radial errors.
// The arithmetic is ce_math.hpp's and accuracy_math.hpp's; tests/ce_figure_restatement.py is the definition.
// A compiler that is not hipcc (the host sanitizer build of the API files, the stand-alone program of tests/test_ce_figure_host.py) gets
// the launchers defined here, as plain loops over the same headers: device memory is host memory there, `c` is not touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/karios_hip.h"
#include "ce_math.hpp"
#include "k_accuracy.hpp"

// device-side state of one figure, kept between the stages of km_ce_figure
struct kce_state {
    ka_state st;              // the sample (ka_compact)
    ka_state scaled;          // n, and sum / mean / std of x, y and the radial error of the scaled sample (ka_block_sums, ka_finish)
    uint32_t ext[8];          // order keys, all kept as maxima: ~min and max of dx, of +-dy, of x, of y
    km_ce_block block;        // what stage KM_CE_SAMPLE hands to the host
    km_ce_tail tail;          // ... and stage KM_CE_CURVES
};
struct kce_axis {
    const float *edges;       // bins + 1, numpy's linspace
    unsigned *count;          // bins, zeroed by the caller
    int bins;                 // 0: this axis is not counted
};
struct kce_spline {
    double tx[ce::KNOTS], ty[ce::KNOTS], c[ce::GRID * ce::GRID];
    float box[4];             // cx[0], cx[-1], cy[0], cy[-1]
};
AC_HD static inline uint32_t kce_min_key(float v) { return ~ac::order_key(v); }
AC_HD static inline float kce_min_value(uint32_t k) { return ac::order_value(~k); }
AC_HD static inline void kce_fill_block(kce_state *s)
{
    km_ce_block &b = s->block;
    b.sample = s->st.n; b.n_nan = s->st.n_nan;
    for (int k = 0; k < 8; k++) b.ext[k] = (k & 1) ? ac::order_value(s->ext[k]) : kce_min_value(s->ext[k]);
    b.mu_x = s->scaled.mean[0]; b.sigma_x = s->scaled.std[0]; b.mu_y = s->scaled.mean[1]; b.sigma_y = s->scaled.std[1];
    b.pad[0] = b.pad[1] = 0.0f;
}
// the two order statistics of the sorted radial errors for 0.9 and 0.95 (compute_percentile's ranks), from keys[0 .. n)
AC_HD static inline void kce_fill_tail(kce_state *s, const unsigned long long *radial_keys, int n_outside)
{
    const double pc[2] = {0.9, 0.95};
    for (int k = 0; k < 2; k++) {
        long long lo, hi;
        const bool ok = s->st.n > 0 && ac::ce_ranks(pc[k], s->st.n, lo, hi);
        s->tail.order[2 * k] = ok ? ac::order_value(ce::key_value(radial_keys[lo])) : ac::bits_f32(0x7fc00000u);
        s->tail.order[2 * k + 1] = ok ? ac::order_value(ce::key_value(radial_keys[hi])) : ac::bits_f32(0x7fc00000u);
    }
    s->tail.n_outside = n_outside;
    s->tail.pad[0] = s->tail.pad[1] = s->tail.pad[2] = 0;
}

#if defined(__HIPCC__)
// the sample's columns x | +-y | c (ka_compact, n_max each) -> d_scaled = x res | y res | radial error (n_max each); the extremes of the
// unscaled and the scaled columns into s->ext; s->scaled starts with the sample's size
int kce_scale(km_ctx *c, const float *d_cols, int n_max, float res, float *d_scaled, kce_state *s);
// s->block from the extremes and the sums
int kce_block(km_ctx *c, kce_state *s);
// both axis histograms in one launch
int kce_axis_hist(km_ctx *c, const float *d_scaled, int n_max, const kce_state *s, kce_axis x, kce_axis y);
// the 10 x 10 counts (d_count zeroed by the caller) on d_edges = 11 edges of x | 11 edges of y
int kce_grid_hist(km_ctx *c, const float *d_scaled, int n_max, const kce_state *s, const float *d_edges, unsigned *d_count);
// the spline's value of every row -> d_z[n_max]; d_keys[2 n_max]: the sort keys of the density, then of the radial error
int kce_density_keys(km_ctx *c, const float *d_scaled, int n_max, const kce_state *s, const kce_spline *d_sp, float *d_z, unsigned long long *d_keys);
// sorts d_keys (d_keys_b: the sort's second buffer) and gathers x, y, z in drawing order and the ascending radial errors; s->tail
int kce_sort_gather(km_ctx *c, const float *d_scaled, const float *d_z, unsigned long long *d_keys, unsigned long long *d_keys_b, int n_max, kce_state *s,
                    float *d_sx, float *d_sy, float *d_sz, float *d_radial);
#else
#include <algorithm>

static inline int kce_scale(km_ctx *, const float *d_cols, int n_max, float res, float *d_scaled, kce_state *s)
{
    const int n = s->st.n;
    for (int k = 0; k < 8; k++) s->ext[k] = 0u;
    for (int i = 0; i < n; i++) {
        const float dx = d_cols[i], dy = d_cols[(size_t)n_max + i];
        const float v[4] = {dx, dy, dx * res, dy * res};
        d_scaled[i] = v[2];
        d_scaled[(size_t)n_max + i] = v[3];
        d_scaled[2 * (size_t)n_max + i] = ac::radial(dx, dy, res);
        for (int k = 0; k < 4; k++) {
            s->ext[2 * k] = std::max(s->ext[2 * k], kce_min_key(v[k]));
            s->ext[2 * k + 1] = std::max(s->ext[2 * k + 1], ac::order_key(v[k]));
        }
    }
    s->scaled = ka_state();
    s->scaled.n = n; s->scaled.n_nan = s->st.n_nan;
    return KM_OK;
}
static inline int kce_block(km_ctx *, kce_state *s) { kce_fill_block(s); return KM_OK; }
static inline int kce_axis_hist(km_ctx *, const float *d_scaled, int n_max, const kce_state *s, kce_axis x, kce_axis y)
{
    const kce_axis ax[2] = {x, y};
    for (int a = 0; a < 2; a++) {
        if (!ax[a].bins) continue;
        const float first = ax[a].edges[0], denom = ax[a].edges[ax[a].bins] - first;
        for (int i = 0; i < s->st.n; i++) ax[a].count[ce::axis_bin(d_scaled[(size_t)a * n_max + i], first, denom, ax[a].bins, ax[a].edges)]++;
    }
    return KM_OK;
}
static inline int kce_grid_hist(km_ctx *, const float *d_scaled, int n_max, const kce_state *s, const float *d_edges, unsigned *d_count)
{
    for (int i = 0; i < s->st.n; i++) {
        const int bx = ce::grid_bin(d_scaled[i], d_edges), by = ce::grid_bin(d_scaled[(size_t)n_max + i], d_edges + ce::GRID + 1);
        if (bx >= 0 && bx < ce::GRID && by >= 0 && by < ce::GRID) d_count[bx * ce::GRID + by]++;
    }
    return KM_OK;
}
static inline int kce_density_keys(km_ctx *, const float *d_scaled, int n_max, const kce_state *s, const kce_spline *d_sp, float *d_z,
                                   unsigned long long *d_keys)
{
    for (int i = 0; i < n_max; i++) {
        if (i >= s->st.n) { d_keys[i] = ce::pad_key(0, (uint32_t)i); d_keys[(size_t)n_max + i] = ce::pad_key(1, (uint32_t)i); continue; }
        d_z[i] = ce::density(d_sp->tx, d_sp->ty, d_sp->c, d_sp->box, d_scaled[i], d_scaled[(size_t)n_max + i]);
        d_keys[i] = ce::sort_key(0, ce::z_key(d_z[i]), (uint32_t)i);
        d_keys[(size_t)n_max + i] = ce::sort_key(1, ac::order_key(d_scaled[2 * (size_t)n_max + i]), (uint32_t)i);
    }
    return KM_OK;
}
static inline int kce_sort_gather(km_ctx *, const float *d_scaled, const float *d_z, unsigned long long *d_keys, unsigned long long *, int n_max,
                                  kce_state *s, float *d_sx, float *d_sy, float *d_sz, float *d_radial)
{
    const int n = s->st.n;
    std::sort(d_keys, d_keys + 2 * (size_t)n_max);
    int outside = 0;
    for (int j = 0; j < n; j++) {
        const uint32_t row = ce::key_row(d_keys[j]);
        d_sx[j] = d_scaled[row]; d_sy[j] = d_scaled[(size_t)n_max + row]; d_sz[j] = d_z[row];
        outside += ac::is_nan(d_z[row]) ? 1 : 0;
        d_radial[j] = ac::order_value(ce::key_value(d_keys[(size_t)n_max + j]));
    }
    kce_fill_tail(s, d_keys + n_max, outside);
    return KM_OK;
}
#endif
