// K7, the launch rules of k_lk.hip and k_lk2.hip: the kernel instance of a window, what is served at all, the kernels' argument block
#pragma once
#include "lk_device.hpp"

// ---- window -> launch shape.  NR = runs of LK_RUN pixels per lane (win rows of ceil(win / LK_RUN) runs over 64 lanes): winSize .. 16
// -> 1, .. 25 -> 2, .. 30 -> 3, .. 35 -> 4, .. 40 -> 5.  MAXIT = dwords a lane keeps in flight per patch while it is staged
// (stage_patch_issue): the smallest count that holds the patch of the class's widest window, so EVERY served window has the
// all-loads-in-flight staging path and takes the byte path only at the image border.  WIN = the window as a compile-time constant
// (the reference's matching_winsize 25 has kernels of its own), 0 = read from the arguments.
#define LK_WIN_MIN 3
#define LK_WIN_MAX 40
struct lk_shape { int nr, maxit, win; };
constexpr int lk2_maxit(int nr) { return nr == 1 ? 3 : nr == 2 ? 4 : nr == 3 ? 6 : nr == 4 ? 8 : 9; }
constexpr lk_shape lk_shape_of(int win)
{
    const int runs = win * ((win + LK_RUN - 1) / LK_RUN), nr = (runs + 63) / 64;
    return {nr, lk2_maxit(nr), win == 25 ? 25 : 0};
}
constexpr bool lk_window_served(int win) { return win >= LK_WIN_MIN && win <= LK_WIN_MAX; }

// What the table promises, for every served window: 1 .. 5 runs per lane (the instances that exist); the second form's (win + 7)^2
// patch passes the size half of lk_patch_inside with MAXIT slots (<= 64 MAXIT dwords, < 1024, <= 64 columns); the first form's
// 2 NR slots hold its (win + 3)^2 template patch - and its (win + 7)^2 search patch for every window but 15 and 16, whose 132 / 138
// dwords exceed the 128 of NR = 1: there the first form stages the search patch through the byte path, inside the image as at its
// border (slower, the same bytes).  The LDS bound stands beside lk2_geo (k_lk2.hip).
constexpr bool lk_table_holds()
{
    for (int win = LK_WIN_MIN; win <= LK_WIN_MAX; win++) {
        const lk_shape s = lk_shape_of(win);
        const int ps = win + 7;
        if (s.nr < 1 || s.nr > 5 || (s.win != 0 && s.win != win) || !lk_patch_fits(ps, ps, s.maxit)) return false;
        if (!lk_patch_fits(win + 3, win + 3, 2 * s.nr) || lk_patch_fits(ps, ps, 2 * s.nr) == (win == 15 || win == 16)) return false;
    }
    return true;
}
static_assert(lk_table_holds(), "a window of 3..40 without a kernel instance or without the all-loads-in-flight staging path");

// ---- which calls are served
inline int lk_check_window(km_ctx *c, int win)
{
    if (win < LK_WIN_MIN) return km_fail(c, KM_E_ARG, "winSize %d must be > 2", win);
    if (win > LK_WIN_MAX) return km_fail(c, KM_E_UNSUPPORTED, "winSize %d (supported 3..40)", win);
    return KM_OK;
}
// the second form: switched on, two-level pyramids, whole levels resident (the first form serves row bands and other pyramids)
inline bool lk2_serves(const km_ctx *c, const km_pyr &A, const km_pyr &B) { return c->opt_lk2 && A.levels == 1 && B.levels == 1 && A.Hres[0] == 0 && B.Hres[0] == 0; }

// ---- the argument block of one tracker run (a table of runs: fill the shared part once, then set pyramids, points and outputs per entry)
inline lk_args lk_fill_args(const km_ctx *c, const km_pyr &A, const km_pyr &B, const float *d_pts_in, const int *d_n, int n_max, int win,
                            int max_count, double epsilon, bool backward, float *d_p1, float *d_p0r, int *d_left_band)
{
    lk_args g;
    g.A = A; g.B = B; g.pts_in = d_pts_in; g.d_n = d_n; g.n_max = n_max; g.win = win; g.backward = backward ? 1 : 0;
    g.max_count = max_count < 0 ? 0 : max_count > 100 ? 100 : max_count;
    const double e = epsilon < 0 ? 0 : epsilon > 10 ? 10 : epsilon;
    g.epsilon = e * e;
    g.general_templates = km_dev_env("KARIOS_HIP_LK_GENERAL") ? 1 : 0; g.lk_reuse = c->opt_lk_reuse ? 1 : 0;
    g.p1 = d_p1; g.p0r = d_p0r; g.left_band = d_left_band;
    return g;
}

// k_lk2.hip: the plain launch of the second form (kl_track chooses the form)
int lk2_track(km_ctx *c, const lk_args &g);
