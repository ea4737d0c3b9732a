// The integer bin rule of the mutual-information kernel (csrc/mi_math.hpp) against floor(32 d / R), for EVERY range R = 1 .. 65535 and the
// samples d = 0, stride, 2 stride, ... and d = R (stride 1: every d, about 2^31 pairs).  The expected quotient and remainder are carried
// from one d to the next: no division in the inner loop.  tests/test_score_host.py builds this file twice (under the address and
// undefined-behaviour sanitizers, and plain -O2) and reads the one line it prints.
//   mi_magic_main <stride>  ->  "pairs <checked> bad <mismatches> first_R <R> first_d <d> max_M <largest constant>"
#include "mi_math.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    const long stride = strtol(argv[1], nullptr, 10);
    if (stride < 1 || stride > mi::R_MAX) return 2;
    unsigned long long pairs = 0, bad = 0;
    unsigned max_M = 0;
    long first_R = -1, first_d = -1;
    auto check = [&](int R, unsigned d, unsigned want, unsigned M, int sh) {
        const int q = mi::quotient(d, M, sh), b = mi::bin_of(q, R);
        const int want_bin = want < (unsigned)mi::BINS - 1 ? (int)want : mi::BINS - 1;
        pairs++;
        if ((unsigned)q != want || b != want_bin) {
            if (!bad) { first_R = R; first_d = (long)d; }
            bad++;
        }
    };
    for (int R = 1; R <= mi::R_MAX; R++) {
        unsigned M;
        int sh;
        mi::magic(R, M, sh);
        if (M > max_M) max_M = M;
        if (sh < 16 || sh > 32) { bad++; if (first_R < 0) first_R = R; continue; }
        // 32 stride = step_q R + step_r: per range, not per sample
        const unsigned step_q = (unsigned)(32 * stride / R), step_r = (unsigned)(32 * stride % R);
        unsigned q = 0, r = 0;
        for (unsigned d = 0; d <= (unsigned)R; d += (unsigned)stride) {
            check(R, d, q, M, sh);
            q += step_q; r += step_r;
            if (r >= (unsigned)R) { r -= (unsigned)R; q++; }
        }
        check(R, (unsigned)R, 32u, M, sh);
    }
    // a constant chip
    unsigned M0;
    int sh0;
    mi::magic(0, M0, sh0);
    if (M0 != 0u || mi::bin_of(mi::quotient(0u, M0, sh0), 0) != mi::BINS / 2) { bad++; if (first_R < 0) first_R = 0; }
    printf("pairs %llu bad %llu first_R %ld first_d %ld max_M %u\n", pairs, bad, first_R, first_d, max_M);
    return bad ? 1 : 0;
}
