// cv2.findHomography(src, dst, cv2.RANSAC, threshold, maxIters=, confidence=) of the global align step
// (karios/matcher/global_align.py:223-230).  tests/ransac_restatement.py is the definition, ransac_math.hpp its C++ form.
//
// The loop of RANSACPointSetRegistrator::run is sequential only in its bookkeeping: the subset of iteration i depends on the points
// alone (the random stream and checkSubset), never on a score.  So the host draws the subsets of a batch of iterations, the device
// solves and scores them all (k_ransac.hip), and the host replays `goodCount > max(best, 3)` and the niters update over the batch's
// counts in iteration order, stopping at the first iteration >= niters.  What was evaluated beyond the stop is thrown away: winner,
// count and the iteration at which the loop ended are the sequential loop's by construction.
//
// Batch schedule: the batches end at B0, 2 B0, 4 B0, ... iterations (the total doubles), never past the current niters.  A batch is
// only launched when the sequential loop would enter it, so evaluated <= max(B0, 2 * iterations the sequential loop runs).
// B0: the scoring kernel gives a wave 256 pairs x 16 iterations at the least, so B0 = 16 * ceil(4 n_cu / ceil(n / 256)) is the
// first batch that hands every SIMD of the chip a wave; at least 64, at most max_iters ("ransac_first_batch" overrides it).
#include "api_internal.hpp"
#include "k_ransac.hpp"
#include "ransac_math.hpp"

#include <string.h>
#include <new>
#include <vector>

namespace {

enum { ST_RAN = 0, ST_EVALUATED, ST_BEST_ITER, ST_BEST_COUNT, ST_LM_ITERS, ST_FIRST_BATCH, ST_BATCHES, ST_WORDS = 8 };
const int MAX_BATCH = 1 << 19;   // iterations of one launch (the scoring grid's second dimension stays below 65 536)

int ransac_args(km_ctx *c, const void *src, ptrdiff_t ss, const void *dst, ptrdiff_t sd, int n, int max_iters, double confidence, const double *H,
                const void *mask, const int *found)
{
    if (n < 4) return km_fail(c, KM_E_ARG, "find_homography_ransac: %d point pairs (at least 4)", n);
    if (!src || !dst || !H || !mask || !found) return km_fail(c, KM_E_ARG, "find_homography_ransac: null argument");
    if (ss < 2 || sd < 2) return km_fail(c, KM_E_ARG, "find_homography_ransac: row strides %td, %td < 2", ss, sd);
    if (!(confidence > 0 && confidence < 1)) return km_fail(c, KM_E_ARG, "find_homography_ransac: confidence %g outside (0, 1)", confidence);
    if (max_iters > (1 << 24)) return km_fail(c, KM_E_ARG, "find_homography_ransac: max_iters %d above %d", max_iters, 1 << 24);
    return KM_OK;
}

int first_batch(const km_ctx *c, int n, int niters)
{
    long long b0 = c->opt_ransac_first_batch;
    if (b0 <= 0) {
        const long long waves = ((long long)n + KRS_WAVE_PAIRS - 1) / KRS_WAVE_PAIRS;
        b0 = KRS_HC_SMALL * ((4ll * c->n_cu + waves - 1) / waves);
        if (b0 < 64) b0 = 64;
    }
    if (b0 > niters) b0 = niters;
    if (b0 > MAX_BATCH) b0 = MAX_BATCH;
    return (int)b0;
}

// d_src / d_dst on the device; d_mask on the device (n bytes); h_mask: host copy of the mask, or null.  H, found, stats, dbg_*: host.
int ransac_dev(km_ctx *c, const float *d_src, ptrdiff_t ss, const float *d_dst, ptrdiff_t sd, int n, double threshold, int max_iters, double confidence,
               double *H, uint8_t *d_mask, uint8_t *h_mask, int *found, int64_t *stats, int *dbg_counts, int *dbg_valid)
{
    int rc;
    int64_t st[ST_WORDS] = {0, 0, -1, 0, 0, 0, 0, 0};
    *found = 0;
    for (int k = 0; k < 9; k++) H[k] = 0;
    if (stats) memcpy(stats, st, sizeof st);
    if (threshold <= 0) threshold = 3;   // findHomography's defaultRANSACReprojThreshold
    const float thr = rs::threshold_sq(threshold);

    float *d_pairs = (float *)km_ws(c, WS_RS_PAIRS, (size_t)n * 4 * sizeof(float));
    if (!d_pairs) return KM_E_NOMEM;
    if ((rc = krs_pack(c, d_src, ss, d_dst, sd, n, d_pairs))) return rc;
    std::vector<float> pairs((size_t)n * 4);
    KM_D2H(c, pairs.data(), d_pairs, pairs.size() * sizeof(float));
    KM_FLUSH(c);
    for (size_t i = 0; i < pairs.size(); i++)
        if (!(fabsf(pairs[i]) <= FLT_MAX))
            return km_fail(c, KM_E_ARG, "find_homography_ransac: %s point %zu has a coordinate that is not finite (%s)", (i & 2) ? "dst" : "src", i / 4,
                           (i & 1) ? "y" : "x");

    std::vector<uint8_t> mask_store;
    if (!h_mask) { mask_store.resize((size_t)n); h_mask = mask_store.data(); }
    std::vector<float> M((size_t)n * 2), m((size_t)n * 2);
    auto finish = [&](int ok, int fill) -> int {
        memset(h_mask, fill, (size_t)n);
        KM_HIP(c, hipMemsetAsync(d_mask, fill, (size_t)n, c->stream));
        KM_HIP(c, hipStreamSynchronize(c->stream));
        *found = ok;
        if (!ok) for (int k = 0; k < 9; k++) H[k] = 0;
        if (stats) memcpy(stats, st, sizeof st);
        return KM_OK;
    };

    if (n == 4) {   // one runKernel, a mask of ones
        for (int i = 0; i < 4; i++) { M[2 * i] = pairs[4 * i]; M[2 * i + 1] = pairs[4 * i + 1]; m[2 * i] = pairs[4 * i + 2]; m[2 * i + 1] = pairs[4 * i + 3]; }
        const int ok = rs::dlt(M.data(), m.data(), 4, H);
        return finish(ok, ok ? 1 : 0);
    }

    rs::Replay r;
    rs::replay_init(r, max_iters);
    const int cap = r.niters;
    int *d_idx = (int *)km_ws(c, WS_RS_IDX, (size_t)cap * 4 * sizeof(int));
    double *d_H64 = (double *)km_ws(c, WS_RS_H64, (size_t)cap * 9 * sizeof(double));
    float *d_Hf = (float *)km_ws(c, WS_RS_HF, (size_t)cap * KRS_HSTRIDE * sizeof(float));
    int *d_count = (int *)km_ws(c, WS_RS_COUNT, ((size_t)cap * 2 + 4) * sizeof(int));
    if (!d_idx || !d_H64 || !d_Hf || !d_count) return KM_E_NOMEM;
    int *d_valid = d_count + cap, *d_total = d_valid + cap;

    const int b0 = first_batch(c, n, r.niters);
    st[ST_FIRST_BATCH] = b0;
    uint64_t state = ~(uint64_t)0;
    std::vector<int> idx, counts, valid;
    int done = 0;         // iterations evaluated so far
    bool exhausted = false;
    while (r.iter < r.niters && !exhausted) {
        long long hi = done == 0 ? b0 : 2ll * done;
        if (hi > r.niters) hi = r.niters;
        if (hi > done + MAX_BATCH) hi = done + MAX_BATCH;
        idx.resize((size_t)(hi - done) * 4);
        int got = 0;
        for (; done + got < hi; got++)
            if (!rs::get_subset(pairs.data(), n, state, &idx[(size_t)got * 4])) { exhausted = true; break; }   // the loop ends at this iteration
        if (got == 0) break;
        counts.resize((size_t)got); valid.resize((size_t)got);
        if ((rc = km_h2d_small(c, d_idx + (size_t)done * 4, idx.data(), (size_t)got * 4 * sizeof(int))) ||
            (rc = krs_solve(c, d_pairs, n, d_idx, done, got, d_H64, d_Hf, d_valid, d_count)) ||
            (rc = krs_score(c, d_pairs, n, d_Hf, done, got, thr, d_count)))
            return rc;
        KM_D2H(c, counts.data(), d_count + done, (size_t)got * sizeof(int));
        KM_D2H(c, valid.data(), d_valid + done, (size_t)got * sizeof(int));
        KM_FLUSH(c);
        if (dbg_counts) memcpy(dbg_counts + done, counts.data(), (size_t)got * sizeof(int));
        if (dbg_valid) memcpy(dbg_valid + done, valid.data(), (size_t)got * sizeof(int));
        rs::replay(r, done + got, counts.data(), valid.data(), n, confidence);
        done += got;
        st[ST_BATCHES]++;
    }
    st[ST_RAN] = r.iter;
    st[ST_EVALUATED] = done;
    if (r.max_good <= 0) return finish(0, 0);

    st[ST_BEST_ITER] = r.best_iter;
    st[ST_BEST_COUNT] = r.max_good;
    int total = 0;
    float Hf[9];
    KM_D2H(c, H, d_H64 + (size_t)r.best_iter * 9, 9 * sizeof(double));
    KM_FLUSH(c);
    for (int k = 0; k < 9; k++) Hf[k] = (float)H[k];
    if ((rc = krs_mask(c, d_pairs, n, Hf, thr, d_mask, d_total))) return rc;
    KM_D2H(c, h_mask, d_mask, (size_t)n);
    KM_D2H(c, &total, d_total, sizeof(int));
    KM_FLUSH(c);
    if (total != r.max_good) return km_fail(c, KM_E_INTERNAL, "find_homography_ransac: the winner's mask holds %d inliers, its count was %d", total, r.max_good);
    // compress to the inliers, runKernel on all of them, Levenberg-Marquardt on the 8 free parameters: sequential float64 on the host
    size_t k = 0;
    for (int i = 0; i < n; i++)
        if (h_mask[i]) { M[2 * k] = pairs[4 * (size_t)i]; M[2 * k + 1] = pairs[4 * (size_t)i + 1]; m[2 * k] = pairs[4 * (size_t)i + 2]; m[2 * k + 1] = pairs[4 * (size_t)i + 3]; k++; }
    st[ST_LM_ITERS] = rs::refine_on_inliers(M.data(), m.data(), (int)k, H);
    *found = 1;
    if (stats) memcpy(stats, st, sizeof st);
    return KM_OK;
}

}  // namespace

extern "C" {

int km_find_homography_ransac_dev(km_ctx *c, const float *d_src, ptrdiff_t stride_src, const float *d_dst, ptrdiff_t stride_dst, int n, double threshold,
                                  int max_iters, double confidence, double *H, uint8_t *d_mask, int *found, int64_t *stats, int *iter_counts, int *iter_valid)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = ransac_args(c, d_src, stride_src, d_dst, stride_dst, n, max_iters, confidence, H, d_mask, found))) return rc;
    try {
        return ransac_dev(c, d_src, stride_src, d_dst, stride_dst, n, threshold, max_iters, confidence, H, d_mask, nullptr, found, stats, iter_counts,
                          iter_valid);
    } catch (const std::bad_alloc &) {   // the host copies of the pairs: nothing throws across the boundary
        return km_fail(c, KM_E_NOMEM, "find_homography_ransac: no host memory for %d pairs", n);
    }
}

int km_find_homography_ransac(km_ctx *c, const float *src, ptrdiff_t stride_src, const float *dst, ptrdiff_t stride_dst, int n, double threshold, int max_iters,
                              double confidence, double *H, uint8_t *mask, int *found, int64_t *stats, int *iter_counts, int *iter_valid)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = ransac_args(c, src, stride_src, dst, stride_dst, n, max_iters, confidence, H, mask, found))) return rc;
    void *d_src, *d_dst;
    uint8_t *d_mask = (uint8_t *)km_ws(c, WS_RS_MASK, (size_t)n);
    if (!d_mask) return KM_E_NOMEM;
    if ((rc = upload_image(c, WS_RAW_A, src, sizeof(float), n, 2, stride_src, &d_src)) || (rc = upload_image(c, WS_RAW_B, dst, sizeof(float), n, 2, stride_dst, &d_dst)))
        return rc;
    try {
        return ransac_dev(c, (const float *)d_src, 2, (const float *)d_dst, 2, n, threshold, max_iters, confidence, H, d_mask, mask, found, stats,
                          iter_counts, iter_valid);
    } catch (const std::bad_alloc &) {
        return km_fail(c, KM_E_NOMEM, "find_homography_ransac: no host memory for %d pairs", n);
    }
}

}  // extern "C"
