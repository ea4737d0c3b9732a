// Descriptor matching of the global align step (karios/matcher/global_align.py:178-202): cv2.BFMatcher(NORM_L2).knnMatch in both
// directions, Lowe's ratio test and the mutual check.  The kernels live in k_match.hip; tests/match_restatement.py is the definition.
// No host synchronisation inside an entry point other than the copy of its results.
#include "api_internal.hpp"
#include "k_match.hpp"

#include <string.h>

namespace {

int rows_args(km_ctx *c, const void *p, int n, ptrdiff_t stride, const char *what)
{
    if (n < 0) return km_fail(c, KM_E_ARG, "%s: %d rows", what, n);
    if (n > 0 && !p) return km_fail(c, KM_E_ARG, "%s: null descriptors", what);
    if (n > 0 && stride < KMT_DIM) return km_fail(c, KM_E_ARG, "%s: row stride %td < %d", what, stride, KMT_DIM);
    return KM_OK;
}

int knn_args(km_ctx *c, const void *q, int n_q, ptrdiff_t sq, const void *t, int n_t, ptrdiff_t st, int dim, int k, const void *idx, const void *dist)
{
    int rc;
    if (dim != KMT_DIM) return km_fail(c, KM_E_UNSUPPORTED, "knn_match_u8: descriptor length %d (128 only)", dim);
    if (k != 1 && k != 2) return km_fail(c, KM_E_ARG, "knn_match_u8: k = %d (1 or 2)", k);
    if ((rc = rows_args(c, q, n_q, sq, "knn_match_u8 query")) || (rc = rows_args(c, t, n_t, st, "knn_match_u8 train"))) return rc;
    if (n_q > 0 && (!idx || !dist)) return km_fail(c, KM_E_ARG, "knn_match_u8: null output");
    return KM_OK;
}

unsigned long long *partials(km_ctx *c, int n_a, int n_b, int k_ab, int k_ba)
{
    size_t need = (size_t)n_a * kmt_chunks(c, n_a, n_b) * k_ab;
    if (k_ba) {
        const size_t back = (size_t)n_b * kmt_chunks(c, n_b, n_a) * k_ba;
        if (back > need) need = back;
    }
    return (unsigned long long *)km_ws(c, WS_MT_PART, need * sizeof(unsigned long long));
}

int knn_dev(km_ctx *c, const uint8_t *d_q, int n_q, ptrdiff_t sq, const uint8_t *d_t, int n_t, ptrdiff_t st, int k, int *d_idx, float *d_dist)
{
    void *pq = km_ws(c, WS_MT_PQ, kmt_packed_bytes(n_q)), *pt = km_ws(c, WS_MT_PT, kmt_packed_bytes(n_t));
    unsigned long long *part = partials(c, n_q, n_t, k, 0);
    if (!pq || !pt || !part) return KM_E_NOMEM;
    kmt_packed Q, T;
    int rc;
    if ((rc = kmt_pack(c, d_q, KM_U8, n_q, sq, pq, nullptr, 0, &Q)) || (rc = kmt_pack(c, d_t, KM_U8, n_t, st, pt, nullptr, 1, &T))) return rc;
    return kmt_knn(c, Q, T, k, part, d_idx, d_dist);
}

int match_args(km_ctx *c, const void *mon, int n_mon, ptrdiff_t smon, const void *ref, int n_ref, ptrdiff_t sref, int dtype, int dim, double ratio,
               int cap, const void *qi, const void *ti, const void *dist, const int *counts)
{
    int rc;
    if (dim != KMT_DIM) return km_fail(c, KM_E_UNSUPPORTED, "match_lowe_mutual: descriptor length %d (128 only)", dim);
    if (dtype != KM_U8 && dtype != KM_F32) return km_fail(c, KM_E_ARG, "match_lowe_mutual: dtype %d (uint8 and float32 only)", dtype);
    if ((rc = rows_args(c, mon, n_mon, smon, "match_lowe_mutual mon")) || (rc = rows_args(c, ref, n_ref, sref, "match_lowe_mutual ref"))) return rc;
    if (ratio != ratio) return km_fail(c, KM_E_ARG, "match_lowe_mutual: ratio is NaN");
    if (cap < 0 || !counts || (cap > 0 && (!qi || !ti || !dist))) return km_fail(c, KM_E_ARG, "match_lowe_mutual: bad output arguments");
    return KM_OK;
}

// pack both sets, knn(mon, ref, 2), knn(ref, mon, 1), filter + ordered compaction into device arrays of `cap` rows; the counters are
// read back (the one synchronisation) and judged
int match_dev(km_ctx *c, const void *d_mon, int n_mon, ptrdiff_t smon, const void *d_ref, int n_ref, ptrdiff_t sref, int dtype, double ratio, int cap,
              int *d_qi, int *d_ti, float *d_dist, int *counts)
{
    void *pq = km_ws(c, WS_MT_PQ, kmt_packed_bytes(n_mon)), *pt = km_ws(c, WS_MT_PT, kmt_packed_bytes(n_ref));
    unsigned long long *part = partials(c, n_mon, n_ref, 2, 1);
    int *fwd_idx = (int *)km_ws(c, WS_MT_FWD, (size_t)n_mon * 2 * (sizeof(int) + sizeof(float)));
    int *bwd_idx = (int *)km_ws(c, WS_MT_BWD, (size_t)n_ref * (sizeof(int) + sizeof(float)));
    unsigned *flag = (unsigned *)km_ws(c, WS_MT_FLAG, (size_t)n_mon * 2 * sizeof(unsigned));
    kmt_state *st = (kmt_state *)km_ws(c, WS_MT_STATE, sizeof(kmt_state));
    if (!pq || !pt || !part || !fwd_idx || !bwd_idx || !flag || !st) return KM_E_NOMEM;
    float *fwd_dist = (float *)(fwd_idx + (size_t)n_mon * 2), *bwd_dist = (float *)(bwd_idx + n_ref);
    kmt_packed Q, T;
    int rc;
    if ((rc = kmt_state_reset(c, st)) || (rc = kmt_pack(c, d_mon, dtype, n_mon, smon, pq, st, 0, &Q)) ||
        (rc = kmt_pack(c, d_ref, dtype, n_ref, sref, pt, st, 1, &T)) || (rc = kmt_knn(c, Q, T, 2, part, fwd_idx, fwd_dist)) ||
        (rc = kmt_knn(c, T, Q, 1, part, bwd_idx, bwd_dist)) ||
        (rc = kmt_filter(c, fwd_idx, fwd_dist, bwd_idx, n_mon, n_ref, ratio, flag, cap, d_qi, d_ti, d_dist, st)))
        return rc;
    kmt_state hs;
    KM_D2H(c, &hs, st, sizeof hs);
    KM_FLUSH(c);
    for (int w = 0; w < 2; w++)
        if (hs.n_bad[w])
            return km_fail(c, KM_E_ARG, "match_lowe_mutual: %s descriptors hold %u elements that are no integers in 0 .. 255, the first at (row %llu, column %llu)",
                           w ? "ref" : "mon", hs.n_bad[w], hs.first_bad[w] / KMT_DIM, hs.first_bad[w] % KMT_DIM);
    memcpy(counts, hs.counts, sizeof hs.counts);
    if (hs.counts[2] > cap) return km_fail(c, KM_E_ARG, "match_lowe_mutual: %d mutual matches, room for %d", hs.counts[2], cap);
    return KM_OK;
}

}  // namespace

extern "C" {

int km_knn_match_u8_dev(km_ctx *c, const uint8_t *d_q, int n_q, ptrdiff_t stride_q, const uint8_t *d_t, int n_t, ptrdiff_t stride_t, int dim, int k,
                        int *d_idx, float *d_dist)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = knn_args(c, d_q, n_q, stride_q, d_t, n_t, stride_t, dim, k, d_idx, d_dist))) return rc;
    if (n_q == 0 || n_t == 0) return KM_OK;
    return knn_dev(c, d_q, n_q, stride_q, d_t, n_t, stride_t, k, d_idx, d_dist);
}

int km_knn_match_u8(km_ctx *c, const uint8_t *q, int n_q, ptrdiff_t stride_q, const uint8_t *t, int n_t, ptrdiff_t stride_t, int dim, int k, int *idx,
                    float *dist)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = knn_args(c, q, n_q, stride_q, t, n_t, stride_t, dim, k, idx, dist))) return rc;
    if (n_q == 0) return KM_OK;
    if (n_t == 0) {
        for (size_t i = 0; i < (size_t)n_q * k; i++) { idx[i] = -1; dist[i] = __builtin_inff(); }
        return KM_OK;
    }
    void *d_q, *d_t;
    const size_t cells = (size_t)n_q * k;
    int *d_idx = (int *)km_ws(c, WS_MT_OUT, cells * (sizeof(int) + sizeof(float)));
    if (!d_idx) return KM_E_NOMEM;
    float *d_dist = (float *)(d_idx + cells);
    if ((rc = upload_image(c, WS_RAW_A, q, 1, n_q, KMT_DIM, stride_q, &d_q)) || (rc = upload_image(c, WS_RAW_B, t, 1, n_t, KMT_DIM, stride_t, &d_t))) return rc;
    if ((rc = knn_dev(c, (const uint8_t *)d_q, n_q, KMT_DIM, (const uint8_t *)d_t, n_t, KMT_DIM, k, d_idx, d_dist))) return rc;
    KM_D2H(c, idx, d_idx, cells * sizeof(int));
    KM_D2H(c, dist, d_dist, cells * sizeof(float));
    KM_FLUSH(c);
    return KM_OK;
}

int km_match_lowe_mutual_dev(km_ctx *c, const void *d_mon, int n_mon, ptrdiff_t stride_mon, const void *d_ref, int n_ref, ptrdiff_t stride_ref, int dtype,
                             int dim, double ratio, int cap, int *d_query_idx, int *d_train_idx, float *d_distance, int *counts)
{
    int rc;
    if ((rc = begin_call(c)) ||
        (rc = match_args(c, d_mon, n_mon, stride_mon, d_ref, n_ref, stride_ref, dtype, dim, ratio, cap, d_query_idx, d_train_idx, d_distance, counts)))
        return rc;
    counts[0] = n_mon; counts[1] = counts[2] = 0;
    if (n_mon == 0 || n_ref == 0) return KM_OK;
    return match_dev(c, d_mon, n_mon, stride_mon, d_ref, n_ref, stride_ref, dtype, ratio, cap, d_query_idx, d_train_idx, d_distance, counts);
}

int km_match_lowe_mutual(km_ctx *c, const void *mon, int n_mon, ptrdiff_t stride_mon, const void *ref, int n_ref, ptrdiff_t stride_ref, int dtype, int dim,
                         double ratio, int cap, int *query_idx, int *train_idx, float *distance, int *counts)
{
    int rc;
    if ((rc = begin_call(c)) || (rc = match_args(c, mon, n_mon, stride_mon, ref, n_ref, stride_ref, dtype, dim, ratio, cap, query_idx, train_idx, distance, counts)))
        return rc;
    counts[0] = n_mon; counts[1] = counts[2] = 0;
    if (n_mon == 0 || n_ref == 0) return KM_OK;
    void *d_mon, *d_ref;
    // no more rows than mon has can pass: the device arrays never need more than that
    const size_t room = (size_t)(cap < n_mon ? cap : n_mon);
    int *d_qi = (int *)km_ws(c, WS_MT_OUT, room * (2 * sizeof(int) + sizeof(float)));
    if (!d_qi) return KM_E_NOMEM;
    int *d_ti = d_qi + room;
    float *d_dist = (float *)(d_ti + room);
    const size_t elem = km_dtype_size(dtype);
    if ((rc = upload_image(c, WS_RAW_A, mon, elem, n_mon, KMT_DIM, stride_mon, &d_mon)) ||
        (rc = upload_image(c, WS_RAW_B, ref, elem, n_ref, KMT_DIM, stride_ref, &d_ref)))
        return rc;
    if ((rc = match_dev(c, d_mon, n_mon, KMT_DIM, d_ref, n_ref, KMT_DIM, dtype, ratio, (int)room, d_qi, d_ti, d_dist, counts))) {
        if (counts[2] > cap) return km_fail(c, KM_E_ARG, "match_lowe_mutual: %d mutual matches, room for %d", counts[2], cap);
        return rc;
    }
    const size_t n = (size_t)counts[2];
    if (n) {
        KM_D2H(c, query_idx, d_qi, n * sizeof(int));
        KM_D2H(c, train_idx, d_ti, n * sizeof(int));
        KM_D2H(c, distance, d_dist, n * sizeof(float));
        KM_FLUSH(c);
    }
    return KM_OK;
}

}  // extern "C"
