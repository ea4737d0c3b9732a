// ransac_math.hpp: cv2.findHomography(..., cv2.RANSAC, ...) of the align step (karios/matcher/global_align.py:223-230) as plain C++,
// shared by the kernels (k_ransac.hip), the host side (api_ransac.hip) and the CPU test (tests/test_ransac_host.py compiles this file
// with g++).  tests/ransac_restatement.py is the definition; every function here is held to it bit for bit, which needs
// -ffp-contract=off on every compiler that reads this text.  Float64 + - * / sqrt only; no libm call on the device path.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif

namespace rs {

enum { MODEL_POINTS = 4, SUBSET_ATTEMPTS = 1000, LM_MAX_ITERS = 10 };

// ---- cv::RNG: multiply-with-carry, RNG((uint64)-1) ----------------------------------------------------------------------------------------
RS_HD inline uint32_t rng_next(uint64_t &state)
{
    state = (uint64_t)(uint32_t)state * 4164903690u + (uint32_t)(state >> 32);
    return (uint32_t)state;
}
RS_HD inline int rng_uniform(uint64_t &state, int n) { return (int)(rng_next(state) % (uint32_t)n); }   // uniform(0, n)

// ---- checkSubset -------------------------------------------------------------------------------------------------------------------------
// p: count points (x, y) interleaved; only the LAST point is tested against the lines through the earlier ones
RS_HD inline bool have_collinear(const float *p, int count)
{
    const int i = count - 1;
    for (int j = 0; j < i; j++) {
        const double dx1 = (double)(p[2 * j] - p[2 * i]), dy1 = (double)(p[2 * j + 1] - p[2 * i + 1]);
        for (int k = 0; k < j; k++) {
            const double dx2 = (double)(p[2 * k] - p[2 * i]), dy2 = (double)(p[2 * k + 1] - p[2 * i + 1]);
            if (fabs(dx2 * dy1 - dy2 * dx1) <= (double)FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
        }
    }
    return false;
}
RS_HD inline double det3_ones(const float *p, int a, int b, int c)   // determinant of the rows (x, y, 1) of points a, b, c
{
    const double a00 = p[2 * a], a01 = p[2 * a + 1], a10 = p[2 * b], a11 = p[2 * b + 1], a20 = p[2 * c], a21 = p[2 * c + 1];
    return a00 * (a11 * 1.0 - a21 * 1.0) - a01 * (a10 * 1.0 - a20 * 1.0) + 1.0 * (a10 * a21 - a20 * a11);
}
RS_HD inline bool check_subset(const float *src, const float *dst)   // 4 pairs
{
    if (have_collinear(src, 4) || have_collinear(dst, 4)) return false;
    const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    int negative = 0;
    for (int i = 0; i < 4; i++) negative += det3_ones(src, tt[i][0], tt[i][1], tt[i][2]) * det3_ones(dst, tt[i][0], tt[i][1], tt[i][2]) < 0 ? 1 : 0;
    return negative == 0 || negative == 4;
}

// getSubset on packed pairs (x, y, mx, my per pair): 4 distinct indices, redrawn on duplicates, at most SUBSET_ATTEMPTS subsets
inline bool get_subset(const float *pairs, int n, uint64_t &state, int idx[4])
{
    for (int attempt = 0; attempt < SUBSET_ATTEMPTS; attempt++) {
        float s[8], d[8];
        for (int i = 0; i < 4; i++) {
            int v;
            for (;;) {
                v = rng_uniform(state, n);
                bool dup = false;
                for (int j = 0; j < i; j++) dup = dup || idx[j] == v;
                if (!dup) break;
            }
            idx[i] = v;
            s[2 * i] = pairs[4 * (size_t)v]; s[2 * i + 1] = pairs[4 * (size_t)v + 1];
            d[2 * i] = pairs[4 * (size_t)v + 2]; d[2 * i + 1] = pairs[4 * (size_t)v + 3];
        }
        if (check_subset(s, d)) return true;
    }
    return false;
}

// RANSACUpdateNumIters (host only: pow and log are libm's)
inline int update_num_iters(double p, double ep, int model_points, int max_iters)
{
    p = p > 0. ? p : 0.; p = p < 1. ? p : 1.;
    ep = ep > 0. ? ep : 0.; ep = ep < 1. ? ep : 1.;
    double num = 1. - p > DBL_MIN ? 1. - p : DBL_MIN;
    double denom = 1. - pow(1. - ep, (double)model_points);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)lrint(num / denom);
}

// ---- OpenCV's Jacobi eigen-solver of a symmetric n x n matrix (upper triangle of A is read and destroyed) -------------------------------------
RS_HD inline double hypot_plain(double a, double b) { return sqrt(a * a + b * b); }   // [def]: three roundings, no scaling

// The working set of one eigen-problem (n <= 9): the matrix, the eigenvectors, the eigenvalues and the two pivot indices.  All of it
// is indexed by computed subscripts, so where it lives decides the solver's latency: plain arrays on the host, one lane's slice of
// LDS in the kernel (k_ransac.hip) - any type with these five accessors serves.
struct PlainStore {
    double A[81], V[81], W[9];
    int R[9], C[9];
    RS_HD double &a(int i) { return A[i]; }
    RS_HD double &v(int i) { return V[i]; }
    RS_HD double &w(int i) { return W[i]; }
    RS_HD int &r(int i) { return R[i]; }
    RS_HD int &c(int i) { return C[i]; }
};

template <class S>
RS_HD inline void jacobi_ind(S &st, int n, int idx)
{
    int m, i;
    double mv;
    if (idx < n - 1) {
        for (m = idx + 1, mv = fabs(st.a(n * idx + m)), i = idx + 2; i < n; i++) {
            const double val = fabs(st.a(n * idx + i));
            if (mv < val) mv = val, m = i;
        }
        st.r(idx) = m;
    }
    if (idx > 0) {
        for (m = 0, mv = fabs(st.a(idx)), i = 1; i < idx; i++) {
            const double val = fabs(st.a(n * i + idx));
            if (mv < val) mv = val, m = i;
        }
        st.c(idx) = m;
    }
}

// in: st.a = the n x n matrix (upper triangle read, destroyed).  out: st.w = n eigenvalues, descending; st.v = n x n, row i =
// eigenvector i.  Returns the rotations done (at most 30 n^2: a loop bound, whatever the input).
template <class S>
RS_HD inline int jacobi(S &st, int n)
{
    int i, k, iters = 0;
    for (i = 0; i < n * n; i++) st.v(i) = 0.;
    for (i = 0; i < n; i++) st.v(n * i + i) = 1.;
    for (k = 0; k < n; k++) {
        st.w(k) = st.a((n + 1) * k);
        jacobi_ind(st, n, k);
    }
    const int max_iters = n * n * 30;
    if (n > 1) for (iters = 0; iters < max_iters; iters++) {
        double mv = fabs(st.a(st.r(0)));
        for (k = 0, i = 1; i < n - 1; i++) {
            const double val = fabs(st.a(n * i + st.r(i)));
            if (mv < val) mv = val, k = i;
        }
        int l = st.r(k);
        for (i = 1; i < n; i++) {
            const double val = fabs(st.a(n * st.c(i) + i));
            if (mv < val) mv = val, k = st.c(i), l = i;
        }
        const double p = st.a(n * k + l);
        if (fabs(p) <= DBL_EPSILON) break;
        const double y = (st.w(l) - st.w(k)) * 0.5;
        double t = fabs(y) + hypot_plain(p, y);
        double s = hypot_plain(p, t);
        const double c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0) s = -s, t = -t;
        st.a(n * k + l) = 0;
        st.w(k) -= t;
        st.w(l) += t;
        double a0, b0;
#define RS_ROTATE(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
        for (i = 0; i < k; i++) RS_ROTATE(st.a(n * i + k), st.a(n * i + l));
        for (i = k + 1; i < l; i++) RS_ROTATE(st.a(n * k + i), st.a(n * i + l));
        for (i = l + 1; i < n; i++) RS_ROTATE(st.a(n * k + i), st.a(n * l + i));
        for (i = 0; i < n; i++) RS_ROTATE(st.v(n * k + i), st.v(n * l + i));
#undef RS_ROTATE
        jacobi_ind(st, n, k);
        jacobi_ind(st, n, l);
    }
    for (k = 0; k < n - 1; k++) {
        int m = k;
        for (i = k + 1; i < n; i++)
            if (st.w(m) < st.w(i)) m = i;
        if (k != m) {
            double tmp = st.w(m); st.w(m) = st.w(k); st.w(k) = tmp;
            for (i = 0; i < n; i++) { tmp = st.v(n * m + i); st.v(n * m + i) = st.v(n * k + i); st.v(n * k + i) = tmp; }
        }
    }
    return iters;
}

// ---- HomographyEstimatorCallback::runKernel: normalised DLT of count >= 4 pairs (M -> m), points interleaved (x, y) -------------------------
// returns 0 (H untouched) when a scale degenerates, else 1.  st: the eigen-solver's working set
template <class S>
RS_HD inline int dlt(const float *M, const float *m, int count, double *H, S &st)
{
    double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
    for (int i = 0; i < count; i++) {
        cmx += (double)m[2 * (size_t)i]; cmy += (double)m[2 * (size_t)i + 1];
        cMx += (double)M[2 * (size_t)i]; cMy += (double)M[2 * (size_t)i + 1];
    }
    cmx /= count; cmy /= count; cMx /= count; cMy /= count;
    for (int i = 0; i < count; i++) {
        smx += fabs((double)m[2 * (size_t)i] - cmx); smy += fabs((double)m[2 * (size_t)i + 1] - cmy);
        sMx += fabs((double)M[2 * (size_t)i] - cMx); sMy += fabs((double)M[2 * (size_t)i + 1] - cMy);
    }
    if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) return 0;
    smx = count / smx; smy = count / smy; sMx = count / sMx; sMy = count / sMy;
    const double invHnorm[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1};
    const double Hnorm2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
    for (int j = 0; j < 81; j++) st.a(j) = 0;
    for (int i = 0; i < count; i++) {
        const double x = ((double)m[2 * (size_t)i] - cmx) * smx, y = ((double)m[2 * (size_t)i + 1] - cmy) * smy;
        const double X = ((double)M[2 * (size_t)i] - cMx) * sMx, Y = ((double)M[2 * (size_t)i + 1] - cMy) * sMy;
        const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
        const double Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
        for (int j = 0; j < 9; j++)
            for (int k = j; k < 9; k++) st.a(9 * j + k) += Lx[j] * Lx[k] + Ly[j] * Ly[k];
    }
    for (int j = 0; j < 9; j++)
        for (int k = 0; k < j; k++) st.a(9 * j + k) = st.a(9 * k + j);
    jacobi(st, 9);
    double H0[9], T[9];
    for (int j = 0; j < 9; j++) H0[j] = st.v(72 + j);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) T[3 * r + c] = invHnorm[3 * r] * H0[c] + invHnorm[3 * r + 1] * H0[3 + c] + invHnorm[3 * r + 2] * H0[6 + c];
    double U[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) U[3 * r + c] = T[3 * r] * Hnorm2[c] + T[3 * r + 1] * Hnorm2[3 + c] + T[3 * r + 2] * Hnorm2[6 + c];
    const double scale = 1. / U[8];
    for (int j = 0; j < 9; j++) H[j] = U[j] * scale + 0.;
    return 1;
}
inline int dlt(const float *M, const float *m, int count, double *H)
{
    PlainStore st;
    return dlt(M, m, count, H, st);
}

// ---- computeError / findInliers: everything float32, left to right ------------------------------------------------------------------------
RS_HD inline float reproj_err(const float *Hf, float x, float y, float mx, float my)
{
    const float ww = 1.f / (Hf[6] * x + Hf[7] * y + 1.f);
    const float dx = (Hf[0] * x + Hf[1] * y + Hf[2]) * ww - mx;
    const float dy = (Hf[3] * x + Hf[4] * y + Hf[5]) * ww - my;
    return dx * dx + dy * dy;
}
RS_HD inline float threshold_sq(double threshold) { return (float)(threshold * threshold); }

// ---- the bookkeeping of RANSACPointSetRegistrator::run over per-iteration results, in iteration order -----------------------------------------
struct Replay {
    int niters, max_good, best_iter, iter;   // iter: iterations the loop has been through so far
};
inline void replay_init(Replay &r, int max_iters) { r.niters = max_iters > 1 ? max_iters : 1; r.max_good = 0; r.best_iter = -1; r.iter = 0; }
// iterations [r.iter, end) with their inlier counts and valid flags (indexed from r.iter); stops at niters
inline void replay(Replay &r, int end, const int *count, const int *valid, int n, double confidence)
{
    const int base = r.iter;
    for (; r.iter < end && r.iter < r.niters; r.iter++) {
        const int good = count[r.iter - base];
        if (!valid[r.iter - base]) continue;
        if (good > (r.max_good > MODEL_POINTS - 1 ? r.max_good : MODEL_POINTS - 1)) {
            r.max_good = good;
            r.best_iter = r.iter;
            r.niters = update_num_iters(confidence, (double)(n - good) / n, MODEL_POINTS, r.niters);
        }
    }
}

// ---- LMSolverImpl::run on HomographyRefineCallback, 8 parameters ------------------------------------------------------------------------------
// residuals (and, with A / v, J^T J and J^T r) at h; sums run over the rows 2 i, 2 i + 1 in index order.  *S = |r|^2, *rinf = max |r|
inline void lm_eval(const float *M, const float *m, int count, const double *h, double *A, double *v, double *S, double *rinf)
{
    double s2 = 0, mx = 0;
    if (A) {
        for (int j = 0; j < 64; j++) A[j] = 0;
        for (int j = 0; j < 8; j++) v[j] = 0;
    }
    for (int i = 0; i < count; i++) {
        const double Mx = M[2 * (size_t)i], My = M[2 * (size_t)i + 1];
        double ww = h[6] * Mx + h[7] * My + 1.;
        ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
        const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
        const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
        const double e0 = xi - (double)m[2 * (size_t)i], e1 = yi - (double)m[2 * (size_t)i + 1];
        s2 += e0 * e0;
        s2 += e1 * e1;
        if (mx < fabs(e0)) mx = fabs(e0);
        if (mx < fabs(e1)) mx = fabs(e1);
        if (A) {
            const double J0[8] = {Mx * ww, My * ww, ww, 0., 0., 0., -Mx * ww * xi, -My * ww * xi};
            const double J1[8] = {0., 0., 0., Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi};
            for (int a = 0; a < 8; a++) {
                for (int b = a; b < 8; b++) {
                    A[8 * a + b] += J0[a] * J0[b];
                    A[8 * a + b] += J1[a] * J1[b];
                }
                v[a] += J0[a] * e0;
                v[a] += J1[a] * e1;
            }
        }
    }
    if (A)
        for (int a = 0; a < 8; a++)
            for (int b = 0; b < a; b++) A[8 * a + b] = A[8 * b + a];
    *S = s2;
    *rinf = mx;
}

// cv::solve / cv::invert with DECOMP_EIG on a symmetric 8 x 8 matrix: Jacobi, then the back-substitution of SVBkSb.
// x: the solution of Ap x = b (b != nullptr), or the diagonal of the inverse (b == nullptr)
inline void eig_solve8(const double *Ap, const double *b, double *x)
{
    PlainStore st;
    for (int j = 0; j < 64; j++) st.A[j] = Ap[j];
    jacobi(st, 8);
    const double *W = st.W, *V = st.V;
    double threshold = 0;
    for (int i = 0; i < 8; i++) { threshold += W[i]; x[i] = 0; }
    threshold *= DBL_EPSILON * 2;
    for (int i = 0; i < 8; i++) {
        double wi = W[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        if (b) {
            double s = 0;
            for (int j = 0; j < 8; j++) s += V[8 * i + j] * b[j];
            s *= wi;
            for (int j = 0; j < 8; j++) x[j] = x[j] + s * V[8 * i + j];
        } else {
            for (int j = 0; j < 8; j++) x[j] = x[j] + V[8 * i + j] * (V[8 * i + j] * wi);
        }
    }
}

// h: the 8 free parameters, in and out.  Returns the iterations run (1 .. LM_MAX_ITERS).
inline int lm_refine(const float *M, const float *m, int count, double *h)
{
    double x[8], xd[8], A[64], Ap[64], v[8], d[8], D[8], S, Sd, rinf, rdinf;
    for (int j = 0; j < 8; j++) x[j] = h[j];
    lm_eval(M, m, count, x, A, v, &S, &rinf);
    for (int j = 0; j < 8; j++) D[j] = A[9 * j];
    const double Rlo = 0.25, Rhi = 0.75;
    double lambda = 1, lc = 0.75;
    int iter = 0;
    for (;;) {
        for (int j = 0; j < 64; j++) Ap[j] = A[j];
        for (int j = 0; j < 8; j++) Ap[9 * j] += lambda * D[j];
        eig_solve8(Ap, v, d);
        for (int j = 0; j < 8; j++) xd[j] = x[j] - d[j];
        lm_eval(M, m, count, xd, nullptr, nullptr, &Sd, &rdinf);
        double dS = 0, t = 0, dinf = 0;
        for (int i = 0; i < 8; i++) {
            double s = 0;
            for (int k = 0; k < 8; k++) s += A[8 * i + k] * d[k];
            dS += d[i] * (-s + 2 * v[i]);
        }
        const double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1);
        if (R > Rhi) {
            lambda *= 0.5;
            if (lambda < lc) lambda = 0;
        } else if (R < Rlo) {
            for (int i = 0; i < 8; i++) t += d[i] * v[i];
            double nu = (Sd - S) / (fabs(t) > DBL_EPSILON ? t : 1) + 2;
            nu = nu > 2. ? nu : 2.; nu = nu < 10. ? nu : 10.;
            if (lambda == 0) {
                double diag[8], maxval = DBL_EPSILON;
                eig_solve8(A, nullptr, diag);
                for (int i = 0; i < 8; i++) maxval = maxval > fabs(diag[i]) ? maxval : fabs(diag[i]);
                lambda = lc = 1. / maxval;
                nu *= 0.5;
            }
            lambda *= nu;
        }
        if (Sd < S) {
            S = Sd;
            for (int j = 0; j < 8; j++) x[j] = xd[j];
            lm_eval(M, m, count, x, A, v, &S, &rinf);
        }
        iter++;
        for (int i = 0; i < 8; i++) dinf = dinf > fabs(d[i]) ? dinf : fabs(d[i]);
        if (!(iter < LM_MAX_ITERS && dinf >= (double)FLT_EPSILON && rinf >= (double)FLT_EPSILON)) break;
    }
    for (int j = 0; j < 8; j++) h[j] = x[j];
    return iter;
}

// the tail of findHomography after a successful RANSAC on more than 4 pairs: M / m hold the `count` inliers, compressed in index
// order; H: the winning model in, the result out.  Returns the LM iterations.
inline int refine_on_inliers(const float *M, const float *m, int count, double *H)
{
    if (count <= 0) return 0;
    dlt(M, m, count, H);
    return lm_refine(M, m, count, H);
}

}  // namespace rs
