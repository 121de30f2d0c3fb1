// orbx_pnp.hip -- PnPsolver (src/PnPsolver.cc): EPnP on RANSAC sets of four matches, every iteration of every relocalisation candidate of
// Tracking::Relocalization (src/Tracking.cc) in one launch chain with one wait.  gfx950 only.
//
//   k_pnp_prepare  mvMaxError[i] = sigma2 * th2 (a float product, :227-229); reads the call's inputs in mapped pinned memory (each byte once) and
//                  leaves what the kernels behind read many times - points, keypoints, limits, sets, headers - in device memory.
//   k_pnp_models   compute_pose (:684-759) per (candidate, iteration), a TEAM of 16 lanes per problem, four problems per wave; the team's
//                  workspace (MtM, its eigenvectors, L, rho, the three solutions) is 5.6 KB of LDS.  See epnp_solve.
//   k_pnp_check    CheckInliers (:421-458), one WAVE per (candidate, iteration): the ballot of 64 matches is the mask word.  The same kernel
//                  checks the refined models and explicit ones.
//   k_pnp_records  one wave per candidate: the running best of iterate (:301-317) as a prefix maximum (count >= minInliers && count > best);
//                  the iterations at which it changes are the RECORDS, record_of[i] the latest record at or before i.
//   k_pnp_refine   Refine (:366-418) once per (candidate, record): EPnP on the record's inlier mask, one workgroup of 128 lanes.  The grid is
//                  sized for the worst case, blocks without a record exit.  Followed by k_pnp_check on the refined models.
//   k_pnp_decide   one workgroup per candidate: the return events (count_i >= minInliers and record_of[i] refined with MORE than minInliers),
//                  the first event and its refined mask, mBestTcw and its mask, the result block, the sequence word.
//
// epnp_solve: every sum over the points of a set is ONE lane's loop over the points in their order (the reference's own order), different
// entries on different lanes: 3 lanes for the centroid, 9 for PW0^T PW0, 78 for the upper triangle of M^T M, 9 / 27 for the centroids and ABt of
// the three solutions, 3 for the reprojection sums.  Nothing is accumulated with atomics, no order depends on the launch.  The barycentric
// coordinates are recomputed where they are used (nine products) and never stored.  The 12x12 eigenproblem is a cyclic two-sided Jacobi with
// lane r owning row / column r of the matrix in LDS; 144 doubles per lane would not fit in registers, 16 lanes a problem keep 4 problems a wave.
// The small dense pieces (3x3 PCA, the three least-squares starts, Gauss-Newton with qr_solve, the 3x3 SVD) run on one lane per solution, fully
// unrolled in registers.
//
// Arithmetic: FP64 as in the reference, in its operation order where the reference fixes one; the library is built with -ffp-contract=off, so
// every product and sum below is its own operation and tests/pnp_ref.py restates them in numpy float64.  The list is in include/orbx.h.
// PARITY UNPINNED AT THE OPENCV LEVEL: cvSVD, cvSolve(CV_SVD), cvInvert(CV_SVD) (here: Jacobi in FP64), the signs of eigen / singular vectors,
// the basis inside the null space of M^T M for a minimal set, rank-deficient control points.  RANSAC sets are drawn ahead by the caller.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "orbx_handle.h"

#define PNP_SWEEPS12 ORBX_PNP_JACOBI_SWEEPS
#define PNP_SWEEPS_SMALL ORBX_PNP_SMALL_SWEEPS
#define PNP_TINY 8.673617379884035e-19      // 2^-60: an off-diagonal entry this small beside its diagonal entries is set to zero unrotated
#define PNP_ORTH 1.7763568394002505e-15     // 2^-49: columns this orthogonal are left alone by the one-sided Jacobi
#define PNP_RANK 4.930380657631324e-32      // 2^-104: squared singular values below this share of the largest are dropped (pseudo-inverse)
#define PNP_FULL ORBX_PNP_FULL_DOUBLES
#define PNP_TEAM 16
#define PNP_REFINE_THREADS 128

enum { F_CWS = ORBX_PNP_F_CWS, F_PCA = ORBX_PNP_F_PCA, F_DC = ORBX_PNP_F_DC, F_UCT = ORBX_PNP_F_UCT, F_CI = ORBX_PNP_F_CI, F_MTM = ORBX_PNP_F_MTM,
       F_D = ORBX_PNP_F_D, F_UT = ORBX_PNP_F_UT, F_L = ORBX_PNP_F_L, F_RHO = ORBX_PNP_F_RHO, F_B0 = ORBX_PNP_F_B0, F_B1 = ORBX_PNP_F_B1,
       F_RS = ORBX_PNP_F_RS, F_TS = ORBX_PNP_F_TS, F_ERR = ORBX_PNP_F_ERR, F_CHOICE = ORBX_PNP_F_CHOICE };

struct PnpCand {                 // one candidate of a call: in mapped pinned memory (host-filled), copied to the device by k_pnp_prepare
    float k[4];                  // fx, fy, cx, cy
    float th2;
    int32_t n, iters, minInliers;
    int32_t mb, ib;              // first match / first iteration of this candidate in the call's arrays
    int32_t words;               // ceil(n / 64)
    int32_t pad;
    unsigned long long wb;       // first mask word
    unsigned long long outOff;   // the candidate's result block in the mapped result buffer
};
static_assert(sizeof(PnpCand) % 8 == 0, "copied in 4-byte words, holds 8-byte members");

struct PnpBlock {                // layout of a candidate's result block (mapped pinned), byte offsets behind the 32-byte head
    size_t r, t, err, refR, refT, refTcw, bestTcw, count, recordOf, recIter, refCount, isEvent, inlFirst, inlBest, total;
    __host__ __device__ PnpBlock(int n, int iters)
    {
        const size_t it = (size_t)iters;
        r = 32; t = r + it * 72; err = t + it * 24; refR = err + it * 8; refT = refR + it * 72; refTcw = refT + it * 24; bestTcw = refTcw + it * 48;
        count = bestTcw + 48; recordOf = count + it * 4; recIter = recordOf + it * 4; refCount = recIter + it * 4; isEvent = refCount + it * 4;
        inlFirst = isEvent + ((it + 3) & ~(size_t)3);
        inlBest = inlFirst + (size_t)n;
        total = (inlBest + (size_t)n + 255) & ~(size_t)255;
    }
};

struct PnpDev {                  // device arrays of a call
    float *world;                // [matches][3]
    float2 *uv;
    float *maxErr;
    int32_t *sets;               // [iterations][4]
    PnpCand *cand;
    double *r, *t, *err, *refR, *refT, *refErr;
    int32_t *count, *refCount, *recordOf, *recIter, *nrec;
    unsigned long long *mask, *refMask;
};

struct PnpIn {                   // the call's inputs, device addresses of mapped pinned memory
    const PnpCand *cand;
    const float *world, *uv, *sigma;
    const int32_t *sets;
};

__global__ __launch_bounds__(256) void k_pnp_prepare(PnpIn I, PnpDev D, int withSets)
{
    const int c = blockIdx.y;
    const PnpCand *hc = I.cand + c;
    const int n = hc->n, iters = hc->iters, mb = hc->mb, ib = hc->ib;
    const float th2 = hc->th2;
    const int stride = gridDim.x * 256, first = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < sizeof(PnpCand) / 4) ((uint32_t *)(D.cand + c))[threadIdx.x] = ((const uint32_t *)hc)[threadIdx.x];
    for (int j = first; withSets && j < 4 * iters; j += stride) D.sets[4 * (size_t)ib + j] = I.sets[4 * (size_t)ib + j];
    for (int i = first; i < n; i += stride) {
        const size_t g = (size_t)mb + i;
        D.world[3 * g] = I.world[3 * g]; D.world[3 * g + 1] = I.world[3 * g + 1]; D.world[3 * g + 2] = I.world[3 * g + 2];
        D.uv[g] = make_float2(I.uv[2 * g], I.uv[2 * g + 1]);
        D.maxErr[g] = I.sigma[g] * th2;      // :229, vector<float> * float
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// EPnP
// ---------------------------------------------------------------------------------------------------------------------------------------
struct PnpPts {                  // the correspondences of one compute_pose: an explicit list (RANSAC set) or a mask row (Refine), in that order
    const int32_t *set;
    const unsigned long long *mask;
    int m, words;
    const float *world;          // the candidate's matches
    const float2 *uv;
};

template <class F> __device__ __forceinline__ void pnp_for_each(const PnpPts &P, F f)
{
    if (P.set) {
        for (int k = 0; k < P.m; k++) f(P.set[k]);
    } else {
        for (int w = 0; w < P.words; w++) {
            unsigned long long b = P.mask[w];
            while (b) { f(64 * w + __ffsll((long long)b) - 1); b &= b - 1; }
        }
    }
}

__device__ __forceinline__ int pnp_first(const PnpPts &P)
{
    if (P.set) return P.m > 0 ? P.set[0] : -1;
    for (int w = 0; w < P.words; w++)
        if (P.mask[w]) return 64 * w + __ffsll((long long)P.mask[w]) - 1;
    return -1;
}

struct EpnpWs {                  // a team's workspace in LDS; f is the stage-output block of orbx_pnp_epnp(full), the Jacobi works in its Ut slot
    double f[PNP_FULL];
    double V[144], ccs[36], pc0[9], abt[27], dr[12], tv[9];
    int order[12];
};

// the plane rotation that annihilates gamma; false (the identity) where gamma is negligible
__device__ __forceinline__ bool jacobi_cst(const double alpha, const double beta, const double gamma, const double small, double &c, double &s, double &t)
{
    c = 1.0; s = 0.0; t = 0.0;
    const bool rotate = !(fabs(gamma) <= small);
    if (rotate) {
        const double zeta = (beta - alpha) / (2.0 * gamma);
        t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        c = 1.0 / sqrt(1.0 + t * t);
        s = c * t;
    }
    return rotate;
}

// One-sided (Hestenes) Jacobi on the columns of the MxK matrix a: a <- a V with orthogonal columns (= U Sigma), then the least-squares /
// pseudo-inverse solution x[K][NB] of a x = b for NB right-hand sides: x = V Sigma^-2 (a V)^T b, dropping negligible singular values.
template <int M, int K> __device__ __forceinline__ void onesided_jacobi(double (&a)[M][K], double (&v)[K][K])
{
#pragma unroll
    for (int i = 0; i < K; i++)
#pragma unroll
        for (int j = 0; j < K; j++) v[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < PNP_SWEEPS_SMALL; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < K - 1; p++) {
#pragma unroll
            for (int q = p + 1; q < K; q++) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int i = 0; i < M; i++) { alpha = alpha + a[i][p] * a[i][p]; beta = beta + a[i][q] * a[i][q]; gamma = gamma + a[i][p] * a[i][q]; }
                double c, s, t;
                if (!jacobi_cst(alpha, beta, gamma, PNP_ORTH * sqrt(alpha * beta), c, s, t)) continue;      // the identity: nothing to apply
                rotated = true;
#pragma unroll
                for (int i = 0; i < M; i++) { const double ap = a[i][p], aq = a[i][q]; a[i][p] = c * ap - s * aq; a[i][q] = s * ap + c * aq; }
#pragma unroll
                for (int i = 0; i < K; i++) { const double vp = v[i][p], vq = v[i][q]; v[i][p] = c * vp - s * vq; v[i][q] = s * vp + c * vq; }
            }
        }
        if (!rotated) break;      // a sweep of identities changed nothing and neither will the next: the same bits as running them all
    }
}

template <int M, int K, int NB> __device__ __forceinline__ void svd_ls(double (&a)[M][K], const double (&b)[M][NB], double (&x)[K][NB])
{
    double v[K][K], s2[K], smax = 0.0;
    onesided_jacobi<M, K>(a, v);
#pragma unroll
    for (int j = 0; j < K; j++) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < M; i++) s = s + a[i][j] * a[i][j];
        s2[j] = s;
        smax = s > smax ? s : smax;
    }
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
        double w[K];
#pragma unroll
        for (int j = 0; j < K; j++) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < M; i++) s = s + a[i][j] * b[i][nb];
            w[j] = s2[j] > smax * PNP_RANK ? s / s2[j] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < K; r++) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < K; j++) s = s + v[r][j] * w[j];
            x[r][nb] = s;
        }
    }
}

// rank of every |d[k]| in descending order, the first of equal ones first: order[rank] = k
__device__ __forceinline__ void pnp_order(const double *d, int n, int *order)
{
    for (int k = 0; k < n; k++) order[k] = k;
    for (int k = 0; k < n; k++) {
        int rank = 0;
        const double dk = fabs(d[k]);
        for (int j = 0; j < n; j++) rank += (fabs(d[j]) > dk || (fabs(d[j]) == dk && j < k)) ? 1 : 0;
        order[rank] = k;
    }
}

// choose_control_points behind the sums (:545-561) and the inverse of compute_barycentric_coordinates (:589-593); one lane
__device__ void pnp_control_points(EpnpWs &W, const double dm)
{
    double a[3][3], v[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { a[i][j] = W.f[F_PCA + 3 * i + j]; v[i][j] = i == j ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < PNP_SWEEPS_SMALL; sweep++) {
#pragma unroll
        for (int p = 0; p < 2; p++) {
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                const double alpha = a[p][p], beta = a[q][q], gamma = a[p][q];
                double c, s, t;
                jacobi_cst(alpha, beta, gamma, PNP_TINY * (fabs(alpha) + fabs(beta)), c, s, t);
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    const double ap = a[r][p], aq = a[r][q], vp = v[r][p], vq = v[r][q];
                    if (r != p && r != q) {
                        a[r][p] = c * ap - s * aq; a[r][q] = s * ap + c * aq;
                        a[p][r] = a[r][p]; a[q][r] = a[r][q];
                    }
                    v[r][p] = c * vp - s * vq; v[r][q] = s * vp + c * vq;
                }
                a[p][p] = alpha - t * gamma; a[q][q] = beta + t * gamma;
                a[p][q] = 0.0; a[q][p] = 0.0;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        W.dr[i] = a[i][i];
#pragma unroll
        for (int j = 0; j < 3; j++) W.tv[3 * i + j] = v[i][j];
    }
    pnp_order(W.dr, 3, W.order);
    for (int i = 0; i < 3; i++) {
        const int o = W.order[i];
        W.f[F_DC + i] = fabs(W.dr[o]);
        for (int j = 0; j < 3; j++) W.f[F_UCT + 3 * i + j] = W.tv[3 * j + o];
    }
    for (int i = 1; i < 4; i++) {
        const double k = sqrt(W.f[F_DC + i - 1] / dm);
        for (int j = 0; j < 3; j++) W.f[F_CWS + 3 * i + j] = W.f[F_CWS + j] + k * W.f[F_UCT + 3 * (i - 1) + j];
    }
    double cc[3][3], eye[3][3], ci[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 1; j < 4; j++) { cc[i][j - 1] = W.f[F_CWS + 3 * j + i] - W.f[F_CWS + i]; eye[i][j - 1] = i == j - 1 ? 1.0 : 0.0; }
    svd_ls<3, 3, 3>(cc, eye, ci);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) W.f[F_CI + 3 * i + j] = ci[i][j];
}

// :595-615 for one point
__device__ __forceinline__ void pnp_alphas(const EpnpWs &W, const float *pw, double (&a)[4])
{
    const double d0 = (double)pw[0] - W.f[F_CWS], d1 = (double)pw[1] - W.f[F_CWS + 1], d2 = (double)pw[2] - W.f[F_CWS + 2];
#pragma unroll
    for (int j = 0; j < 3; j++) a[1 + j] = (W.f[F_CI + 3 * j] * d0 + W.f[F_CI + 3 * j + 1] * d1) + W.f[F_CI + 3 * j + 2] * d2;
    a[0] = ((1.0 - a[1]) - a[2]) - a[3];
}

__device__ __forceinline__ double pnp_sel4(const double (&a)[4], int k) { return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : a[3]; }

// qr_solve (:1251-1385) for the 6x4 system of gauss_newton, operation by operation; false = the reference's "A is singular" return, X untouched
__device__ __forceinline__ bool pnp_qr_solve(double (&A)[24], double (&b)[6], double (&X)[4])
{
    double A1[4], A2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double eta = fabs(A[4 * k + k]);
#pragma unroll
        for (int i = k + 1; i < 6; i++) {      // the reference's pointer is advanced behind the comparison: rows k .. 4 are looked at
            const double elt = fabs(A[4 * (i - 1) + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0.0) return false;
        const double inv_eta = 1. / eta;
        double sum = 0.0;
#pragma unroll
        for (int i = k; i < 6; i++) { A[4 * i + k] = A[4 * i + k] * inv_eta; sum = sum + A[4 * i + k] * A[4 * i + k]; }
        double sigma = sqrt(sum);
        if (A[4 * k + k] < 0) sigma = -sigma;
        A[4 * k + k] = A[4 * k + k] + sigma;
        A1[k] = sigma * A[4 * k + k];
        A2[k] = -eta * sigma;
#pragma unroll
        for (int j = k + 1; j < 4; j++) {
            double s = 0.0;
#pragma unroll
            for (int i = k; i < 6; i++) s = s + A[4 * i + k] * A[4 * i + j];
            const double tau = s / A1[k];
#pragma unroll
            for (int i = k; i < 6; i++) A[4 * i + j] = A[4 * i + j] - tau * A[4 * i + k];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double tau = 0.0;
#pragma unroll
        for (int i = j; i < 6; i++) tau = tau + A[4 * i + j] * b[i];
        tau = tau / A1[j];
#pragma unroll
        for (int i = j; i < 6; i++) b[i] = b[i] - tau * A[4 * i + j];
    }
    X[3] = b[3] / A2[3];
#pragma unroll
    for (int i = 2; i >= 0; i--) {
        double s = 0.0;
#pragma unroll
        for (int j = i + 1; j < 4; j++) s = s + A[4 * i + j] * X[j];
        X[i] = (b[i] - s) / A2[i];
    }
    return true;
}

template <int K> __device__ __forceinline__ void pnp_betas_ls(const EpnpWs &W, const int (&cols)[K], double (&x)[K])
{
    double a[6][K], b[6][1], xs[K][1];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        b[i][0] = W.f[F_RHO + i];
#pragma unroll
        for (int j = 0; j < K; j++) a[i][j] = W.f[F_L + 10 * i + cols[j]];
    }
    svd_ls<6, K, 1>(a, b, xs);
#pragma unroll
    for (int j = 0; j < K; j++) x[j] = xs[j][0];
}

// find_betas_approx_1/2/3 (:937-1039), gauss_newton (:1213-1247), compute_ccs (:649-665) and solve_for_sign (:897-914) of solution `a`; one lane
__device__ void pnp_solution(EpnpWs &W, const int a, const PnpPts &P)
{
    double betas[4] = {0.0, 0.0, 0.0, 0.0};
    if (a == 0) {
        const int cols[4] = {0, 1, 3, 6};
        double b4[4];
        pnp_betas_ls<4>(W, cols, b4);
        if (b4[0] < 0) { betas[0] = sqrt(-b4[0]); betas[1] = -b4[1] / betas[0]; betas[2] = -b4[2] / betas[0]; betas[3] = -b4[3] / betas[0]; }
        else { betas[0] = sqrt(b4[0]); betas[1] = b4[1] / betas[0]; betas[2] = b4[2] / betas[0]; betas[3] = b4[3] / betas[0]; }
    } else if (a == 1) {
        const int cols[3] = {0, 1, 2};
        double b3[3];
        pnp_betas_ls<3>(W, cols, b3);
        if (b3[0] < 0) { betas[0] = sqrt(-b3[0]); betas[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0; }
        else { betas[0] = sqrt(b3[0]); betas[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0; }
        if (b3[1] < 0) betas[0] = -betas[0];
    } else {
        const int cols[5] = {0, 1, 2, 3, 4};
        double b5[5];
        pnp_betas_ls<5>(W, cols, b5);
        if (b5[0] < 0) { betas[0] = sqrt(-b5[0]); betas[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0; }
        else { betas[0] = sqrt(b5[0]); betas[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0; }
        if (b5[1] < 0) betas[0] = -betas[0];
        betas[2] = b5[3] / betas[0];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) W.f[F_B0 + 4 * a + j] = betas[j];
#pragma unroll 1
    for (int k = 0; k < 5; k++) {
        double A[24], b[6], x[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double L[10];
#pragma unroll
            for (int j = 0; j < 10; j++) L[j] = W.f[F_L + 10 * i + j];
            A[4 * i] = (((2 * L[0]) * betas[0] + L[1] * betas[1]) + L[3] * betas[2]) + L[6] * betas[3];
            A[4 * i + 1] = ((L[1] * betas[0] + (2 * L[2]) * betas[1]) + L[4] * betas[2]) + L[7] * betas[3];
            A[4 * i + 2] = ((L[3] * betas[0] + L[4] * betas[1]) + (2 * L[5]) * betas[2]) + L[8] * betas[3];
            A[4 * i + 3] = ((L[6] * betas[0] + L[7] * betas[1]) + L[8] * betas[2]) + (2 * L[9]) * betas[3];
            b[i] = W.f[F_RHO + i] - ((((((((((L[0] * betas[0]) * betas[0] + (L[1] * betas[0]) * betas[1]) + (L[2] * betas[1]) * betas[1]) + (L[3] * betas[0]) * betas[2]) +
                                           (L[4] * betas[1]) * betas[2]) + (L[5] * betas[2]) * betas[2]) + (L[6] * betas[0]) * betas[3]) + (L[7] * betas[1]) * betas[3]) +
                                       (L[8] * betas[2]) * betas[3]) + (L[9] * betas[3]) * betas[3]);
        }
        pnp_qr_solve(A, b, x);
#pragma unroll
        for (int i = 0; i < 4; i++) betas[i] = betas[i] + x[i];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) W.f[F_B1 + 4 * a + j] = betas[j];
    double ccs[12];
#pragma unroll
    for (int j = 0; j < 12; j++) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) s = s + betas[i] * W.f[F_UT + 12 * (11 - i) + j];
        ccs[j] = s;
    }
    const int i0 = pnp_first(P);
    bool neg = false;
    if (i0 >= 0) {
        double al[4];
        pnp_alphas(W, P.world + 3 * (size_t)i0, al);
        neg = (((al[0] * ccs[2] + al[1] * ccs[5]) + al[2] * ccs[8]) + al[3] * ccs[11]) < 0.0;
    }
#pragma unroll
    for (int j = 0; j < 12; j++) W.ccs[12 * a + j] = neg ? -ccs[j] : ccs[j];
}

// estimate_R_and_t behind the sums (:863-885) and reprojection_error (:790-813) of solution `a`; one lane
__device__ void pnp_pose(EpnpWs &W, const int a, const PnpPts &P, const double fu, const double fv, const double uc, const double vc, const double dm)
{
    double B[3][3], v[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) B[i][j] = W.abt[9 * a + 3 * i + j];
    onesided_jacobi<3, 3>(B, v);
    double U[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double sig = sqrt((B[0][k] * B[0][k] + B[1][k] * B[1][k]) + B[2][k] * B[2][k]);
#pragma unroll
        for (int i = 0; i < 3; i++) U[i][k] = B[i][k] / sig;
    }
    double R[3][3], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = (U[i][0] * v[j][0] + U[i][1] * v[j][1]) + U[i][2] * v[j][2];
    const double det = (((((R[0][0] * R[1][1]) * R[2][2] + (R[0][1] * R[1][2]) * R[2][0]) + (R[0][2] * R[1][0]) * R[2][1]) - (R[0][2] * R[1][1]) * R[2][0]) -
                        (R[0][1] * R[1][0]) * R[2][2]) - (R[0][0] * R[1][2]) * R[2][1];
    if (det < 0) { R[2][0] = -R[2][0]; R[2][1] = -R[2][1]; R[2][2] = -R[2][2]; }
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = W.pc0[3 * a + i] - ((R[i][0] * W.f[F_CWS] + R[i][1] * W.f[F_CWS + 1]) + R[i][2] * W.f[F_CWS + 2]);
    double sum2 = 0.0;
    pnp_for_each(P, [&](int i) {
        const double x = (double)P.world[3 * (size_t)i], y = (double)P.world[3 * (size_t)i + 1], z = (double)P.world[3 * (size_t)i + 2];
        const double Xc = ((R[0][0] * x + R[0][1] * y) + R[0][2] * z) + t[0], Yc = ((R[1][0] * x + R[1][1] * y) + R[1][2] * z) + t[1];
        const double inv_Zc = 1.0 / (((R[2][0] * x + R[2][1] * y) + R[2][2] * z) + t[2]);
        const double ue = uc + (fu * Xc) * inv_Zc, ve = vc + (fv * Yc) * inv_Zc;
        const float2 p = P.uv[i];
        const double u = (double)p.x, vv = (double)p.y;
        sum2 = sum2 + sqrt((u - ue) * (u - ue) + (vv - ve) * (vv - ve));
    });
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) W.f[F_RS + 9 * a + 3 * i + j] = R[i][j];
        W.f[F_TS + 3 * a + i] = t[i];
    }
    W.f[F_ERR + a] = sum2 / dm;
}

// camera-frame coordinate j of a point from its barycentric coordinates and solution a's control points (:669-681)
__device__ __forceinline__ double pnp_pc(const EpnpWs &W, const int a, const int j, const double (&al)[4])
{
    const double *c = W.ccs + 12 * a;
    return ((al[0] * c[j] + al[1] * c[3 + j]) + al[2] * c[6 + j]) + al[3] * c[9 + j];
}

// compute_pose (:684-759) by a team of T lanes of ONE workgroup whose every thread calls this (the barriers are the workgroup's)
template <int T> __device__ void epnp_solve(EpnpWs &W, const int lane, const PnpPts P, const double fu, const double fv, const double uc, const double vc, const bool active,
                                            double *Rout, double *tout, double *errOut, double *full, double *alphasOut)
{
    const double dm = (double)P.m;
    if (lane < 3) {      // :511-518
        double s = 0.0;
        pnp_for_each(P, [&](int i) { s = s + (double)P.world[3 * (size_t)i + lane]; });
        W.f[F_CWS + lane] = s / dm;
    }
    __syncthreads();
    if (lane < 9) {      // :536-544
        const int a = lane / 3, b = lane % 3;
        const double ca = W.f[F_CWS + a], cb = W.f[F_CWS + b];
        double s = 0.0;
        pnp_for_each(P, [&](int i) { s = s + ((double)P.world[3 * (size_t)i + a] - ca) * ((double)P.world[3 * (size_t)i + b] - cb); });
        W.f[F_PCA + lane] = s;
    }
    __syncthreads();
    if (lane == 0) pnp_control_points(W, dm);
    __syncthreads();
    if (alphasOut && active && P.set)
        for (int k = lane; k < P.m; k += T) {
            double al[4];
            pnp_alphas(W, P.world + 3 * (size_t)P.set[k], al);
            for (int j = 0; j < 4; j++) alphasOut[4 * (size_t)k + j] = al[j];
        }
    // fill_M (:627-645) and M^T M (:707), the upper triangle entry by entry
    for (int e = lane; e < 78; e += T) {
        int r = 0, rem = e;
        while (rem >= 12 - r) { rem -= 12 - r; r++; }
        const int c = r + rem;
        const int kr = r / 3, jr = r % 3, kc = c / 3, jc = c % 3;
        double acc = 0.0;
        pnp_for_each(P, [&](int i) {
            double al[4];
            pnp_alphas(W, P.world + 3 * (size_t)i, al);
            const float2 p = P.uv[i];
            const double du = uc - (double)p.x, dv = vc - (double)p.y;
            const double ar = pnp_sel4(al, kr), ac = pnp_sel4(al, kc);
            const double m1r = jr == 0 ? ar * fu : jr == 1 ? 0.0 : ar * du, m1c = jc == 0 ? ac * fu : jc == 1 ? 0.0 : ac * du;
            const double m2r = jr == 0 ? 0.0 : jr == 1 ? ar * fv : ar * dv, m2c = jc == 0 ? 0.0 : jc == 1 ? ac * fv : ac * dv;
            acc = (acc + m1r * m1c) + m2r * m2c;
        });
        W.f[F_MTM + 12 * r + c] = acc; W.f[F_MTM + 12 * c + r] = acc;
        W.f[F_UT + 12 * r + c] = acc; W.f[F_UT + 12 * c + r] = acc;
    }
    for (int e = lane; e < 144; e += T) W.V[e] = e / 12 == e % 12 ? 1.0 : 0.0;
    __syncthreads();
    // the eigenvectors of M^T M (:708): cyclic two-sided Jacobi, lane r owns row / column r; the diagonal moves by t * gamma (the classical update,
    // which keeps the eigenvalues to a few ulp of the norm), the matrix stays exactly symmetric
    {
        double *A = W.f + F_UT;
        const int r = lane;
#pragma unroll 1
        for (int sweep = 0; sweep < PNP_SWEEPS12; sweep++) {
            // The early exits are votes of the wave: a workgroup of k_pnp_models is ONE wave of four teams, which must meet the same barriers, and
            // the lanes of k_pnp_refine's one team all read the same three entries, so both of its waves vote alike.  A team that has settled
            // applies identities while the others finish: the same bits.
            bool rotated = false;
#pragma unroll 1
            for (int p = 0; p < 11; p++) {
#pragma unroll 1
                for (int q = p + 1; q < 12; q++) {
                    const double alpha = A[13 * p], beta = A[13 * q], gamma = A[12 * p + q];
                    if (__all(gamma == 0.0 || !active)) continue;      // already annihilated: the identity, and nothing to set to zero
                    double c, s, t;
                    const bool rot = jacobi_cst(alpha, beta, gamma, PNP_TINY * (fabs(alpha) + fabs(beta)), c, s, t);
                    rotated = __any(rot && active) || rotated;
                    __syncthreads();
                    if (r < 12) {
                        if (r == p) { A[13 * p] = alpha - t * gamma; A[12 * p + q] = 0.0; }
                        else if (r == q) { A[13 * q] = beta + t * gamma; A[12 * q + p] = 0.0; }
                        else {
                            const double ap = A[12 * r + p], aq = A[12 * r + q];
                            const double np_ = c * ap - s * aq, nq = s * ap + c * aq;
                            A[12 * r + p] = np_; A[12 * p + r] = np_;
                            A[12 * r + q] = nq; A[12 * q + r] = nq;
                        }
                        const double vp = W.V[12 * r + p], vq = W.V[12 * r + q];
                        W.V[12 * r + p] = c * vp - s * vq; W.V[12 * r + q] = s * vp + c * vq;
                    }
                    __syncthreads();
                }
            }
            if (!rotated) break;      // a sweep without a rotation leaves every off-diagonal entry exactly zero: the later sweeps are identities
        }
        if (lane == 0) {
            for (int k = 0; k < 12; k++) W.dr[k] = A[13 * k];
            pnp_order(W.dr, 12, W.order);
            for (int k = 0; k < 12; k++) W.f[F_D + k] = fabs(W.dr[W.order[k]]);
        }
        __syncthreads();
        for (int e = lane; e < 144; e += T) A[e] = W.V[12 * (e % 12) + W.order[e / 12]];      // Ut: row k = the eigenvector of the k-th largest
    }
    __syncthreads();
    if (lane < 6) {      // compute_L_6x10 (:1042-1101), compute_rho (:1104-1113): row `lane`
        const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
        const int a = pa[lane], b = pb[lane];
        double dv[4][3];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double *v = W.f + F_UT + 12 * (11 - i);
#pragma unroll
            for (int k = 0; k < 3; k++) dv[i][k] = v[3 * a + k] - v[3 * b + k];
        }
        auto dot = [&](int i, int j) { return (dv[i][0] * dv[j][0] + dv[i][1] * dv[j][1]) + dv[i][2] * dv[j][2]; };
        double *row = W.f + F_L + 10 * lane;
        row[0] = dot(0, 0); row[1] = 2.0 * dot(0, 1); row[2] = dot(1, 1); row[3] = 2.0 * dot(0, 2); row[4] = 2.0 * dot(1, 2);
        row[5] = dot(2, 2); row[6] = 2.0 * dot(0, 3); row[7] = 2.0 * dot(1, 3); row[8] = 2.0 * dot(2, 3); row[9] = dot(3, 3);
        const double *c1 = W.f + F_CWS + 3 * a, *c2 = W.f + F_CWS + 3 * b;
        W.f[F_RHO + lane] = ((c1[0] - c2[0]) * (c1[0] - c2[0]) + (c1[1] - c2[1]) * (c1[1] - c2[1])) + (c1[2] - c2[2]) * (c1[2] - c2[2]);
    }
    __syncthreads();
    if (lane < 3) pnp_solution(W, lane, P);
    __syncthreads();
    for (int e = lane; e < 9; e += T) {      // :822-838, pc0 of the three solutions (pw0 is cws[0]: the same sum, the same quotient)
        const int a = e / 3, j = e % 3;
        double s = 0.0;
        pnp_for_each(P, [&](int i) {
            double al[4];
            pnp_alphas(W, P.world + 3 * (size_t)i, al);
            s = s + pnp_pc(W, a, j, al);
        });
        W.pc0[e] = s / dm;
    }
    __syncthreads();
    for (int e = lane; e < 27; e += T) {      // :848-861
        const int a = e / 9, j = (e % 9) / 3, k = e % 3;
        const double pcj = W.pc0[3 * a + j], pwk = W.f[F_CWS + k];
        double s = 0.0;
        pnp_for_each(P, [&](int i) {
            double al[4];
            pnp_alphas(W, P.world + 3 * (size_t)i, al);
            s = s + (pnp_pc(W, a, j, al) - pcj) * ((double)P.world[3 * (size_t)i + k] - pwk);
        });
        W.abt[e] = s;
    }
    __syncthreads();
    if (lane < 3) pnp_pose(W, lane, P, fu, fv, uc, vc, dm);
    __syncthreads();
    if (lane == 0) {      // :750-752
        int N = 1;
        if (W.f[F_ERR + 1] < W.f[F_ERR]) N = 2;
        if (W.f[F_ERR + 2] < W.f[F_ERR + N - 1]) N = 3;
        W.f[F_CHOICE] = (double)N;
        W.order[0] = N - 1;
    }
    __syncthreads();
    if (active) {
        const int ch = W.order[0];
        for (int e = lane; e < 9; e += T) Rout[e] = W.f[F_RS + 9 * ch + e];
        if (lane < 3) tout[lane] = W.f[F_TS + 3 * ch + lane];
        if (lane == 0) *errOut = W.f[F_ERR + ch];
        if (full)
            for (int e = lane; e < PNP_FULL; e += T) full[e] = W.f[e];
    }
    __syncthreads();
}

// sets / outputs are passed apart from D: orbx_pnp_epnp runs explicit sets of any size into buffers of its own
__global__ __launch_bounds__(64) void k_pnp_models(PnpDev D, const int32_t *__restrict__ sets, int setSize, double *__restrict__ R, double *__restrict__ t, double *__restrict__ err,
                                                   double *__restrict__ full, double *__restrict__ alphas)
{
    __shared__ EpnpWs ws[64 / PNP_TEAM];
    const PnpCand *hc = D.cand + blockIdx.y;
    const int team = threadIdx.x / PNP_TEAM, lane = threadIdx.x % PNP_TEAM;
    const int it = blockIdx.x * (64 / PNP_TEAM) + team;
    const bool active = it < hc->iters;
    const size_t g = (size_t)hc->ib + (active ? it : 0), mb = (size_t)hc->mb;
    PnpPts P;
    P.set = sets + (size_t)setSize * g; P.mask = nullptr; P.m = active ? setSize : 0; P.words = 0;
    P.world = D.world + 3 * mb; P.uv = D.uv + mb;
    epnp_solve<PNP_TEAM>(ws[team], lane, P, (double)hc->k[0], (double)hc->k[1], (double)hc->k[2], (double)hc->k[3], active, R + 9 * g, t + 3 * g, err + g,
                         full ? full + (size_t)PNP_FULL * g : nullptr, alphas ? alphas + 4 * (size_t)setSize * g : nullptr);
}

__global__ __launch_bounds__(PNP_REFINE_THREADS) void k_pnp_refine(PnpDev D)
{
    __shared__ EpnpWs ws;
    const int c = blockIdx.y, r = blockIdx.x;
    const PnpCand *hc = D.cand + c;
    if (r >= D.nrec[c]) return;      // uniform in the workgroup
    const size_t ib = (size_t)hc->ib, mb = (size_t)hc->mb;
    const int it = D.recIter[ib + r];
    PnpPts P;
    P.set = nullptr; P.mask = D.mask + hc->wb + (size_t)it * hc->words; P.m = D.count[ib + it]; P.words = hc->words;
    P.world = D.world + 3 * mb; P.uv = D.uv + mb;
    const size_t g = ib + r;
    epnp_solve<PNP_REFINE_THREADS>(ws, threadIdx.x, P, (double)hc->k[0], (double)hc->k[1], (double)hc->k[2], (double)hc->k[3], true, D.refR + 9 * g, D.refT + 3 * g, D.refErr + g,
                                   nullptr, nullptr);
}

#define PNP_CHECK_WAVES 4
// CheckInliers (:421-458).  limits == nullptr: every iteration of the candidate; else limits[candidate] models (the records' refined poses)
__global__ __launch_bounds__(64 * PNP_CHECK_WAVES) void k_pnp_check(PnpDev D, const double *__restrict__ R, const double *__restrict__ t, const int32_t *__restrict__ limits,
                                                                     int32_t *__restrict__ count, unsigned long long *__restrict__ mask)
{
    const PnpCand *hc = D.cand + blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int it = blockIdx.x * PNP_CHECK_WAVES + (threadIdx.x >> 6);      // uniform in a wave
    if (it >= (limits ? limits[blockIdx.y] : hc->iters)) return;
    const int n = hc->n;
    const size_t g = (size_t)hc->ib + it, mb = (size_t)hc->mb;
    double A[9], b[3];
#pragma unroll
    for (int j = 0; j < 9; j++) A[j] = R[9 * g + j];
#pragma unroll
    for (int j = 0; j < 3; j++) b[j] = t[3 * g + j];
    const double fu = (double)hc->k[0], fv = (double)hc->k[1], uc = (double)hc->k[2], vc = (double)hc->k[3];
    unsigned long long *row = mask + hc->wb + (size_t)it * hc->words;
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool inl = false;
        if (i < n) {
            const size_t k = mb + i;
            const double x = (double)D.world[3 * k], y = (double)D.world[3 * k + 1], z = (double)D.world[3 * k + 2];
            const float Xc = (float)((((A[0] * x + A[1] * y) + A[2] * z) + b[0]));
            const float Yc = (float)((((A[3] * x + A[4] * y) + A[5] * z) + b[1]));
            const float invZc = (float)(1.0 / (((A[6] * x + A[7] * y) + A[8] * z) + b[2]));
            const double ue = uc + (fu * (double)Xc) * (double)invZc, ve = vc + (fv * (double)Yc) * (double)invZc;
            const float2 p = D.uv[k];
            const float distX = (float)((double)p.x - ue), distY = (float)((double)p.y - ve);
            const float error2 = distX * distX + distY * distY;
            inl = error2 < D.maxErr[k];
        }
        const unsigned long long m = __ballot(inl);
        if (lane == 0) row[base >> 6] = m;
        cnt += __popcll(m);
    }
    if (lane == 0) count[g] = cnt;
}

__global__ __launch_bounds__(64) void k_pnp_records(PnpDev D)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    const PnpCand *hc = D.cand + c;
    const int iters = hc->iters, minInl = hc->minInliers;
    const size_t ib = (size_t)hc->ib;
    int carry = 0, nrec = 0;      // mnBestInliers starts at 0
    for (int base = 0; base < iters; base += 64) {
        const int it = base + tid;
        const int cnt = it < iters ? D.count[ib + it] : 0;
        const int v = cnt >= minInl ? cnt : 0;
        int incl = v;      // (inclusive maximum scan, written out here and in k_sim3_decide: as a shared helper both kernels come out with other instructions)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (tid >= d) incl = max(incl, o);
        }
        int excl = __shfl_up(incl, 1);
        excl = tid == 0 ? carry : max(excl, carry);
        const bool rec = it < iters && v > excl;
        const unsigned long long br = __ballot(rec);
        const int before = nrec + __popcll(br & ((tid == 63) ? ~0ull : ((1ull << (tid + 1)) - 1ull)));      // records at or before `it`
        if (it < iters) D.recordOf[ib + it] = before - 1;
        if (rec) D.recIter[ib + before - 1] = it;
        nrec += __popcll(br);
        carry = max(carry, __shfl(incl, 63));
    }
    if (tid == 0) D.nrec[c] = nrec;
}

#define PNP_DECIDE_THREADS 256
__global__ __launch_bounds__(PNP_DECIDE_THREADS) void k_pnp_decide(PnpDev D, uint8_t *__restrict__ out, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    __shared__ int32_t sFirst;
    const int c = blockIdx.x, tid = threadIdx.x;
    const PnpCand *hc = D.cand + c;
    const int n = hc->n, iters = hc->iters, minInl = hc->minInliers;
    const int nrec = iters > 0 ? D.nrec[c] : 0;
    const size_t ib = (size_t)hc->ib;
    const PnpBlock L(n, iters);
    uint8_t *blk = out + hc->outOff;
    if (tid < 64) {
        int first = -1;
        for (int base = 0; base < iters; base += 64) {
            const int it = base + tid;
            bool ev = false;
            if (it < iters) {
                const int rec = D.recordOf[ib + it];
                ev = D.count[ib + it] >= minInl && rec >= 0 && D.refCount[ib + rec] > minInl;
                blk[L.isEvent + it] = ev ? 1 : 0;
            }
            const unsigned long long be = __ballot(ev);
            if (first < 0 && be) first = base + __ffsll((long long)be) - 1;
        }
        if (tid == 0) sFirst = first;
    }
    __syncthreads();
    const int first = sFirst;
    const int best = nrec > 0 ? D.recIter[ib + nrec - 1] : -1;
    if (tid == 0) {
        int32_t *head = (int32_t *)blk;
        head[0] = first; head[1] = best; head[2] = n < minInl ? 1 : 0; head[3] = nrec; head[4] = minInl; head[5] = 0; head[6] = 0; head[7] = 0;
    }
    double *oR = (double *)(blk + L.r), *oT = (double *)(blk + L.t), *oE = (double *)(blk + L.err), *oRR = (double *)(blk + L.refR), *oRT = (double *)(blk + L.refT);
    float *oTcw = (float *)(blk + L.refTcw), *oBest = (float *)(blk + L.bestTcw);
    int32_t *oc = (int32_t *)(blk + L.count), *oro = (int32_t *)(blk + L.recordOf), *ori = (int32_t *)(blk + L.recIter), *orc = (int32_t *)(blk + L.refCount);
    for (int j = tid; j < iters; j += PNP_DECIDE_THREADS) {
        oc[j] = D.count[ib + j]; oro[j] = D.recordOf[ib + j]; oE[j] = D.err[ib + j];
        ori[j] = j < nrec ? D.recIter[ib + j] : -1; orc[j] = j < nrec ? D.refCount[ib + j] : 0;
    }
    for (int j = tid; j < 9 * iters; j += PNP_DECIDE_THREADS) { oR[j] = D.r[9 * ib + j]; oRR[j] = j < 9 * nrec ? D.refR[9 * ib + j] : 0.0; }
    for (int j = tid; j < 3 * iters; j += PNP_DECIDE_THREADS) { oT[j] = D.t[3 * ib + j]; oRT[j] = j < 3 * nrec ? D.refT[3 * ib + j] : 0.0; }
    // :407-413 / :310-316: Rcw | tcw narrowed to float, rows of [R | t]
    for (int j = tid; j < 12 * iters; j += PNP_DECIDE_THREADS) {
        const int r = j / 12, e = j % 12, row = e / 4, col = e % 4;
        oTcw[j] = r < nrec ? (float)(col < 3 ? D.refR[9 * (ib + r) + 3 * row + col] : D.refT[3 * (ib + r) + row]) : 0.0f;
    }
    if (tid < 12) {
        const int row = tid / 4, col = tid % 4;
        oBest[tid] = best >= 0 ? (float)(col < 3 ? D.r[9 * (ib + best) + 3 * row + col] : D.t[3 * (ib + best) + row]) : 0.0f;
    }
    const int frec = first >= 0 ? D.recordOf[ib + first] : 0;
    const unsigned long long *rowF = D.refMask + hc->wb + (size_t)frec * hc->words;
    const unsigned long long *rowB = D.mask + hc->wb + (size_t)(best < 0 ? 0 : best) * hc->words;
    for (int i = tid; i < n; i += PNP_DECIDE_THREADS) {
        blk[L.inlFirst + i] = first < 0 ? 0 : (uint8_t)((rowF[i >> 6] >> (i & 63)) & 1ull);
        blk[L.inlBest + i] = best < 0 ? 0 : (uint8_t)((rowB[i >> 6] >> (i & 63)) & 1ull);
    }
    orbx_publish(counter, flag, seq, gridDim.x);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------------
struct orbx_pnp_solver : OrbxHandle {
    int maxCands = 0, maxMatches = 0, maxIters = 0;
    OrbxCallTimer timer;
    bool solved = false;
    OrbxCallBox box;
    OrbxOwnedBuf<float> pts;                // 6 floats per match
    OrbxOwnedBuf<double> models;            // 26 doubles per iteration
    OrbxOwnedBuf<int32_t> sets, ints, nrec, cmCount, epSets;
    OrbxOwnedBuf<PnpCand> cand;
    OrbxOwnedBuf<unsigned long long> mask, cmMask;
    OrbxOwnedBuf<double> epOut, epFull, epAlphas;
    std::vector<PnpCand> last;            // the candidates of the last solve (orbx_pnp_inliers)
    std::vector<int32_t> lastNrec;        // ... and how many records each of them has (orbx_pnp_device_rows_internal)
};

namespace {
PnpDev dev_view(orbx_pnp_solver *h)
{
    const size_t P = (size_t)h->maxCands * h->maxMatches, I = (size_t)h->maxCands * h->maxIters, W = (size_t)(h->maxMatches + 63) / 64;
    PnpDev D;
    float *p = h->pts.p;
    D.world = p; D.uv = (float2 *)(p + 3 * P); D.maxErr = p + 5 * P;
    double *m = h->models.p;
    D.r = m; D.t = m + 9 * I; D.err = m + 12 * I; D.refR = m + 13 * I; D.refT = m + 22 * I; D.refErr = m + 25 * I;
    int32_t *q = h->ints.p;
    D.count = q; D.refCount = q + I; D.recordOf = q + 2 * I; D.recIter = q + 3 * I;
    D.nrec = h->nrec.p; D.sets = h->sets.p; D.cand = h->cand.p; D.mask = h->mask.p; D.refMask = h->mask.p + I * W;
    return D;
}

struct PnpParams { int minInliers, maxIts; float eps; };

// SetRansacParameters (:181-223) with the reference's libm calls
PnpParams ransac_parameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, int N)
{
    PnpParams o;
    int nMinInliers = (int)((float)N * epsilon);      // int N * float: a float product, truncated
    if (nMinInliers < minInliers) nMinInliers = minInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    o.minInliers = nMinInliers;
    if (epsilon < (float)nMinInliers / N) epsilon = (float)nMinInliers / N;
    o.eps = epsilon;
    int nIterations;
    if (nMinInliers == N) nIterations = 1;
    else {
        const double x = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
        // the reference converts x to int unchecked; out of range or NaN (N < minInliers) is what the x86 conversion makes of it
        nIterations = (x >= -2147483648.0 && x <= 2147483647.0) ? (int)x : INT_MIN;
    }
    o.maxIts = std::max(1, std::min(nIterations, maxIterations));
    return o;
}

struct PnpStaged { OrbxStaged sg; OrbxSlot<double, ORBX_STAGE_IN> extraA, extraB; OrbxSlot<uint8_t, ORBX_STAGE_OUT> res; };      // res: the candidates' PnpBlocks

int check_problem(const orbx_pnp_solver *h, const orbx_pnp_problem *P, int c, bool withSets, int &iters, int &minInl)
{
    if (P->n < 0 || P->iterations < 0 || (P->n > 0 && (!P->p2d || !P->p3dw || !P->sigma2))) {
        orbx_set_error("candidate %d: n = %d, iterations = %d or a NULL array", c, P->n, P->iterations);
        return ORBX_ERR_ARG;
    }
    if (P->n > h->maxMatches) { orbx_set_error("candidate %d: %d matches, the solver was created for %d", c, P->n, h->maxMatches); return ORBX_ERR_CAPACITY; }
    iters = 0;
    minInl = ransac_parameters(P->probability, P->min_inliers, P->max_iterations, P->min_set, P->epsilon, P->n).minInliers;
    if (!withSets) return ORBX_OK;
    iters = P->n < minInl ? 0 : P->iterations;      // :250-254
    if (iters > h->maxIters) { orbx_set_error("candidate %d: %d iterations, the solver was created for %d", c, iters, h->maxIters); return ORBX_ERR_CAPACITY; }
    if (iters > 0 && (P->n < 4 || !P->sets)) { orbx_set_error("candidate %d: %d matches, a set needs 4 (or NULL sets)", c, P->n); return ORBX_ERR_ARG; }
    for (int i = 0; i < iters; i++) {
        const int32_t *s = P->sets + 4 * (size_t)i;
        for (int j = 0; j < 4; j++) {
            if (s[j] < 0 || s[j] >= P->n) { orbx_set_error("candidate %d: sets[%d][%d] = %d is outside the %d matches", c, i, j, s[j], P->n); return ORBX_ERR_ARG; }
            for (int k = 0; k < j; k++)
                if (s[k] == s[j]) { orbx_set_error("candidate %d: sets[%d] repeats an index", c, i); return ORBX_ERR_ARG; }
        }
    }
    return ORBX_OK;
}

// headers + arrays of `nc` candidates into the mapped input buffer; iters[c] = iterations to run (sets are staged when withSets); extraA / extraB doubles of
// room for the caller behind them; outBytes of results, 0 = the candidates' PnpBlocks
PnpStaged stage(orbx_pnp_solver *h, const orbx_pnp_problem *Ps, int nc, const std::vector<int> &iters, const std::vector<int> &minInl, bool withSets, size_t extraA, size_t extraB,
                size_t outBytes, std::vector<PnpCand> &cands, PnpIn &I, int *rc)
{
    size_t totN = 0, totIt = 0, totW = 0, off = 0;
    cands.assign((size_t)nc, PnpCand());
    for (int c = 0; c < nc; c++) {
        const orbx_pnp_problem &P = Ps[c];
        PnpCand &H = cands[c];
        H.k[0] = P.fx; H.k[1] = P.fy; H.k[2] = P.cx; H.k[3] = P.cy; H.th2 = P.th2;
        H.n = P.n; H.iters = iters[c]; H.minInliers = minInl[c];
        H.mb = (int32_t)totN; H.ib = (int32_t)totIt; H.words = (P.n + 63) / 64; H.pad = 0; H.wb = totW; H.outOff = off;
        totN += (size_t)P.n; totIt += (size_t)iters[c]; totW += (size_t)H.words * (size_t)iters[c];
        off += PnpBlock(P.n, iters[c]).total;
    }
    OrbxCallBox &bx = h->box;
    auto [pin, pout] = bx.plan();
    // the candidates' arrays lie concatenated, candidate c's at element mb (matches) / ib (sets) of its region: holes, filled below
    const auto sCand = pin.add(cands.data(), (size_t)nc);
    const auto sWorld = pin.hole<float>(totN * 3), sUv = pin.hole<float>(totN * 2), sSigma = pin.hole<float>(totN);
    const auto sSets = pin.hole<int32_t>(withSets ? totIt * 4 : 0);
    const auto sA = pin.hole<double>(extraA), sB = pin.hole<double>(extraB);
    const auto rRes = pout.hole<uint8_t>(outBytes ? outBytes : off);
    const PnpStaged S = {bx.begin(h->stream, rc), sA, sB, rRes};
    if (*rc != ORBX_OK) return S;
    for (int c = 0; c < nc; c++) {
        const orbx_pnp_problem &P = Ps[c];
        const PnpCand &H = cands[c];
        const size_t n = (size_t)P.n, mb = (size_t)H.mb;
        orbx_put_at(S.sg, sWorld, 3 * mb, P.p3dw, 3 * n); orbx_put_at(S.sg, sUv, 2 * mb, P.p2d, 2 * n); orbx_put_at(S.sg, sSigma, mb, P.sigma2, n);
        if (withSets) orbx_put_at(S.sg, sSets, 4 * (size_t)H.ib, P.sets, 4 * (size_t)H.iters);
    }
    I.cand = S.sg.dev(sCand);
    I.world = S.sg.dev(sWorld); I.uv = S.sg.dev(sUv); I.sigma = S.sg.dev(sSigma);
    I.sets = S.sg.dev(sSets);
    return S;
}

unsigned prepare_blocks(int maxN, int maxIt) { return (unsigned)std::max(1, (std::max(maxN, 4 * maxIt) + 255) / 256); }

}  // namespace

extern "C" int orbx_pnp_ransac_parameters(double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2, int n, int *min_inliers_out,
                                          int *iterations_out, float *epsilon_out)
{
    (void)th2;      // only mvMaxError depends on it
    if (n < 0) { orbx_set_error("n = %d", n); return ORBX_ERR_ARG; }
    const PnpParams o = ransac_parameters(probability, min_inliers, max_iterations, min_set, epsilon, n);
    if (min_inliers_out) *min_inliers_out = o.minInliers;
    if (iterations_out) *iterations_out = o.maxIts;
    if (epsilon_out) *epsilon_out = o.eps;
    return ORBX_OK;
}

extern "C" int orbx_pnp_solver_create(int device, int max_candidates, int max_matches, int max_iterations, orbx_pnp_solver **out)
{
    if (!out || max_candidates < 1 || max_candidates > 4096 || max_matches < 4 || max_matches > ORBX_PNP_MAX_MATCHES || max_iterations < 1 || max_iterations > (1 << 16)) {
        orbx_set_error("bad PnP solver arguments (max_candidates >= 1, 4 <= max_matches <= %d, max_iterations >= 1)", ORBX_PNP_MAX_MATCHES);
        return ORBX_ERR_ARG;
    }
    *out = nullptr;
    orbx_pnp_solver *h = new orbx_pnp_solver();
    h->maxCands = max_candidates; h->maxMatches = max_matches; h->maxIters = max_iterations;
    const size_t P = (size_t)max_candidates * max_matches, I = (size_t)max_candidates * max_iterations, W = (size_t)(max_matches + 63) / 64;
    int rc;
    if ((rc = h->open(device)) || (rc = h->timer.create()) || (rc = h->pts.ensure(6 * P)) || (rc = h->models.ensure(26 * I)) || (rc = h->sets.ensure(4 * I)) || (rc = h->ints.ensure(4 * I)) || (rc = h->nrec.ensure((size_t)max_candidates)) ||
        (rc = h->cmCount.ensure((size_t)max_iterations)) || (rc = h->cand.ensure((size_t)max_candidates)) || (rc = h->mask.ensure(2 * I * W)) ||
        (rc = h->cmMask.ensure((size_t)max_iterations * W))) {
        orbx_pnp_solver_destroy(h);
        return rc;
    }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_pnp_solver_destroy(orbx_pnp_solver *h) { orbx_destroy_handle(h); }

extern "C" int orbx_pnp_solve(orbx_pnp_solver *h, const orbx_pnp_problem *Ps, int nc, const orbx_pnp_result *Rs)
{
    if (!h || !Ps || !Rs || nc < 1) { orbx_set_error("NULL argument or ncandidates = %d < 1", nc); return ORBX_ERR_ARG; }
    if (nc > h->maxCands) { orbx_set_error("%d candidates, the solver was created for %d", nc, h->maxCands); return ORBX_ERR_CAPACITY; }
    int rc, maxN = 0, maxIt = 0, maxRec = 0;
    std::vector<int> iters((size_t)nc, 0), minInl((size_t)nc, 0);
    for (int c = 0; c < nc; c++) {
        if ((rc = check_problem(h, Ps + c, c, true, iters[c], minInl[c])) != ORBX_OK) return rc;
        maxN = std::max(maxN, Ps[c].n); maxIt = std::max(maxIt, iters[c]);
        // a record needs count >= minInliers and a count above the record before it: at most n - minInliers + 1 of them
        if (iters[c] > 0) maxRec = std::max(maxRec, std::min(iters[c], Ps[c].n - minInl[c] + 1));
    }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    std::vector<PnpCand> cands;
    PnpIn I;
    const PnpStaged S = stage(h, Ps, nc, iters, minInl, true, 0, 0, 0, cands, I, &rc);
    if (rc != ORBX_OK) return rc;
    OrbxCallBox &bx = h->box;
    const PnpDev D = dev_view(h);
    h->solved = false;

    const unsigned long long seq = bx.arm();
    if ((rc = h->timer.begin(h->stream)) != ORBX_OK) return rc;
    hipLaunchKernelGGL(k_pnp_prepare, dim3(prepare_blocks(maxN, maxIt), (unsigned)nc), dim3(256), 0, h->stream, I, D, 1);
    ORBX_LAUNCH_COUNT(h->timer);
    if (maxIt > 0) {
        const unsigned teams = 64 / PNP_TEAM;
        hipLaunchKernelGGL(k_pnp_models, dim3((unsigned)((maxIt + teams - 1) / teams), (unsigned)nc), dim3(64), 0, h->stream, D, (const int32_t *)D.sets, 4, D.r, D.t, D.err, (double *)nullptr,
                           (double *)nullptr);
        ORBX_LAUNCH_COUNT(h->timer);
        hipLaunchKernelGGL(k_pnp_check, dim3((unsigned)((maxIt + PNP_CHECK_WAVES - 1) / PNP_CHECK_WAVES), (unsigned)nc), dim3(64 * PNP_CHECK_WAVES), 0, h->stream, D, (const double *)D.r,
                           (const double *)D.t, (const int32_t *)nullptr, D.count, D.mask);
        ORBX_LAUNCH_COUNT(h->timer);
        hipLaunchKernelGGL(k_pnp_records, dim3((unsigned)nc), dim3(64), 0, h->stream, D);
        ORBX_LAUNCH_COUNT(h->timer);
        if (maxRec > 0) {
            hipLaunchKernelGGL(k_pnp_refine, dim3((unsigned)maxRec, (unsigned)nc), dim3(PNP_REFINE_THREADS), 0, h->stream, D);
            ORBX_LAUNCH_COUNT(h->timer);
            hipLaunchKernelGGL(k_pnp_check, dim3((unsigned)((maxRec + PNP_CHECK_WAVES - 1) / PNP_CHECK_WAVES), (unsigned)nc), dim3(64 * PNP_CHECK_WAVES), 0, h->stream, D,
                               (const double *)D.refR, (const double *)D.refT, (const int32_t *)D.nrec, D.refCount, D.refMask);
            ORBX_LAUNCH_COUNT(h->timer);
            }
    }
    hipLaunchKernelGGL(k_pnp_decide, dim3((unsigned)nc), dim3(PNP_DECIDE_THREADS), 0, h->stream, D, S.sg.dev(S.res), bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_COUNT(h->timer);
    if ((rc = h->timer.end(h->stream)) != ORBX_OK) return rc;
    if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;      // the one synchronisation
    h->last = cands; h->solved = true;
    h->lastNrec.assign((size_t)nc, 0);

    bool diag = false;
    for (int c = 0; c < nc; c++) {
        const orbx_pnp_result &R = Rs[c];
        const PnpCand &H = cands[c];
        const size_t it = (size_t)H.iters, n = (size_t)H.n;
        const PnpBlock B(H.n, H.iters);
        const uint8_t *blk = S.sg.host(S.res) + H.outOff;
        const int32_t *head = (const int32_t *)blk;
        if (R.first_event) *R.first_event = head[0];
        if (R.best_iteration) *R.best_iteration = head[1];
        if (R.no_more) *R.no_more = head[2];
        if (R.nrecords) *R.nrecords = head[3];
        h->lastNrec[(size_t)c] = head[3];
        if (R.min_inliers) *R.min_inliers = head[4];
        if (R.count && it) memcpy(R.count, blk + B.count, it * 4);
        if (R.r && it) memcpy(R.r, blk + B.r, it * 72);
        if (R.t && it) memcpy(R.t, blk + B.t, it * 24);
        if (R.err && it) memcpy(R.err, blk + B.err, it * 8);
        if (R.record_of && it) memcpy(R.record_of, blk + B.recordOf, it * 4);
        if (R.record_iteration && it) memcpy(R.record_iteration, blk + B.recIter, it * 4);
        if (R.refined_count && it) memcpy(R.refined_count, blk + B.refCount, it * 4);
        if (R.refined_r && it) memcpy(R.refined_r, blk + B.refR, it * 72);
        if (R.refined_t && it) memcpy(R.refined_t, blk + B.refT, it * 24);
        if (R.refined_tcw && it) memcpy(R.refined_tcw, blk + B.refTcw, it * 48);
        if (R.best_tcw) memcpy(R.best_tcw, blk + B.bestTcw, 48);
        if (R.is_event && it) memcpy(R.is_event, blk + B.isEvent, it);
        if (R.inliers_first && n) memcpy(R.inliers_first, blk + B.inlFirst, n);
        if (R.inliers_best && n) memcpy(R.inliers_best, blk + B.inlBest, n);
        diag = diag || R.max_error;
    }
    if (diag) {
        // the per-match array (tests, diagnostics): a copy of its own
        ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
        for (int c = 0; c < nc; c++)
            if (Rs[c].max_error && cands[c].n) ORBX_HIP_CHECK(hipMemcpy(Rs[c].max_error, D.maxErr + cands[c].mb, (size_t)cands[c].n * 4, hipMemcpyDeviceToHost));
    }
    return ORBX_OK;
}

// Where the last solve left a candidate's refined records in DEVICE memory (orbx_internal.h; orbx_reloc.hip reads them in place)
int orbx_pnp_device_rows_internal(orbx_pnp_solver *h, int candidate, int device, OrbxPnpRows *out)
{
    if (!h || !out) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (!h->solved) { orbx_set_error("the PnP solver has no orbx_pnp_solve call to read from"); return ORBX_ERR_ARG; }
    if (h->device != device) { orbx_set_error("the PnP solver lives on device %d, the caller on device %d", h->device, device); return ORBX_ERR_ARG; }
    if (candidate < 0 || candidate >= (int)h->last.size()) { orbx_set_error("candidate %d outside the last solve (%d candidates)", candidate, (int)h->last.size()); return ORBX_ERR_ARG; }
    const PnpCand &H = h->last[(size_t)candidate];
    const PnpDev D = dev_view(h);
    out->refR = D.refR + 9 * (size_t)H.ib; out->refT = D.refT + 3 * (size_t)H.ib; out->refMask = D.refMask + H.wb;
    out->n = H.n; out->words = H.words; out->nrec = h->lastNrec[(size_t)candidate];
    return ORBX_OK;
}

extern "C" int orbx_pnp_inliers(orbx_pnp_solver *h, int candidate, int index, int refined, uint8_t *inliers)
{
    if (!h || !inliers) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (!h->solved) { orbx_set_error("no orbx_pnp_solve call to read from"); return ORBX_ERR_STATE; }
    if (candidate < 0 || candidate >= (int)h->last.size() || index < 0 || index >= h->last[candidate].iters) {
        orbx_set_error("candidate %d / index %d outside the last solve", candidate, index);
        return ORBX_ERR_ARG;
    }
    const PnpCand &H = h->last[candidate];
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const PnpDev D = dev_view(h);
    if (refined) {
        int32_t nrec = 0;
        ORBX_HIP_CHECK(hipMemcpy(&nrec, D.nrec + candidate, 4, hipMemcpyDeviceToHost));
        if (index >= nrec) { orbx_set_error("candidate %d has %d records, not %d", candidate, nrec, index + 1); return ORBX_ERR_ARG; }
    }
    std::vector<unsigned long long> row((size_t)H.words);
    if (H.words) ORBX_HIP_CHECK(hipMemcpy(row.data(), (refined ? D.refMask : D.mask) + H.wb + (size_t)index * H.words, (size_t)H.words * 8, hipMemcpyDeviceToHost));
    expand_mask(row.data(), H.n, inliers);
    return ORBX_OK;
}

extern "C" int orbx_pnp_check_models(orbx_pnp_solver *h, const orbx_pnp_problem *P, const double *R, const double *t, int m, int32_t *count, uint8_t *inliers)
{
    if (!h || !P || !R || !t || !count) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (m < 1) { orbx_set_error("m = %d models", m); return ORBX_ERR_ARG; }
    if (m > h->maxIters) { orbx_set_error("%d models, the solver holds %d", m, h->maxIters); return ORBX_ERR_CAPACITY; }
    int rc, unused = 0, minInl = 0;
    if ((rc = check_problem(h, P, 0, false, unused, minInl)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    std::vector<PnpCand> cands;
    PnpIn I;
    const std::vector<int> iters(1, m), mins(1, minInl);
    const PnpStaged S = stage(h, P, 1, iters, mins, false, (size_t)m * 9, (size_t)m * 3, 256, cands, I, &rc);
    if (rc != ORBX_OK) return rc;
    orbx_put_at(S.sg, S.extraA, 0, R, (size_t)m * 9); orbx_put_at(S.sg, S.extraB, 0, t, (size_t)m * 3);
    // the last solve's matches on the device are overwritten, its masks are not: orbx_pnp_inliers keeps working
    const PnpDev D = dev_view(h);
    hipLaunchKernelGGL(k_pnp_prepare, dim3(prepare_blocks(P->n, 0), 1), dim3(256), 0, h->stream, I, D, 0);
    ORBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pnp_check, dim3((unsigned)((m + PNP_CHECK_WAVES - 1) / PNP_CHECK_WAVES), 1), dim3(64 * PNP_CHECK_WAVES), 0, h->stream, D, (const double *)S.sg.dev(S.extraA),
                       (const double *)S.sg.dev(S.extraB), (const int32_t *)nullptr, h->cmCount.p, h->cmMask.p);
    ORBX_LAUNCH_CHECK();
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    ORBX_HIP_CHECK(hipMemcpy(count, h->cmCount.p, (size_t)m * 4, hipMemcpyDeviceToHost));
    if (inliers && P->n > 0) {
        const size_t W = (size_t)cands[0].words;
        std::vector<unsigned long long> rows(W * (size_t)m);
        ORBX_HIP_CHECK(hipMemcpy(rows.data(), h->cmMask.p, rows.size() * 8, hipMemcpyDeviceToHost));
        for (int k = 0; k < m; k++) expand_mask(rows.data() + W * (size_t)k, P->n, inliers + (size_t)k * (size_t)P->n);
    }
    return ORBX_OK;
}

extern "C" int orbx_pnp_epnp(orbx_pnp_solver *h, const orbx_pnp_problem *P, const int32_t *sets, int m, int set_size, double *R, double *t, double *err, double *full, double *alphas)
{
    if (!h || !P || !sets || !R || !t || !err) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (m < 1 || set_size < 4) { orbx_set_error("m = %d sets of %d indices (a set needs 4)", m, set_size); return ORBX_ERR_ARG; }
    if (m > h->maxIters) { orbx_set_error("%d sets, the solver holds %d", m, h->maxIters); return ORBX_ERR_CAPACITY; }
    int rc, unused = 0, minInl = 0;
    if ((rc = check_problem(h, P, 0, false, unused, minInl)) != ORBX_OK) return rc;
    if (set_size > P->n) { orbx_set_error("sets of %d indices into %d matches", set_size, P->n); return ORBX_ERR_ARG; }
    {
        std::vector<uint8_t> seen((size_t)P->n);
        for (int i = 0; i < m; i++) {
            std::fill(seen.begin(), seen.end(), 0);
            for (int j = 0; j < set_size; j++) {
                const int32_t s = sets[(size_t)i * set_size + j];
                if (s < 0 || s >= P->n) { orbx_set_error("sets[%d][%d] = %d is outside the %d matches", i, j, s, P->n); return ORBX_ERR_ARG; }
                if (seen[s]) { orbx_set_error("sets[%d] repeats an index", i); return ORBX_ERR_ARG; }
                seen[s] = 1;
            }
        }
    }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const size_t nsets = (size_t)m * set_size;
    if ((rc = h->epSets.ensure(nsets)) || (rc = h->epOut.ensure((size_t)m * 13)) || (full && (rc = h->epFull.ensure((size_t)m * PNP_FULL))) ||
        (alphas && (rc = h->epAlphas.ensure(nsets * 4))))
        return rc;
    std::vector<PnpCand> cands;
    PnpIn I;
    const std::vector<int> iters(1, m), mins(1, minInl);
    stage(h, P, 1, iters, mins, false, 0, 0, 256, cands, I, &rc);
    if (rc != ORBX_OK) return rc;
    const PnpDev D = dev_view(h);
    double *o = h->epOut.p;
    hipLaunchKernelGGL(k_pnp_prepare, dim3(prepare_blocks(P->n, 0), 1), dim3(256), 0, h->stream, I, D, 0);
    ORBX_LAUNCH_CHECK();
    ORBX_HIP_CHECK(hipMemcpyAsync(h->epSets.p, sets, nsets * 4, hipMemcpyHostToDevice, h->stream));
    const unsigned teams = 64 / PNP_TEAM;
    hipLaunchKernelGGL(k_pnp_models, dim3((unsigned)((m + teams - 1) / teams), 1), dim3(64), 0, h->stream, D, (const int32_t *)h->epSets.p, set_size, o, o + 9 * (size_t)m, o + 12 * (size_t)m,
                       full ? h->epFull.p : (double *)nullptr, alphas ? h->epAlphas.p : (double *)nullptr);
    ORBX_LAUNCH_CHECK();
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    ORBX_HIP_CHECK(hipMemcpy(R, o, (size_t)m * 72, hipMemcpyDeviceToHost));
    ORBX_HIP_CHECK(hipMemcpy(t, o + 9 * (size_t)m, (size_t)m * 24, hipMemcpyDeviceToHost));
    ORBX_HIP_CHECK(hipMemcpy(err, o + 12 * (size_t)m, (size_t)m * 8, hipMemcpyDeviceToHost));
    if (full) ORBX_HIP_CHECK(hipMemcpy(full, h->epFull.p, (size_t)m * PNP_FULL * 8, hipMemcpyDeviceToHost));
    if (alphas) ORBX_HIP_CHECK(hipMemcpy(alphas, h->epAlphas.p, nsets * 32, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

extern "C" int orbx_pnp_last_timing(orbx_pnp_solver *h, float *device_ms, int *launches)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    return h->timer.read(h->device, device_ms, launches, "no orbx_pnp_solve call to report");
}
