// orbx_optimize_sim3.hip -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1364-1590) with the vendored g2o's Levenberg driver, every problem of a
// call (the Sim3 events of LoopClosing::ComputeSim3's candidates) in ONE launch with one wait.  gfx950 only.
//
//   k_optsim3   one workgroup of 256 threads per problem.  Thread t owns pairs t, t + 256, ...: the two camera points (the float arithmetic of
//               k_sim3_prepare, orbx_sim3.hip, widened), the two observations, the two weights and the four error components of its pairs live in
//               registers for the whole call.  A linearisation: lanes 0-13 of wave 0 form the 14 perturbed estimates Sim3(+-1e-9 e_d) * S and
//               their inverses ONCE and leave them in LDS; every thread takes g2o's central differences of its edges through them
//               (base_binary_edge.hpp:147-200; neither edge defines linearizeOplus), the Huber quadratic form, and its share of the 28 + 7 + 1
//               sums of H, b and the robust chi2; the sums meet in a fixed order (DPP butterflies inside a wave, the four waves' sums added by every
//               thread in the same order: no floating-point atomics).  One thread solves the 7x7 system by LDL^T and takes the Levenberg decision
//               (optimization_algorithm_levenberg.cpp:61-164).  Two rounds, the chi2 tests on the errors as the LAST trial left them.
//   LIN = true  the same device functions run ONE linearisation at an explicit estimate and write errors, chi2, Jacobians, H and b
//               (orbx_optimize_sim3_linearize).
//
// Latency bound FP64 on one CU per problem: what a call gains is the batch and the host's g2o graph.
// Arithmetic: every product, sum and quotient is its own IEEE operation (-ffp-contract=off, no fused multiply-add, no reciprocal
// approximations), in the order tests/optsim3_ref.py restates; the list is in include/orbx.h above orbx_sim3_optimizer_create.
// PARITY UNPINNED: the device library's sin / cos / exp, Eigen's Quaterniond(R) branch choice beyond rounding, LDL^T pivoting (Eigen's LDLT
// pivots; this one does not), the order of the sums over the edges.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "orbx_handle.h"
#include "orbx_optsim3.h"

#define OS_THREADS 256
#define OS_NRED 36      /* 28 upper-triangle entries of H, 7 of b, the robust chi2 */

struct OsLinBlock {              // layout of orbx_optimize_sim3_linearize's results
    size_t err, chi, jac, H, b, total;
    __host__ __device__ OsLinBlock(int n)
    {
        const size_t m = (size_t)n;
        err = 0; chi = err + 32 * m; jac = chi + 16 * m; H = jac + 224 * m; b = H + 49 * 8;
        total = (b + 56 + 255) & ~(size_t)255;
    }
};

// obs - cam_map(project(S.map(X))): EdgeSim3ProjectXYZ with (S, X2, obs1, K1), EdgeInverseSim3ProjectXYZ with (S^-1, X1, obs2, K2)
__device__ __forceinline__ void os_edge_error(const OsSim3 &S, const float (&X)[3], const float (&obs)[2], const double (&K)[4], double (&e)[2])
{
    const double v[3] = {(double)X[0], (double)X[1], (double)X[2]};
    double p[3];
    os_map(S, v, p);
    e[0] = (double)obs[0] - ((p[0] / p[2]) * K[0] + K[2]);
    e[1] = (double)obs[1] - ((p[1] / p[2]) * K[1] + K[3]);
}

__device__ __forceinline__ void os_huber(double delta, double e2, double &rho0, double &rho1)      // RobustKernelHuber::robustify
{
    const double dsqr = delta * delta;
    if (e2 <= dsqr) { rho0 = e2; rho1 = 1.0; }
    else { const double sqrte = sqrt(e2); rho0 = (2.0 * sqrte) * delta - dsqr; rho1 = delta / sqrte; }
}

__device__ __forceinline__ double os_chi2(const double (&e)[2], double w) { return w * (e[0] * e[0] + e[1] * e[1]); }

struct OsShared {
    OsSim3 est, save, pert[14], pertInv[14];
    double red[4][OS_NRED];
    double jac[28 * OS_THREADS];      // a linearisation's Jacobian entries, [k][thread]
    double H[49], b[7], x[7];
    double lambda, ni, cur, rho;
    int ok, iterOk, nBadIt, count;
};

// The 14 perturbed estimates of a linearisation and their inverses: lane 2 d is +delta e_d, lane 2 d + 1 is -delta e_d, through oplus
// (update[6] = 0 with fix_scale: both estimates of column 6 are then the same, and the column is exactly zero)
__device__ __forceinline__ void os_perturb(OsShared &sh, int tid, bool fixScale)
{
    if (tid < 14) {
        const int d = tid >> 1;
        const double delta = 1e-9, val = (tid & 1) ? -delta : delta;
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = k == d ? val : 0.0;
        if (fixScale) u[6] = 0.0;
        OsSim3 E, P, Pi;
        os_exp(u, E);
        const OsSim3 S = sh.est;
        os_mul(E, S, P);
        os_inverse(P, Pi);
        sh.pert[tid] = P; sh.pertInv[tid] = Pi;
    }
}

// One pair of a linearisation: errors at the estimate (kept in er), the central differences, the Huber quadratic form into acc.
// J[0..7) / [7..14) = rows 0 / 1 of the e12 edge, [14..21) / [21..28) of the e21 edge.
__device__ __forceinline__ void os_pair_build(OsShared &sh, const OsSim3 &S, const OsSim3 &Si, const float (&x1)[3], const float (&x2)[3], const float (&o1)[2],
                                              const float (&o2)[2], float w1f, float w2f, const double (&K1)[4], const double (&K2)[4], double hub, double (&er)[4],
                                              double (&J)[28], double (&chi)[2], double (&acc)[OS_NRED])
{
    double e12[2], e21[2];
    os_edge_error(S, x2, o1, K1, e12);
    os_edge_error(Si, x1, o2, K2, e21);
    er[0] = e12[0]; er[1] = e12[1]; er[2] = e21[0]; er[3] = e21[1];
    const double scalar = 1.0 / (2.0 * 1e-9);
    // The columns in a loop that is NOT unrolled, each through the thread's own column of an LDS tile: unrolled, the scheduler loads the 14 x 16
    // doubles of estimates ahead and the kernel spills several hundred registers once a thread owns two pairs.
    double *Jt = sh.jac + threadIdx.x;
#pragma unroll 1
    for (int d = 0; d < 7; d++) {
        const OsSim3 Pp = sh.pert[2 * d], Pm = sh.pert[2 * d + 1], Qp = sh.pertInv[2 * d], Qm = sh.pertInv[2 * d + 1];
        double a[2], b[2];
        os_edge_error(Pp, x2, o1, K1, a); os_edge_error(Pm, x2, o1, K1, b);
        Jt[OS_THREADS * d] = scalar * (a[0] - b[0]); Jt[OS_THREADS * (7 + d)] = scalar * (a[1] - b[1]);
        os_edge_error(Qp, x1, o2, K2, a); os_edge_error(Qm, x1, o2, K2, b);
        Jt[OS_THREADS * (14 + d)] = scalar * (a[0] - b[0]); Jt[OS_THREADS * (21 + d)] = scalar * (a[1] - b[1]);
    }
#pragma unroll
    for (int k = 0; k < 28; k++) J[k] = Jt[OS_THREADS * k];
    const double w[2] = {(double)w1f, (double)w2f};
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const double r[2] = {er[2 * e], er[2 * e + 1]};
        chi[e] = os_chi2(r, w[e]);
        double rho0, rho1;
        os_huber(hub, chi[e], rho0, rho1);
        acc[35] += rho0;
        const double W = rho1 * w[e];
        const double c0 = (-(w[e] * r[0])) * rho1, c1 = (-(w[e] * r[1])) * rho1;
        const double *J0 = J + 14 * e, *J1 = J + 14 * e + 7;
        int k = 0;
#pragma unroll
        for (int i = 0; i < 7; i++) {
#pragma unroll
            for (int j = i; j < 7; j++, k++) acc[k] += J0[i] * (W * J0[j]) + J1[i] * (W * J1[j]);
            acc[28 + i] += J0[i] * c0 + J1[i] * c1;
        }
    }
}

template <int NE, bool LIN>
__device__ __forceinline__ void os_run(const OsIn &I, uint8_t *__restrict__ out, OsShared &sh)
{
    const int tid = threadIdx.x;
    const OsProb *hp = I.prob + blockIdx.x;
    const int n = hp->n, mb = hp->mb;
    const bool fixScale = hp->fixScale != 0;
    const float th2f = hp->th2;
    const double th2 = (double)th2f, hub = (double)sqrtf(th2f);
    uint8_t *blk = out + hp->outOff;
    const OsBlock L(n);
    const OsLinBlock LL(n);
    double K1[4], K2[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { K1[j] = (double)hp->k1[j]; K2[j] = (double)hp->k2[j]; }

    // ---- the thread's pairs: the constructor arithmetic of k_sim3_prepare, float, then held as floats (widened where they are used)
    float x1[NE][3], x2[NE][3], o1[NE][2], o2[NE][2], w1[NE], w2[NE];
    double er[NE][4];
    unsigned aM = 0;             // bit j: pair tid + 256 j is in the graph
    {
        float R1[9], t1[3], R2[9], t2[3];
#pragma unroll
        for (int j = 0; j < 9; j++) { R1[j] = hp->rcw1[j]; R2[j] = hp->rcw2[j]; }
#pragma unroll
        for (int j = 0; j < 3; j++) { t1[j] = hp->tcw1[j]; t2[j] = hp->tcw2[j]; }
#pragma unroll
        for (int j = 0; j < NE; j++) {
            const int i = tid + OS_THREADS * j;
            const bool live = i < n;
            const size_t g = (size_t)mb + (live ? i : 0);
            float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f};
            if (live) {
                a[0] = I.world1[3 * g]; a[1] = I.world1[3 * g + 1]; a[2] = I.world1[3 * g + 2];
                b[0] = I.world2[3 * g]; b[1] = I.world2[3 * g + 1]; b[2] = I.world2[3 * g + 2];
            }
#pragma unroll
            for (int r = 0; r < 3; r++) {
                x1[j][r] = ((R1[3 * r] * a[0] + R1[3 * r + 1] * a[1]) + R1[3 * r + 2] * a[2]) + t1[r];
                x2[j][r] = ((R2[3 * r] * b[0] + R2[3 * r + 1] * b[1]) + R2[3 * r + 2] * b[2]) + t2[r];
            }
            o1[j][0] = live ? I.obs1[2 * g] : 0.f; o1[j][1] = live ? I.obs1[2 * g + 1] : 0.f;
            o2[j][0] = live ? I.obs2[2 * g] : 0.f; o2[j][1] = live ? I.obs2[2 * g + 1] : 0.f;
            w1[j] = live ? I.inv1[g] : 0.f; w2[j] = live ? I.inv2[g] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; r++) er[j][r] = 0.0;
            bool on = live;
            if (LIN && live && I.active) on = I.active[i] != 0;
            if (on) aM |= 1u << j;
            if (!LIN && live) {
                float *ox1 = (float *)(blk + L.x1), *ox2 = (float *)(blk + L.x2);
#pragma unroll
                for (int r = 0; r < 3; r++) { ox1[3 * i + r] = x1[j][r]; ox2[3 * i + r] = x2[j][r]; }
            }
        }
    }
    OsSim3 S0;                   // g2o::Sim3(Quaterniond(R), t, s): every thread holds the input estimate
    {
        double R[9];
#pragma unroll
        for (int j = 0; j < 9; j++) R[j] = hp->r12[j];
        os_quat_from_R(R, S0.q);
#pragma unroll
        for (int j = 0; j < 3; j++) S0.t[j] = hp->t12[j];
        S0.s = hp->s12;
    }
    if (tid == 0) {
        sh.est = LIN ? I.lin : S0;
#pragma unroll
        for (int j = 0; j < 7; j++) sh.x[j] = 0.0;
    }
    __syncthreads();

    if (LIN) {
        os_perturb(sh, tid, fixScale);
        __syncthreads();
        const OsSim3 S = sh.est;
        OsSim3 Si;
        os_inverse(S, Si);
        double acc[OS_NRED];
#pragma unroll
        for (int k = 0; k < OS_NRED; k++) acc[k] = 0.0;
        double *oe = (double *)(blk + LL.err), *oc = (double *)(blk + LL.chi), *oj = (double *)(blk + LL.jac);
#pragma unroll
        for (int j = 0; j < NE; j++) {
            const int i = tid + OS_THREADS * j;
            if (i >= n) continue;
            double J[28], chi[2] = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 28; k++) J[k] = 0.0;
            if ((aM >> j) & 1u) os_pair_build(sh, S, Si, x1[j], x2[j], o1[j], o2[j], w1[j], w2[j], K1, K2, hub, er[j], J, chi, acc);
#pragma unroll
            for (int k = 0; k < 4; k++) oe[4 * (size_t)i + k] = er[j][k];
            oc[2 * (size_t)i] = chi[0]; oc[2 * (size_t)i + 1] = chi[1];
#pragma unroll
            for (int k = 0; k < 28; k++) oj[28 * (size_t)i + k] = J[k];
        }
        block_sum_f64(acc, sh.red, tid);
        if (tid == 0) {
            double *oH = (double *)(blk + LL.H), *ob = (double *)(blk + LL.b);
            int k = 0;
            for (int i = 0; i < 7; i++) {
                for (int j = i; j < 7; j++, k++) { oH[7 * i + j] = acc[k]; oH[7 * j + i] = acc[k]; }
                ob[i] = acc[28 + i];
            }
        }
        return;
    }

    int32_t *head = (int32_t *)blk;
    double *oEst = (double *)(blk + L.est), *oStats = (double *)(blk + L.stats);
    double *oChi[2] = {(double *)(blk + L.chi1), (double *)(blk + L.chi2)};
    uint8_t *oRem[2] = {blk + L.remFirst, blk + L.remFinal};
    if (tid < 4) oStats[tid] = 0.0;
    int nBad = 0, nIn = 0;
    bool giveUp = n == 0;        // no edge: optimize() does nothing, nCorrespondences - nBad = 0 < 10
    for (int round = 0; round < 2 && !giveUp; round++) {
        const int maxIt = round == 0 ? 5 : (nBad > 0 ? 10 : 5);
        if (tid == 0) {
            sh.iterOk = 1; sh.nBadIt = 0; sh.count = 0;
#pragma unroll
            for (int j = 0; j < 7; j++) sh.x[j] = 0.0;      // the solver's x of this optimize()
        }
        __syncthreads();
        int itersDone = 0;
        double lastChi = 0.0;
        for (int it = 0; it < maxIt; it++) {
            if (!sh.iterOk) break;
            // ---- computeActiveErrors, activeRobustChi2, buildSystem
            os_perturb(sh, tid, fixScale);
            __syncthreads();
            {
                const OsSim3 S = sh.est;
                OsSim3 Si;
                os_inverse(S, Si);
                double acc[OS_NRED];
#pragma unroll
                for (int k = 0; k < OS_NRED; k++) acc[k] = 0.0;
#pragma unroll
                for (int j = 0; j < NE; j++) {
                    if (!((aM >> j) & 1u)) continue;
                    double J[28], chi[2];
                    os_pair_build(sh, S, Si, x1[j], x2[j], o1[j], o2[j], w1[j], w2[j], K1, K2, hub, er[j], J, chi, acc);
                }
                block_sum_f64(acc, sh.red, tid);
                if (tid == 0) {
                    int k = 0;
#pragma unroll
                    for (int i = 0; i < 7; i++) {
#pragma unroll
                        for (int j = i; j < 7; j++, k++) { sh.H[7 * i + j] = acc[k]; sh.H[7 * j + i] = acc[k]; }
                        sh.b[i] = acc[28 + i];
                    }
                    sh.cur = acc[35];
                    if (it == 0) {   // computeLambdaInit, at iteration 0 of EACH optimize()
                        double mx = 0.0;
#pragma unroll
                        for (int q = 0; q < 7; q++) mx = fmax(fabs(sh.H[8 * q]), mx);
                        sh.lambda = 1e-5 * mx; sh.ni = 2.0;
                        sh.nBadIt = 0;
                    }
                }
                __syncthreads();
            }
            const double iniChi = sh.cur;
            int qmax = 0;
            do {
                if (tid == 0) {
                    sh.save = sh.est;   // push()
                    // (H + lambda I) x = b by LDL^T without pivoting; a non-positive or non-finite factor is "not positive" (linear_solver_dense.h)
                    double A[49];
#pragma unroll
                    for (int i = 0; i < 49; i++) A[i] = sh.H[i];
#pragma unroll
                    for (int i = 0; i < 7; i++) A[8 * i] += sh.lambda;
                    double Dg[7];
                    bool ok = true;
#pragma unroll
                    for (int j = 0; j < 7; j++) {
                        double LD[7];
                        double dj = A[8 * j];
#pragma unroll
                        for (int k = 0; k < j; k++) { LD[k] = A[7 * j + k] * Dg[k]; dj = dj - A[7 * j + k] * LD[k]; }
                        ok = ok && (dj > 0.0) && isfinite(dj);
                        Dg[j] = dj;
#pragma unroll
                        for (int i = j + 1; i < 7; i++) {
                            double lij = A[7 * i + j];
#pragma unroll
                            for (int k = 0; k < j; k++) lij = lij - A[7 * i + k] * LD[k];
                            A[7 * i + j] = lij / dj;
                        }
                    }
                    double xx[7];
#pragma unroll
                    for (int i = 0; i < 7; i++) {
                        double s = sh.b[i];
#pragma unroll
                        for (int k = 0; k < i; k++) s = s - A[7 * i + k] * xx[k];
                        xx[i] = s;
                    }
#pragma unroll
                    for (int i = 0; i < 7; i++) xx[i] = xx[i] / Dg[i];
#pragma unroll
                    for (int i = 6; i >= 0; i--) {
                        double s = xx[i];
#pragma unroll
                        for (int k = i + 1; k < 7; k++) s = s - A[7 * k + i] * xx[k];
                        xx[i] = s;
                    }
                    if (ok) {
#pragma unroll
                        for (int i = 0; i < 7; i++) sh.x[i] = xx[i];
                    }
                    sh.ok = ok ? 1 : 0;
                    // oplusImpl: update[6] = 0 with fix_scale, written into the solver's x; a failed solve applies the stale x, pop() restores
                    if (fixScale) sh.x[6] = 0.0;
                    double u[7];
#pragma unroll
                    for (int i = 0; i < 7; i++) u[i] = sh.x[i];
                    OsSim3 E, Nw;
                    os_exp(u, E);
                    const OsSim3 S = sh.est;
                    os_mul(E, S, Nw);
                    sh.est = Nw;
                }
                __syncthreads();
                {
                    const OsSim3 S = sh.est;
                    OsSim3 Si;
                    os_inverse(S, Si);
                    double cacc[1] = {0.0};
#pragma unroll
                    for (int j = 0; j < NE; j++) {
                        if (!((aM >> j) & 1u)) continue;
                        double e12[2], e21[2];
                        os_edge_error(S, x2[j], o1[j], K1, e12);
                        os_edge_error(Si, x1[j], o2[j], K2, e21);
                        er[j][0] = e12[0]; er[j][1] = e12[1]; er[j][2] = e21[0]; er[j][3] = e21[1];
                        double r0, r1;
                        os_huber(hub, os_chi2(e12, (double)w1[j]), r0, r1);
                        cacc[0] += r0;
                        os_huber(hub, os_chi2(e21, (double)w2[j]), r0, r1);
                        cacc[0] += r0;
                    }
                    block_sum_f64(cacc, sh.red, tid);
                    if (tid == 0) {
                        double tempChi = cacc[0];
                        if (!sh.ok) tempChi = DBL_MAX;
                        double rho = sh.cur - tempChi, scale = 0.0;
#pragma unroll
                        for (int j = 0; j < 7; j++) scale = scale + sh.x[j] * (sh.lambda * sh.x[j] + sh.b[j]);
                        scale = scale + 1e-3;
                        rho = rho / scale;
                        if (rho > 0.0 && isfinite(tempChi)) {
                            const double t2r = 2.0 * rho - 1.0;
                            double alpha = 1.0 - (t2r * t2r) * t2r;      // pow(x, 3)
                            alpha = fmin(alpha, 2.0 / 3.0);
                            sh.lambda = sh.lambda * fmax(1.0 / 3.0, alpha);
                            sh.ni = 2.0;
                            sh.cur = tempChi;
                        } else {
                            sh.lambda = sh.lambda * sh.ni;
                            sh.ni = sh.ni * 2.0;
                            sh.est = sh.save;   // pop()
                        }
                        sh.rho = rho;
                        const int q1 = qmax + 1;
                        if (!(rho < 0.0 && q1 < 10)) {
                            if (q1 == 10 || rho == 0.0) sh.iterOk = 0;
                            else {
                                if ((iniChi - sh.cur) * 1e3 < iniChi) sh.nBadIt++; else sh.nBadIt = 0;
                                if (sh.nBadIt >= 3) sh.iterOk = 0;
                            }
                        }
                    }
                    __syncthreads();
                }
                qmax++;
            } while (sh.rho < 0.0 && qmax < 10);
            itersDone++;
            lastChi = sh.cur;
            __syncthreads();      // (every thread has read sh.rho / sh.cur before the next iteration's thread 0 writes them)
        }
        if (tid == 0) { oStats[2 * round] = (double)itersDone; oStats[2 * round + 1] = lastChi; }
        // ---- e12->chi2() > th2 || e21->chi2() > th2 on _error as the last trial left it
        int bad = 0;
#pragma unroll
        for (int j = 0; j < NE; j++) {
            const int i = tid + OS_THREADS * j;
            if (i >= n) continue;
            const bool on = (aM >> j) & 1u;
            const double e12[2] = {er[j][0], er[j][1]}, e21[2] = {er[j][2], er[j][3]};
            const double c12 = on ? os_chi2(e12, (double)w1[j]) : -1.0, c21 = on ? os_chi2(e21, (double)w2[j]) : -1.0;
            const bool rm = on && (c12 > th2 || c21 > th2);
            oChi[round][2 * (size_t)i] = c12; oChi[round][2 * (size_t)i + 1] = c21;
            oRem[round][i] = rm ? 1 : 0;
            if (round == 0) { oChi[1][2 * (size_t)i] = -1.0; oChi[1][2 * (size_t)i + 1] = -1.0; oRem[1][i] = 0; }
            bad += rm ? 1 : 0;
            if (round == 0 && rm) aM &= ~(1u << j);
        }
        if (bad) atomicAdd(&sh.count, bad);
        __syncthreads();
        const int total = sh.count;
        __syncthreads();
        if (round == 0) { nBad = total; giveUp = n - nBad < 10; }
        else nIn = (n - nBad) - total;
    }
    if (tid == 0) {
        const OsSim3 F = giveUp ? S0 : sh.est;      // return 0: g2oS12 stays as passed in
        head[0] = giveUp ? 0 : nIn; head[1] = nBad; head[2] = giveUp ? 1 : 0; head[3] = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) oEst[j] = F.q[j];
#pragma unroll
        for (int j = 0; j < 3; j++) oEst[4 + j] = F.t[j];
        oEst[7] = F.s;
        double R[9];
        os_quat_to_R(F.q, R);
        float *orr = (float *)(blk + L.r12);
#pragma unroll
        for (int j = 0; j < 9; j++) orr[j] = (float)R[j];
    }
}

template <int NE, bool LIN>
__global__ __launch_bounds__(OS_THREADS) void k_optsim3(OsIn I, uint8_t *__restrict__ out, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    __shared__ OsShared sh;
    os_run<NE, LIN>(I, out, sh);
    orbx_publish(counter, flag, seq, gridDim.x);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------------
struct orbx_sim3_optimizer : OrbxHandle {
    int maxProblems = 0, maxPairs = 0;
    OrbxCallTimer timer;
    OrbxCallBox box;
};

namespace {
int os_check_problem(const orbx_sim3_optimizer *h, const orbx_sim3_opt_problem *P, int c)
{
    if (P->n < 0 || (P->n > 0 && (!P->world1 || !P->world2 || !P->obs1 || !P->obs2 || !P->inv_sigma2_1 || !P->inv_sigma2_2))) {
        orbx_set_error("problem %d: n = %d or a NULL array", c, P->n);
        return ORBX_ERR_ARG;
    }
    const float k[8] = {P->fx1, P->fy1, P->cx1, P->cy1, P->fx2, P->fy2, P->cx2, P->cy2};
    for (int j = 0; j < 8; j++)
        if (!std::isfinite(k[j])) { orbx_set_error("problem %d: non-finite intrinsics", c); return ORBX_ERR_ARG; }
    if (!std::isfinite(P->th2) || P->th2 < 0.f) { orbx_set_error("problem %d: th2 = %g", c, (double)P->th2); return ORBX_ERR_ARG; }
    if (P->n > h->maxPairs) { orbx_set_error("problem %d: %d pairs, the optimiser was created for %d", c, P->n, h->maxPairs); return ORBX_ERR_CAPACITY; }
    return ORBX_OK;
}

// headers + arrays of `np` problems into the mapped input buffer; offs[c] = the problem's result block (lin: OsLinBlock)
struct OsStaged { OrbxStaged sg; OrbxSlot<uint8_t, ORBX_STAGE_OUT> res; };      // res: the problems' result blocks
OsStaged os_stage(orbx_sim3_optimizer *h, const orbx_sim3_opt_problem *Ps, int np, bool lin, const uint8_t *active, std::vector<OsProb> &probs, OsIn &I, int *rc)
{
    size_t totN = 0, off = 0;
    probs.assign((size_t)np, OsProb());
    for (int c = 0; c < np; c++) {
        const orbx_sim3_opt_problem &P = Ps[c];
        OsProb &H = probs[c];
        memcpy(H.rcw1, P.rcw1, 36); memcpy(H.tcw1, P.tcw1, 12); memcpy(H.rcw2, P.rcw2, 36); memcpy(H.tcw2, P.tcw2, 12);
        H.k1[0] = P.fx1; H.k1[1] = P.fy1; H.k1[2] = P.cx1; H.k1[3] = P.cy1; H.k2[0] = P.fx2; H.k2[1] = P.fy2; H.k2[2] = P.cx2; H.k2[3] = P.cy2;
        memcpy(H.r12, P.r12, 72); memcpy(H.t12, P.t12, 24); H.s12 = P.s12;
        H.th2 = P.th2; H.n = P.n; H.fixScale = P.fix_scale ? 1 : 0; H.mb = (int32_t)totN; H.outOff = off;
        totN += (size_t)P.n;
        off += lin ? OsLinBlock(P.n).total : OsBlock(P.n).total;
    }
    OrbxCallBox &bx = h->box;
    auto [pin, pout] = bx.plan();
    // the problems' arrays lie concatenated, problem c's at element mb of its region: holes, filled below
    const auto sProb = pin.add(probs.data(), (size_t)np);
    const auto sW1 = pin.hole<float>(totN * 3), sW2 = pin.hole<float>(totN * 3), sO1 = pin.hole<float>(totN * 2), sO2 = pin.hole<float>(totN * 2);
    const auto sI1 = pin.hole<float>(totN), sI2 = pin.hole<float>(totN);
    const auto sAct = pin.hole<uint8_t>(active ? totN : 0);
    const auto rRes = pout.hole<uint8_t>(off);
    const OsStaged S = {bx.begin(h->stream, rc), rRes};
    if (*rc != ORBX_OK) return S;
    for (int c = 0; c < np; c++) {
        const orbx_sim3_opt_problem &P = Ps[c];
        const size_t n = (size_t)P.n, mb = (size_t)probs[c].mb;
        orbx_put_at(S.sg, sW1, 3 * mb, P.world1, 3 * n); orbx_put_at(S.sg, sW2, 3 * mb, P.world2, 3 * n);
        orbx_put_at(S.sg, sO1, 2 * mb, P.obs1, 2 * n); orbx_put_at(S.sg, sO2, 2 * mb, P.obs2, 2 * n);
        orbx_put_at(S.sg, sI1, mb, P.inv_sigma2_1, n); orbx_put_at(S.sg, sI2, mb, P.inv_sigma2_2, n);
        if (active) orbx_put_at(S.sg, sAct, mb, active, n);
    }
    I.prob = S.sg.dev(sProb);
    I.world1 = S.sg.dev(sW1); I.world2 = S.sg.dev(sW2);
    I.obs1 = S.sg.dev(sO1); I.obs2 = S.sg.dev(sO2);
    I.inv1 = S.sg.dev(sI1); I.inv2 = S.sg.dev(sI2);
    I.active = active ? S.sg.dev(sAct) : nullptr;
    memset(&I.lin, 0, sizeof(I.lin));
    return S;
}

template <bool LIN> void os_launch(hipStream_t st, int maxN, int np, const OsIn &I, uint8_t *res, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    const dim3 g((unsigned)np), b(OS_THREADS);
    if (maxN <= OS_THREADS) hipLaunchKernelGGL((k_optsim3<1, LIN>), g, b, 0, st, I, res, counter, flag, seq);
    else if (maxN <= 2 * OS_THREADS) hipLaunchKernelGGL((k_optsim3<2, LIN>), g, b, 0, st, I, res, counter, flag, seq);
    else hipLaunchKernelGGL((k_optsim3<4, LIN>), g, b, 0, st, I, res, counter, flag, seq);
}
}  // namespace

// the launch of orbx_optimize_sim3 as a link of another file's chain (orbx_optsim3.h)
void orbx_optsim3_enqueue(hipStream_t st, const OsIn &I, uint8_t *out, int np, int maxN, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    os_launch<false>(st, maxN, np, I, out, counter, flag, seq);
}

extern "C" int orbx_sim3_optimizer_create(int device, int max_problems, int max_pairs, orbx_sim3_optimizer **out)
{
    if (!out || max_problems < 1 || max_problems > 4096 || max_pairs < 1 || max_pairs > ORBX_SIM3_OPT_MAX_PAIRS) {
        orbx_set_error("bad Sim3 optimiser arguments (1 <= max_problems <= 4096, 1 <= max_pairs <= %d)", ORBX_SIM3_OPT_MAX_PAIRS);
        return ORBX_ERR_ARG;
    }
    *out = nullptr;
    orbx_sim3_optimizer *h = new orbx_sim3_optimizer();
    h->maxProblems = max_problems; h->maxPairs = max_pairs;
    int rc;
    if ((rc = h->open(device)) || (rc = h->timer.create())) { orbx_destroy_handle(h); return rc; }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_sim3_optimizer_destroy(orbx_sim3_optimizer *h) { orbx_destroy_handle(h); }

extern "C" int orbx_optimize_sim3(orbx_sim3_optimizer *h, const orbx_sim3_opt_problem *Ps, int np, const orbx_sim3_opt_result *Rs)
{
    if (!h || !Ps || !Rs || np < 1) { orbx_set_error("NULL argument or nproblems = %d < 1", np); return ORBX_ERR_ARG; }
    if (np > h->maxProblems) { orbx_set_error("%d problems, the optimiser was created for %d", np, h->maxProblems); return ORBX_ERR_CAPACITY; }
    int rc, maxN = 0;
    for (int c = 0; c < np; c++) {
        if ((rc = os_check_problem(h, Ps + c, c)) != ORBX_OK) return rc;
        maxN = std::max(maxN, Ps[c].n);
    }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    std::vector<OsProb> probs;
    OsIn I;
    const OsStaged S = os_stage(h, Ps, np, false, nullptr, probs, I, &rc);
    if (rc != ORBX_OK) return rc;
    OrbxCallBox &bx = h->box;
    const unsigned long long seq = bx.arm();
    if ((rc = h->timer.begin(h->stream)) != ORBX_OK) return rc;
    orbx_optsim3_enqueue(h->stream, I, S.sg.dev(S.res), np, maxN, bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_COUNT(h->timer);
    if ((rc = h->timer.end(h->stream)) != ORBX_OK) return rc;
    if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;      // the one synchronisation

    for (int c = 0; c < np; c++) {
        const orbx_sim3_opt_result &R = Rs[c];
        const size_t n = (size_t)probs[c].n;
        const OsBlock B(probs[c].n);
        const uint8_t *blk = S.sg.host(S.res) + probs[c].outOff;
        const int32_t *head = (const int32_t *)blk;
        const double *est = (const double *)(blk + B.est);
        if (R.n_inliers) *R.n_inliers = head[0];
        if (R.n_bad) *R.n_bad = head[1];
        if (R.quat) memcpy(R.quat, est, 32);
        if (R.t) memcpy(R.t, est + 4, 24);
        if (R.s) *R.s = est[7];
        if (R.r12) memcpy(R.r12, blk + B.r12, 36);
        if (R.stats) memcpy(R.stats, blk + B.stats, 32);
        if (!n) continue;
        if (R.removed_first) memcpy(R.removed_first, blk + B.remFirst, n);
        if (R.removed_final) memcpy(R.removed_final, blk + B.remFinal, n);
        if (R.chi2_round1) memcpy(R.chi2_round1, blk + B.chi1, 16 * n);
        if (R.chi2_round2) memcpy(R.chi2_round2, blk + B.chi2, 16 * n);
        if (R.x3dc1) memcpy(R.x3dc1, blk + B.x1, 12 * n);
        if (R.x3dc2) memcpy(R.x3dc2, blk + B.x2, 12 * n);
    }
    return ORBX_OK;
}

extern "C" int orbx_optimize_sim3_linearize(orbx_sim3_optimizer *h, const orbx_sim3_opt_problem *P, const double *quat, const double *t, double s, const uint8_t *active,
                                            double *errors, double *chi2, double *jac, double *H, double *b)
{
    if (!h || !P || !quat || !t) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = os_check_problem(h, P, 0)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    std::vector<OsProb> probs;
    OsIn I;
    const OsStaged S = os_stage(h, P, 1, true, P->n > 0 ? active : nullptr, probs, I, &rc);
    if (rc != ORBX_OK) return rc;
    for (int j = 0; j < 4; j++) I.lin.q[j] = quat[j];
    for (int j = 0; j < 3; j++) I.lin.t[j] = t[j];
    I.lin.s = s;
    OrbxCallBox &bx = h->box;
    const unsigned long long seq = bx.arm();
    os_launch<true>(h->stream, P->n, 1, I, S.sg.dev(S.res), bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_CHECK();
    if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;
    const size_t n = (size_t)P->n;
    const OsLinBlock B(P->n);
    const uint8_t *blk = S.sg.host(S.res);
    if (errors && n) memcpy(errors, blk + B.err, 32 * n);
    if (chi2 && n) memcpy(chi2, blk + B.chi, 16 * n);
    if (jac && n) memcpy(jac, blk + B.jac, 224 * n);
    if (H) memcpy(H, blk + B.H, 49 * 8);
    if (b) memcpy(b, blk + B.b, 56);
    return ORBX_OK;
}

extern "C" int orbx_sim3_optimizer_last_timing(orbx_sim3_optimizer *h, float *device_ms, int *launches)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    return h->timer.read(h->device, device_ms, launches, "no orbx_optimize_sim3 call to report");
}
