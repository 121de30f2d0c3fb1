// orbx_essential_graph.hip -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1017-1339) with the vendored g2o: the Sim3 pose graph of
// LoopClosing::CorrectLoop under g2o's Levenberg driver, and the pose / map-point write-back.  gfx950 only.
//
//   k_eg_init        copies the vertex estimates into the working buffer and forms the measurements Sji = Sjw * Swi
//   k_eg_linearize   16 threads per edge: thread c < 14 takes column c % 7 of the Jacobian of vertex c / 7 by g2o's central differences through
//                    oplus (base_binary_edge.hpp:147-200; EdgeSim3 defines no linearizeOplus), thread 14 the error at the estimate
//   k_eg_assemble    one wave per block of H (stored on the pattern of L, fill blocks zero): lane (r, c) adds the edges of the block's list in
//                    edge order, each term a sum over the seven error rows in row order; lanes 49-55 of a diagonal block do b.  No atomics.
//   k_eg_solve       ONE workgroup: L = H + lambda I, right-looking block LDL^T over the columns in elimination order (per column: thread 0
//                    factors the 7x7 diagonal block and solves its part of L z = b, 7 m threads the rows of the m blocks below it, then
//                    49 m (m + 1) / 2 threads the trailing update), z / d, L^T x = z from the last column up, x . (lambda x + b), and the
//                    trial estimates.  Column steps depend on one another, so they live in one workgroup behind barriers: nothing waits across
//                    workgroups.  Latency bound on one CU: ~3 barriers and one 7-pivot chain per column.
//   k_eg_error       per edge log(C * v1 * v2^-1) and e^T e
//   k_eg_reduce      chi2 in a fixed order (thread t adds edges t, t + 256, ...; then a binary tree), the trial's record into mapped pinned memory,
//                    the sequence word behind it
//   k_eg_writeback   estimates, inverses, Tiw = [R | t / s] as floats, corrected map points
//
// The host takes each trial's Levenberg decision from that record (optimization_algorithm_levenberg.cpp:61-164; scalar work in g2o too): no copy
// engine and no stream synchronisation inside the loop.  The symbolic phase (order, pattern of L, the assembly lists) runs on the host once per call.
// Arithmetic: every product, sum and quotient is its own IEEE operation (-ffp-contract=off), in the order tests/essential_graph_ref.py restates.
// exp, sin, cos, log and acos are series of IEEE operations of this file's own (EgMath), restated with everything else.
// PARITY UNPINNED against the reference: libm's last bits of those five, W.lu().solve(t) of Sim3::log (the adjugate here), Eigen's sparse
// LDL^T and its ordering, the order of the block sums.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "orbx_handle.h"
#include "orbx_sim3_group.h"

#define EG_THREADS 256
#define EG_SOLVE_THREADS 1024      /* k_eg_solve's one workgroup */
#define EG_MAX_ITER 1024      /* iterations a caller may ask for (the reference runs 20) */

struct EgRecord { double chi, scale; long long ok, ticks; };      // one trial, in mapped pinned memory
static_assert(sizeof(EgRecord) == 32, "record layout");

struct EgDev {                   // device addresses of a call
    int N, E, M, nf, nOff, fixScale;
    const OsSim3 *est0, *meas0, *at;      // inputs (device copy of the staged call): vScw, NonCorrected-or-vScw, the estimates to start from
    const int32_t *edges;                 // [E][3]
    const float *points;
    const int32_t *ref, *pos;             // pos[N]: position of a vertex in the elimination order, -1 = fixed
    const int32_t *colPtr, *rowIdx;       // pattern of L below the diagonal, by column
    const int32_t *aPtr, *aItem;          // per block of L (nf diagonal blocks, then the nOff blocks below): edge << 2 | code
    OsSim3 *est[2], *meas;
    double *J, *err, *chiE;               // [E][2][7][7], [E][7], [E]
    double *H, *L, *W;                    // [(nf + nOff)][49] twice, [nOff][49]
    double *b, *y, *d, *xs, *x;           // [nf][7] each
    double *dev;                          // {scale, ok, ticks} of the last k_eg_solve
};

// ---- the elementary functions, pinned: exp, sin, cos, log and acos as argument reductions and Horner series of IEEE operations, so that
// tests/essential_graph_ref.py states them bit for bit (the device library's and numpy's agree only to an ulp, and a Levenberg decision next to
// the minimum is taken on the last bits of chi2).  Each is within a few ulps of the correctly rounded value: far inside what g2o's central
// differences leave of the reference's own result.  The coefficients are 1 / n!, (-1)^n / (2n + 1)!, (-1)^n / (2n)!, 2 / (2n + 1) and
// (2n)! / (4^n n!^2 (2n + 1)), rounded to double.
#define EG_EXP_C {1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889, 0.0001984126984126984, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08, 2.08767569878681e-09, 1.6059043836821613e-10}
#define EG_SIN_C {1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06, -2.505210838544172e-08, 1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15, -8.22063524662433e-18}
#define EG_COS_C {1.0, -0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07, 2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14, -1.5619206968586225e-16, 4.110317623312165e-19}
#define EG_LOG_C {2.0, 0.6666666666666666, 0.4, 0.2857142857142857, 0.2222222222222222, 0.18181818181818182, 0.15384615384615385, 0.13333333333333333, 0.11764705882352941, 0.10526315789473684, 0.09523809523809523, 0.08695652173913043, 0.08}
#define EG_ASIN_C {1.0, 0.16666666666666666, 0.075, 0.044642857142857144, 0.030381944444444444, 0.022372159090909092, 0.017352764423076924, 0.01396484375, 0.011551800896139705, 0.009761609529194078, 0.008390335809616815, 0.0073125258735988454, 0.006447210311889649, 0.005740037670841924, 0.005153309682319905, 0.004660143486915096, 0.004240907093679363, 0.003880964558837669, 0.0035692053938259347, 0.003297059503473485, 0.0030578216492580306, 0.002846178401108942, 0.00265787063820729, 0.0024894486782468836, 0.002338091892111975, 0.0022014739737101384, 0.0020776610325181676, 0.0019650336162772837}
struct EgMath {
    template <int N> static __device__ __forceinline__ double horner(const double (&c)[N], double x)
    {
        double p = c[N - 1];
#pragma unroll
        for (int n = N - 2; n >= 0; n--) p = p * x + c[n];
        return p;
    }
    static __device__ __forceinline__ double exp_(double x)
    {
        const double c[14] = EG_EXP_C;
        const double k = rint(x * 1.44269504088896338700e+00);
        const double r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
        return ldexp(horner(c, r), (int)k);
    }
    static __device__ __forceinline__ void sincos_(double t, double &sn, double &cs)
    {
        const double sc[10] = EG_SIN_C, cc[11] = EG_COS_C;
        const double k = rint(t * 6.36619772367581382433e-01);
        const double r = (t - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11, r2 = r * r;
        const double s = r * horner(sc, r2), c = horner(cc, r2);
        const int q = (int)((long long)k & 3);
        sn = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
        cs = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
    }
    static __device__ __forceinline__ double sin_(double t) { double s, c; sincos_(t, s, c); return s; }
    static __device__ __forceinline__ double cos_(double t) { double s, c; sincos_(t, s, c); return c; }
    static __device__ __forceinline__ double log_(double x)
    {
        const double lc[13] = EG_LOG_C;
        int e;
        double m = frexp(x, &e);
        if (m < 0.70710678118654752440) { m = m * 2.0; e = e - 1; }
        const double f = (m - 1.0) / (m + 1.0), r = f * horner(lc, f * f), ed = (double)e;
        return ed * 6.93147180369123816490e-01 + (ed * 1.90821492927058770002e-10 + r);
    }
    static __device__ __forceinline__ double acos_(double d)
    {
        const double ac[28] = EG_ASIN_C;
        const bool hi = d > 0.5, lo = d < -0.5;
        const double z2 = hi ? (1.0 - d) * 0.5 : lo ? (1.0 + d) * 0.5 : d * d;
        const double z = (hi || lo) ? sqrt(z2) : d;
        const double a = z * horner(ac, z2);
        return hi ? a + a : lo ? 3.141592653589793 - (a + a) : 1.5707963267948966 - a;
    }
};

// ---- Sim3::log(), sim3.h:148-230; W u = t by the adjugate ----------------------------------------------------------------------------------
__device__ __forceinline__ void eg_log(const OsSim3 &S, double (&o)[7])
{
    const double s = S.s, sigma = EgMath::log_(s), eps = 0.00001;
    double R[9];
    os_quat_to_R(S.q, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const bool nearI = d > 1.0 - eps, smallS = fabs(sigma) < eps;
    double om[3], A, B, C, theta = 0.0;
    if (nearI) { om[0] = 0.5 * dR[0]; om[1] = 0.5 * dR[1]; om[2] = 0.5 * dR[2]; }
    else {
        theta = EgMath::acos_(d);
        const double f = theta / (2.0 * sqrt(1.0 - d * d));
        om[0] = f * dR[0]; om[1] = f * dR[1]; om[2] = f * dR[2];
    }
    if (smallS) {
        C = 1.0;
        if (nearI) { A = 1.0 / 2.0; B = 1.0 / 6.0; }
        else {
            const double theta2 = theta * theta;
            A = (1.0 - EgMath::cos_(theta)) / theta2;
            B = (theta - EgMath::sin_(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        const double sigma2 = sigma * sigma;
        if (nearI) {
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double theta2 = theta * theta, a = s * EgMath::sin_(theta), b = s * EgMath::cos_(theta), c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2;
        }
    }
    const double Om[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
    double W[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double o2 = (Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j];
            W[3 * i + j] = (A * Om[3 * i + j] + B * o2) + C * (i == j ? 1.0 : 0.0);
        }
    const double a00 = W[4] * W[8] - W[5] * W[7], a01 = W[2] * W[7] - W[1] * W[8], a02 = W[1] * W[5] - W[2] * W[4];
    const double a10 = W[5] * W[6] - W[3] * W[8], a11 = W[0] * W[8] - W[2] * W[6], a12 = W[2] * W[3] - W[0] * W[5];
    const double a20 = W[3] * W[7] - W[4] * W[6], a21 = W[1] * W[6] - W[0] * W[7], a22 = W[0] * W[4] - W[1] * W[3];
    const double det = (W[0] * a00 + W[1] * a10) + W[2] * a20;
    const double *t = S.t;
    o[0] = om[0]; o[1] = om[1]; o[2] = om[2];
    o[3] = ((a00 * t[0] + a01 * t[1]) + a02 * t[2]) / det;
    o[4] = ((a10 * t[0] + a11 * t[1]) + a12 * t[2]) / det;
    o[5] = ((a20 * t[0] + a21 * t[1]) + a22 * t[2]) / det;
    o[6] = sigma;
}

// EdgeSim3::computeError: (C * v1) * v2^-1, then log()
__device__ __forceinline__ void eg_edge_error(const OsSim3 &C, const OsSim3 &v1, const OsSim3 &v2, double (&e)[7])
{
    OsSim3 a, bi, r;
    os_mul(C, v1, a);
    os_inverse(v2, bi);
    os_mul(a, bi, r);
    eg_log(r, e);
}

__device__ __forceinline__ void eg_oplus(const OsSim3 &S, const double (&x)[7], bool fixScale, OsSim3 &o)
{
    double u[7];
#pragma unroll
    for (int k = 0; k < 7; k++) u[k] = x[k];
    if (fixScale) u[6] = 0.0;
    OsSim3 E;
    os_exp<EgMath>(u, E);
    os_mul(E, S, o);
}

// thread t adds v[t], v[t + 256], ...; then a binary tree over the 256 partial sums.  Every thread returns the sum.
// (an FP64 LDS tree: a third order of additions, neither of orbx_wave.h's two, with a barrier pattern of its own - it stays here)
__device__ __forceinline__ double eg_block_sum(double part, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = part;
    __syncthreads();
    for (int s = EG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(EG_THREADS) void k_eg_init(EgDev D)
{
    const int i = blockIdx.x * EG_THREADS + threadIdx.x;
    if (i < D.N) D.est[0][i] = D.at[i];
    if (i < D.E) {
        const int vi = D.edges[3 * i], vj = D.edges[3 * i + 1], kind = D.edges[3 * i + 2];
        const OsSim3 *src = kind == 0 ? D.est0 : D.meas0;
        const OsSim3 Siw = src[vi], Sjw = src[vj];
        OsSim3 Swi, Sji;
        os_inverse(Siw, Swi);
        os_mul(Sjw, Swi, Sji);
        D.meas[i] = Sji;
    }
}

__global__ __launch_bounds__(EG_THREADS) void k_eg_linearize(EgDev D, int buf)
{
    const int g = blockIdx.x * EG_THREADS + threadIdx.x, e = g >> 4, c = g & 15;
    if (e >= D.E || c == 15) return;
    const int vi = D.edges[3 * e], vj = D.edges[3 * e + 1];
    const OsSim3 C = D.meas[e], Si = D.est[buf][vi], Sj = D.est[buf][vj];
    if (c == 14) {
        double er[7];
        eg_edge_error(C, Si, Sj, er);
#pragma unroll
        for (int k = 0; k < 7; k++) D.err[7 * (size_t)e + k] = er[k];
        return;
    }
    const int v = c / 7, dcol = c % 7;
    double *Jc = D.J + 98 * (size_t)e + 49 * v + dcol;      // J[e][v][row][dcol]
    if (D.pos[v == 0 ? vi : vj] < 0) {                        // the fixed vertex has no block
#pragma unroll
        for (int k = 0; k < 7; k++) Jc[7 * k] = 0.0;
        return;
    }
    const double delta = 1e-9, scalar = 1.0 / (2.0 * delta);
    double ep[7], em[7];
#pragma unroll 1
    for (int sgn = 0; sgn < 2; sgn++) {
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = k == dcol ? (sgn ? -delta : delta) : 0.0;
        OsSim3 P;
        eg_oplus(v == 0 ? Si : Sj, u, D.fixScale != 0, P);
        double er[7];
        if (v == 0) eg_edge_error(C, P, Sj, er); else eg_edge_error(C, Si, P, er);
#pragma unroll
        for (int k = 0; k < 7; k++) { if (sgn) em[k] = er[k]; else ep[k] = er[k]; }
    }
#pragma unroll
    for (int k = 0; k < 7; k++) Jc[7 * k] = scalar * (ep[k] - em[k]);
}

__global__ __launch_bounds__(EG_THREADS) void k_eg_assemble(EgDev D)
{
    const int blk = blockIdx.x * (EG_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blk >= D.nf + D.nOff) return;
    const int i0 = D.aPtr[blk], i1 = D.aPtr[blk + 1];
    if (lane < 49) {
        const int r = lane / 7, c = lane % 7;
        double acc = 0.0;
        for (int it = i0; it < i1; it++) {
            const int item = D.aItem[it], e = item >> 2, code = item & 3;
            const double *J0 = D.J + 98 * (size_t)e, *J1 = J0 + 49;
            const double *A = (code == 0 || code == 2) ? J0 : J1, *B = (code == 0 || code == 3) ? J0 : J1;
            double t = A[r] * B[c];
#pragma unroll
            for (int k = 1; k < 7; k++) t = t + A[7 * k + r] * B[7 * k + c];
            acc = acc + t;
        }
        D.H[49 * (size_t)blk + lane] = acc;
    } else if (lane < 56 && blk < D.nf) {
        const int r = lane - 49;
        double acc = 0.0;
        for (int it = i0; it < i1; it++) {
            const int item = D.aItem[it], e = item >> 2, code = item & 3;
            const double *A = D.J + 98 * (size_t)e + 49 * code, *er = D.err + 7 * (size_t)e;      // a diagonal block's codes are 0 / 1 = the vertex
            double t = A[r] * (-er[0]);
#pragma unroll
            for (int k = 1; k < 7; k++) t = t + A[7 * k + r] * (-er[k]);
            acc = acc + t;
        }
        D.b[7 * (size_t)blk + r] = acc;
    }
}

// EG_SOLVE_THREADS threads: the trailing update of a column is 49 m (m + 1) / 2 independent entries, ~10^4 with twenty blocks below the diagonal.
// (H + lambda I) x = b, then the trial estimates est[buf ^ 1] = Sim3(x) * est[buf] (update != 0).  One workgroup.
__global__ __launch_bounds__(EG_SOLVE_THREADS) void k_eg_solve(EgDev D, double lambda, int buf, int update)
{
    __shared__ double sL[49], sD[7], sZ[7], red[EG_THREADS];
    __shared__ int sOk;
    const int tid = threadIdx.x, nf = D.nf;
    const long long t0 = wall_clock64();
    const size_t nDiag = 49 * (size_t)nf, nAll = 49 * (size_t)(nf + D.nOff);
    for (size_t i = tid; i < nAll; i += EG_SOLVE_THREADS) {
        double v = D.H[i];
        if (i < nDiag && (i % 49) % 8 == 0) v = v + lambda;
        D.L[i] = v;
    }
    for (int i = tid; i < 7 * nf; i += EG_SOLVE_THREADS) D.y[i] = D.b[i];
    if (tid == 0) sOk = 1;
    __syncthreads();
    for (int j = 0; j < nf; j++) {
        const int cs = D.colPtr[j], m = D.colPtr[j + 1] - cs;
        if (tid == 0) {      // the diagonal block: scalar LDL^T without pivoting, and this column's part of L z = b
            double A[49], Dg[7];
            double *Lj = D.L + 49 * (size_t)j;
#pragma unroll
            for (int i = 0; i < 49; i++) A[i] = Lj[i];
            bool ok = true;
#pragma unroll
            for (int q = 0; q < 7; q++) {
                double LD[7];
                double dq = A[8 * q];
#pragma unroll
                for (int k = 0; k < q; k++) { LD[k] = A[7 * q + k] * Dg[k]; dq = dq - A[7 * q + k] * LD[k]; }
                ok = ok && (dq > 0.0) && isfinite(dq);
                Dg[q] = dq;
#pragma unroll
                for (int i = q + 1; i < 7; i++) {
                    double l = A[7 * i + q];
#pragma unroll
                    for (int k = 0; k < q; k++) l = l - A[7 * i + k] * LD[k];
                    A[7 * i + q] = l / dq;
                }
            }
            if (!ok) sOk = 0;
            double z[7];
#pragma unroll
            for (int i = 0; i < 7; i++) {
                double s = D.y[7 * j + i];
#pragma unroll
                for (int k = 0; k < i; k++) s = s - A[7 * i + k] * z[k];
                z[i] = s;
            }
#pragma unroll
            for (int i = 0; i < 49; i++) { sL[i] = A[i]; Lj[i] = A[i]; }
#pragma unroll
            for (int i = 0; i < 7; i++) { sD[i] = Dg[i]; sZ[i] = z[i]; D.d[7 * j + i] = Dg[i]; D.y[7 * j + i] = z[i]; }
        }
        __syncthreads();
        for (int idx = tid; idx < 7 * m; idx += EG_SOLVE_THREADS) {      // rows of the blocks below: w = a L_jj^-T (= l D), l = w / d
            const int a = idx / 7, r = idx % 7;
            double *row = D.L + 49 * (size_t)(nf + cs + a) + 7 * r, *wr = D.W + 49 * (size_t)(cs + a) + 7 * r;
            double w[7];
#pragma unroll
            for (int c = 0; c < 7; c++) {
                double s = row[c];
#pragma unroll
                for (int k = 0; k < c; k++) s = s - w[k] * sL[7 * c + k];
                w[c] = s;
            }
#pragma unroll
            for (int c = 0; c < 7; c++) { wr[c] = w[c]; row[c] = w[c] / sD[c]; }
        }
        __syncthreads();
        const int npair = m * (m + 1) / 2;
        for (int idx = tid; idx < 49 * npair; idx += EG_SOLVE_THREADS) {      // trailing update: block (ra, rb) -= W_a L_b^T
            const int p = idx / 49, en = idx % 49, r = en / 7, c = en % 7;
            int a = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
            while (a * (a + 1) / 2 > p) a--;
            while ((a + 1) * (a + 2) / 2 <= p) a++;
            const int bq = p - a * (a + 1) / 2;
            const int ra = D.rowIdx[cs + a], rb = D.rowIdx[cs + bq];
            int tb = -1;
            if (a == bq) tb = ra;
            else {
                int lo = D.colPtr[rb], hi = D.colPtr[rb + 1] - 1;
                while (lo <= hi) {
                    const int mid = (lo + hi) >> 1, rv = D.rowIdx[mid];
                    if (rv == ra) { tb = nf + mid; break; }
                    if (rv < ra) lo = mid + 1; else hi = mid - 1;
                }
            }
            if (tb < 0) continue;      // (the symbolic phase makes every target exist)
            const double *wa = D.W + 49 * (size_t)(cs + a) + 7 * r, *lb = D.L + 49 * (size_t)(nf + cs + bq) + 7 * c;
            double *tg = D.L + 49 * (size_t)tb + en;
            double acc = *tg;
#pragma unroll
            for (int k = 0; k < 7; k++) acc = acc - wa[k] * lb[k];
            *tg = acc;
        }
        for (int idx = tid; idx < 7 * m; idx += EG_SOLVE_THREADS) {           // y_ra -= L_a z
            const int a = idx / 7, r = idx % 7, ra = D.rowIdx[cs + a];
            const double *la = D.L + 49 * (size_t)(nf + cs + a) + 7 * r;
            double acc = D.y[7 * ra + r];
#pragma unroll
            for (int k = 0; k < 7; k++) acc = acc - la[k] * sZ[k];
            D.y[7 * ra + r] = acc;
        }
        __syncthreads();
    }
    for (int i = tid; i < 7 * nf; i += EG_SOLVE_THREADS) D.y[i] = D.y[i] / D.d[i];
    __syncthreads();
    for (int j = nf - 1; j >= 0; j--) {      // L^T x = z
        const int cs = D.colPtr[j], m = D.colPtr[j + 1] - cs;
        if (tid < 7) {
            double acc = D.y[7 * j + tid];
            for (int a = 0; a < m; a++) {
                const double *la = D.L + 49 * (size_t)(nf + cs + a), *xa = D.xs + 7 * D.rowIdx[cs + a];
#pragma unroll
                for (int k = 0; k < 7; k++) acc = acc - la[7 * k + tid] * xa[k];
            }
            sZ[tid] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            const double *Lj = D.L + 49 * (size_t)j;
            double x[7];
#pragma unroll
            for (int i = 6; i >= 0; i--) {
                double s = sZ[i];
#pragma unroll
                for (int k = i + 1; k < 7; k++) s = s - Lj[7 * k + i] * x[k];
                x[i] = s;
            }
#pragma unroll
            for (int i = 0; i < 7; i++) D.xs[7 * j + i] = x[i];
        }
        __syncthreads();
    }
    const bool ok = sOk != 0;
    if (ok)      // a failed solve leaves the solver's x as it was (linear_solver: x is only written on success)
        for (int i = tid; i < 7 * nf; i += EG_SOLVE_THREADS) D.x[i] = (D.fixScale && i % 7 == 6) ? 0.0 : D.xs[i];
    __syncthreads();
    // x . (lambda x + b) in the order of eg_block_sum: the first EG_THREADS threads add i = t, t + EG_THREADS, ..., then the binary tree
    double part = 0.0;
    if (tid < EG_THREADS)
        for (int i = tid; i < 7 * nf; i += EG_THREADS) { const double xv = D.x[i]; part = part + xv * (lambda * xv + D.b[i]); }
    __syncthreads();
    if (tid < EG_THREADS) red[tid] = part;
    __syncthreads();
    for (int s = EG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const double scale = red[0];
    if (update)
        for (int v = tid; v < D.N; v += EG_SOLVE_THREADS) {
            const int p = D.pos[v];
            const OsSim3 S = D.est[buf][v];
            OsSim3 T = S;
            if (p >= 0) {
                double u[7];
#pragma unroll
                for (int k = 0; k < 7; k++) u[k] = D.x[7 * p + k];
                eg_oplus(S, u, D.fixScale != 0, T);
            }
            D.est[buf ^ 1][v] = T;
        }
    if (tid == 0) { D.dev[0] = scale; D.dev[1] = ok ? 1.0 : 0.0; D.dev[2] = (double)(wall_clock64() - t0); }
}

__global__ __launch_bounds__(EG_THREADS) void k_eg_error(EgDev D, int buf)
{
    const int e = blockIdx.x * EG_THREADS + threadIdx.x;
    if (e >= D.E) return;
    const int vi = D.edges[3 * e], vj = D.edges[3 * e + 1];
    double er[7];
    eg_edge_error(D.meas[e], D.est[buf][vi], D.est[buf][vj], er);
    double c = er[0] * er[0];
#pragma unroll
    for (int k = 1; k < 7; k++) c = c + er[k] * er[k];
#pragma unroll
    for (int k = 0; k < 7; k++) D.err[7 * (size_t)e + k] = er[k];
    D.chiE[e] = c;
}

__global__ __launch_bounds__(EG_THREADS) void k_eg_reduce(EgDev D, EgRecord *rec, int solved, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    __shared__ double red[EG_THREADS];
    double part = 0.0;
    for (int e = threadIdx.x; e < D.E; e += EG_THREADS) part = part + D.chiE[e];
    const double chi = eg_block_sum(part, red);
    if (threadIdx.x == 0) {
        rec->chi = chi;
        rec->scale = solved ? D.dev[0] : 0.0;
        rec->ok = solved ? (D.dev[1] != 0.0 ? 1 : 0) : 1;
        rec->ticks = solved ? (long long)D.dev[2] : 0;
    }
    orbx_publish(counter, flag, seq, 1);
}

struct EgOut { OsSim3 *est, *inv; float *tiw, *points; };      // mapped pinned

__global__ __launch_bounds__(EG_THREADS) void k_eg_writeback(EgDev D, int buf, EgOut O, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    const int i = blockIdx.x * EG_THREADS + threadIdx.x;
    if (i < D.N) {
        const OsSim3 F = D.est[buf][i];
        OsSim3 Fi;
        os_inverse(F, Fi);
        O.est[i] = F; O.inv[i] = Fi;
        double R[9];
        os_quat_to_R(F.q, R);
        const double f = 1.0 / F.s;      // eigt *= (1. / s)
        float *T = O.tiw + 12 * (size_t)i;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
            T[4 * r + 3] = (float)(F.t[r] * f);
        }
    }
    if (i < D.M) {
        const int r = D.ref[i];
        OsSim3 Srw, Swr;
        Srw.q[0] = 0.0; Srw.q[1] = 0.0; Srw.q[2] = 0.0; Srw.q[3] = 1.0; Srw.t[0] = 0.0; Srw.t[1] = 0.0; Srw.t[2] = 0.0; Srw.s = 1.0;      // g2o::Sim3()
        Swr = Srw;
        if (r >= 0) { Srw = D.est0[r]; const OsSim3 F = D.est[buf][r]; os_inverse(F, Swr); }
        const double p[3] = {(double)D.points[3 * (size_t)i], (double)D.points[3 * (size_t)i + 1], (double)D.points[3 * (size_t)i + 2]};
        double a[3], b[3];
        os_map(Srw, p, a);
        os_map(Swr, a, b);
#pragma unroll
        for (int k = 0; k < 3; k++) O.points[3 * (size_t)i + k] = (float)b[k];
    }
    orbx_publish(counter, flag, seq, gridDim.x);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------------
struct EgSymbolic {
    int N = 0, E = 0, nf = 0, nOff = 0;
    std::vector<int32_t> pos, order, colPtr, rowIdx, aPtr, aItem;
};

struct orbx_essential_graph : OrbxHandle {
    int maxKf = 0, maxEdges = 0, maxPoints = 0, maxFill = 0;
    OrbxCallTimer timer;
    bool linearized = false;
    double solveTicks = 0.0;
    OrbxCallBox box;
    OrbxOwnedBuf<uint8_t> arena;       // the staged inputs on the device
    OrbxOwnedBuf<double> work;         // every working array of a call
    EgSymbolic sym;                  // of the last call (orbx_essential_graph_solve runs on it)
    EgDev dev;
    std::vector<int32_t> edges;      // of the last linearisation
};

namespace {
int eg_blocks(int n) { return (n + EG_THREADS - 1) / EG_THREADS; }

int eg_check(const orbx_essential_graph *h, const orbx_essential_graph_problem *P, const double *at)
{
    if (P->n < 1 || !P->est) { orbx_set_error("n = %d < 1 or est == NULL", P->n); return ORBX_ERR_ARG; }
    if (P->fixed < 0 || P->fixed >= P->n) { orbx_set_error("fixed index %d outside [0, %d)", P->fixed, P->n); return ORBX_ERR_ARG; }
    if (P->n_edges < 0 || P->n_points < 0 || (P->n_edges > 0 && !P->edges) || (P->n_points > 0 && (!P->points || !P->point_ref))) {
        orbx_set_error("negative count or NULL array (%d edges, %d points)", P->n_edges, P->n_points);
        return ORBX_ERR_ARG;
    }
    if (P->iterations > EG_MAX_ITER) { orbx_set_error("%d iterations, at most %d", P->iterations, EG_MAX_ITER); return ORBX_ERR_ARG; }
    if (!std::isfinite(P->lambda_init)) { orbx_set_error("non-finite lambda_init"); return ORBX_ERR_ARG; }
    const double *sets[3] = {P->est, P->meas, at};
    for (int k = 0; k < 3; k++) {
        if (!sets[k]) continue;
        for (int i = 0; i < P->n; i++) {
            for (int j = 0; j < 8; j++)
                if (!std::isfinite(sets[k][8 * (size_t)i + j])) { orbx_set_error("keyframe %d: non-finite Sim3", i); return ORBX_ERR_ARG; }
            if (!(sets[k][8 * (size_t)i + 7] > 0.0)) { orbx_set_error("keyframe %d: scale %g <= 0", i, sets[k][8 * (size_t)i + 7]); return ORBX_ERR_ARG; }
        }
    }
    for (int e = 0; e < P->n_edges; e++) {
        const int32_t i = P->edges[3 * (size_t)e], j = P->edges[3 * (size_t)e + 1], kind = P->edges[3 * (size_t)e + 2];
        if (i < 0 || i >= P->n || j < 0 || j >= P->n || i == j || (kind != 0 && kind != 1)) {
            orbx_set_error("edge %d: (%d, %d, kind %d) with %d keyframes", e, i, j, kind, P->n);
            return ORBX_ERR_ARG;
        }
    }
    for (int i = 0; i < P->n_points; i++) {
        if (P->point_ref[i] < -1 || P->point_ref[i] >= P->n) { orbx_set_error("point %d: reference %d outside [-1, %d)", i, P->point_ref[i], P->n); return ORBX_ERR_ARG; }
        for (int j = 0; j < 3; j++)
            if (!std::isfinite(P->points[3 * (size_t)i + j])) { orbx_set_error("point %d: non-finite position", i); return ORBX_ERR_ARG; }
    }
    if (P->n > h->maxKf) { orbx_set_error("%d keyframes, the handle was created for %d", P->n, h->maxKf); return ORBX_ERR_CAPACITY; }
    if (P->n_edges > h->maxEdges) { orbx_set_error("%d edges, the handle was created for %d", P->n_edges, h->maxEdges); return ORBX_ERR_CAPACITY; }
    if (P->n_points > h->maxPoints) { orbx_set_error("%d points, the handle was created for %d", P->n_points, h->maxPoints); return ORBX_ERR_CAPACITY; }
    return ORBX_OK;
}

// Elimination order (the free vertices in the caller's order), the exact block pattern of L (every column's pattern is merged into its
// parent's, the first row below the diagonal) and the assembly lists.
int eg_symbolic(const orbx_essential_graph *h, const orbx_essential_graph_problem *P, EgSymbolic &S)
{
    const int N = P->n, E = P->n_edges;
    S.N = N; S.E = E; S.nf = N - 1;
    S.pos.assign((size_t)N, -1); S.order.clear();
    for (int v = 0; v < N; v++)
        if (v != P->fixed) { S.pos[v] = (int32_t)S.order.size(); S.order.push_back(v); }
    const int nf = S.nf;
    std::vector<std::vector<int32_t>> col((size_t)nf);
    for (int e = 0; e < E; e++) {
        const int pi = S.pos[P->edges[3 * (size_t)e]], pj = S.pos[P->edges[3 * (size_t)e + 1]];
        if (pi < 0 || pj < 0) continue;
        col[std::min(pi, pj)].push_back(std::max(pi, pj));
    }
    size_t fill = (size_t)nf;
    std::vector<int32_t> merged;
    for (int q = 0; q < nf; q++) {
        std::vector<int32_t> &c = col[q];
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        fill += c.size();
        if (fill > (size_t)h->maxFill) { orbx_set_error("the factor has more than %d blocks, the handle's fill budget", h->maxFill); return ORBX_ERR_CAPACITY; }
        if (c.size() > 1) {
            std::vector<int32_t> &par = col[c[0]];
            merged.clear();
            merged.insert(merged.end(), par.begin(), par.end());
            merged.insert(merged.end(), c.begin() + 1, c.end());
            par.swap(merged);      // (sorted and made unique when its own turn comes)
        }
    }
    S.colPtr.assign((size_t)nf + 1, 0); S.rowIdx.clear();
    for (int q = 0; q < nf; q++) { S.rowIdx.insert(S.rowIdx.end(), col[q].begin(), col[q].end()); S.colPtr[q + 1] = (int32_t)S.rowIdx.size(); }
    S.nOff = (int)S.rowIdx.size();
    const int nL = nf + S.nOff;
    auto offBlock = [&](int p, int q) {      // p > q
        const int32_t *b0 = S.rowIdx.data() + S.colPtr[q], *b1 = S.rowIdx.data() + S.colPtr[q + 1];
        return nf + (int)(std::lower_bound(b0, b1, p) - S.rowIdx.data());
    };
    S.aPtr.assign((size_t)nL + 1, 0);
    for (int pass = 0; pass < 2; pass++) {
        std::vector<int32_t> fillPos(S.aPtr.begin(), S.aPtr.end() - 1);
        for (int e = 0; e < E; e++) {
            const int pi = S.pos[P->edges[3 * (size_t)e]], pj = S.pos[P->edges[3 * (size_t)e + 1]];
            int blk[3], code[3], nb = 0;
            if (pi >= 0) { blk[nb] = pi; code[nb++] = 0; }
            if (pj >= 0) { blk[nb] = pj; code[nb++] = 1; }
            if (pi >= 0 && pj >= 0) { blk[nb] = pi > pj ? offBlock(pi, pj) : offBlock(pj, pi); code[nb++] = pi > pj ? 2 : 3; }
            for (int k = 0; k < nb; k++) {
                if (pass == 0) S.aPtr[(size_t)blk[k] + 1]++;
                else S.aItem[(size_t)fillPos[blk[k]]++] = (int32_t)(e << 2 | code[k]);
            }
        }
        if (pass == 0) {
            for (int k = 0; k < nL; k++) S.aPtr[(size_t)k + 1] += S.aPtr[k];
            S.aItem.assign((size_t)S.aPtr[nL], 0);
        }
    }
    return ORBX_OK;
}

// the call's inputs in the call box (mapped pinned): planned before the box's begin() ...
struct EgSlots {
    OrbxSlot<double, ORBX_STAGE_IN> est, meas, at;
    OrbxSlot<int32_t, ORBX_STAGE_IN> edges, ref, pos, colPtr, rowIdx, aPtr, aItem;
    OrbxSlot<float, ORBX_STAGE_IN> points;
    EgSlots(OrbxInPlan &pin, const EgSymbolic &S, const orbx_essential_graph_problem *P, const double *at0)
    {
        const size_t N = (size_t)P->n, E = (size_t)P->n_edges, M = (size_t)P->n_points, nf = (size_t)S.nf, nOff = (size_t)S.nOff, nL = nf + nOff;
        est = pin.add(P->est, 8 * N); meas = pin.add(P->meas ? P->meas : P->est, 8 * N); at = pin.add(at0 ? at0 : P->est, 8 * N);
        edges = pin.add(P->edges, 3 * E);
        points = pin.add(P->points, 3 * M); ref = pin.add(P->point_ref, M);
        pos = pin.add(S.pos.data(), N); colPtr = pin.add(S.colPtr.data(), nf + 1); rowIdx = pin.add(S.rowIdx.data(), nOff);
        aPtr = pin.add(S.aPtr.data(), nL + 1); aItem = pin.add(S.aItem.data(), S.aItem.size());
    }
};

// ... and behind it copied to the device once; lays the working arrays out
int eg_stage(orbx_essential_graph *h, const orbx_essential_graph_problem *P, const EgSlots &I)
{
    const EgSymbolic &S = h->sym;
    const size_t N = (size_t)P->n, E = (size_t)P->n_edges, nf = (size_t)S.nf, nOff = (size_t)S.nOff, nL = nf + nOff;
    int rc;
    uint8_t *A;
    if ((rc = orbx_stage_to_arena(h->box, h->arena, h->stream, 256, &A)) != ORBX_OK) return rc;
    ORBX_LAUNCH_COUNT(h->timer);
    // working arrays, in doubles (an OsSim3 is eight)
    size_t w = 0;
    auto take = [&](size_t n) { const size_t at0 = w; w += (n + 31) & ~(size_t)31; return at0; };
    const size_t wE0 = take(8 * N), wE1 = take(8 * N), wMeas = take(8 * E), wJ = take(98 * E), wErr = take(7 * E), wChi = take(E), wH = take(49 * nL), wL = take(49 * nL),
                 wW = take(49 * nOff), wb = take(7 * nf), wy = take(7 * nf), wd = take(7 * nf), wxs = take(7 * nf), wx = take(7 * nf), wdev = take(4);
    if ((rc = h->work.ensure(w)) != ORBX_OK) return rc;
    EgDev &D = h->dev;
    double *Wk = h->work.p;
    D.N = P->n; D.E = P->n_edges; D.M = P->n_points; D.nf = S.nf; D.nOff = S.nOff; D.fixScale = P->fix_scale ? 1 : 0;
    D.est0 = (const OsSim3 *)I.est.in(A); D.meas0 = (const OsSim3 *)I.meas.in(A); D.at = (const OsSim3 *)I.at.in(A);
    D.edges = I.edges.in(A); D.points = I.points.in(A); D.ref = I.ref.in(A); D.pos = I.pos.in(A);
    D.colPtr = I.colPtr.in(A); D.rowIdx = I.rowIdx.in(A); D.aPtr = I.aPtr.in(A); D.aItem = I.aItem.in(A);
    D.est[0] = (OsSim3 *)(Wk + wE0); D.est[1] = (OsSim3 *)(Wk + wE1); D.meas = (OsSim3 *)(Wk + wMeas);
    D.J = Wk + wJ; D.err = Wk + wErr; D.chiE = Wk + wChi; D.H = Wk + wH; D.L = Wk + wL; D.W = Wk + wW;
    D.b = Wk + wb; D.y = Wk + wy; D.d = Wk + wd; D.xs = Wk + wxs; D.x = Wk + wx; D.dev = Wk + wdev;
    ORBX_HIP_CHECK(hipMemsetAsync(D.x, 0, 8 * (7 * nf + 32), h->stream));      // the solver's x and the solve record
    hipLaunchKernelGGL(k_eg_init, dim3((unsigned)eg_blocks(std::max(P->n, P->n_edges))), dim3(EG_THREADS), 0, h->stream, D);
    ORBX_LAUNCH_COUNT(h->timer);
    return ORBX_OK;
}

// errors + chi2 of est[buf] into record `rec` of the result buffer; the caller waits
int eg_chi(orbx_essential_graph *h, int buf, EgRecord *rec, int solved)
{
    OrbxCallBox &bx = h->box;
    hipLaunchKernelGGL(k_eg_error, dim3((unsigned)eg_blocks(h->dev.E)), dim3(EG_THREADS), 0, h->stream, h->dev, buf);
    ORBX_LAUNCH_COUNT(h->timer);
    const unsigned long long seq = bx.arm();
    hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(EG_THREADS), 0, h->stream, h->dev, rec, solved, bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_COUNT(h->timer);
    return ORBX_OK;
}

int eg_linearize(orbx_essential_graph *h, int buf)
{
    hipLaunchKernelGGL(k_eg_linearize, dim3((unsigned)eg_blocks(16 * h->dev.E)), dim3(EG_THREADS), 0, h->stream, h->dev, buf);
    ORBX_LAUNCH_COUNT(h->timer);
    hipLaunchKernelGGL(k_eg_assemble, dim3((unsigned)((h->dev.nf + h->dev.nOff + 3) / 4)), dim3(EG_THREADS), 0, h->stream, h->dev);
    ORBX_LAUNCH_COUNT(h->timer);
    return ORBX_OK;
}
}  // namespace

extern "C" int orbx_essential_graph_create(int device, int max_keyframes, int max_edges, int max_points, int max_fill_blocks, orbx_essential_graph **out)
{
    if (!out || max_keyframes < 1 || max_edges < 0 || max_points < 0 || max_fill_blocks < 1 || max_edges > (1 << 26)) {      // (16 threads per edge in one int grid)
        orbx_set_error("bad essential graph arguments (max_keyframes >= 1, 0 <= max_edges <= 2^26, max_points >= 0, max_fill_blocks >= 1)");
        return ORBX_ERR_ARG;
    }
    *out = nullptr;
    orbx_essential_graph *h = new orbx_essential_graph();
    h->maxKf = max_keyframes; h->maxEdges = max_edges; h->maxPoints = max_points; h->maxFill = max_fill_blocks;
    int rc;
    if ((rc = h->open(device)) || (rc = h->timer.create())) { orbx_destroy_handle(h); return rc; }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_essential_graph_destroy(orbx_essential_graph *h) { orbx_destroy_handle(h); }

extern "C" int orbx_optimize_essential_graph(orbx_essential_graph *h, const orbx_essential_graph_problem *P, const orbx_essential_graph_result *R)
{
    if (!h || !P || !R) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = eg_check(h, P, nullptr)) != ORBX_OK) return rc;
    h->linearized = false;
    if ((rc = eg_symbolic(h, P, h->sym)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const int iterations = P->iterations > 0 ? P->iterations : 20;
    const size_t N = (size_t)P->n, M = (size_t)P->n_points;
    h->solveTicks = 0.0;
    OrbxCallBox &bx = h->box;
    if (bx.pending) { ORBX_HIP_CHECK(hipStreamSynchronize(h->stream)); bx.pending = false; }
    auto [pin, pout] = bx.plan();
    const EgSlots I(pin, h->sym, P, nullptr);
    const auto rRec = pout.hole<EgRecord>(2);
    const auto rEst = pout.hole<OsSim3>(N), rInv = pout.hole<OsSim3>(N);
    const auto rTiw = pout.hole<float>(12 * N), rPts = pout.hole<float>(3 * M);
    if ((rc = h->timer.begin(h->stream)) != ORBX_OK) return rc;
    const OrbxStaged sg = bx.begin(h->stream, &rc);
    if (rc != ORBX_OK || (rc = eg_stage(h, P, I)) != ORBX_OK) return rc;
    const EgRecord *rec = sg.host(rRec);
    EgRecord *const recDev = sg.dev(rRec);

    double chi0 = 0.0, cur = 0.0, lambda = P->lambda_init > 0.0 ? P->lambda_init : 1e-16, ni = 2.0, rho = 0.0;
    int buf = 0, done = 0, ended = ORBX_EG_END_ITERATIONS, nBad = 0;
    if (P->n_edges > 0) {
        if ((rc = eg_chi(h, buf, recDev, 0)) != ORBX_OK) return rc;
        if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;
        chi0 = cur = rec->chi;
        for (int it = 0; it < iterations; it++) {
            if ((rc = eg_linearize(h, buf)) != ORBX_OK) return rc;
            const double ini = cur;
            int qmax = 0;
            do {
                hipLaunchKernelGGL(k_eg_solve, dim3(1), dim3(EG_SOLVE_THREADS), 0, h->stream, h->dev, lambda, buf, 1);
                ORBX_LAUNCH_COUNT(h->timer);
                if ((rc = eg_chi(h, buf ^ 1, recDev, 1)) != ORBX_OK) return rc;
                if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;
                h->solveTicks += (double)rec->ticks;
                const double temp = rec->ok ? rec->chi : DBL_MAX, scale = rec->scale + 1e-3;
                rho = (cur - temp) / scale;
                if (rho > 0.0 && std::isfinite(temp)) {
                    const double t2r = 2.0 * rho - 1.0;
                    double alpha = 1.0 - (t2r * t2r) * t2r;
                    alpha = std::min(alpha, 2.0 / 3.0);
                    lambda = lambda * std::max(1.0 / 3.0, alpha);
                    ni = 2.0;
                    cur = temp;
                    buf ^= 1;      // the trial becomes the estimate; a rejected one is simply left behind (pop())
                } else {
                    lambda = lambda * ni;
                    ni = ni * 2.0;
                }
                qmax++;
            } while (rho < 0.0 && qmax < ORBX_EG_MAX_TRIALS);
            if (R->iter_trials) R->iter_trials[done] = qmax;
            if (R->iter_chi2) R->iter_chi2[done] = cur;
            if (R->iter_lambda) R->iter_lambda[done] = lambda;
            if (R->iter_rho) R->iter_rho[done] = rho;
            done++;
            bool stop = false;
            if (qmax == ORBX_EG_MAX_TRIALS || rho == 0.0) { stop = true; ended = qmax == ORBX_EG_MAX_TRIALS ? ORBX_EG_END_TRIALS : ORBX_EG_END_RHO0; }
            else {
                nBad = (ini - cur) * 1e3 < ini ? nBad + 1 : 0;
                if (nBad >= 3) { stop = true; ended = ORBX_EG_END_THREE; }
            }
            if (stop) break;
        }
    }
    EgOut O;
    O.est = sg.dev(rEst); O.inv = sg.dev(rInv); O.tiw = sg.dev(rTiw); O.points = sg.dev(rPts);
    const unsigned long long seq = bx.arm();
    hipLaunchKernelGGL(k_eg_writeback, dim3((unsigned)eg_blocks(std::max(P->n, P->n_points))), dim3(EG_THREADS), 0, h->stream, h->dev, buf, O, bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_COUNT(h->timer);
    if ((rc = h->timer.end(h->stream)) != ORBX_OK) return rc;
    if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;
    if (R->est) memcpy(R->est, sg.host(rEst), 64 * N);
    if (R->inv) memcpy(R->inv, sg.host(rInv), 64 * N);
    if (R->tiw) memcpy(R->tiw, sg.host(rTiw), 48 * N);
    if (R->points && M) memcpy(R->points, sg.host(rPts), 12 * M);
    if (R->chi2) { R->chi2[0] = chi0; R->chi2[1] = cur; }
    if (R->iterations) *R->iterations = done;
    if (R->ended) *R->ended = ended;
    if (R->order && h->sym.nf) memcpy(R->order, h->sym.order.data(), 4 * (size_t)h->sym.nf);
    if (R->fill_blocks) *R->fill_blocks = h->sym.nf + h->sym.nOff;
    return ORBX_OK;
}

extern "C" int orbx_essential_graph_linearize(orbx_essential_graph *h, const orbx_essential_graph_problem *P, const double *at, double *meas, double *errors, double *chi2,
                                              double *jac, double *h_diag, double *h_off, double *b)
{
    if (!h || !P) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = eg_check(h, P, at)) != ORBX_OK) return rc;
    h->linearized = false;
    if ((rc = eg_symbolic(h, P, h->sym)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    OrbxCallBox &bx = h->box;
    if (bx.pending) { ORBX_HIP_CHECK(hipStreamSynchronize(h->stream)); bx.pending = false; }
    h->timer.launches = 0;
    auto [pin, pout] = bx.plan();
    const EgSlots I(pin, h->sym, P, at);
    const auto rRec = pout.hole<EgRecord>(1);
    const OrbxStaged sg = bx.begin(h->stream, &rc);
    if (rc != ORBX_OK || (rc = eg_stage(h, P, I)) != ORBX_OK) return rc;
    const size_t N = (size_t)P->n, E = (size_t)P->n_edges;
    const EgSymbolic &S = h->sym;
    const EgDev &D = h->dev;
    double chi = 0.0;
    std::vector<double> Hh, bh;
    if (E) {
        if ((rc = eg_chi(h, 0, sg.dev(rRec), 0)) != ORBX_OK) return rc;
        if ((rc = eg_linearize(h, 0)) != ORBX_OK) return rc;
        if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;
        chi = sg.host(rRec)->chi;
    }
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));      // (a tap: plain copies)
    if (E) {
        if (meas) ORBX_HIP_CHECK(hipMemcpy(meas, D.meas, 64 * E, hipMemcpyDeviceToHost));
        if (errors) ORBX_HIP_CHECK(hipMemcpy(errors, D.err, 56 * E, hipMemcpyDeviceToHost));
        if (jac) ORBX_HIP_CHECK(hipMemcpy(jac, D.J, 784 * E, hipMemcpyDeviceToHost));
        Hh.resize(49 * (size_t)(S.nf + S.nOff)); bh.resize(7 * (size_t)S.nf);
        if (!Hh.empty()) ORBX_HIP_CHECK(hipMemcpy(Hh.data(), D.H, 8 * Hh.size(), hipMemcpyDeviceToHost));
        if (!bh.empty()) ORBX_HIP_CHECK(hipMemcpy(bh.data(), D.b, 8 * bh.size(), hipMemcpyDeviceToHost));
    }
    if (chi2) *chi2 = chi;
    if (h_diag) memset(h_diag, 0, 392 * N);
    if (b) memset(b, 0, 56 * N);
    if (h_off && E) memset(h_off, 0, 392 * E);
    if (E) {
        for (int p = 0; p < S.nf; p++) {
            const size_t v = (size_t)S.order[p];
            if (h_diag) memcpy(h_diag + 49 * v, Hh.data() + 49 * (size_t)p, 392);
            if (b) memcpy(b + 7 * v, bh.data() + 7 * (size_t)p, 56);
        }
        if (h_off)
            for (size_t e = 0; e < E; e++) {
                const int pi = S.pos[P->edges[3 * e]], pj = S.pos[P->edges[3 * e + 1]];
                if (pi < 0 || pj < 0) continue;
                const int p = std::max(pi, pj), q = std::min(pi, pj);
                const int32_t *b0 = S.rowIdx.data() + S.colPtr[q], *b1 = S.rowIdx.data() + S.colPtr[q + 1];
                const double *src = Hh.data() + 49 * (size_t)(S.nf + (std::lower_bound(b0, b1, p) - S.rowIdx.data()));
                for (int r = 0; r < 7; r++)
                    for (int c = 0; c < 7; c++) h_off[49 * e + 7 * r + c] = pi > pj ? src[7 * r + c] : src[7 * c + r];      // stored with the later position's rows
            }
    }
    h->linearized = E > 0;
    return ORBX_OK;
}

extern "C" int orbx_essential_graph_solve(orbx_essential_graph *h, double lambda, double *x, int32_t *ok)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (!h->linearized) { orbx_set_error("no orbx_essential_graph_linearize call to solve"); return ORBX_ERR_STATE; }
    if (!std::isfinite(lambda)) { orbx_set_error("non-finite lambda"); return ORBX_ERR_ARG; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const EgSymbolic &S = h->sym;
    const EgDev &D = h->dev;
    hipLaunchKernelGGL(k_eg_solve, dim3(1), dim3(EG_SOLVE_THREADS), 0, h->stream, D, lambda, 0, 0);
    ORBX_LAUNCH_CHECK();
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    std::vector<double> xs(7 * (size_t)S.nf + 1), rec(4);
    ORBX_HIP_CHECK(hipMemcpy(xs.data(), D.xs, 56 * (size_t)S.nf, hipMemcpyDeviceToHost));
    ORBX_HIP_CHECK(hipMemcpy(rec.data(), D.dev, 32, hipMemcpyDeviceToHost));
    const bool solved = rec[1] != 0.0;
    if (ok) *ok = solved ? 1 : 0;
    if (x) {
        memset(x, 0, 56 * (size_t)S.N);      // zeros on a failed factorisation: what the substitutions leave then means nothing
        for (int p = 0; solved && p < S.nf; p++) memcpy(x + 7 * (size_t)S.order[p], xs.data() + 7 * (size_t)p, 56);
    }
    return ORBX_OK;
}

extern "C" int orbx_essential_graph_last_timing(orbx_essential_graph *h, float *device_ms, int *launches, float *solve_ms)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (const int rc = h->timer.read(h->device, device_ms, launches, "no orbx_optimize_essential_graph call to report")) return rc;
    if (solve_ms) *solve_ms = (float)(h->solveTicks / 1e5);      // wall_clock64: 100 MHz
    return ORBX_OK;
}
