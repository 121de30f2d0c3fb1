// orbx_initializer.hip -- monocular initialisation: Initializer::Initialize (src/Initializer.cc:68-230) and everything below it.  gfx950 only.
//
//   k_stage_copy      the call's inputs, mapped pinned memory -> device memory (every later kernel reads them many times)
//   k_init_models     one wave per (iteration, model): the 16x9 (ComputeH21, :419-530) or 8x9 (ComputeF21, :532-613) float system of the
//                     iteration's eight normalised pairs, its null vector by a one-sided Jacobi in FP64 - the 9 columns (16 rows of A over 9 of
//                     V) live in LDS, the four disjoint column pairs of a round-robin round rotate concurrently on 16 lanes each - the rank-2
//                     step for F, the denormalisation, H12 = H21^-1, and CheckHomography / CheckFundamental (:616-953) over all matches: the
//                     chi2 terms 64 matches at a time, the score summed in match order.  Latency bound: 2 x iterations waves, each a chain of
//                     dependent FP64 rotations and then of dependent float additions.  The same kernel scores explicit models.
//   k_init_decompose  two waves: first argmax of the F / H scores, then DecomposeE (:1798-1845, four motions) on one lane of the first and
//                     ReconstructH's Faugeras decomposition (:1150-1345, eight motions) on one lane of the second; 3x3 Jacobi SVD in FP64.
//   k_init_check_rt   CheckRT (:1578-1797): one lane per (hypothesis, match); Triangulate (:1461-1498) through jacobi_null.
//   k_init_rank       four workgroups per hypothesis: nGood and the cosine at sorted index min(50, nGood - 1) by rank counting in LDS.
//   k_init_decide     one workgroup: RH, ReconstructF's (:1030-1125) or ReconstructH's (:1380-1430) selection, the result block in mapped
//                     pinned memory, the sequence word.
//
// Arithmetic: float where the reference is float, in its operation order; 1.0 / x is a double quotient narrowed to float; Mat::dot and
// cv::norm accumulate in double; 3-term matrix products left to right in float; Mat / double divides in double.  The library is built
// with -ffp-contract=off: every product and sum below is its own operation.  The host part (compaction of vMatches12, Normalize :1501-1575)
// is compiled with the same flags.
#include <math.h>

#include <algorithm>
#include <vector>

#include "orbx_match_internal.h"

// Sweeps of the two Jacobi iterations.  Chosen on the CPU with the same iterations restated in numpy float64
// (tests/initializer_ref.py::jacobi_null9 / jacobi_svd3) over every RANSAC set of the test scenes (2022 systems of each kind) and every 3x3
// matrix decomposed on them: no float32 bit of the null vector changes after 8 sweeps (F; H after 6), 8 + 2 = 10; U, w and Vt of the 3x3 SVD
// stop changing after 4 sweeps, 8 are run.  tests/test_initializer.py::test_jacobi_sweeps_settled asserts that two sweeps fewer, the chosen
// counts and two more give the same bits.
#define INIT_NULL_SWEEPS 10
#define INIT_SVD3_SWEEPS 8

#define INIT_COL_PITCH 26      /* doubles per LDS column: 16 rows of A, 9 of V, one of padding */

struct InitBest {              // device: what k_init_decompose, k_init_rank leave for the kernels behind them (and for the diagnostics)
    int32_t bestH, bestF;
    float sh, sf;
    float hypR[ORBX_INIT_HYPOTHESES * 9], hypT[ORBX_INIT_HYPOTHESES * 3];
    int32_t hypValid[ORBX_INIT_HYPOTHESES], hypGood[ORBX_INIT_HYPOTHESES];
    float hypCos[ORBX_INIT_HYPOTHESES];
};
struct InitHead {              // mapped pinned: the head of the result block, p3d[n1][3] and triangulated[n1] follow
    int32_t success, model, hyp, nInlH, nInlF;
    float rh;
    float r21[9], t21[3];
    InitBest best;
};

struct InitModelArgs {
    const float4 *nrm, *raw;          // per match: u1, v1, u2, v2 normalised / in pixels
    const int32_t *sets;
    const float *explicitModels;      // NULL = the chain; else nmodels x 9 of kind `kind`
    int kind, N, iters, nmodels;
    float t1[9], t2inv[9], t2t[9];
    float invSigma2;
    float *hn, *fpre, *fn, *h21, *h12, *f21, *score;
    uint8_t *inl;                     // [nmodels][N]
};

__device__ __host__ __forceinline__ void mul3(const float (&A)[9], const float (&B)[9], float (&C)[9])
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// Mat::inv of a 3x3 float matrix: cofactors over the determinant in double, narrowed to float
__device__ __host__ __forceinline__ void inv3(const float (&M)[9], float (&R)[9])
{
    const double m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5], m20 = M[6], m21 = M[7], m22 = M[8];
    const double c00 = m11 * m22 - m12 * m21, c01 = m02 * m21 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c10 = m12 * m20 - m10 * m22, c11 = m00 * m22 - m02 * m20, c12 = m02 * m10 - m00 * m12;
    const double c20 = m10 * m21 - m11 * m20, c21 = m01 * m20 - m00 * m21, c22 = m00 * m11 - m01 * m10;
    const double det = (m00 * c00 + m01 * c10) + m02 * c20;
    R[0] = (float)(c00 / det); R[1] = (float)(c01 / det); R[2] = (float)(c02 / det);
    R[3] = (float)(c10 / det); R[4] = (float)(c11 / det); R[5] = (float)(c12 / det);
    R[6] = (float)(c20 / det); R[7] = (float)(c21 / det); R[8] = (float)(c22 / det);
}

__device__ __forceinline__ double det3d(const float (&M)[9])
{
    const double m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5], m20 = M[6], m21 = M[7], m22 = M[8];
    return (m00 * (m11 * m22 - m12 * m21) + m01 * (m12 * m20 - m10 * m22)) + m02 * (m10 * m21 - m11 * m20);
}

__device__ __forceinline__ void jacobi_rotation(double alpha, double beta, double gamma, double &c, double &s)
{
    c = 1.0; s = 0.0;
    if (gamma != 0.0) {
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        c = 1.0 / sqrt(1.0 + t * t);
        s = c * t;
    }
}

// SVD of a 3x3 float matrix, A = U diag(w) Vt, narrowed to float as cv::SVD leaves it for a float matrix: one-sided Jacobi in FP64 on the
// columns (cyclic (0,1) (0,2) (1,2)), singular values = column norms sorted descending (stable), U's columns = the rotated columns over
// their norms.  crossU3: U's third column = u1 x u2 instead (DecomposeE: the third singular value of an essential matrix is rounding
// noise, and so would be the column over it; the sign of that column is arbitrary in any SVD).  Registers only.
__device__ __forceinline__ void svd3(const float (&A)[9], bool crossU3, float (&U)[9], float (&w)[3], float (&Vt)[9])
{
    double a[3][3], v[3][3];      // [column][row]
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) { a[c][r] = (double)A[3 * r + c]; v[c][r] = r == c ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < INIT_SVD3_SWEEPS; sweep++) {
#pragma unroll
        for (int p = 0; p < 2; p++) {
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                const double alpha = (a[p][0] * a[p][0] + a[p][1] * a[p][1]) + a[p][2] * a[p][2];
                const double beta = (a[q][0] * a[q][0] + a[q][1] * a[q][1]) + a[q][2] * a[q][2];
                const double gamma = (a[p][0] * a[q][0] + a[p][1] * a[q][1]) + a[p][2] * a[q][2];
                double c, s;
                jacobi_rotation(alpha, beta, gamma, c, s);
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    const double ap = a[p][r], aq = a[q][r], vp = v[p][r], vq = v[q][r];
                    a[p][r] = c * ap - s * aq; a[q][r] = s * ap + c * aq;
                    v[p][r] = c * vp - s * vq; v[q][r] = s * vp + c * vq;
                }
            }
        }
    }
    double n[3];
#pragma unroll
    for (int c = 0; c < 3; c++) n[c] = sqrt((a[c][0] * a[c][0] + a[c][1] * a[c][1]) + a[c][2] * a[c][2]);
    // stable descending order: bubble sort with strict comparisons, the columns themselves are exchanged
#define SVD3_CSWAP(p, q)                                                                                         \
    {                                                                                                            \
        const bool sw = n[q] > n[p];                                                                             \
        const double tn = n[p]; n[p] = sw ? n[q] : n[p]; n[q] = sw ? tn : n[q];                                  \
        _Pragma("unroll") for (int r = 0; r < 3; r++) {                                                          \
            const double ta = a[p][r]; a[p][r] = sw ? a[q][r] : a[p][r]; a[q][r] = sw ? ta : a[q][r];            \
            const double tv = v[p][r]; v[p][r] = sw ? v[q][r] : v[p][r]; v[q][r] = sw ? tv : v[q][r];            \
        }                                                                                                        \
    }
    SVD3_CSWAP(0, 1) SVD3_CSWAP(1, 2) SVD3_CSWAP(0, 1)
#undef SVD3_CSWAP
    double u[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) u[c][r] = a[c][r] / n[c];
    if (crossU3) {
        u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
        u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
        u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        w[c] = (float)n[c];
#pragma unroll
        for (int r = 0; r < 3; r++) { U[3 * r + c] = (float)u[c][r]; Vt[3 * c + r] = (float)v[c][r]; }
    }
}

// entry (r, c) of ComputeH21's A (:472-502): rows 2i, 2i+1 from pair i = (u1, v1, u2, v2)
__device__ __forceinline__ float entry_h(const float (*pts)[4], int r, int c)
{
    const int i = r >> 1;
    const float u1 = pts[i][0], v1 = pts[i][1], u2 = pts[i][2], v2 = pts[i][3];
    if (!(r & 1)) {
        switch (c) {
        case 3: return -u1;
        case 4: return -v1;
        case 5: return -1.0f;
        case 6: return v2 * u1;
        case 7: return v2 * v1;
        case 8: return v2;
        default: return 0.0f;
        }
    }
    switch (c) {
    case 0: return u1;
    case 1: return v1;
    case 2: return 1.0f;
    case 6: return (-u2) * u1;
    case 7: return (-u2) * v1;
    case 8: return -u2;
    default: return 0.0f;
    }
}
// entry (r, c) of ComputeF21's A (:561-577): row i from pair i; rows 8..15 are padding
__device__ __forceinline__ float entry_f(const float (*pts)[4], int r, int c)
{
    if (r >= 8) return 0.0f;
    const float u1 = pts[r][0], v1 = pts[r][1], u2 = pts[r][2], v2 = pts[r][3];
    switch (c) {
    case 0: return u2 * u1;
    case 1: return u2 * v1;
    case 2: return u2;
    case 3: return v2 * u1;
    case 4: return v2 * v1;
    case 5: return v2;
    case 6: return u1;
    case 7: return v1;
    default: return 1.0f;
    }
}

// grid = nmodels workgroups of one wave.  The chain: workgroup b < iters is H of iteration b, b >= iters is F of iteration b - iters.
__global__ __launch_bounds__(64) void k_init_models(InitModelArgs P)
{
    __shared__ double col[9][INIT_COL_PITCH];
    __shared__ double n2s[9];
    __shared__ float pts[8][4];
    __shared__ float terms[128];
    const int lane = threadIdx.x, b = blockIdx.x;
    const bool expl = P.explicitModels != nullptr;
    const bool isF = expl ? P.kind == 1 : b >= P.iters;
    const int it = (!expl && isF) ? b - P.iters : b;
    float M21[9], M12[9];
#pragma unroll
    for (int j = 0; j < 9; j++) M12[j] = 0.0f;
    if (!expl) {
        if (lane < 8) {
            const float4 q = P.nrm[P.sets[8 * it + lane]];
            pts[lane][0] = q.x; pts[lane][1] = q.y; pts[lane][2] = q.z; pts[lane][3] = q.w;
        }
        __syncthreads();
        for (int e = lane; e < 9 * 25; e += 64) {
            const int c = e / 25, r = e - 25 * c;
            double val;
            if (r >= 16) val = (r - 16 == c) ? 1.0 : 0.0;
            else val = (double)(isF ? entry_f(pts, r, c) : entry_h(pts, r, c));
            col[c][r] = val;
        }
        __syncthreads();
        // One-sided Jacobi.  Round rnd = 0..8 of the circle method over 9 columns and a bye: the pairs ((rnd + k) % 9, (rnd - k) % 9), k = 1..4, are
        // disjoint; 16-lane group k - 1 takes pair k, lane l of it row l of A and, for l < 9, row l of V.  Only A's rows enter the dot products.
        const int g = lane >> 4, l = lane & 15;
#pragma unroll 1
        for (int sweep = 0; sweep < INIT_NULL_SWEEPS; sweep++) {
#pragma unroll 1
            for (int rnd = 0; rnd < 9; rnd++) {
                const int ca = (rnd + g + 1) % 9, cb = (rnd + 8 - g) % 9;
                const int p = min(ca, cb), q = max(ca, cb);
                const double x0 = col[p][l], y0 = col[q][l];
                double x1 = 0.0, y1 = 0.0;
                if (l < 9) { x1 = col[p][16 + l]; y1 = col[q][16 + l]; }
                double alpha = x0 * x0, beta = y0 * y0, gamma = x0 * y0;
                // (not wave_sum_xor<16>: the three chains interleaved, shuffled at full width, are the instruction order the FP64 results were pinned with)
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    alpha = alpha + __shfl_xor(alpha, o);
                    beta = beta + __shfl_xor(beta, o);
                    gamma = gamma + __shfl_xor(gamma, o);
                }
                double c, s;
                jacobi_rotation(alpha, beta, gamma, c, s);
                col[p][l] = c * x0 - s * y0;
                col[q][l] = s * x0 + c * y0;
                if (l < 9) { col[p][16 + l] = c * x1 - s * y1; col[q][16 + l] = s * x1 + c * y1; }
                __syncthreads();
            }
        }
        if (lane < 9) {
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < 16; r++) s = s + col[lane][r] * col[lane][r];
            n2s[lane] = s;
        }
        __syncthreads();
        int k = 0;
#pragma unroll
        for (int c = 1; c < 9; c++) k = n2s[c] < n2s[k] ? c : k;      // the first of equal norms
        float nv[9];
#pragma unroll
        for (int j = 0; j < 9; j++) nv[j] = (float)col[k][16 + j];
        float tmp[9];
        if (!isF) {
            if (lane < 9) P.hn[9 * it + lane] = (float)col[k][16 + lane];
            mul3(P.t2inv, nv, tmp);
            mul3(tmp, P.t1, M21);      // H21i = T2inv * Hn * T1 (:308)
        } else {
            if (lane < 9) P.fpre[9 * it + lane] = (float)col[k][16 + lane];
            float U[9], w[3], Vt[9], D[9], fn[9];
            svd3(nv, false, U, w, Vt);
#pragma unroll
            for (int j = 0; j < 9; j++) D[j] = 0.0f;
            D[0] = w[0]; D[4] = w[1];      // w.at<float>(2) = 0 (:608)
            mul3(U, D, tmp);
            mul3(tmp, Vt, fn);             // u * diag(w) * vt (:610)
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < 9; j++) P.fn[9 * it + j] = fn[j];
            }
            mul3(P.t2t, fn, tmp);
            mul3(tmp, P.t1, M21);          // F21i = T2t * Fn * T1 (:385)
        }
    } else {
#pragma unroll
        for (int j = 0; j < 9; j++) M21[j] = P.explicitModels[9 * (size_t)b + j];
    }
    if (!isF) inv3(M21, M12);              // H12i = H21i.inv() (:310)
    if (lane == 0) {
        float *dst = isF ? P.f21 : P.h21;
#pragma unroll
        for (int j = 0; j < 9; j++) dst[9 * it + j] = M21[j];
        if (!isF) {
#pragma unroll
            for (int j = 0; j < 9; j++) P.h12[9 * it + j] = M12[j];
        }
    }
    // ---- CheckHomography (:616-810) / CheckFundamental (:813-953) ----
    const float th = isF ? 3.841f : 5.991f, thScore = 5.991f;
    float score = 0.0f;
    for (int base = 0; base < P.N; base += 64) {
        const int m = base + lane;
        float ta = 0.0f, tb = 0.0f;
        if (m < P.N) {
            const float4 q = P.raw[m];
            const float u1 = q.x, v1 = q.y, u2 = q.z, v2 = q.w;
            float chi1, chi2;
            if (!isF) {
                const float w2 = (float)(1.0 / (double)((M12[6] * u2 + M12[7] * v2) + M12[8]));
                const float u2in1 = ((M12[0] * u2 + M12[1] * v2) + M12[2]) * w2;
                const float v2in1 = ((M12[3] * u2 + M12[4] * v2) + M12[5]) * w2;
                chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * P.invSigma2;
                const float w1 = (float)(1.0 / (double)((M21[6] * u1 + M21[7] * v1) + M21[8]));
                const float u1in2 = ((M21[0] * u1 + M21[1] * v1) + M21[2]) * w1;
                const float v1in2 = ((M21[3] * u1 + M21[4] * v1) + M21[5]) * w1;
                chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * P.invSigma2;
            } else {
                const float a2 = (M21[0] * u1 + M21[1] * v1) + M21[2];
                const float b2 = (M21[3] * u1 + M21[4] * v1) + M21[5];
                const float c2 = (M21[6] * u1 + M21[7] * v1) + M21[8];
                const float num2 = (a2 * u2 + b2 * v2) + c2;
                chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * P.invSigma2;
                const float a1 = (M21[0] * u2 + M21[3] * v2) + M21[6];
                const float b1 = (M21[1] * u2 + M21[4] * v2) + M21[7];
                const float c1 = (M21[2] * u2 + M21[5] * v2) + M21[8];
                const float num1 = (a1 * u1 + b1 * v1) + c1;
                chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * P.invSigma2;
            }
            const bool in1 = !(chi1 > th), in2 = !(chi2 > th);
            ta = in1 ? thScore - chi1 : 0.0f;      // a rejected term adds +0: the sum's bits are those of the reference's conditional additions
            tb = in2 ? thScore - chi2 : 0.0f;
            P.inl[(size_t)b * P.N + m] = (in1 && in2) ? 1 : 0;
        }
        terms[2 * lane] = ta; terms[2 * lane + 1] = tb;
        __syncthreads();
        const int cnt = 2 * min(64, P.N - base);
        for (int j = 0; j < cnt; j++) score = score + terms[j];      // in match order, every lane the same sum
        __syncthreads();
    }
    if (lane == 0) P.score[b] = score;
}

// first argmax over score[0..n): the iteration FindHomography / FindFundamental keep (currentScore > score, strict, :319 / :392)
__device__ __forceinline__ int wave_first_argmax(const float *score, int n, int lane, float &best)
{
    float bv = -1.0f;
    int bi = 0x7fffffff;
    for (int i = lane; i < n; i += 64) { const float v = score[i]; if (v > bv) { bv = v; bi = i; } }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (bi == 0x7fffffff) { bi = 0; bv = score[0]; }
    best = bv;
    return bi;
}

__device__ __forceinline__ void store_motion(InitBest *B, int k, const float (&R)[9], const float (&t)[3], int valid)
{
#pragma unroll
    for (int j = 0; j < 9; j++) B->hypR[9 * k + j] = R[j];
#pragma unroll
    for (int j = 0; j < 3; j++) B->hypT[3 * k + j] = t[j];
    B->hypValid[k] = valid;
}

__device__ __forceinline__ void unit3(const float (&t)[3], float (&o)[3])
{
    const double n = sqrt(((double)t[0] * (double)t[0] + (double)t[1] * (double)t[1]) + (double)t[2] * (double)t[2]);      // cv::norm
#pragma unroll
    for (int j = 0; j < 3; j++) o[j] = (float)((double)t[j] / n);
}

__global__ __launch_bounds__(128) void k_init_decompose(const float *__restrict__ score, int iters, const float *__restrict__ h21, const float *__restrict__ f21, float fx, float fy,
                                                        float cx, float cy, InitBest *__restrict__ B)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float Km[9] = {fx, 0.0f, cx, 0.0f, fy, cy, 0.0f, 0.0f, 1.0f};
    float bs;
    const int bi = wave_first_argmax(score + (wave == 0 ? iters : 0), iters, lane, bs);
    if (lane != 0) return;
    float tmp[9];
    if (wave == 0) {
        // ---- ReconstructF's motions: E21 = K.t() * F21 * K (:1042), DecomposeE (:1798-1845) ----
        B->bestF = bi; B->sf = bs;
        const float Kt[9] = {fx, 0.0f, 0.0f, 0.0f, fy, 0.0f, cx, cy, 1.0f};
        float F[9], E[9], U[9], w[3], Vt[9];
#pragma unroll
        for (int j = 0; j < 9; j++) F[j] = f21[9 * bi + j];
        mul3(Kt, F, tmp);
        mul3(tmp, Km, E);
        svd3(E, true, U, w, Vt);
        const float t0[3] = {U[2], U[5], U[8]};
        float t[3], tn[3];
        unit3(t0, t);
#pragma unroll
        for (int j = 0; j < 3; j++) tn[j] = -t[j];
        const float W[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f}, Wt[9] = {0.0f, 1.0f, 0.0f, -1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
        float R1[9], R2[9];
        mul3(U, W, tmp);
        mul3(tmp, Vt, R1);
        if (det3d(R1) < 0.0) {
#pragma unroll
            for (int j = 0; j < 9; j++) R1[j] = -R1[j];
        }
        mul3(U, Wt, tmp);
        mul3(tmp, Vt, R2);
        if (det3d(R2) < 0.0) {
#pragma unroll
            for (int j = 0; j < 9; j++) R2[j] = -R2[j];
        }
        store_motion(B, 0, R1, t, 1); store_motion(B, 1, R2, t, 1); store_motion(B, 2, R1, tn, 1); store_motion(B, 3, R2, tn, 1);
    } else {
        // ---- ReconstructH's motions (:1150-1345) ----
        B->bestH = bi; B->sh = bs;
        float invK[9], H[9], A[9], U[9], w[3], Vt[9];
        inv3(Km, invK);
#pragma unroll
        for (int j = 0; j < 9; j++) H[j] = h21[9 * bi + j];
        mul3(invK, H, tmp);
        mul3(tmp, Km, A);
        svd3(A, false, U, w, Vt);
        const float s = (float)(det3d(U) * det3d(Vt));
        const float d1 = w[0], d2 = w[1], d3 = w[2];
        const double q12 = (double)(d1 / d2), q23 = (double)(d2 / d3);
        const bool valid = !(q12 < 1.00001 || q23 < 1.00001) && isfinite(q12) && isfinite(q23);
        const float zeroR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, zeroT[3] = {0, 0, 0};
        if (!valid) {
#pragma unroll
            for (int k = 4; k < 12; k++) store_motion(B, k, zeroR, zeroT, 0);
            return;
        }
        const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
        const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
        const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
        const float auxSt = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
        const float ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
        const float st[4] = {auxSt, -auxSt, -auxSt, auxSt};
        const float auxSp = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
        const float cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
        const float sp[4] = {auxSp, -auxSp, -auxSp, auxSp};
        float sU[9];
#pragma unroll
        for (int j = 0; j < 9; j++) sU[j] = s * U[j];
#pragma unroll
        for (int fam = 0; fam < 2; fam++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, tp[3], R[9], t[3], tu[3];
                if (fam == 0) {
                    Rp[0] = ct; Rp[2] = -st[i]; Rp[6] = st[i]; Rp[8] = ct;
                    const float k = d1 - d3;
                    tp[0] = x1[i] * k; tp[1] = 0.0f * k; tp[2] = (-x3[i]) * k;
                } else {
                    Rp[0] = cp; Rp[2] = sp[i]; Rp[4] = -1.0f; Rp[6] = sp[i]; Rp[8] = -cp;
                    const float k = d1 + d3;
                    tp[0] = x1[i] * k; tp[1] = 0.0f * k; tp[2] = x3[i] * k;
                }
                mul3(sU, Rp, tmp);
                mul3(tmp, Vt, R);
#pragma unroll
                for (int r = 0; r < 3; r++) t[r] = (U[3 * r] * tp[0] + U[3 * r + 1] * tp[1]) + U[3 * r + 2] * tp[2];
                unit3(t, tu);
                store_motion(B, 4 + 4 * fam + i, R, tu, 1);
            }
        }
    }
}

struct InitRtArgs {
    const float4 *raw;
    const float *hypR, *hypT;          // [nh][9], [nh][3]
    const int32_t *hypValid;           // [nh] or NULL
    const uint8_t *inlBase;            // the chain: [2 * iters][N], best row read from `best`; explicit: [N]
    const InitBest *best;              // NULL = explicit
    int iters, N;
    float fx, fy, cx, cy, th2;
    uint8_t *status;                   // [nh][N]
    float *p3d, *cosp;                 // [nh][N][3], [nh][N]
};

// grid (ceil(N / 256), hypotheses)
__global__ __launch_bounds__(256) void k_init_check_rt(InitRtArgs P)
{
    const int h = blockIdx.y, m = blockIdx.x * 256 + threadIdx.x;
    if (m >= P.N) return;
    const bool valid = P.hypValid ? P.hypValid[h] != 0 : true;
    size_t row = 0;
    if (P.best) row = h < 4 ? (size_t)(P.iters + P.best->bestF) : (size_t)P.best->bestH;
    const bool inl = P.inlBase[row * P.N + m] != 0;
    float p[3] = {0.0f, 0.0f, 0.0f}, cosp = 0.0f;
    int st = ORBX_INIT_NOT_INLIER;
    if (valid && inl) {
        float R[9], t[3];
#pragma unroll
        for (int j = 0; j < 9; j++) R[j] = P.hypR[9 * h + j];
#pragma unroll
        for (int j = 0; j < 3; j++) t[j] = P.hypT[3 * h + j];
        const float4 q = P.raw[m];
        const float K[9] = {P.fx, 0.0f, P.cx, 0.0f, P.fy, P.cy, 0.0f, 0.0f, 1.0f};
        // P1 = K [I | 0], P2 = K * [R | t] (:1620-1640)
        const float P1[3][4] = {{P.fx, 0.0f, P.cx, 0.0f}, {0.0f, P.fy, P.cy, 0.0f}, {0.0f, 0.0f, 1.0f, 0.0f}};
        float P2[3][4];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) P2[i][j] = (K[3 * i] * R[j] + K[3 * i + 1] * R[3 + j]) + K[3 * i + 2] * R[6 + j];
            P2[i][3] = (K[3 * i] * t[0] + K[3 * i + 1] * t[1]) + K[3 * i + 2] * t[2];
        }
        float r0[4], r1[4], r2[4], r3[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            r0[c] = q.x * P1[2][c] - P1[0][c];
            r1[c] = q.y * P1[2][c] - P1[1][c];
            r2[c] = q.z * P2[2][c] - P2[0][c];
            r3[c] = q.w * P2[2][c] - P2[1][c];
        }
        double nv[4];
        jacobi_null(r0, r1, r2, r3, nv);
#pragma unroll
        for (int i = 0; i < 3; i++) p[i] = (float)(nv[i] / nv[3]);
        if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) {
            st = ORBX_INIT_NONFINITE;
            p[0] = p[1] = p[2] = 0.0f;
        } else {
            float O2[3], n2[3], p2[3];
#pragma unroll
            for (int i = 0; i < 3; i++) O2[i] = ((-R[i]) * t[0] + (-R[3 + i]) * t[1]) + (-R[6 + i]) * t[2];      // -R.t() * t
            const double pd0 = p[0], pd1 = p[1], pd2 = p[2];
            const float dist1 = (float)sqrt((pd0 * pd0 + pd1 * pd1) + pd2 * pd2);
#pragma unroll
            for (int i = 0; i < 3; i++) n2[i] = p[i] - O2[i];
            const double nd0 = n2[0], nd1 = n2[1], nd2 = n2[2];
            const float dist2 = (float)sqrt((nd0 * nd0 + nd1 * nd1) + nd2 * nd2);
            cosp = (float)(((pd0 * nd0 + pd1 * nd1) + pd2 * nd2) / (double)(dist1 * dist2));
            const bool low = (double)cosp < 0.99998;
#pragma unroll
            for (int i = 0; i < 3; i++) p2[i] = ((R[3 * i] * p[0] + R[3 * i + 1] * p[1]) + R[3 * i + 2] * p[2]) + t[i];
            if (p[2] <= 0 && low) st = ORBX_INIT_BEHIND1;
            else if (p2[2] <= 0 && low) st = ORBX_INIT_BEHIND2;
            else {
                const float invZ1 = (float)(1.0 / (double)p[2]);
                const float ex1 = (P.fx * p[0] * invZ1 + P.cx) - q.x, ey1 = (P.fy * p[1] * invZ1 + P.cy) - q.y;
                const float invZ2 = (float)(1.0 / (double)p2[2]);
                const float ex2 = (P.fx * p2[0] * invZ2 + P.cx) - q.z, ey2 = (P.fy * p2[1] * invZ2 + P.cy) - q.w;
                if (ex1 * ex1 + ey1 * ey1 > P.th2) st = ORBX_INIT_REPROJ1;
                else if (ex2 * ex2 + ey2 * ey2 > P.th2) st = ORBX_INIT_REPROJ2;
                else st = low ? ORBX_INIT_GOOD : ORBX_INIT_GOOD_LOW_PARALLAX;
            }
        }
    }
    const size_t o = (size_t)h * P.N + m;
    P.status[o] = (uint8_t)st;
    P.p3d[3 * o] = p[0]; P.p3d[3 * o + 1] = p[1]; P.p3d[3 * o + 2] = p[2];
    P.cosp[o] = cosp;
}

#define RANK_THREADS 256
#define RANK_SPLIT 4
// grid (hypotheses, RANK_SPLIT); dynamic LDS: N floats rounded up to 4.  good[h] = nGood; cosSel[h] = sorted cosine number min(50, nGood - 1)
// (:1775-1790), 1.0 when nothing is good (acos(1) = 0 = the reference's parallax of that case).  Equal cosines are ranked by match index.
// Every workgroup of a hypothesis stages all its cosines and ranks its own share of them against all (16 bytes per LDS read); exactly one
// lane of one of them holds rank `want` and stores.  (One workgroup of 1024 lanes with 4-byte reads spent 63 us at N = 1000 issuing LDS reads.)
__global__ __launch_bounds__(RANK_THREADS) void k_init_rank(const uint8_t *__restrict__ status, const float *__restrict__ cosp, int N, int32_t *__restrict__ good, float *__restrict__ cosSel)
{
    extern __shared__ float4 lc4[];
    float *lc = (float *)lc4;
    __shared__ int cnt;
    const int h = blockIdx.x, tid = threadIdx.x, N4 = (N + 3) >> 2;
    if (tid == 0) cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < 4 * N4; i += RANK_THREADS) {
        bool g = false;
        if (i < N) { const unsigned st = status[(size_t)h * N + i]; g = st == ORBX_INIT_GOOD || st == ORBX_INIT_GOOD_LOW_PARALLAX; }
        lc[i] = g ? cosp[(size_t)h * N + i] : INFINITY;
        mine += g ? 1 : 0;
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    const int n = cnt;
    if (tid == 0 && blockIdx.y == 0) { good[h] = n; if (n == 0) cosSel[h] = 1.0f; }
    if (n == 0) return;
    const int want = min(50, n - 1);
    for (int i = blockIdx.y * RANK_THREADS + tid; i < N; i += RANK_THREADS * RANK_SPLIT) {
        const float c = lc[i];
        if (c == INFINITY) continue;
        int rank = 0;
        for (int j4 = 0; j4 < N4; j4++) {
            const float4 d = lc4[j4];
            const int j = 4 * j4;
            rank += (d.x < c || (d.x == c && j < i)) ? 1 : 0;
            rank += (d.y < c || (d.y == c && j + 1 < i)) ? 1 : 0;
            rank += (d.z < c || (d.z == c && j + 2 < i)) ? 1 : 0;
            rank += (d.w < c || (d.w == c && j + 3 < i)) ? 1 : 0;
        }
        if (rank == want) cosSel[h] = c;
    }
}

struct InitDecideArgs {
    InitBest *best;
    const uint8_t *inlBase; int iters, N, n1;
    const int32_t *slot;               // [n1]: the match of frame-1 keypoint i1, or -1
    const uint8_t *status; const float *p3d;      // k_init_check_rt's
    float cosGt, cosGe;                // parallax > / >= min_parallax  <=>  cosine <= cosGt / cosGe
    int minTriangulated;
    InitHead *head; float *outP3d; uint8_t *outTri;      // mapped pinned
    unsigned *counter; unsigned long long *flag; unsigned long long seq;
};

__global__ __launch_bounds__(256) void k_init_decide(InitDecideArgs P)
{
    __shared__ int nIn[2], sel;
    const int tid = threadIdx.x;
    if (tid < 2) nIn[tid] = 0;
    __syncthreads();
    const InitBest &B = *P.best;
    const uint8_t *inlH = P.inlBase + (size_t)B.bestH * P.N, *inlF = P.inlBase + (size_t)(P.iters + B.bestF) * P.N;
    int ch = 0, cf = 0;
    for (int i = tid; i < P.N; i += 256) { ch += inlH[i] ? 1 : 0; cf += inlF[i] ? 1 : 0; }
    if (ch) atomicAdd(&nIn[0], ch);
    if (cf) atomicAdd(&nIn[1], cf);
    __syncthreads();
    if (tid == 0) {
        const float rh = B.sh / (B.sh + B.sf);      // :203
        int hyp = -1, model;
        if (rh > 0.40f) {
            // ReconstructH's selection (:1380-1430)
            model = 0;
            if (B.hypValid[4]) {
                int bestGood = 0, second = 0, idx = -1;
                for (int i = 4; i < 12; i++) {
                    const int g = B.hypGood[i];
                    if (g > bestGood) { second = bestGood; bestGood = g; idx = i; }
                    else if (g > second) second = g;
                }
                if (idx >= 0 && (double)second < 0.75 * (double)bestGood && B.hypCos[idx] <= P.cosGe && bestGood > P.minTriangulated && (double)bestGood > 0.9 * (double)nIn[0]) hyp = idx;
            }
        } else {
            // ReconstructF's selection (:1030-1125); only the FIRST hypothesis that reaches maxGood is asked for its parallax (the else-if chain)
            model = 1;
            int mx = 0;
            for (int i = 0; i < 4; i++) mx = max(mx, B.hypGood[i]);
            const int nMin = max((int)(0.9 * (double)nIn[1]), P.minTriangulated);
            int nsimilar = 0, first = -1;
            for (int i = 0; i < 4; i++) {
                nsimilar += (double)B.hypGood[i] > 0.7 * (double)mx ? 1 : 0;
                if (first < 0 && B.hypGood[i] == mx) first = i;
            }
            if (!(mx < nMin || nsimilar > 1) && B.hypCos[first] <= P.cosGt) hyp = first;
        }
        InitHead *H = P.head;
        H->success = hyp >= 0 ? 1 : 0; H->model = model; H->hyp = hyp; H->nInlH = nIn[0]; H->nInlF = nIn[1]; H->rh = rh;
        for (int j = 0; j < 9; j++) H->r21[j] = hyp >= 0 ? B.hypR[9 * hyp + j] : 0.0f;
        for (int j = 0; j < 3; j++) H->t21[j] = hyp >= 0 ? B.hypT[3 * hyp + j] : 0.0f;
        H->best = B;
        sel = hyp;
    }
    __syncthreads();
    const int hyp = sel;
    for (int i = tid; i < P.n1; i += 256) {
        float x = 0.0f, y = 0.0f, z = 0.0f;
        uint8_t tri = 0;
        const int m = P.slot[i];
        if (hyp >= 0 && m >= 0) {
            const size_t o = (size_t)hyp * P.N + m;
            const unsigned st = P.status[o];
            if (st == ORBX_INIT_GOOD || st == ORBX_INIT_GOOD_LOW_PARALLAX) { x = P.p3d[3 * o]; y = P.p3d[3 * o + 1]; z = P.p3d[3 * o + 2]; tri = st == ORBX_INIT_GOOD ? 1 : 0; }
        }
        P.outP3d[3 * (size_t)i] = x; P.outP3d[3 * (size_t)i + 1] = y; P.outP3d[3 * (size_t)i + 2] = z;
        P.outTri[i] = tri;
    }
    orbx_publish(P.counter, P.flag, P.seq, 1);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------------
struct orbx_initializer : OrbxHandle {
    int maxMatches = 0, maxIters = 0;
    OrbxCallTimer timer;
    OrbxCallBox box;                   // inputs and results of a call: mapped pinned memory + the sequence word
    OrbxOwnedBuf<uint8_t> arena;         // the inputs on the device (k_stage_copy), same offsets as in box.in
    OrbxOwnedBuf<float> hn, fpre, fn, h21, h12, f21, score, crtP3d, crtCos, rankCos;
    OrbxOwnedBuf<uint8_t> inl, crtStatus;
    OrbxOwnedBuf<int32_t> rankGood;
    OrbxOwnedBuf<InitBest> best;
};

namespace {
// Normalize (:1501-1575) over all keypoints of a frame: the mean and the mean absolute deviation are sequential float sums
void normalize_host(const float *xy, int n, std::vector<float> &pn, float (&T)[9])
{
    float meanX = 0, meanY = 0;
    for (int i = 0; i < n; i++) { meanX += xy[2 * i]; meanY += xy[2 * i + 1]; }
    meanX = meanX / n; meanY = meanY / n;
    float meanDevX = 0, meanDevY = 0;
    pn.resize(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        pn[2 * i] = xy[2 * i] - meanX; pn[2 * i + 1] = xy[2 * i + 1] - meanY;
        meanDevX += fabsf(pn[2 * i]); meanDevY += fabsf(pn[2 * i + 1]);
    }
    meanDevX = meanDevX / n; meanDevY = meanDevY / n;
    const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
    for (int i = 0; i < n; i++) { pn[2 * i] = pn[2 * i] * sX; pn[2 * i + 1] = pn[2 * i + 1] * sY; }
    const float t[9] = {sX, 0.0f, -meanX * sX, 0.0f, sY, -meanY * sY, 0.0f, 0.0f, 1.0f};
    memcpy(T, t, sizeof(t));
}

float parallax_deg(float c)      // acos(vCosParallax[idx]) * 180 / CV_PI (:1787)
{
    const float a = acosf(c);
    return (float)((double)(a * 180.0f) / 3.1415926535897932384626433832795);
}

// the largest cosine whose parallax still passes `parallax > minParallax` (strict) or `>=`; parallax_deg falls as the cosine grows
float cos_bound(float minParallax, bool strict)
{
    auto pass = [&](float c) { const float p = parallax_deg(c); return strict ? p > minParallax : p >= minParallax; };
    if (pass(1.0f)) return 1.0f;
    if (!pass(-1.0f)) return -2.0f;
    float lo = -1.0f, hi = 1.0f;      // pass(lo), !pass(hi)
    while (nextafterf(lo, 2.0f) < hi) {
        float mid = (float)(((double)lo + (double)hi) / 2.0);
        if (!(mid > lo && mid < hi)) mid = nextafterf(lo, 2.0f);
        if (pass(mid)) lo = mid; else hi = mid;
    }
    return lo;
}

struct Staged {      // the matches in box.in / the arena
    OrbxSlot<float, ORBX_STAGE_IN> raw, nrm;
    OrbxSlot<int32_t, ORBX_STAGE_IN> slot;
    int N = 0;
    float t1[9], t2[9];
};

int check_matches(const orbx_init_matches *M)
{
    if (!M || !M->keys1_xy || !M->keys2_xy || !M->matches12 || M->n1 < 1 || M->n2 < 1) { orbx_set_error("bad match arguments"); return ORBX_ERR_ARG; }
    for (int i = 0; i < M->n1; i++)
        if (M->matches12[i] >= M->n2) { orbx_set_error("matches12[%d] = %d is outside frame 2 (%d keypoints)", i, M->matches12[i], M->n2); return ORBX_ERR_ARG; }
    return ORBX_OK;
}

// vMatches12 compacted in i1 order (:96-109) into the mapped input buffer; with `normalise`, Normalize of both frames too.  plan_matches reserves the
// three arrays at the head of the box's input plan (the caller adds its own - sets, models, motions ... - behind them), fill_matches writes them
// after the box's begin().
int plan_matches(orbx_initializer *h, const orbx_init_matches *M, OrbxInPlan &pin, Staged &S)
{
    int N = 0;
    for (int i = 0; i < M->n1; i++) N += M->matches12[i] >= 0 ? 1 : 0;
    if (N > h->maxMatches) { orbx_set_error("%d matches, the initializer was created for %d", N, h->maxMatches); return ORBX_ERR_CAPACITY; }
    S.N = N;
    S.raw = pin.hole<float>((size_t)N * 4); S.nrm = pin.hole<float>((size_t)N * 4); S.slot = pin.hole<int32_t>((size_t)M->n1);
    return ORBX_OK;
}

void fill_matches(const orbx_init_matches *M, bool normalise, const OrbxStaged &sg, Staged &S)
{
    std::vector<float> pn1, pn2;
    if (normalise) { normalize_host(M->keys1_xy, M->n1, pn1, S.t1); normalize_host(M->keys2_xy, M->n2, pn2, S.t2); }
    float *raw = sg.host(S.raw), *nrm = sg.host(S.nrm);
    int32_t *slot = sg.host(S.slot);
    int m = 0;
    for (int i = 0; i < M->n1; i++) {
        const int j = M->matches12[i];
        slot[i] = j >= 0 ? m : -1;
        if (j < 0) continue;
        raw[4 * m] = M->keys1_xy[2 * i]; raw[4 * m + 1] = M->keys1_xy[2 * i + 1]; raw[4 * m + 2] = M->keys2_xy[2 * j]; raw[4 * m + 3] = M->keys2_xy[2 * j + 1];
        if (normalise) { nrm[4 * m] = pn1[2 * i]; nrm[4 * m + 1] = pn1[2 * i + 1]; nrm[4 * m + 2] = pn2[2 * j]; nrm[4 * m + 3] = pn2[2 * j + 1]; }
        else nrm[4 * m] = nrm[4 * m + 1] = nrm[4 * m + 2] = nrm[4 * m + 3] = 0.0f;
        m++;
    }
}

// the box's inputs into the arena (every later kernel reads them many times); the arena keeps 256 bytes behind them
int stage_to_arena(orbx_initializer *h, uint8_t **ar)
{
    const int rc = orbx_stage_to_arena(h->box, h->arena, h->stream, 64, ar, h->box.inPlan.total() + 256);
    if (rc != ORBX_OK) return rc;
    ORBX_LAUNCH_CHECK();
    return ORBX_OK;
}

int ensure_models(orbx_initializer *h)
{
    const size_t I = 2 * (size_t)h->maxIters, N = (size_t)h->maxMatches;
    int rc;
    if ((rc = h->hn.ensure(9 * I)) || (rc = h->fpre.ensure(9 * I)) || (rc = h->fn.ensure(9 * I)) || (rc = h->h21.ensure(9 * I)) || (rc = h->h12.ensure(9 * I)) ||
        (rc = h->f21.ensure(9 * I)) || (rc = h->score.ensure(I)) || (rc = h->inl.ensure(I * N)) || (rc = h->crtStatus.ensure(ORBX_INIT_HYPOTHESES * N)) ||
        (rc = h->crtP3d.ensure(3 * ORBX_INIT_HYPOTHESES * N)) || (rc = h->crtCos.ensure(ORBX_INIT_HYPOTHESES * N)) || (rc = h->best.ensure(1)) ||
        (rc = h->rankCos.ensure(ORBX_INIT_HYPOTHESES)) || (rc = h->rankGood.ensure(ORBX_INIT_HYPOTHESES)))
        return rc;
    return ORBX_OK;
}
}  // namespace

extern "C" int orbx_initializer_create(int device, int max_matches, int max_iterations, orbx_initializer **out)
{
    if (!out || max_matches < 8 || max_matches > ORBX_INIT_MAX_MATCHES || max_iterations < 1 || max_iterations > (1 << 20)) {
        orbx_set_error("bad initializer arguments (8 <= max_matches <= %d, max_iterations >= 1)", ORBX_INIT_MAX_MATCHES);
        return ORBX_ERR_ARG;
    }
    *out = nullptr;
    orbx_initializer *h = new orbx_initializer();
    h->maxMatches = max_matches; h->maxIters = max_iterations;
    int rc;
    if ((rc = h->open(device)) || (rc = h->timer.create()) || (rc = ensure_models(h))) { orbx_destroy_handle(h); return rc; }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_initializer_destroy(orbx_initializer *h) { orbx_destroy_handle(h); }

static void fill_model_args(orbx_initializer *h, const Staged &S, const uint8_t *ar, InitModelArgs &A)
{
    A.nrm = (const float4 *)S.nrm.in(ar); A.raw = (const float4 *)S.raw.in(ar);
    A.sets = nullptr; A.explicitModels = nullptr; A.kind = 0; A.N = S.N; A.iters = 0; A.nmodels = 0;
    A.hn = h->hn.p; A.fpre = h->fpre.p; A.fn = h->fn.p; A.h21 = h->h21.p; A.h12 = h->h12.p; A.f21 = h->f21.p; A.score = h->score.p; A.inl = h->inl.p;
    for (int j = 0; j < 9; j++) A.t1[j] = A.t2inv[j] = A.t2t[j] = 0.0f;
}

static float inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

extern "C" int orbx_initialize(orbx_initializer *h, const orbx_init_problem *P, const orbx_init_result *res)
{
    if (!h || !P || !res) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    const orbx_init_matches M = {P->keys1_xy, P->keys2_xy, P->n1, P->n2, P->matches12};
    int rc;
    if ((rc = check_matches(&M)) != ORBX_OK) return rc;
    if (P->iterations < 1 || !P->sets) { orbx_set_error("iterations %d < 1 or NULL sets", P->iterations); return ORBX_ERR_ARG; }
    if (P->iterations > h->maxIters) { orbx_set_error("%d iterations, the initializer was created for %d", P->iterations, h->maxIters); return ORBX_ERR_CAPACITY; }
    int N = 0;
    for (int i = 0; i < P->n1; i++) N += P->matches12[i] >= 0 ? 1 : 0;
    if (N < 8) { orbx_set_error("%d matches: the minimal sets need 8", N); return ORBX_ERR_ARG; }
    const int iters = P->iterations;
    for (int i = 0; i < 8 * iters; i++)
        if (P->sets[i] < 0 || P->sets[i] >= N) { orbx_set_error("sets[%d][%d] = %d is outside the %d matches", i / 8, i % 8, P->sets[i], N); return ORBX_ERR_ARG; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const size_t n1 = (size_t)P->n1;
    Staged S;
    OrbxCallBox &bx = h->box;
    auto [pin, pout] = bx.plan();
    if ((rc = plan_matches(h, &M, pin, S)) != ORBX_OK) return rc;
    const auto sSets = pin.add(P->sets, (size_t)iters * 8);
    const auto rHead = pout.hole<InitHead>(1);
    const auto rP3d = pout.hole<float>(n1 * 3);
    const auto rTri = pout.hole<uint8_t>(n1);
    const OrbxStaged sg = bx.begin(h->stream, &rc);
    if (rc != ORBX_OK) return rc;
    fill_matches(&M, true, sg, S);

    const unsigned long long seq = bx.arm();
    if ((rc = h->timer.begin(h->stream)) != ORBX_OK) return rc;
    uint8_t *ar;
    if ((rc = stage_to_arena(h, &ar)) != ORBX_OK) return rc;
    InitModelArgs A;
    fill_model_args(h, S, ar, A);
    A.sets = sSets.in(ar); A.iters = iters; A.nmodels = 2 * iters;
    memcpy(A.t1, S.t1, sizeof(A.t1));
    inv3(S.t2, A.t2inv);                                   // T2.inv() (:260)
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) A.t2t[3 * i + j] = S.t2[3 * j + i];      // T2.t() (:354)
    A.invSigma2 = inv_sigma2(P->sigma);
    hipLaunchKernelGGL(k_init_models, dim3((unsigned)(2 * iters)), dim3(64), 0, h->stream, A);
    ORBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_init_decompose, dim3(1), dim3(128), 0, h->stream, (const float *)h->score.p, iters, (const float *)h->h21.p, (const float *)h->f21.p, P->fx, P->fy, P->cx, P->cy,
                       h->best.p);
    ORBX_LAUNCH_CHECK();
    InitRtArgs R;
    R.raw = A.raw; R.hypR = h->best.p->hypR; R.hypT = h->best.p->hypT; R.hypValid = h->best.p->hypValid; R.inlBase = h->inl.p; R.best = h->best.p; R.iters = iters; R.N = N;
    R.fx = P->fx; R.fy = P->fy; R.cx = P->cx; R.cy = P->cy;
    R.th2 = (float)(4.0 * (double)(P->sigma * P->sigma));      // 4.0 * mSigma2 (:1063)
    R.status = h->crtStatus.p; R.p3d = h->crtP3d.p; R.cosp = h->crtCos.p;
    hipLaunchKernelGGL(k_init_check_rt, dim3((unsigned)((N + 255) / 256), ORBX_INIT_HYPOTHESES), dim3(256), 0, h->stream, R);
    ORBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_init_rank, dim3(ORBX_INIT_HYPOTHESES, RANK_SPLIT), dim3(RANK_THREADS), (size_t)((N + 3) & ~3) * 4, h->stream, (const uint8_t *)h->crtStatus.p, (const float *)h->crtCos.p, N,
                       h->best.p->hypGood, h->best.p->hypCos);
    ORBX_LAUNCH_CHECK();
    InitDecideArgs D;
    D.best = h->best.p; D.inlBase = h->inl.p; D.iters = iters; D.N = N; D.n1 = P->n1;
    D.slot = S.slot.in(ar); D.status = h->crtStatus.p; D.p3d = h->crtP3d.p;
    D.cosGt = cos_bound(P->min_parallax, true); D.cosGe = cos_bound(P->min_parallax, false);
    D.minTriangulated = P->min_triangulated;
    D.head = sg.dev(rHead); D.outP3d = sg.dev(rP3d); D.outTri = sg.dev(rTri);
    D.counter = bx.counter; D.flag = bx.flagDev; D.seq = seq;
    hipLaunchKernelGGL(k_init_decide, dim3(1), dim3(256), 0, h->stream, D);
    ORBX_LAUNCH_CHECK();
    if ((rc = h->timer.end(h->stream)) != ORBX_OK) return rc;
    h->timer.launches = 6;
    if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;      // the one synchronisation

    const InitHead *H = sg.host(rHead);
    if (res->success) *res->success = H->success;
    if (res->model) *res->model = H->model;
    if (res->hyp) *res->hyp = H->hyp;
    if (res->r21) memcpy(res->r21, H->r21, sizeof(H->r21));
    if (res->t21) memcpy(res->t21, H->t21, sizeof(H->t21));
    if (res->p3d) memcpy(res->p3d, sg.host(rP3d), n1 * 12);
    if (res->triangulated) memcpy(res->triangulated, sg.host(rTri), n1);
    if (res->n_matches) *res->n_matches = N;
    if (res->t1) memcpy(res->t1, S.t1, sizeof(S.t1));
    if (res->t2) memcpy(res->t2, S.t2, sizeof(S.t2));
    const InitBest &B = H->best;
    if (res->best_h) *res->best_h = B.bestH;
    if (res->best_f) *res->best_f = B.bestF;
    if (res->sh) *res->sh = B.sh;
    if (res->sf) *res->sf = B.sf;
    if (res->rh) *res->rh = H->rh;
    if (res->hyp_r) memcpy(res->hyp_r, B.hypR, sizeof(B.hypR));
    if (res->hyp_t) memcpy(res->hyp_t, B.hypT, sizeof(B.hypT));
    for (int k = 0; k < ORBX_INIT_HYPOTHESES; k++) {
        if (res->hyp_valid) res->hyp_valid[k] = (uint8_t)B.hypValid[k];
        if (res->hyp_good) res->hyp_good[k] = B.hypGood[k];
        if (res->hyp_cos_parallax) res->hyp_cos_parallax[k] = B.hypCos[k];
        if (res->hyp_parallax_deg) res->hyp_parallax_deg[k] = parallax_deg(B.hypCos[k]);
    }
    if (res->hn || res->fpre || res->fn || res->h21 || res->h12 || res->f21 || res->score_h || res->score_f || res->inliers_h || res->inliers_f || res->hyp_status || res->hyp_p3d || res->hyp_cos) {
        // the per-iteration and per-match arrays (tests, diagnostics): copies of their own
        ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
        const size_t b9 = (size_t)iters * 9 * sizeof(float);
        if (res->hn) ORBX_HIP_CHECK(hipMemcpy(res->hn, h->hn.p, b9, hipMemcpyDeviceToHost));
        if (res->fpre) ORBX_HIP_CHECK(hipMemcpy(res->fpre, h->fpre.p, b9, hipMemcpyDeviceToHost));
        if (res->fn) ORBX_HIP_CHECK(hipMemcpy(res->fn, h->fn.p, b9, hipMemcpyDeviceToHost));
        if (res->h21) ORBX_HIP_CHECK(hipMemcpy(res->h21, h->h21.p, b9, hipMemcpyDeviceToHost));
        if (res->h12) ORBX_HIP_CHECK(hipMemcpy(res->h12, h->h12.p, b9, hipMemcpyDeviceToHost));
        if (res->f21) ORBX_HIP_CHECK(hipMemcpy(res->f21, h->f21.p, b9, hipMemcpyDeviceToHost));
        if (res->score_h) ORBX_HIP_CHECK(hipMemcpy(res->score_h, h->score.p, (size_t)iters * 4, hipMemcpyDeviceToHost));
        if (res->score_f) ORBX_HIP_CHECK(hipMemcpy(res->score_f, h->score.p + iters, (size_t)iters * 4, hipMemcpyDeviceToHost));
        if (res->inliers_h) ORBX_HIP_CHECK(hipMemcpy(res->inliers_h, h->inl.p + (size_t)B.bestH * N, (size_t)N, hipMemcpyDeviceToHost));
        if (res->inliers_f) ORBX_HIP_CHECK(hipMemcpy(res->inliers_f, h->inl.p + (size_t)(iters + B.bestF) * N, (size_t)N, hipMemcpyDeviceToHost));
        if (res->hyp_status) ORBX_HIP_CHECK(hipMemcpy(res->hyp_status, h->crtStatus.p, (size_t)ORBX_INIT_HYPOTHESES * N, hipMemcpyDeviceToHost));
        if (res->hyp_p3d) ORBX_HIP_CHECK(hipMemcpy(res->hyp_p3d, h->crtP3d.p, (size_t)ORBX_INIT_HYPOTHESES * N * 12, hipMemcpyDeviceToHost));
        if (res->hyp_cos) ORBX_HIP_CHECK(hipMemcpy(res->hyp_cos, h->crtCos.p, (size_t)ORBX_INIT_HYPOTHESES * N * 4, hipMemcpyDeviceToHost));
    }
    return ORBX_OK;
}

extern "C" int orbx_init_score_models(orbx_initializer *h, const orbx_init_matches *M, const float *models, int m, int kind, float sigma, float *scores, uint8_t *inliers)
{
    if (!h || !models || !scores || !inliers) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = check_matches(M)) != ORBX_OK) return rc;
    if (m < 1 || (kind != 0 && kind != 1)) { orbx_set_error("m = %d models of kind %d (0 = H, 1 = F)", m, kind); return ORBX_ERR_ARG; }
    if (m > 2 * h->maxIters) { orbx_set_error("%d models, the initializer holds %d", m, 2 * h->maxIters); return ORBX_ERR_CAPACITY; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    Staged S;
    auto [pin, pout] = h->box.plan();
    (void)pout;
    if ((rc = plan_matches(h, M, pin, S)) != ORBX_OK) return rc;
    const auto sModels = pin.add(models, (size_t)m * 9);
    const OrbxStaged sg = h->box.begin(h->stream, &rc);
    if (rc != ORBX_OK) return rc;
    fill_matches(M, false, sg, S);
    if (S.N < 1) { orbx_set_error("no matches"); return ORBX_ERR_ARG; }
    uint8_t *ar;
    if ((rc = stage_to_arena(h, &ar)) != ORBX_OK) return rc;
    InitModelArgs A;
    fill_model_args(h, S, ar, A);
    A.explicitModels = sModels.in(ar); A.kind = kind; A.nmodels = m; A.iters = m;
    A.invSigma2 = inv_sigma2(sigma);
    hipLaunchKernelGGL(k_init_models, dim3((unsigned)m), dim3(64), 0, h->stream, A);
    ORBX_LAUNCH_CHECK();
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    ORBX_HIP_CHECK(hipMemcpy(scores, h->score.p, (size_t)m * 4, hipMemcpyDeviceToHost));
    ORBX_HIP_CHECK(hipMemcpy(inliers, h->inl.p, (size_t)m * S.N, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

extern "C" int orbx_init_check_rt(orbx_initializer *h, const orbx_init_matches *M, const uint8_t *inliers, const float *r, const float *t, int m, float fx, float fy, float cx, float cy,
                                  float th2, int32_t *good, uint8_t *vb_good, float *p3d, float *cos_parallax, uint8_t *status)
{
    if (!h || !inliers || !r || !t) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = check_matches(M)) != ORBX_OK) return rc;
    if (m < 1 || m > ORBX_INIT_HYPOTHESES) { orbx_set_error("m = %d motions outside 1..%d", m, ORBX_INIT_HYPOTHESES); return ORBX_ERR_ARG; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    Staged S;
    int N = 0;
    for (int i = 0; i < M->n1; i++) N += M->matches12[i] >= 0 ? 1 : 0;
    if (N < 1) { orbx_set_error("no matches"); return ORBX_ERR_ARG; }
    auto [pin, pout] = h->box.plan();
    (void)pout;
    if ((rc = plan_matches(h, M, pin, S)) != ORBX_OK) return rc;
    const auto sInl = pin.add(inliers, (size_t)N);
    const auto sR = pin.add(r, (size_t)m * 9), sT = pin.add(t, (size_t)m * 3);
    const OrbxStaged sg = h->box.begin(h->stream, &rc);
    if (rc != ORBX_OK) return rc;
    fill_matches(M, false, sg, S);
    uint8_t *ar;
    if ((rc = stage_to_arena(h, &ar)) != ORBX_OK) return rc;
    InitRtArgs R;
    R.raw = (const float4 *)S.raw.in(ar); R.hypR = sR.in(ar); R.hypT = sT.in(ar); R.hypValid = nullptr;
    R.inlBase = sInl.in(ar); R.best = nullptr; R.iters = 0; R.N = N;
    R.fx = fx; R.fy = fy; R.cx = cx; R.cy = cy; R.th2 = th2;
    R.status = h->crtStatus.p; R.p3d = h->crtP3d.p; R.cosp = h->crtCos.p;
    hipLaunchKernelGGL(k_init_check_rt, dim3((unsigned)((N + 255) / 256), (unsigned)m), dim3(256), 0, h->stream, R);
    ORBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_init_rank, dim3((unsigned)m, RANK_SPLIT), dim3(RANK_THREADS), (size_t)((N + 3) & ~3) * 4, h->stream, (const uint8_t *)h->crtStatus.p, (const float *)h->crtCos.p, N, h->rankGood.p,
                       h->rankCos.p);
    ORBX_LAUNCH_CHECK();
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    std::vector<uint8_t> st((size_t)m * N);
    std::vector<float> pts((size_t)m * N * 3);
    ORBX_HIP_CHECK(hipMemcpy(st.data(), h->crtStatus.p, st.size(), hipMemcpyDeviceToHost));
    ORBX_HIP_CHECK(hipMemcpy(pts.data(), h->crtP3d.p, pts.size() * 4, hipMemcpyDeviceToHost));
    if (good) ORBX_HIP_CHECK(hipMemcpy(good, h->rankGood.p, (size_t)m * 4, hipMemcpyDeviceToHost));
    if (cos_parallax) ORBX_HIP_CHECK(hipMemcpy(cos_parallax, h->rankCos.p, (size_t)m * 4, hipMemcpyDeviceToHost));
    if (status) memcpy(status, st.data(), st.size());
    const int32_t *slot = sg.host(S.slot);
    const size_t n1 = (size_t)M->n1;
    for (int k = 0; k < m; k++)
        for (size_t i = 0; i < n1; i++) {
            const int j = slot[i];
            const unsigned s = j >= 0 ? st[(size_t)k * N + j] : 0u;
            const bool stored = s == ORBX_INIT_GOOD || s == ORBX_INIT_GOOD_LOW_PARALLAX;
            if (vb_good) vb_good[k * n1 + i] = s == ORBX_INIT_GOOD ? 1 : 0;
            if (p3d)
                for (int c = 0; c < 3; c++) p3d[3 * (k * n1 + i) + c] = stored ? pts[3 * ((size_t)k * N + j) + c] : 0.0f;
        }
    return ORBX_OK;
}

extern "C" int orbx_initializer_last_timing(orbx_initializer *h, float *device_ms, int *launches)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    return h->timer.read(h->device, device_ms, launches, "no orbx_initialize call to report");
}
