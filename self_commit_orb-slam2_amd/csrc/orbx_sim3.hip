// orbx_sim3.hip -- Sim3Solver (src/Sim3Solver.cc): Horn 1987 on RANSAC triples, every iteration of every loop candidate of
// LoopClosing::ComputeSim3 (src/LoopClosing.cc:300-560) in one launch chain with one wait.  gfx950 only.
//
//   k_sim3_prepare  the constructor (:48-140) per kept pair: X3Dc = Rcw * Xw + tcw, FromCameraToImage (:526-545), the two error limits.  It reads
//                   the call's inputs in mapped pinned memory (each byte once) and leaves what the kernels behind read many times - the twelve
//                   floats per pair, the sets, the candidate headers - in device memory: the staging copy and the constructor are one launch.
//   k_sim3_models   ComputeSim3 (:309-448), one LANE per (candidate, iteration): three point pairs, a 4x4 symmetric Jacobi in FP64, atan2 /
//                   Rodrigues in double; everything is indexed by compile-time constants and lives in registers.
//   k_sim3_check    CheckInliers / Project (:451-523), one WAVE per (candidate, iteration): the lanes walk the pairs 64 at a time, the ballot is
//                   the mask word [candidate][iteration][ceil(n / 64)], its population count the count.  The same kernel checks explicit models.
//   k_sim3_decide   one workgroup per candidate: the running best of iterate (:199-285) as a prefix maximum over the counts (count >= best
//                   updates), the return events (an update with count > min_inliers), the first event and its mask, the last update, the result
//                   block in mapped pinned memory, the sequence word.
//
// Latency bound: a few thousand short waves.  The models are not fused into the check (as k_init_models fuses them) because a model is a chain of
// ~400 dependent FP64 operations on ONE lane: fused, every wave would wait for it with 63 idle lanes; apart, 64 models share a wave.
//
// Arithmetic: float where the reference is float, in its operation order; the list is in include/orbx.h above orbx_sim3_solver_create.  The
// library is built with -ffp-contract=off: every product and sum below is its own operation.
// PARITY UNPINNED AT THE OPENCV LEVEL: cv::eigen in float (here: Jacobi in FP64, narrowed), cv::Rodrigues, the accumulation inside cv::gemm and
// Mat / int; the device library's atan2, sin and cos are not pinned either.  RANSAC sets are drawn ahead by the caller, so a caller's rand()
// sequence is consumed in another order than the reference's lazy, interleaved draws: no parity is claimed for them.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "orbx_handle.h"

// Sweeps of the 4x4 Jacobi: ORBX_SIM3_JACOBI_SWEEPS of include/orbx.h, where the choice is recorded
#define SIM3_SWEEPS ORBX_SIM3_JACOBI_SWEEPS

struct Sim3Cand {                // one candidate of a call: in mapped pinned memory (host-filled), copied to the device by k_sim3_prepare
    float rcw1[9], tcw1[3], rcw2[9], tcw2[3];
    float k1[4], k2[4];          // fx, fy, cx, cy
    int32_t n, iters, minInliers, fixScale;
    int32_t mb, ib;              // first pair / first iteration of this candidate in the call's arrays
    int32_t words;               // ceil(n / 64)
    int32_t pad;
    unsigned long long wb;       // first mask word
    unsigned long long outOff;   // the candidate's result block in the mapped result buffer
};
static_assert(sizeof(Sim3Cand) % 8 == 0, "copied in 4-byte words, holds 8-byte members");

struct Sim3Block {               // layout of a candidate's result block (mapped pinned)
    size_t count, r12, t12, s12, isEvent, inliers, total;      // byte offsets behind the 16-byte head {first_event, best_iteration, no_more, 0}
    __host__ __device__ Sim3Block(int n, int iters)
    {
        const size_t it = (size_t)iters;
        count = 16; r12 = count + it * 4; t12 = r12 + it * 36; s12 = t12 + it * 12; isEvent = s12 + it * 4;
        inliers = isEvent + ((it + 3) & ~(size_t)3);
        total = (inliers + (size_t)n + 255) & ~(size_t)255;
    }
};

struct Sim3Dev {                 // device arrays of a call
    float *x3dc1, *x3dc2;        // [pairs][3]
    float2 *p1im1, *p2im2;
    float *maxErr1, *maxErr2;
    int32_t *sets;               // [iterations][3]
    Sim3Cand *cand;
    float *r12, *t12, *s12, *nmat, *quat, *t12m, *t21m;
    int32_t *count;
    unsigned long long *mask;
};

struct Sim3In {                  // the call's inputs, device addresses of mapped pinned memory
    const Sim3Cand *cand;
    const float *world1, *world2, *sigma1, *sigma2;
    const int32_t *sets;
};

__global__ __launch_bounds__(256) void k_sim3_prepare(Sim3In I, Sim3Dev D, int withSets)
{
    const int c = blockIdx.y;
    const Sim3Cand *hc = I.cand + c;
    const int n = hc->n, iters = hc->iters, mb = hc->mb, ib = hc->ib;
    const int stride = gridDim.x * 256, first = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < sizeof(Sim3Cand) / 4) ((uint32_t *)(D.cand + c))[threadIdx.x] = ((const uint32_t *)hc)[threadIdx.x];
    for (int j = first; withSets && j < 3 * iters; j += stride) D.sets[3 * (size_t)ib + j] = I.sets[3 * (size_t)ib + j];
    if (first >= n) return;
    float R1[9], t1[3], R2[9], t2[3], k1[4], k2[4];
#pragma unroll
    for (int j = 0; j < 9; j++) { R1[j] = hc->rcw1[j]; R2[j] = hc->rcw2[j]; }
#pragma unroll
    for (int j = 0; j < 3; j++) { t1[j] = hc->tcw1[j]; t2[j] = hc->tcw2[j]; }
#pragma unroll
    for (int j = 0; j < 4; j++) { k1[j] = hc->k1[j]; k2[j] = hc->k2[j]; }
    for (int i = first; i < n; i += stride) {
        const size_t g = (size_t)mb + i;
        const float w1[3] = {I.world1[3 * g], I.world1[3 * g + 1], I.world1[3 * g + 2]};
        const float w2[3] = {I.world2[3 * g], I.world2[3 * g + 1], I.world2[3 * g + 2]};
        float a[3], b[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            a[r] = ((R1[3 * r] * w1[0] + R1[3 * r + 1] * w1[1]) + R1[3 * r + 2] * w1[2]) + t1[r];
            b[r] = ((R2[3 * r] * w2[0] + R2[3 * r + 1] * w2[1]) + R2[3 * r + 2] * w2[2]) + t2[r];
            D.x3dc1[3 * g + r] = a[r]; D.x3dc2[3 * g + r] = b[r];
        }
        const float iz1 = 1.0f / a[2], iz2 = 1.0f / b[2];
        D.p1im1[g] = make_float2(k1[0] * (a[0] * iz1) + k1[2], k1[1] * (a[1] * iz1) + k1[3]);
        D.p2im2[g] = make_float2(k2[0] * (b[0] * iz2) + k2[2], k2[1] * (b[1] * iz2) + k2[3]);
        // std::vector<size_t>::push_back(9.210 * sigmaSquare): the double product truncated to an unsigned integer, compared as a float
        D.maxErr1[g] = (float)(unsigned long long)(9.210 * (double)I.sigma1[g]);
        D.maxErr2[g] = (float)(unsigned long long)(9.210 * (double)I.sigma2[g]);
    }
}

// Eigenvector of the largest eigenvalue of the symmetric 4x4 float matrix N: cyclic two-sided Jacobi in FP64 - the rotation of (p, q) is applied
// to the columns, then to the rows, of the full matrix, and to the columns of V - then the column of V under the largest diagonal entry, the
// first of equal ones.  tests/sim3_ref.py::jacobi_eig4 restates it operation by operation.
__device__ __forceinline__ void jacobi_eig4(const float (&N)[16], float (&q)[4])
{
    double a[4][4], v[4][4];      // [row][column]
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) { a[r][c] = (double)N[4 * r + c]; v[r][c] = r == c ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < SIM3_SWEEPS; sweep++) {
#pragma unroll
        for (int p = 0; p < 3; p++) {
#pragma unroll
            for (int qq = p + 1; qq < 4; qq++) {
                const double alpha = a[p][p], beta = a[qq][qq], gamma = a[p][qq];
                double c = 1.0, s = 0.0;
                if (gamma != 0.0) {
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = c * t;
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double ap = a[r][p], aq = a[r][qq], vp = v[r][p], vq = v[r][qq];
                    a[r][p] = c * ap - s * aq; a[r][qq] = s * ap + c * aq;
                    v[r][p] = c * vp - s * vq; v[r][qq] = s * vp + c * vq;
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double ap = a[p][r], aq = a[qq][r];
                    a[p][r] = c * ap - s * aq; a[qq][r] = s * ap + c * aq;
                }
            }
        }
    }
    double best = 0.0, e[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const bool take = c == 0 || a[c][c] > best;
        best = take ? a[c][c] : best;
#pragma unroll
        for (int r = 0; r < 4; r++) e[r] = take ? v[r][c] : e[r];
    }
#pragma unroll
    for (int r = 0; r < 4; r++) q[r] = (float)e[r];
}

// ComputeCentroid (:295-305) of the 3x3 P (columns = points): C = reduce(SUM) / cols, Pr = P - C
__device__ __forceinline__ void centroid3(const float (&P)[3][3], float (&Pr)[3][3], float (&C)[3])
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float sum = (P[r][0] + P[r][1]) + P[r][2];
        C[r] = (float)((double)sum / 3.0);
#pragma unroll
        for (int j = 0; j < 3; j++) Pr[r][j] = P[r][j] - C[r];
    }
}

__global__ __launch_bounds__(64) void k_sim3_models(Sim3Dev D)
{
    const Sim3Cand *hc = D.cand + blockIdx.y;
    const int it = blockIdx.x * 64 + threadIdx.x;
    if (it >= hc->iters) return;
    const size_t g = (size_t)hc->ib + it, mb = (size_t)hc->mb;
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const size_t idx = mb + (size_t)D.sets[3 * g + j];
#pragma unroll
        for (int r = 0; r < 3; r++) { P1[r][j] = D.x3dc1[3 * idx + r]; P2[r][j] = D.x3dc2[3 * idx + r]; }
    }
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
    centroid3(P1, Pr1, O1);
    centroid3(P2, Pr2, O2);
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = (Pr2[i][0] * Pr1[j][0] + Pr2[i][1] * Pr1[j][1]) + Pr2[i][2] * Pr1[j][2];
    const float N11 = (M[0][0] + M[1][1]) + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
    const float N22 = (M[0][0] - M[1][1]) - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
    const float N33 = (-M[0][0] + M[1][1]) - M[2][2], N34 = M[1][2] + M[2][1], N44 = (-M[0][0] - M[1][1]) + M[2][2];
    const float N[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float q[4];
    jacobi_eig4(N, q);
#pragma unroll
    for (int j = 0; j < 16; j++) D.nmat[16 * g + j] = N[j];
#pragma unroll
    for (int j = 0; j < 4; j++) D.quat[4 * g + j] = q[j];

    // :372-386
    const double nrm = sqrt(((double)q[1] * (double)q[1] + (double)q[2] * (double)q[2]) + (double)q[3] * (double)q[3]);
    const double ang = atan2(nrm, (double)q[0]);
    const double scale = (2.0 * ang) / nrm;
    const float vec[3] = {(float)(scale * (double)q[1]), (float)(scale * (double)q[2]), (float)(scale * (double)q[3])};
    float R[3][3];
    {
        double rx = (double)vec[0], ry = (double)vec[1], rz = (double)vec[2];
        const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
        if (theta < DBL_EPSILON) {
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) R[i][j] = i == j ? 1.0f : 0.0f;
        } else {
            const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, itheta = 1.0 / theta;
            rx = rx * itheta; ry = ry * itheta; rz = rz * itheta;
            const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
            const double rxm[9] = {0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0};
#pragma unroll
            for (int k = 0; k < 9; k++) R[k / 3][k % 3] = (float)((c * (k % 4 == 0 ? 1.0 : 0.0) + c1 * rrt[k]) + s * rxm[k]);
        }
    }
    // :390-418
    float P3[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) P3[i][j] = (R[i][0] * Pr2[0][j] + R[i][1] * Pr2[1][j]) + R[i][2] * Pr2[2][j];
    float s12 = 1.0f;
    if (!hc->fixScale) {
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) { nom = nom + (double)Pr1[i][j] * (double)P3[i][j]; den = den + (double)(P3[i][j] * P3[i][j]); }
        s12 = (float)(nom / den);
    }
    // :422-447
    float sR[3][3], t[3], sRinv[3][3], tinv[3];
    const double inv = 1.0 / (double)s12;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { sR[i][j] = s12 * R[i][j]; sRinv[i][j] = (float)(inv * (double)R[j][i]); }
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = O1[i] - ((sR[i][0] * O2[0] + sR[i][1] * O2[1]) + sR[i][2] * O2[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) tinv[i] = ((-sRinv[i][0]) * t[0] + (-sRinv[i][1]) * t[1]) + (-sRinv[i][2]) * t[2];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            D.r12[9 * g + 3 * i + j] = R[i][j];
            D.t12m[16 * g + 4 * i + j] = sR[i][j];
            D.t21m[16 * g + 4 * i + j] = sRinv[i][j];
        }
        D.t12[3 * g + i] = t[i];
        D.t12m[16 * g + 4 * i + 3] = t[i];
        D.t21m[16 * g + 4 * i + 3] = tinv[i];
        D.t12m[16 * g + 12 + i] = 0.0f; D.t21m[16 * g + 12 + i] = 0.0f;
    }
    D.t12m[16 * g + 15] = 1.0f; D.t21m[16 * g + 15] = 1.0f;
    D.s12[g] = s12;
}

#define SIM3_CHECK_WAVES 4
// t12m / t21m / count / mask are passed apart from D: orbx_sim3_check_models runs explicit models into buffers of its own
__global__ __launch_bounds__(64 * SIM3_CHECK_WAVES) void k_sim3_check(Sim3Dev D, const float *__restrict__ t12m, const float *__restrict__ t21m, int32_t *__restrict__ count,
                                                                       unsigned long long *__restrict__ mask)
{
    const Sim3Cand *hc = D.cand + blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int it = blockIdx.x * SIM3_CHECK_WAVES + (threadIdx.x >> 6);      // uniform in a wave
    if (it >= hc->iters) return;
    const int n = hc->n;
    const size_t g = (size_t)hc->ib + it, mb = (size_t)hc->mb;
    float A[12], B[12];      // the upper three rows of T12 / T21
#pragma unroll
    for (int j = 0; j < 12; j++) { A[j] = t12m[16 * g + j]; B[j] = t21m[16 * g + j]; }
    const float fx1 = hc->k1[0], fy1 = hc->k1[1], cx1 = hc->k1[2], cy1 = hc->k1[3];
    const float fx2 = hc->k2[0], fy2 = hc->k2[1], cx2 = hc->k2[2], cy2 = hc->k2[3];
    unsigned long long *row = mask + hc->wb + (size_t)it * hc->words;
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool inl = false;
        if (i < n) {
            const size_t k = mb + i;
            const float x1 = D.x3dc1[3 * k], y1 = D.x3dc1[3 * k + 1], z1 = D.x3dc1[3 * k + 2];
            const float x2 = D.x3dc2[3 * k], y2 = D.x3dc2[3 * k + 1], z2 = D.x3dc2[3 * k + 2];
            // Project(mvX3Dc2, vP2im1, mT12i, mK1)
            const float ax = ((A[0] * x2 + A[1] * y2) + A[2] * z2) + A[3], ay = ((A[4] * x2 + A[5] * y2) + A[6] * z2) + A[7];
            const float az = ((A[8] * x2 + A[9] * y2) + A[10] * z2) + A[11];
            const float ia = 1.0f / az;
            const float u21 = fx1 * (ax * ia) + cx1, v21 = fy1 * (ay * ia) + cy1;
            // Project(mvX3Dc1, vP1im2, mT21i, mK2)
            const float bx = ((B[0] * x1 + B[1] * y1) + B[2] * z1) + B[3], by = ((B[4] * x1 + B[5] * y1) + B[6] * z1) + B[7];
            const float bz = ((B[8] * x1 + B[9] * y1) + B[10] * z1) + B[11];
            const float ib = 1.0f / bz;
            const float u12 = fx2 * (bx * ib) + cx2, v12 = fy2 * (by * ib) + cy2;
            const float2 p1 = D.p1im1[k], p2 = D.p2im2[k];
            const float d1x = p1.x - u21, d1y = p1.y - v21, d2x = u12 - p2.x, d2y = v12 - p2.y;
            const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
            const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
            inl = err1 < D.maxErr1[k] && err2 < D.maxErr2[k];
        }
        const unsigned long long m = __ballot(inl);
        if (lane == 0) row[base >> 6] = m;
        cnt += __popcll(m);
    }
    if (lane == 0) count[g] = cnt;
}

#define SIM3_DECIDE_THREADS 256
__global__ __launch_bounds__(SIM3_DECIDE_THREADS) void k_sim3_decide(Sim3Dev D, uint8_t *__restrict__ out, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    __shared__ int32_t sFirst, sLast;
    const Sim3Cand *hc = D.cand + blockIdx.x;
    const int n = hc->n, iters = hc->iters, minInl = hc->minInliers, tid = threadIdx.x;
    const size_t ib = (size_t)hc->ib;
    const Sim3Block L(n, iters);
    uint8_t *blk = out + hc->outOff;
    if (tid < 64) {
        int carry = 0, first = -1, last = -1;      // mnBestInliers starts at 0
        for (int base = 0; base < iters; base += 64) {
            const int it = base + tid;
            const int v = it < iters ? D.count[ib + it] : -1;
            int incl = v;      // (inclusive maximum scan, written out here and in k_pnp_records: as a shared helper both kernels come out with other instructions)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl, d);
                if (tid >= d) incl = max(incl, o);
            }
            int excl = __shfl_up(incl, 1);
            excl = tid == 0 ? carry : max(excl, carry);
            const bool upd = it < iters && v >= excl;
            const bool ev = upd && v > minInl;
            if (it < iters) blk[L.isEvent + it] = ev ? 1 : 0;
            const unsigned long long bu = __ballot(upd), be = __ballot(ev);
            if (first < 0 && be) first = base + __ffsll((long long)be) - 1;
            if (bu) last = base + 63 - __clzll((long long)bu);
            carry = max(carry, __shfl(incl, 63));
        }
        if (tid == 0) { sFirst = first; sLast = last; }
    }
    __syncthreads();
    const int first = sFirst;
    if (tid == 0) {
        int32_t *head = (int32_t *)blk;
        head[0] = first; head[1] = sLast; head[2] = (n < minInl || first < 0) ? 1 : 0; head[3] = 0;
    }
    int32_t *oc = (int32_t *)(blk + L.count);
    float *orr = (float *)(blk + L.r12), *ot = (float *)(blk + L.t12), *os = (float *)(blk + L.s12);
    for (int j = tid; j < iters; j += SIM3_DECIDE_THREADS) { oc[j] = D.count[ib + j]; os[j] = D.s12[ib + j]; }
    for (int j = tid; j < 9 * iters; j += SIM3_DECIDE_THREADS) orr[j] = D.r12[9 * ib + j];
    for (int j = tid; j < 3 * iters; j += SIM3_DECIDE_THREADS) ot[j] = D.t12[3 * ib + j];
    const unsigned long long *row = D.mask + hc->wb + (size_t)(first < 0 ? 0 : first) * hc->words;
    for (int i = tid; i < n; i += SIM3_DECIDE_THREADS) blk[L.inliers + i] = first < 0 ? 0 : (uint8_t)((row[i >> 6] >> (i & 63)) & 1ull);
    orbx_publish(counter, flag, seq, gridDim.x);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------------
struct orbx_sim3_solver : OrbxHandle {
    int maxCands = 0, maxMatches = 0, maxIters = 0;
    OrbxCallTimer timer;
    bool solved = false;
    OrbxCallBox box;
    OrbxOwnedBuf<float> pairs, models;      // 12 floats per pair; 56 floats per iteration
    OrbxOwnedBuf<int32_t> sets, count, cmCount;
    OrbxOwnedBuf<Sim3Cand> cand;
    OrbxOwnedBuf<unsigned long long> mask, cmMask;
    std::vector<Sim3Cand> last;           // the candidates of the last solve (orbx_sim3_inliers)
};

namespace {
Sim3Dev dev_view(orbx_sim3_solver *h)
{
    const size_t P = (size_t)h->maxCands * h->maxMatches, I = (size_t)h->maxCands * h->maxIters;
    Sim3Dev D;
    float *p = h->pairs.p;
    D.x3dc1 = p; D.x3dc2 = p + 3 * P; D.p1im1 = (float2 *)(p + 6 * P); D.p2im2 = (float2 *)(p + 8 * P); D.maxErr1 = p + 10 * P; D.maxErr2 = p + 11 * P;
    float *m = h->models.p;
    D.nmat = m; D.t12m = m + 16 * I; D.t21m = m + 32 * I; D.r12 = m + 48 * I; D.quat = m + 57 * I; D.t12 = m + 61 * I; D.s12 = m + 64 * I;
    D.sets = h->sets.p; D.cand = h->cand.p; D.count = h->count.p; D.mask = h->mask.p;
    return D;
}

struct Sim3Staged { OrbxStaged sg; OrbxSlot<float, ORBX_STAGE_IN> extraA, extraB; OrbxSlot<uint8_t, ORBX_STAGE_OUT> res; };      // res: the candidates' Sim3Blocks

int check_problem(const orbx_sim3_solver *h, const orbx_sim3_problem *P, int c, bool withSets, int &iters)
{
    if (P->n < 0 || P->iterations < 0 || (P->n > 0 && (!P->world1 || !P->world2 || !P->sigma2_1 || !P->sigma2_2))) {
        orbx_set_error("candidate %d: n = %d, iterations = %d or a NULL array", c, P->n, P->iterations);
        return ORBX_ERR_ARG;
    }
    if (P->n > h->maxMatches) { orbx_set_error("candidate %d: %d matches, the solver was created for %d", c, P->n, h->maxMatches); return ORBX_ERR_CAPACITY; }
    iters = 0;
    if (!withSets) return ORBX_OK;
    iters = P->n < P->min_inliers ? 0 : P->iterations;      // :206-210
    if (iters > h->maxIters) { orbx_set_error("candidate %d: %d iterations, the solver was created for %d", c, iters, h->maxIters); return ORBX_ERR_CAPACITY; }
    if (iters > 0 && (P->n < 3 || !P->sets)) { orbx_set_error("candidate %d: %d matches, a set needs 3 (or NULL sets)", c, P->n); return ORBX_ERR_ARG; }
    for (int i = 0; i < iters; i++) {
        const int32_t *s = P->sets + 3 * (size_t)i;
        for (int j = 0; j < 3; j++)
            if (s[j] < 0 || s[j] >= P->n) { orbx_set_error("candidate %d: sets[%d][%d] = %d is outside the %d matches", c, i, j, s[j], P->n); return ORBX_ERR_ARG; }
        if (s[0] == s[1] || s[0] == s[2] || s[1] == s[2]) { orbx_set_error("candidate %d: sets[%d] repeats an index", c, i); return ORBX_ERR_ARG; }
    }
    return ORBX_OK;
}

// headers + arrays of `nc` candidates into the mapped input buffer; iters[c] = iterations to run (sets are staged when withSets); extraA / extraB floats of
// room for the caller behind them; outBytes of results, 0 = the candidates' Sim3Blocks
Sim3Staged stage(orbx_sim3_solver *h, const orbx_sim3_problem *Ps, int nc, const std::vector<int> &iters, bool withSets, size_t extraA, size_t extraB, size_t outBytes,
                 std::vector<Sim3Cand> &cands, Sim3In &I, int *rc)
{
    size_t totN = 0, totIt = 0, totW = 0, off = 0;
    cands.assign((size_t)nc, Sim3Cand());
    for (int c = 0; c < nc; c++) {
        const orbx_sim3_problem &P = Ps[c];
        Sim3Cand &H = cands[c];
        memcpy(H.rcw1, P.rcw1, 36); memcpy(H.tcw1, P.tcw1, 12); memcpy(H.rcw2, P.rcw2, 36); memcpy(H.tcw2, P.tcw2, 12);
        H.k1[0] = P.fx1; H.k1[1] = P.fy1; H.k1[2] = P.cx1; H.k1[3] = P.cy1; H.k2[0] = P.fx2; H.k2[1] = P.fy2; H.k2[2] = P.cx2; H.k2[3] = P.cy2;
        H.n = P.n; H.iters = iters[c]; H.minInliers = P.min_inliers; H.fixScale = P.fix_scale ? 1 : 0;
        H.mb = (int32_t)totN; H.ib = (int32_t)totIt; H.words = (P.n + 63) / 64; H.pad = 0; H.wb = totW; H.outOff = off;
        totN += (size_t)P.n; totIt += (size_t)iters[c]; totW += (size_t)H.words * (size_t)iters[c];
        off += Sim3Block(P.n, iters[c]).total;
    }
    OrbxCallBox &bx = h->box;
    auto [pin, pout] = bx.plan();
    // the candidates' arrays lie concatenated, candidate c's at element mb (matches) / ib (sets) of its region: holes, filled below
    const auto sCand = pin.add(cands.data(), (size_t)nc);
    const auto sW1 = pin.hole<float>(totN * 3), sW2 = pin.hole<float>(totN * 3), sS1 = pin.hole<float>(totN), sS2 = pin.hole<float>(totN);
    const auto sSets = pin.hole<int32_t>(withSets ? totIt * 3 : 0);
    const auto sA = pin.hole<float>(extraA), sB = pin.hole<float>(extraB);
    const auto rRes = pout.hole<uint8_t>(outBytes ? outBytes : off);
    const Sim3Staged S = {bx.begin(h->stream, rc), sA, sB, rRes};
    if (*rc != ORBX_OK) return S;
    for (int c = 0; c < nc; c++) {
        const orbx_sim3_problem &P = Ps[c];
        const Sim3Cand &H = cands[c];
        const size_t n = (size_t)P.n, mb = (size_t)H.mb;
        orbx_put_at(S.sg, sW1, 3 * mb, P.world1, 3 * n); orbx_put_at(S.sg, sW2, 3 * mb, P.world2, 3 * n);
        orbx_put_at(S.sg, sS1, mb, P.sigma2_1, n); orbx_put_at(S.sg, sS2, mb, P.sigma2_2, n);
        if (withSets) orbx_put_at(S.sg, sSets, 3 * (size_t)H.ib, P.sets, 3 * (size_t)H.iters);
    }
    I.cand = S.sg.dev(sCand);
    I.world1 = S.sg.dev(sW1); I.world2 = S.sg.dev(sW2);
    I.sigma1 = S.sg.dev(sS1); I.sigma2 = S.sg.dev(sS2);
    I.sets = S.sg.dev(sSets);
    return S;
}

unsigned prepare_blocks(int maxN, int maxIt) { return (unsigned)std::max(1, (std::max(maxN, 3 * maxIt) + 255) / 256); }

}  // namespace

extern "C" int orbx_sim3_ransac_iterations(double probability, int min_inliers, int max_iterations, int n)
{
    // :156-192; N is an int there: (float)minInliers / N is a float quotient, pow / log promote it to double
    int nIterations;
    if (min_inliers == n) nIterations = 1;
    else {
        const float epsilon = (float)min_inliers / n;
        const double x = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
        // the reference converts x to int unchecked; out of range or NaN (n < min_inliers) is what the x86 conversion makes of it
        nIterations = (x >= -2147483648.0 && x <= 2147483647.0) ? (int)x : INT_MIN;
    }
    return std::max(1, std::min(nIterations, max_iterations));
}

extern "C" int orbx_sim3_solver_create(int device, int max_candidates, int max_matches, int max_iterations, orbx_sim3_solver **out)
{
    if (!out || max_candidates < 1 || max_candidates > 4096 || max_matches < 3 || max_matches > ORBX_SIM3_MAX_MATCHES || max_iterations < 1 || max_iterations > (1 << 16)) {
        orbx_set_error("bad Sim3 solver arguments (max_candidates >= 1, 3 <= max_matches <= %d, max_iterations >= 1)", ORBX_SIM3_MAX_MATCHES);
        return ORBX_ERR_ARG;
    }
    *out = nullptr;
    orbx_sim3_solver *h = new orbx_sim3_solver();
    h->maxCands = max_candidates; h->maxMatches = max_matches; h->maxIters = max_iterations;
    const size_t P = (size_t)max_candidates * max_matches, I = (size_t)max_candidates * max_iterations, W = (size_t)(max_matches + 63) / 64;
    int rc;
    if ((rc = h->open(device)) || (rc = h->timer.create()) || (rc = h->pairs.ensure(12 * P)) || (rc = h->models.ensure(65 * I)) || (rc = h->sets.ensure(3 * I)) || (rc = h->count.ensure(I)) || (rc = h->cmCount.ensure((size_t)max_iterations)) ||
        (rc = h->cand.ensure((size_t)max_candidates)) || (rc = h->mask.ensure(I * W)) || (rc = h->cmMask.ensure((size_t)max_iterations * W))) {
        orbx_sim3_solver_destroy(h);
        return rc;
    }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_sim3_solver_destroy(orbx_sim3_solver *h) { orbx_destroy_handle(h); }

extern "C" int orbx_sim3_solve(orbx_sim3_solver *h, const orbx_sim3_problem *Ps, int nc, const orbx_sim3_result *Rs)
{
    if (!h || !Ps || !Rs || nc < 1) { orbx_set_error("NULL argument or ncandidates = %d < 1", nc); return ORBX_ERR_ARG; }
    if (nc > h->maxCands) { orbx_set_error("%d candidates, the solver was created for %d", nc, h->maxCands); return ORBX_ERR_CAPACITY; }
    int rc, maxN = 0, maxIt = 0;
    std::vector<int> iters((size_t)nc, 0);
    for (int c = 0; c < nc; c++) {
        if ((rc = check_problem(h, Ps + c, c, true, iters[c])) != ORBX_OK) return rc;
        maxN = std::max(maxN, Ps[c].n); maxIt = std::max(maxIt, iters[c]);
    }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    std::vector<Sim3Cand> cands;
    Sim3In I;
    const Sim3Staged S = stage(h, Ps, nc, iters, true, 0, 0, 0, cands, I, &rc);
    if (rc != ORBX_OK) return rc;
    OrbxCallBox &bx = h->box;
    const Sim3Dev D = dev_view(h);
    h->solved = false;

    const unsigned long long seq = bx.arm();
    if ((rc = h->timer.begin(h->stream)) != ORBX_OK) return rc;
    hipLaunchKernelGGL(k_sim3_prepare, dim3(prepare_blocks(maxN, maxIt), (unsigned)nc), dim3(256), 0, h->stream, I, D, 1);
    ORBX_LAUNCH_COUNT(h->timer);
    if (maxIt > 0) {
        hipLaunchKernelGGL(k_sim3_models, dim3((unsigned)((maxIt + 63) / 64), (unsigned)nc), dim3(64), 0, h->stream, D);
        ORBX_LAUNCH_COUNT(h->timer);
        hipLaunchKernelGGL(k_sim3_check, dim3((unsigned)((maxIt + SIM3_CHECK_WAVES - 1) / SIM3_CHECK_WAVES), (unsigned)nc), dim3(64 * SIM3_CHECK_WAVES), 0, h->stream, D, (const float *)D.t12m,
                           (const float *)D.t21m, D.count, D.mask);
        ORBX_LAUNCH_COUNT(h->timer);
    }
    hipLaunchKernelGGL(k_sim3_decide, dim3((unsigned)nc), dim3(SIM3_DECIDE_THREADS), 0, h->stream, D, S.sg.dev(S.res), bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_COUNT(h->timer);
    if ((rc = h->timer.end(h->stream)) != ORBX_OK) return rc;
    if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;      // the one synchronisation
    h->last = cands; h->solved = true;

    bool diag = false;
    for (int c = 0; c < nc; c++) {
        const orbx_sim3_result &R = Rs[c];
        const Sim3Cand &H = cands[c];
        const size_t it = (size_t)H.iters, n = (size_t)H.n;
        const Sim3Block B(H.n, H.iters);
        const uint8_t *blk = S.sg.host(S.res) + H.outOff;
        const int32_t *head = (const int32_t *)blk;
        if (R.first_event) *R.first_event = head[0];
        if (R.best_iteration) *R.best_iteration = head[1];
        if (R.no_more) *R.no_more = head[2];
        if (R.count && it) memcpy(R.count, blk + B.count, it * 4);
        if (R.r12 && it) memcpy(R.r12, blk + B.r12, it * 36);
        if (R.t12 && it) memcpy(R.t12, blk + B.t12, it * 12);
        if (R.s12 && it) memcpy(R.s12, blk + B.s12, it * 4);
        if (R.is_event && it) memcpy(R.is_event, blk + B.isEvent, it);
        if (R.inliers_first && n) memcpy(R.inliers_first, blk + B.inliers, n);
        diag = diag || R.x3dc1 || R.x3dc2 || R.p1im1 || R.p2im2 || R.max_err1 || R.max_err2 || R.nmat || R.quat || R.t12m || R.t21m;
    }
    if (diag) {
        // the per-pair and per-iteration arrays (tests, diagnostics): copies of their own
        ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
        for (int c = 0; c < nc; c++) {
            const orbx_sim3_result &R = Rs[c];
            const Sim3Cand &H = cands[c];
            const size_t it = (size_t)H.iters, n = (size_t)H.n, mb = (size_t)H.mb, ib = (size_t)H.ib;
#define SIM3_DL(dst, src, first, count) if ((dst) && (count)) ORBX_HIP_CHECK(hipMemcpy((dst), (src) + (first), (count) * sizeof(*(src)), hipMemcpyDeviceToHost))
            SIM3_DL(R.x3dc1, D.x3dc1, 3 * mb, 3 * n); SIM3_DL(R.x3dc2, D.x3dc2, 3 * mb, 3 * n);
            SIM3_DL(R.p1im1, (float *)D.p1im1, 2 * mb, 2 * n); SIM3_DL(R.p2im2, (float *)D.p2im2, 2 * mb, 2 * n);
            SIM3_DL(R.max_err1, D.maxErr1, mb, n); SIM3_DL(R.max_err2, D.maxErr2, mb, n);
            SIM3_DL(R.nmat, D.nmat, 16 * ib, 16 * it); SIM3_DL(R.quat, D.quat, 4 * ib, 4 * it);
            SIM3_DL(R.t12m, D.t12m, 16 * ib, 16 * it); SIM3_DL(R.t21m, D.t21m, 16 * ib, 16 * it);
#undef SIM3_DL
        }
    }
    return ORBX_OK;
}

extern "C" int orbx_sim3_inliers(orbx_sim3_solver *h, int candidate, int iteration, uint8_t *inliers)
{
    if (!h || !inliers) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (!h->solved) { orbx_set_error("no orbx_sim3_solve call to read from"); return ORBX_ERR_STATE; }
    if (candidate < 0 || candidate >= (int)h->last.size() || iteration < 0 || iteration >= h->last[candidate].iters) {
        orbx_set_error("candidate %d / iteration %d outside the last solve", candidate, iteration);
        return ORBX_ERR_ARG;
    }
    const Sim3Cand &H = h->last[candidate];
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    std::vector<unsigned long long> row((size_t)H.words);
    if (H.words) ORBX_HIP_CHECK(hipMemcpy(row.data(), h->mask.p + H.wb + (size_t)iteration * H.words, (size_t)H.words * 8, hipMemcpyDeviceToHost));
    expand_mask(row.data(), H.n, inliers);
    return ORBX_OK;
}

int orbx_sim3_device_rows_internal(orbx_sim3_solver *h, int candidate, int device, OrbxSim3Rows *out)
{
    if (!h || !out) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (!h->solved) { orbx_set_error("the Sim3 solver has no orbx_sim3_solve call to read from"); return ORBX_ERR_ARG; }
    if (h->device != device) { orbx_set_error("the Sim3 solver lives on device %d, the caller on device %d", h->device, device); return ORBX_ERR_ARG; }
    if (candidate < 0 || candidate >= (int)h->last.size()) { orbx_set_error("candidate %d outside the last solve (%d candidates)", candidate, (int)h->last.size()); return ORBX_ERR_ARG; }
    const Sim3Cand &H = h->last[(size_t)candidate];
    const Sim3Dev D = dev_view(h);
    out->r12 = D.r12 + 9 * (size_t)H.ib; out->t12 = D.t12 + 3 * (size_t)H.ib; out->s12 = D.s12 + H.ib; out->mask = D.mask + H.wb;
    out->n = H.n; out->words = H.words; out->iters = H.iters;
    return ORBX_OK;
}

extern "C" int orbx_sim3_check_models(orbx_sim3_solver *h, const orbx_sim3_problem *P, const float *t12, const float *t21, int m, int32_t *count, uint8_t *inliers)
{
    if (!h || !P || !t12 || !t21 || !count) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (m < 1) { orbx_set_error("m = %d models", m); return ORBX_ERR_ARG; }
    if (m > h->maxIters) { orbx_set_error("%d models, the solver holds %d", m, h->maxIters); return ORBX_ERR_CAPACITY; }
    int rc, unused = 0;
    if ((rc = check_problem(h, P, 0, false, unused)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    std::vector<Sim3Cand> cands;
    Sim3In I;
    const std::vector<int> iters(1, m);
    const Sim3Staged S = stage(h, P, 1, iters, false, (size_t)m * 16, (size_t)m * 16, 256, cands, I, &rc);
    if (rc != ORBX_OK) return rc;
    orbx_put_at(S.sg, S.extraA, 0, t12, (size_t)m * 16); orbx_put_at(S.sg, S.extraB, 0, t21, (size_t)m * 16);
    // the last solve's pairs on the device are overwritten, its masks are not: orbx_sim3_inliers keeps working
    const Sim3Dev D = dev_view(h);
    hipLaunchKernelGGL(k_sim3_prepare, dim3(prepare_blocks(P->n, 0), 1), dim3(256), 0, h->stream, I, D, 0);
    ORBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sim3_check, dim3((unsigned)((m + SIM3_CHECK_WAVES - 1) / SIM3_CHECK_WAVES), 1), dim3(64 * SIM3_CHECK_WAVES), 0, h->stream, D, (const float *)S.sg.dev(S.extraA),
                       (const float *)S.sg.dev(S.extraB), h->cmCount.p, h->cmMask.p);
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

extern "C" int orbx_sim3_last_timing(orbx_sim3_solver *h, float *device_ms, int *launches)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    return h->timer.read(h->device, device_ms, launches, "no orbx_sim3_solve call to report");
}
