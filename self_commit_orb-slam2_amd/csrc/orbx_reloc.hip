// orbx_reloc.hip -- the refine loop of Tracking::Relocalization (src/Tracking.cc:2135-2223) for ALL hypotheses of ALL candidates as ONE launch chain with
// ONE host wait (include/orbx.h: orbx_relocalize_refine), and its projection stage on explicit inputs (orbx_reloc_project).  At the end of the file the
// HEAD of the function (:2063-2095, orbx_reloc_match_candidates): SearchByBoW against all candidates through orbx_match::enqueue_bow_candidates and
//   k_reloc_pnp_gather  :2075 and src/PnPsolver.cc:136-158  the < 15 decision and the arrays the PnPsolver constructor collects, every result + the
//                       sequence word
//
// The numeric steps had kernels: Optimizer::PoseOptimization (k_pose_opt in orbx_lba.hip, here as a batch of H frames through
// orbx_pose_opt_enqueue_batch) and the greedy part of SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (k_area_topk / k_area_greedy in
// orbx_match_proj.hip, here through orbx_match::enqueue_area_greedy).  This file adds what the reference does around them on the host:
//   k_reloc_from_pnp  (hypotheses named as records of a PnP solve) pose and inlier mask of each record, read where orbx_pnp_solve left them on the device
//   k_reloc_seed      :2137-2152  mvpMapPoints and sFound from the inlier mask, + the pose problem of pose 1
//   k_reloc_decide    :2159-2169 / :2188-2194 / :2207-2209  what follows a PoseOptimization: mvbOutlier, the dropped outliers, the exit taken, sFound rebuilt
//   k_reloc_project   src/ORBmatcher.cc:1735-1790  Ow, the projection, the image bounds, dist3D, PredictScale, the radius and the level window per slot
//   k_reloc_apply     :1819-1860  the matches into mvpMapPoints, the rotation histogram, ComputeThreeMaxima, the un-assignment; the exit taken;
//                     the pose problem of the next pose
//   k_reloc_finish    the walk over `sequence`, the winner, every result + the sequence word
// Every stage is enqueued unconditionally; a hypothesis that has taken its exit carries a non-zero status word and its workgroups leave at once.
// One workgroup per hypothesis (a frame has a few thousand features, the chain is bound by latency): compaction order from a ballot rank (orbx_wave.h),
// no atomics on global memory.
#include "orbx_match_internal.h"
#include <algorithm>
#include <vector>

namespace {

#define RL_THREADS 1024
// per-hypothesis integer results (device, then mapped host memory)
#define RI_NGOOD 0      /* [3] */
#define RI_NADD 3       /* [2] */
#define RI_NCORR 5      /* [3] */
#define RI_STAGE 8
#define RI_SUCCESS 9
#define RI_WORDS 16

struct RelocCam { float fx, fy, cx, cy, minX, maxX, minY, maxY; int nlevels; float ratioTh[ORBX_MAX_LEVELS], scale[ORBX_MAX_LEVELS]; };

struct RelocDev {
    int H, N, P, cap, nlevels, checkOri;
    // the frame
    const orbx_keypoint *kp; const float *uRight, *invS2;
    // the candidates, slot s of candidate c at hypBase[h] + s
    const uint8_t *valid; const float *pos, *maxD, *minD, *kfAngle; const int32_t *bow;      // bow: [C * N]
    // the hypotheses
    const int32_t *hypCand, *hypBase, *hypNp; const float *hypTcw; const uint8_t *hypMask;
    // state
    int32_t *mvp, *featSlot, *status, *count, *gate, *ret, *ints, *asg;
    float *Xw, *obs, *is2, *poseCur, *poseOut, *qu, *qv, *qr;
    int32_t *qLo, *qHi;
    uint8_t *outlEdge, *outl, *found, *blocked, *active;
    double *stats, *statsAll;
};

// the features that hold a point, compacted in ascending feature order into hypothesis h's pose problem (the form of k_track_gather_last); the count
// k_pose_opt reads and the word that gates it
__device__ __forceinline__ void reloc_gather(const RelocDev &D, int h, bool running, int poseIdx, int *sh)
{
    const int tid = threadIdx.x, N = D.N;
    const size_t cb = (size_t)D.hypBase[h], eb = (size_t)h * D.cap;
    int base = 0;
    for (int i0 = 0; i0 < N; i0 += RL_THREADS) {
        const int i = i0 + tid;
        const int mi = i < N ? D.mvp[(size_t)h * N + i] : -1;
        const bool has = mi >= 0;
        const int slot = block_ballot_rank<RL_THREADS>(has, &base, sh);
        if (i < N) D.featSlot[(size_t)h * N + i] = has ? slot : -1;
        if (has && slot < D.cap) {
            const orbx_keypoint k = D.kp[i];
            const float *X = D.pos + 3 * (cb + mi);
            float *xw = D.Xw + 3 * (eb + slot), *ob = D.obs + 3 * (eb + slot);
            xw[0] = X[0]; xw[1] = X[1]; xw[2] = X[2];
            ob[0] = k.x; ob[1] = k.y; ob[2] = D.uRight[i];
            D.is2[eb + slot] = D.invS2[min(max(k.octave, 0), D.nlevels - 1)];
        }
    }
    if (tid == 0) {
        D.count[h] = base;
        D.gate[h] = running ? base : -1;
        if (running) D.ints[h * RI_WORDS + RI_NCORR + poseIdx] = base;
    }
}

// form (b) of the hypotheses: pose and mask of record rows[h] of a PnP solve, read where that chain left them, into the arrays form (a) stages
struct PnpHypRow { const double *R, *T; const unsigned long long *mask; };      // one record: 9 doubles, 3 doubles, its mask row
__global__ __launch_bounds__(RL_THREADS) void k_reloc_from_pnp(const PnpHypRow *__restrict__ rows, const int32_t *__restrict__ hypCand, const int32_t *__restrict__ matchOf /* [C * N] */,
                                                               int N, float *__restrict__ tcw, uint8_t *__restrict__ mask)
{
    const int h = blockIdx.x, tid = threadIdx.x;
    const PnpHypRow r = rows[h];
    if (tid < 16) {      // src/PnPsolver.cc:407-413: Rcw | tcw narrowed to float
        const int row = tid >> 2, col = tid & 3;
        tcw[h * 16 + tid] = row == 3 ? (col == 3 ? 1.f : 0.f) : (float)(col < 3 ? r.R[3 * row + col] : r.T[row]);
    }
    const int32_t *mo = matchOf + (size_t)hypCand[h] * N;
    for (int j = tid; j < N; j += RL_THREADS) {
        const int i = mo[j];      // the compacted match that sits on feature j, or -1
        mask[(size_t)h * N + j] = i >= 0 ? (uint8_t)((r.mask[i >> 6] >> (i & 63)) & 1ull) : 0;
    }
}

// :2137-2152 and the problem of pose 1
__global__ __launch_bounds__(RL_THREADS) void k_reloc_seed(RelocDev D)
{
    __shared__ int sh[RL_THREADS / 64];
    const int h = blockIdx.x, tid = threadIdx.x, N = D.N, c = D.hypCand[h], np = D.hypNp[h];
    for (int s = tid; s < D.P; s += RL_THREADS) D.found[(size_t)h * D.P + s] = 0;
    if (tid < 16) D.poseCur[h * 16 + tid] = D.hypTcw[h * 16 + tid];
    if (tid < RI_WORDS) D.ints[h * RI_WORDS + tid] = 0;
    if (tid < 24) D.statsAll[h * 24 + tid] = 0.0;
    if (tid == 0) D.status[h] = 0;
    __syncthreads();
    for (int j = tid; j < N; j += RL_THREADS) {
        const int b = D.hypMask[(size_t)h * N + j] ? D.bow[(size_t)c * N + j] : -1;
        D.mvp[(size_t)h * N + j] = b;
        D.outl[(size_t)h * N + j] = 0;
        if (b >= 0 && b < np) D.found[(size_t)h * D.P + b] = 1;      // sFound.insert
    }
    __syncthreads();
    reloc_gather(D, h, true, 0, sh);
}

// behind pose `p` (0, 1, 2): nGood, mvbOutlier, the outliers that leave, the exit
__global__ __launch_bounds__(RL_THREADS) void k_reloc_decide(RelocDev D, int p)
{
    const int h = blockIdx.x, tid = threadIdx.x, N = D.N;
    if (D.status[h] != 0) return;
    const int nGood = D.ret[h];
    int *I = D.ints + h * RI_WORDS;
    // exits: 0 nGood1 < 10 | 1 nGood1 >= 50 | 3 nGood2 >= 50 | 4 nGood2 <= 30 | 6 nGood3 >= 50 | 7 nGood3 < 50   (2 and 5: k_reloc_apply)
    int exitCode = -1;
    bool drop;
    if (p == 0) { drop = nGood >= 10; exitCode = nGood < 10 ? 0 : nGood >= 50 ? 1 : -1; }                         // :2159, :2162-2164, :2169
    else if (p == 1) { drop = false; exitCode = nGood >= 50 ? 3 : nGood <= 30 ? 4 : -1; }                         // :2188 (the outliers stay)
    else { drop = true; exitCode = nGood >= 50 ? 6 : 7; }                                                         // :2207-2209
    const bool goOn = exitCode < 0;
    if (goOn && p == 1)
        for (int s = tid; s < D.P; s += RL_THREADS) D.found[(size_t)h * D.P + s] = 0;                             // sFound.clear(), :2191
    __syncthreads();
    for (int j = tid; j < N; j += RL_THREADS) {
        const size_t g = (size_t)h * N + j;
        const int sl = D.featSlot[g];
        int mi = D.mvp[g];
        if (sl >= 0 && sl < D.cap) {
            const uint8_t o = D.outlEdge[(size_t)h * D.cap + sl];
            D.outl[g] = o;                                                                                         // pFrame->mvbOutlier[idx]
            if (drop && o) { mi = -1; D.mvp[g] = -1; }
        }
        if (goOn) {
            D.blocked[g] = mi >= 0 ? 1 : 0;                                                                       // CurrentFrame.mvpMapPoints[i2], src/ORBmatcher.cc:1804
            if (p == 1 && mi >= 0) D.found[(size_t)h * D.P + mi] = 1;                                             // :2192-2194
        }
    }
    if (tid < 16) D.poseCur[h * 16 + tid] = D.poseOut[h * 16 + tid];
    if (tid < 8) D.statsAll[h * 24 + p * 8 + tid] = D.stats[h * 8 + tid];
    __syncthreads();      // (every thread has read the status word)
    if (tid == 0) {
        I[RI_NGOOD + p] = nGood;
        if (!goOn) { I[RI_STAGE] = exitCode; I[RI_SUCCESS] = (exitCode == 1 || exitCode == 3 || exitCode == 6) ? 1 : 0; D.status[h] = 1 + exitCode; }
    }
}

// src/ORBmatcher.cc:1757-1790 for one slot from its values.  false: the point does not reach the search.  Arithmetic in the reference's order: 3x3 * 3x1
// products in float left to right, cv::norm in double (as frustum_eval in orbx_match_proj.hip); no depth test (the reference has none here).
__device__ __forceinline__ bool reloc_project_eval(const RelocCam &K, const float *T, const float P[3], float maxD, float minD, float th, float &u, float &v, float &radius,
                                                   int &level)
{
    float Pc[3], Ow[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        float s = T[r * 4 + 0] * P[0];
        s = s + T[r * 4 + 1] * P[1];
        s = s + T[r * 4 + 2] * P[2];
        Pc[r] = s + T[r * 4 + 3];                                                // Rcw*x3Dw+tcw, :1758
        float o = (-T[0 * 4 + r]) * T[0 * 4 + 3];                                // Ow = -Rcw.t()*tcw, :1737
        o = o + (-T[1 * 4 + r]) * T[1 * 4 + 3];
        o = o + (-T[2 * 4 + r]) * T[2 * 4 + 3];
        Ow[r] = o;
    }
    const float invz = 1.0f / Pc[2];                                             // :1762 (a double quotient rounded to float: the float quotient)
    u = K.fx * Pc[0] * invz + K.cx; v = K.fy * Pc[1] * invz + K.cy;
    if (!(u >= K.minX && u <= K.maxX)) return false;                             // :1767-1770 (a NaN, z = 0 with x = 0, leaves here: its cell window would be undefined)
    if (!(v >= K.minY && v <= K.maxY)) return false;
    const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
    const float dist = (float)sqrt((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1] + (double)PO[2] * (double)PO[2]);   // cv::norm, :1774
    const float maxDistance = 1.2f * maxD, minDistance = 0.8f * minD;            // Get{Max,Min}DistanceInvariance
    if (dist < minDistance || dist > maxDistance) return false;                  // :1780
    const float ratio = maxD / dist;                                             // MapPoint::PredictScale, src/MapPoint.cc:571-586
    int lvl = K.nlevels - 1;
    for (int k = K.nlevels - 2; k >= 0; k--)
        if (!(ratio > K.ratioTh[k])) lvl = k;
    level = lvl;
    radius = th * K.scale[lvl];                                                  // :1788
    return true;
}

// one thread per slot of hypothesis blockIdx.y.  status == nullptr: run (orbx_reloc_project)
__global__ __launch_bounds__(256) void k_reloc_project(RelocCam K, const int32_t *__restrict__ status, const int32_t *__restrict__ hypBase, const int32_t *__restrict__ hypNp,
                                                       const float *__restrict__ pose, const uint8_t *__restrict__ valid, const float *__restrict__ pos,
                                                       const float *__restrict__ maxD, const float *__restrict__ minD, const uint8_t *__restrict__ found, int P, float th,
                                                       float *__restrict__ qu, float *__restrict__ qv, float *__restrict__ qr, int32_t *__restrict__ qLo,
                                                       int32_t *__restrict__ qHi, uint8_t *__restrict__ active)
{
    const int h = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (status && status[h] != 0) return;
    if (i >= hypNp[h]) return;
    const size_t s = (size_t)hypBase[h] + i, q = (size_t)h * P + i;
    float u = 0.f, v = 0.f, r = 0.f;
    int lvl = 0;
    bool ok = valid[s] != 0 && found[q] == 0;                                    // pMP && !isBad() && !sAlreadyFound.count(pMP), :1752-1754
    if (ok) {
        const float X[3] = {pos[3 * s], pos[3 * s + 1], pos[3 * s + 2]};
        ok = reloc_project_eval(K, pose + 16 * h, X, maxD[s], minD[s], th, u, v, r, lvl);
    }
    qu[q] = ok ? u : 0.f; qv[q] = ok ? v : 0.f; qr[q] = ok ? r : 0.f;
    qLo[q] = ok ? lvl - 1 : 0; qHi[q] = ok ? lvl + 1 : 0;                        // GetFeaturesInArea(u, v, radius, nPredictedLevel-1, nPredictedLevel+1), :1791
    active[q] = ok ? 1 : 0;
}

// behind search `q` (0: th 10 / ORBdist 100, 1: th 3 / ORBdist 64): :1819-1860, the exit, and the problem of the next pose
__global__ __launch_bounds__(RL_THREADS) void k_reloc_apply(RelocDev D, int q)
{
    __shared__ int sh[RL_THREADS / 64];
    __shared__ int hist[HISTO_LENGTH + 2], sInd[3], sKept;
    const int h = blockIdx.x, tid = threadIdx.x, N = D.N;
    const bool was = D.status[h] == 0;
    bool running = was;
    if (was) {      // (uniform)
        const int np = D.hypNp[h];
        const size_t cb = (size_t)D.hypBase[h];
        if (tid < HISTO_LENGTH + 2) hist[tid] = 0;
        if (tid == 0) sKept = 0;
        __syncthreads();
        const float factor = HISTO_LENGTH / 360.0f;
        for (int i = tid; i < np; i += RL_THREADS) {
            const int a = D.asg[(size_t)h * D.P + i];
            if (a < 0 || a >= N) continue;
            D.mvp[(size_t)h * N + a] = i;                                                                          // :1820
            if (D.checkOri) {
                float rot = D.kfAngle[cb + i] - D.kp[a].angle;                                                     // :1826-1831
                if (rot < 0.0f) rot += 360.0f;
                int bin = (int)roundf(rot * factor);
                if (bin == HISTO_LENGTH) bin = 0;
                atomicAdd(&hist[min(max(bin, 0), HISTO_LENGTH - 1)], 1);
            }
        }
        __syncthreads();
        if (tid < 64) {
            int i1 = -1, i2 = -1, i3 = -1;
            if (D.checkOri) three_maxima_wave(hist, tid, i1, i2, i3);                                              // :1847
            if (tid == 0) { sInd[0] = i1; sInd[1] = i2; sInd[2] = i3; }
        }
        __syncthreads();
        int kept = 0;
        for (int i = tid; i < np; i += RL_THREADS) {
            const int a = D.asg[(size_t)h * D.P + i];
            if (a < 0 || a >= N) continue;
            bool keep = true;
            if (D.checkOri) {
                float rot = D.kfAngle[cb + i] - D.kp[a].angle;
                if (rot < 0.0f) rot += 360.0f;
                int bin = (int)roundf(rot * factor);
                if (bin == HISTO_LENGTH) bin = 0;
                bin = min(max(bin, 0), HISTO_LENGTH - 1);
                keep = bin == sInd[0] || bin == sInd[1] || bin == sInd[2];
                if (!keep) D.mvp[(size_t)h * N + a] = -1;                                                          // :1855
            }
            kept += keep ? 1 : 0;
        }
        kept = wave_sum_dpp(kept);
        if ((tid & 63) == 0 && kept) atomicAdd(&sKept, kept);
        __syncthreads();
        const int nadd = sKept;
        int *I = D.ints + h * RI_WORDS;
        const int nGood = I[RI_NGOOD + q];
        running = nadd + nGood >= 50;                                                                              // :2179 / :2203
        __syncthreads();      // (every thread has read the status word and the counts)
        if (tid == 0) {
            I[RI_NADD + q] = nadd;
            if (!running) { I[RI_STAGE] = q == 0 ? 2 : 5; I[RI_SUCCESS] = 0; D.status[h] = 1 + (q == 0 ? 2 : 5); }
        }
    }
    if (!running) {      // (uniform) left here or earlier: the pose launch behind is gated off, nothing is gathered
        if (tid == 0) D.gate[h] = -1;
        return;
    }
    reloc_gather(D, h, true, q + 1, sh);
}

struct RelocOut { int32_t *ints; float *pose; double *stats; int32_t *mapPoint; uint8_t *outlier; int32_t *pick; };      // mapped host memory; pick: winner, hypothesis, candidate

__global__ __launch_bounds__(RL_THREADS) void k_reloc_finish(RelocDev D, const int32_t *__restrict__ seqv, int S, RelocOut O, unsigned long long *pubFlag, unsigned long long pubSeq)
{
    __shared__ int sWin;
    const int tid = threadIdx.x;
    if (tid == 0) sWin = S;
    __syncthreads();
    for (int s = tid; s < S; s += RL_THREADS)
        if (D.ints[seqv[s] * RI_WORDS + RI_SUCCESS]) atomicMin(&sWin, s);                                          // the first returned pose that is accepted, :2218
    __syncthreads();
    const int win = sWin < S ? sWin : -1;
    const int hc = seqv[win >= 0 ? win : S - 1];      // nothing won: what the last processed pose left in mCurrentFrame
    for (int k = tid; k < D.H * RI_WORDS; k += RL_THREADS) O.ints[k] = D.ints[k];
    for (int k = tid; k < D.H * 16; k += RL_THREADS) O.pose[k] = D.poseCur[k];
    for (int k = tid; k < D.H * 24; k += RL_THREADS) O.stats[k] = D.statsAll[k];
    for (int j = tid; j < D.N; j += RL_THREADS) { O.mapPoint[j] = D.mvp[(size_t)hc * D.N + j]; O.outlier[j] = D.outl[(size_t)hc * D.N + j]; }
    if (tid == 0) { O.pick[0] = win; O.pick[1] = hc; O.pick[2] = D.hypCand[hc]; }
    orbx_publish(nullptr, pubFlag, pubSeq, 1u);
}

struct RelocSlots {      // the device working arrays of one call, planned once per call into m->rlWork
    OrbxSlot<int32_t, ORBX_STAGE_WORK> mvp, featSlot, status, count, gate, ret, ints, asg, dst, nm, qLo, qHi;
    OrbxSlot<float, ORBX_STAGE_WORK> Xw, obs, is2, poseCur, poseOut, qu, qv, qr, pnpTcw;
    OrbxSlot<uint8_t, ORBX_STAGE_WORK> outlEdge, outl, found, blocked, active, pnpMask;
    OrbxSlot<double, ORBX_STAGE_WORK> stats, statsAll;
    uint8_t *base = nullptr;
    int plan(orbx_matcher *m, size_t H, size_t N, size_t P, size_t cap, bool fromPnp)
    {
        OrbxWorkPlan &wp = m->rlPlan;
        wp.reset();
        mvp = wp.hole<int32_t>(H * N); featSlot = wp.hole<int32_t>(H * N); status = wp.hole<int32_t>(H); count = wp.hole<int32_t>(H); gate = wp.hole<int32_t>(H);
        ret = wp.hole<int32_t>(H); ints = wp.hole<int32_t>(H * RI_WORDS); asg = wp.hole<int32_t>(H * P); dst = wp.hole<int32_t>(H * P); nm = wp.hole<int32_t>(H);
        qLo = wp.hole<int32_t>(H * P); qHi = wp.hole<int32_t>(H * P);
        Xw = wp.hole<float>(H * cap * 3); obs = wp.hole<float>(H * cap * 3); is2 = wp.hole<float>(H * cap); poseCur = wp.hole<float>(H * 16); poseOut = wp.hole<float>(H * 16);
        qu = wp.hole<float>(H * P); qv = wp.hole<float>(H * P); qr = wp.hole<float>(H * P);
        outlEdge = wp.hole<uint8_t>(H * cap); outl = wp.hole<uint8_t>(H * N); found = wp.hole<uint8_t>(H * P); blocked = wp.hole<uint8_t>(H * N); active = wp.hole<uint8_t>(H * P);
        stats = wp.hole<double>(H * 8); statsAll = wp.hole<double>(H * 24);
        pnpTcw = wp.hole<float>(fromPnp ? H * 16 : 0); pnpMask = wp.hole<uint8_t>(fromPnp ? H * N : 0);
        const int rc = m->rlWork.ensure(wp.total());
        base = m->rlWork.p;
        return rc;
    }
};

int fill_cam(RelocCam &K, const orbx_reloc_frame *fr)
{
    K.fx = fr->fx; K.fy = fr->fy; K.cx = fr->cx; K.cy = fr->cy;
    K.minX = fr->frame.min_x; K.maxX = fr->max_x; K.minY = fr->frame.min_y; K.maxY = fr->max_y; K.nlevels = fr->nlevels;
    for (int k = 0; k < ORBX_MAX_LEVELS; k++) {
        K.ratioTh[k] = k + 1 < fr->nlevels ? fr->ratio_thresholds[k] : 0.0f;
        K.scale[k] = k < fr->nlevels ? fr->scale_factors[k] : 0.0f;
    }
    return ORBX_OK;
}

int check_frame(const orbx_reloc_frame *fr, bool needFeatures)
{
    if (!fr->scale_factors || !fr->ratio_thresholds || fr->nlevels < 1 || fr->nlevels > ORBX_MAX_LEVELS) {
        orbx_set_error("bad scale tables (%d levels, 1..%d)", fr->nlevels, ORBX_MAX_LEVELS);
        return ORBX_ERR_ARG;
    }
    if (needFeatures && (!fr->frame.counts || !fr->frame.keypoints_un || !fr->frame.descriptors || !fr->frame.u_right || !fr->inv_level_sigma2)) {
        orbx_set_error("NULL array in the frame arguments");
        return ORBX_ERR_ARG;
    }
    return ORBX_OK;
}

int check_candidate(const orbx_reloc_candidate *c, bool needBow)
{
    if (c->npoints < 0) { orbx_set_error("npoints %d < 0", c->npoints); return ORBX_ERR_ARG; }
    if (c->npoints > 0 && (!c->valid || !c->world_pos || !c->max_distance || !c->min_distance)) { orbx_set_error("NULL array in a candidate"); return ORBX_ERR_ARG; }
    if (needBow && (!c->bow_match || (c->npoints > 0 && (!c->descriptors || !c->kf_angle)))) { orbx_set_error("NULL array in a candidate"); return ORBX_ERR_ARG; }
    return ORBX_OK;
}

}  // namespace

extern "C" int orbx_reloc_project(orbx_matcher *m, const orbx_reloc_frame *fr, const orbx_reloc_candidate *cand, const float *tcw, const uint8_t *found, float th, float *u,
                                  float *v, float *radius, int32_t *min_level, int32_t *max_level, uint8_t *active)
{
    if (!m || !fr || !cand || !tcw || !u || !v || !radius || !min_level || !max_level || !active) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = check_frame(fr, false)) != ORBX_OK || (rc = check_candidate(cand, false)) != ORBX_OK) return rc;
    const int np = cand->npoints;
    if (np == 0) return ORBX_OK;
    if (np > m->maxFeatures || np > 65535) { orbx_set_error("%d slots exceed the matcher's max_features %d", np, m->maxFeatures); return ORBX_ERR_CAPACITY; }
    ORBX_HIP_CHECK(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    OrbxCallBox &bx = m->box;
    const size_t P = (size_t)np;
    float pose[16];
    memcpy(pose, tcw, 48);
    pose[12] = pose[13] = pose[14] = 0.f; pose[15] = 1.f;
    const int32_t hv[2] = {0, np};
    std::vector<uint8_t> zero;
    if (!found) zero.assign(P, 0);
    auto [pin, pout] = bx.plan();
    const auto sPose = pin.add(pose, 16);
    const auto sHv = pin.add(hv, 2);
    const auto sVal = pin.add(cand->valid, P), sFound = pin.add(found ? found : zero.data(), P);
    const auto sPos = pin.add(cand->world_pos, P * 3), sMax = pin.add(cand->max_distance, P), sMin = pin.add(cand->min_distance, P);
    const auto rU = pout.hole<float>(P), rV = pout.hole<float>(P), rR = pout.hole<float>(P);
    const auto rLo = pout.hole<int32_t>(P), rHi = pout.hole<int32_t>(P);
    const auto rAct = pout.hole<uint8_t>(P);
    const OrbxStaged sg = bx.begin(st, &rc);
    if (rc != ORBX_OK) return rc;
    RelocCam K;
    fill_cam(K, fr);
    hipLaunchKernelGGL(k_reloc_project, dim3((unsigned)((np + 255) / 256), 1u), dim3(256), 0, st, K, (const int32_t *)nullptr, sg.dev(sHv), sg.dev(sHv) + 1, sg.dev(sPose),
                       sg.dev(sVal), sg.dev(sPos), sg.dev(sMax), sg.dev(sMin), sg.dev(sFound), np, th, sg.dev(rU), sg.dev(rV), sg.dev(rR), sg.dev(rLo), sg.dev(rHi), sg.dev(rAct));
    ORBX_LAUNCH_CHECK();
    ORBX_HIP_CHECK(hipStreamSynchronize(st));
    memcpy(u, sg.host(rU), P * 4); memcpy(v, sg.host(rV), P * 4); memcpy(radius, sg.host(rR), P * 4);
    memcpy(min_level, sg.host(rLo), P * 4); memcpy(max_level, sg.host(rHi), P * 4); memcpy(active, sg.host(rAct), P);
    return ORBX_OK;
}

extern "C" int orbx_relocalize_refine(orbx_matcher *m, const orbx_reloc_frame *fr, const orbx_reloc_candidate *cands, int ncands, const orbx_reloc_hypotheses *hyp,
                                      orbx_reloc_result *res)
{
    if (!m || !fr || !cands || !hyp || !res) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = check_frame(fr, true)) != ORBX_OK) return rc;
    const int n = fr->frame.counts[0], H = hyp->count, S = hyp->sequence_length;
    if (n < 1 || ncands < 1 || H < 1 || S < 1) { orbx_set_error("empty problem (features %d, candidates %d, hypotheses %d, sequence %d)", n, ncands, H, S); return ORBX_ERR_ARG; }
    const bool fromPnp = hyp->pnp != nullptr;
    if (!hyp->candidate || !hyp->sequence || (fromPnp ? (!hyp->record || !hyp->keypoint_index || !hyp->keypoint_count) : (!hyp->tcw || !hyp->inliers))) {
        orbx_set_error("NULL array in the hypotheses");
        return ORBX_ERR_ARG;
    }
    if (H > ORBX_RELOC_MAX_HYPOTHESES || S > ORBX_RELOC_MAX_SEQUENCE) {
        orbx_set_error("%d hypotheses / %d sequence entries exceed %d / %d", H, S, ORBX_RELOC_MAX_HYPOTHESES, ORBX_RELOC_MAX_SEQUENCE);
        return ORBX_ERR_CAPACITY;
    }
    if (n > m->maxFeatures || n > 65535) { orbx_set_error("%d features exceed the matcher's max_features %d", n, m->maxFeatures); return ORBX_ERR_CAPACITY; }
    const size_t N = (size_t)n;
    std::vector<int32_t> cBase((size_t)ncands), cValid((size_t)ncands);
    size_t total = 0;
    int maxNp = 1;
    for (int c = 0; c < ncands; c++) {
        if ((rc = check_candidate(&cands[c], true)) != ORBX_OK) return rc;
        const int np = cands[c].npoints;
        if (np > m->maxFeatures || np > 65535) { orbx_set_error("%d slots exceed the matcher's max_features %d", np, m->maxFeatures); return ORBX_ERR_CAPACITY; }
        for (size_t j = 0; j < N; j++)
            if (cands[c].bow_match[j] < -1 || cands[c].bow_match[j] >= np) { orbx_set_error("bow_match[%zu] = %d of candidate %d outside -1..%d", j, cands[c].bow_match[j], c, np - 1); return ORBX_ERR_ARG; }
        int nv = 0;
        for (int s = 0; s < np; s++) nv += cands[c].valid[s] ? 1 : 0;
        cBase[(size_t)c] = (int32_t)total; cValid[(size_t)c] = nv;
        total += (size_t)np;
        maxNp = std::max(maxNp, np);
    }
    // every correspondence takes a feature of its own; the seeds are known here, a search adds at most the candidate's valid slots
    int bound1 = 0, boundLater = 0;
    std::vector<int32_t> hBase((size_t)H), hNp((size_t)H);
    // form (b): where the PnP chain left each hypothesis' record, and per named candidate the compacted match that sits on each feature
    std::vector<PnpHypRow> rows;
    std::vector<int32_t> matchOf;
    if (fromPnp) {
        rows.resize((size_t)H);
        matchOf.assign((size_t)ncands * N, -1);
        std::vector<char> done((size_t)ncands, 0);
        for (int h = 0; h < H; h++) {
            const int c = hyp->candidate[h];
            if (c < 0 || c >= ncands) { orbx_set_error("hypothesis %d names candidate %d of %d", h, c, ncands); return ORBX_ERR_ARG; }
            OrbxPnpRows pr;
            if ((rc = orbx_pnp_device_rows_internal(hyp->pnp, c, m->device, &pr)) != ORBX_OK) return rc;
            const int r = hyp->record[h];
            if (r < 0 || r >= pr.nrec) { orbx_set_error("hypothesis %d names record %d of candidate %d, which has %d", h, r, c, pr.nrec); return ORBX_ERR_ARG; }
            rows[(size_t)h] = PnpHypRow{pr.refR + 9 * (size_t)r, pr.refT + 3 * (size_t)r, pr.refMask + (size_t)r * pr.words};
            if (done[(size_t)c]) continue;
            done[(size_t)c] = 1;
            if (hyp->keypoint_count[c] != pr.n || (pr.n > 0 && !hyp->keypoint_index[c])) {
                orbx_set_error("keypoint_index of candidate %d has %d entries, the PnP solve had %d matches", c, hyp->keypoint_count[c], pr.n);
                return ORBX_ERR_ARG;
            }
            for (int i = 0; i < pr.n; i++) {
                const int j = hyp->keypoint_index[c][i];
                if (j < 0 || j >= n || matchOf[(size_t)c * N + j] >= 0) { orbx_set_error("keypoint_index[%d][%d] = %d is outside 0..%d or names a feature twice", c, i, j, n - 1); return ORBX_ERR_ARG; }
                matchOf[(size_t)c * N + j] = i;
            }
        }
    }
    for (int h = 0; h < H; h++) {
        const int c = hyp->candidate[h];
        if (c < 0 || c >= ncands) { orbx_set_error("hypothesis %d names candidate %d of %d", h, c, ncands); return ORBX_ERR_ARG; }
        int seeds = 0;      // form (b): the mask is on the device; every match of the solve that holds a BoW point may be a seed
        for (size_t j = 0; j < N; j++) seeds += ((fromPnp ? matchOf[(size_t)c * N + j] >= 0 : hyp->inliers[(size_t)h * N + j] != 0) && cands[c].bow_match[j] >= 0) ? 1 : 0;
        bound1 = std::max(bound1, seeds);
        boundLater = std::max(boundLater, (int)std::min<long long>(n, (long long)seeds + cValid[(size_t)c]));
        hBase[(size_t)h] = cBase[(size_t)c]; hNp[(size_t)h] = cands[c].npoints;
    }
    for (int s = 0; s < S; s++)
        if (hyp->sequence[s] < 0 || hyp->sequence[s] >= H) { orbx_set_error("sequence[%d] = %d outside 0..%d", s, hyp->sequence[s], H - 1); return ORBX_ERR_ARG; }
    if (boundLater > ORBX_TRACK_MAX_CORRESPONDENCES) {
        orbx_set_error("%d possible correspondences exceed the pose kernel's limit %d", boundLater, ORBX_TRACK_MAX_CORRESPONDENCES);
        return ORBX_ERR_CAPACITY;
    }
    if (N * 4 + (size_t)maxNp * 6 + 16 > 160 * 1024) { orbx_set_error("capacities too large for the LDS tile of the replay"); return ORBX_ERR_CAPACITY; }
    ORBX_HIP_CHECK(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    OrbxCallBox &bx = m->box;
    const size_t T = std::max<size_t>(total, 1), P = (size_t)maxNp, HH = (size_t)H, cap = (size_t)std::max(boundLater, 1);
    const int32_t cnt[1] = {n};
    auto [pin, pout] = bx.plan();
    const auto sKp = pin.add(fr->frame.keypoints_un, N);
    const auto sDesc = pin.add(fr->frame.descriptors, N * 32);
    const auto sUr = pin.add(fr->frame.u_right, N);
    const auto sCnt = pin.add(cnt, 1);
    const auto sIs = pin.add(fr->inv_level_sigma2, (size_t)fr->nlevels);
    const auto sVal = pin.hole<uint8_t>(T), sCd = pin.hole<uint8_t>(T * 32);
    const auto sPos = pin.hole<float>(T * 3), sMax = pin.hole<float>(T), sMin = pin.hole<float>(T), sAng = pin.hole<float>(T);
    const auto sBow = pin.hole<int32_t>((size_t)ncands * N);
    const auto sHc = pin.add(hyp->candidate, HH), sHb = pin.add(hBase.data(), HH), sHn = pin.add(hNp.data(), HH), sSeq = pin.add(hyp->sequence, (size_t)S);
    const auto sTcw = pin.hole<float>(HH * 16), sCam = pin.hole<float>(HH * 5);
    const auto sMask = pin.add(hyp->inliers, fromPnp ? 0 : HH * N);
    const auto sRows = pin.add(rows.data(), fromPnp ? HH : 0);
    const auto sMatchOf = pin.add(matchOf.data(), fromPnp ? (size_t)ncands * N : 0);
    const auto rInts = pout.hole<int32_t>(HH * RI_WORDS);
    const auto rPose = pout.hole<float>(HH * 16);
    const auto rStats = pout.hole<double>(HH * 24);
    const auto rMp = pout.hole<int32_t>(N);
    const auto rOutl = pout.hole<uint8_t>(N);
    const auto rPick = pout.hole<int32_t>(4);
    const OrbxStaged sg = bx.begin(st, &rc);
    if (rc != ORBX_OK) return rc;
    for (int c = 0; c < ncands; c++) {
        const size_t b = (size_t)cBase[(size_t)c], np = (size_t)cands[c].npoints;
        orbx_put_at(sg, sVal, b, cands[c].valid, np); orbx_put_at(sg, sCd, b * 32, cands[c].descriptors, np * 32);
        orbx_put_at(sg, sPos, b * 3, cands[c].world_pos, np * 3); orbx_put_at(sg, sMax, b, cands[c].max_distance, np); orbx_put_at(sg, sMin, b, cands[c].min_distance, np);
        orbx_put_at(sg, sAng, b, cands[c].kf_angle, np); orbx_put_at(sg, sBow, (size_t)c * N, cands[c].bow_match, N);
    }
    for (int h = 0; h < H; h++) {
        float *t = sg.host(sTcw) + 16 * (size_t)h, *k = sg.host(sCam) + 5 * (size_t)h;
        if (!fromPnp) memcpy(t, hyp->tcw + 12 * (size_t)h, 48);
        t[12] = t[13] = t[14] = 0.f; t[15] = 1.f;
        k[0] = fr->fx; k[1] = fr->fy; k[2] = fr->cx; k[3] = fr->cy; k[4] = fr->mbf;
    }
    RelocSlots w;
    if ((rc = w.plan(m, HH, N, P, cap, fromPnp)) != ORBX_OK) return rc;
    if ((rc = m->topk64.ensure(HH * P * TOPK)) != ORBX_OK) return rc;      // (enqueue_area_greedy's candidate lists: no allocation between the chain's launches)
    uint8_t *ar;
    if ((rc = orbx_stage_to_arena(bx, m->arena, st, 512, &ar)) != ORBX_OK) return rc;
    ORBX_LAUNCH_CHECK();
    uint8_t *wb = w.base;
    RelocDev D;
    D.H = H; D.N = n; D.P = maxNp; D.cap = (int)cap; D.nlevels = fr->nlevels; D.checkOri = fr->check_orientation ? 1 : 0;
    D.kp = sKp.in(ar); D.uRight = sUr.in(ar); D.invS2 = sIs.in(ar);
    D.valid = sVal.in(ar); D.pos = sPos.in(ar); D.maxD = sMax.in(ar); D.minD = sMin.in(ar); D.kfAngle = sAng.in(ar); D.bow = sBow.in(ar);
    D.hypCand = sHc.in(ar); D.hypBase = sHb.in(ar); D.hypNp = sHn.in(ar); D.hypTcw = sTcw.in(ar); D.hypMask = sMask.in(ar);
    D.mvp = w.mvp.in(wb); D.featSlot = w.featSlot.in(wb); D.status = w.status.in(wb); D.count = w.count.in(wb); D.gate = w.gate.in(wb); D.ret = w.ret.in(wb);
    D.ints = w.ints.in(wb); D.asg = w.asg.in(wb);
    D.Xw = w.Xw.in(wb); D.obs = w.obs.in(wb); D.is2 = w.is2.in(wb); D.poseCur = w.poseCur.in(wb); D.poseOut = w.poseOut.in(wb);
    D.qu = w.qu.in(wb); D.qv = w.qv.in(wb); D.qr = w.qr.in(wb); D.qLo = w.qLo.in(wb); D.qHi = w.qHi.in(wb);
    D.outlEdge = w.outlEdge.in(wb); D.outl = w.outl.in(wb); D.found = w.found.in(wb); D.blocked = w.blocked.in(wb); D.active = w.active.in(wb);
    D.stats = w.stats.in(wb); D.statsAll = w.statsAll.in(wb);
    RelocCam K;
    fill_cam(K, fr);
    OrbxPoseOptArgs pa;
    pa.pose0 = D.poseCur; pa.cam = sCam.in(ar); pa.Xw = D.Xw; pa.obs = D.obs; pa.invS2 = D.is2; pa.counts = D.count; pa.cap = (int)cap;
    pa.poseOut = D.poseOut; pa.outlier = D.outlEdge; pa.ret = D.ret; pa.stats = D.stats; pa.gate = D.gate;
    const ProjFrameDev F = {sKp.in(ar), sDesc.in(ar), sUr.in(ar), nullptr, sCnt.in(ar), n, fr->frame.min_x, fr->frame.min_y, fr->frame.grid_width_inv, fr->frame.grid_height_inv};
    const AreaQueriesArgs Q = {D.qu, D.qv, D.qr, D.qLo, D.qHi, D.active, sCd.in(ar), D.hypNp, maxNp, fr->frame.min_x, fr->frame.min_y};
    const AreaChainDev C = {D.status, D.hypBase, D.blocked};
    const dim3 gH((unsigned)H), gP((unsigned)((maxNp + 255) / 256), (unsigned)H);
    if (fromPnp) {
        D.hypTcw = w.pnpTcw.in(wb); D.hypMask = w.pnpMask.in(wb);
        hipLaunchKernelGGL(k_reloc_from_pnp, gH, dim3(RL_THREADS), 0, st, sRows.in(ar), D.hypCand, sMatchOf.in(ar), n, w.pnpTcw.in(wb), w.pnpMask.in(wb));
        ORBX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_reloc_seed, gH, dim3(RL_THREADS), 0, st, D);
    ORBX_LAUNCH_CHECK();
    for (int p = 0; p < 3; p++) {
        pa.maxCount = std::max(p == 0 ? bound1 : boundLater, 1);
        if ((rc = orbx_pose_opt_enqueue_batch(st, pa, H)) != ORBX_OK) return rc;
        hipLaunchKernelGGL(k_reloc_decide, gH, dim3(RL_THREADS), 0, st, D, p);
        ORBX_LAUNCH_CHECK();
        if (p == 2) break;
        hipLaunchKernelGGL(k_reloc_project, gP, dim3(256), 0, st, K, (const int32_t *)D.status, D.hypBase, D.hypNp, (const float *)D.poseCur, D.valid, D.pos, D.maxD, D.minD,
                           (const uint8_t *)D.found, maxNp, p == 0 ? 10.0f : 3.0f, D.qu, D.qv, D.qr, D.qLo, D.qHi, D.active);
        ORBX_LAUNCH_CHECK();
        if ((rc = orbx_match::enqueue_area_greedy(m, st, F, Q, C, H, p == 0 ? 100 : 64, D.asg, w.dst.in(wb), w.nm.in(wb))) != ORBX_OK) return rc;
        hipLaunchKernelGGL(k_reloc_apply, gH, dim3(RL_THREADS), 0, st, D, p);
        ORBX_LAUNCH_CHECK();
    }
    const RelocOut O = {sg.dev(rInts), sg.dev(rPose), sg.dev(rStats), sg.dev(rMp), sg.dev(rOutl), sg.dev(rPick)};
    const unsigned long long seq = bx.arm();
    hipLaunchKernelGGL(k_reloc_finish, dim3(1), dim3(RL_THREADS), 0, st, D, sSeq.in(ar), S, O, bx.flagDev, seq);
    ORBX_LAUNCH_CHECK();
    if ((rc = bx.wait(st)) != ORBX_OK) return rc;
    const int32_t *hi = sg.host(rInts), *pk = sg.host(rPick);
    for (int h = 0; h < H; h++) {
        const int32_t *I = hi + h * RI_WORDS;
        if (res->stage) res->stage[h] = I[RI_STAGE];
        if (res->success) res->success[h] = I[RI_SUCCESS];
        for (int k = 0; k < 3; k++) { if (res->ngood) res->ngood[3 * h + k] = I[RI_NGOOD + k]; if (res->n_correspondences) res->n_correspondences[3 * h + k] = I[RI_NCORR + k]; }
        for (int k = 0; k < 2; k++) if (res->nadditional) res->nadditional[2 * h + k] = I[RI_NADD + k];
    }
    if (res->pose) memcpy(res->pose, sg.host(rPose), HH * 64);
    if (res->stats) memcpy(res->stats, sg.host(rStats), HH * 24 * 8);
    if (res->map_point) memcpy(res->map_point, sg.host(rMp), N * 4);
    if (res->outlier) memcpy(res->outlier, sg.host(rOutl), N);
    res->winner = pk[0]; res->hypothesis = pk[1]; res->candidate = pk[2];
    return ORBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The head of Tracking::Relocalization: K searches, the < 15 decision, the PnP solvers' arrays (include/orbx.h: orbx_reloc_match_candidates)
// ---------------------------------------------------------------------------------------------------------------------------------------------
namespace {

struct RelocMatchOut { int32_t *matches, *keyIndex; float *p2d, *sigma2, *p3dw; int32_t *ints; };      // mapped host memory; ints[3 k ..]: n, nmatches, discarded

// One workgroup per candidate: its row of matches goes out as the search left it; if the search returned >= 15 (:2075) the frame features that hold a match,
// in ascending order (rank from a ballot, as k_reloc_seed's gather), become mvKeyPointIndices / mvP2D / mvSigma2 / mvP3Dw (src/PnPsolver.cc:136-158; the
// search only matches non-bad points, so :142 holds for each).  A discarded candidate's arrays are not written.
__global__ __launch_bounds__(RL_THREADS) void k_reloc_pnp_gather(const int32_t *__restrict__ mat, const int32_t *__restrict__ nm, int stride, int N,
                                                                 const orbx_keypoint *__restrict__ kpUn, const float *__restrict__ levelS2, int nlevels,
                                                                 const float *__restrict__ pos, int capA, RelocMatchOut O, unsigned *counter, unsigned long long *pubFlag,
                                                                 unsigned long long pubSeq)
{
    __shared__ int sh[RL_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int32_t *mk = mat + (size_t)k * stride;
    const float *pk = pos + 3 * (size_t)k * capA;
    const int nms = nm[k];
    const bool keep = nms >= 15;
    const size_t row = (size_t)k * N;
    int base = 0;
    for (int i0 = 0; i0 < N; i0 += RL_THREADS) {
        const int i = i0 + tid;
        const int mi = i < N ? mk[i] : -1;
        const bool has = keep && mi >= 0;
        if (i < N) O.matches[row + i] = mi;
        const int slot = block_ballot_rank<RL_THREADS>(has, &base, sh);
        if (has) {
            const orbx_keypoint kp = kpUn[i];
            const size_t e = row + slot;
            O.keyIndex[e] = i;
            O.p2d[2 * e] = kp.x; O.p2d[2 * e + 1] = kp.y;
            O.sigma2[e] = levelS2[min(max(kp.octave, 0), nlevels - 1)];
            O.p3dw[3 * e] = pk[3 * (size_t)mi]; O.p3dw[3 * e + 1] = pk[3 * (size_t)mi + 1]; O.p3dw[3 * e + 2] = pk[3 * (size_t)mi + 2];
        }
    }
    if (tid == 0) { O.ints[3 * k] = keep ? base : 0; O.ints[3 * k + 1] = nms; O.ints[3 * k + 2] = keep ? 0 : 1; }
    orbx_publish(counter, pubFlag, pubSeq, gridDim.x);
}

}  // namespace

extern "C" int orbx_reloc_match_candidates(orbx_matcher *m, const orbx_reloc_match_frame *fr, const orbx_reloc_match_keyframe *kfs, int K, float nn_ratio, int check_orientation,
                                           const orbx_reloc_match_result *res)
{
    if (!m || !fr || !kfs || !res) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (K < 1) { orbx_set_error("no candidate"); return ORBX_ERR_ARG; }
    if (!fr->features || !fr->features->counts || !fr->level_sigma2) { orbx_set_error("NULL counts or level table"); return ORBX_ERR_ARG; }
    if (fr->nlevels < 1 || fr->nlevels > 64) { orbx_set_error("bad level table (%d levels, 1..64)", fr->nlevels); return ORBX_ERR_ARG; }
    const orbx_feature_set *b = fr->features;
    const int n = b->counts[0];
    if (n > 0 && (!b->keypoints || !b->descriptors || !fr->keypoints_un)) { orbx_set_error("NULL array in the frame arguments"); return ORBX_ERR_ARG; }
    int capA = 0, withGroups = 0, withValid = 0, live = 0;
    std::vector<int32_t> cnt((size_t)K + 1, 0), iota((size_t)2 * K, 0);
    for (int k = 0; k < K; k++) {
        iota[(size_t)k] = k;
        if (kfs[k].is_bad) continue;
        const orbx_feature_set *a = kfs[k].features;
        if (!a || !a->counts) { orbx_set_error("NULL features of candidate %d", k); return ORBX_ERR_ARG; }
        const int nA = a->counts[0];
        if (nA <= 0) continue;
        if (!a->keypoints || !a->descriptors || !kfs[k].world_pos) { orbx_set_error("NULL array in candidate %d", k); return ORBX_ERR_ARG; }
        cnt[(size_t)k] = nA;
        capA = std::max(capA, nA);
        live++; withGroups += a->groups ? 1 : 0; withValid += a->valid ? 1 : 0;
    }
    if (withGroups != 0 && withGroups != live) { orbx_set_error("groups on %d of %d candidates (every keyframe or none)", withGroups, live); return ORBX_ERR_ARG; }
    cnt[(size_t)K] = std::max(n, 0);
    if (n <= 0 || capA <= 0) {      // nothing to search: every candidate is discarded (:2066 / :2075), without a launch
        for (int k = 0; k < K; k++) {
            if (res->n) res->n[k] = 0;
            if (res->nmatches) res->nmatches[k] = 0;
            if (res->discarded) res->discarded[k] = 1;
            for (int i = 0; i < n; i++) if (res->matches) res->matches[(size_t)k * n + i] = -1;
        }
        return ORBX_OK;
    }
    if (K > m->maxPairs) { orbx_set_error("%d candidates exceed the matcher's max_pairs %d", K, m->maxPairs); return ORBX_ERR_CAPACITY; }
    if (n > m->maxFeatures || capA > m->maxFeatures) { orbx_set_error("%d / %d features exceed the matcher's max_features %d", capA, n, m->maxFeatures); return ORBX_ERR_CAPACITY; }
    if (n > 4000) { orbx_set_error("%d frame features exceed the pair kernel's LDS bound 4000", n); return ORBX_ERR_CAPACITY; }
    if (capA > 65535 || orbx_match::bow_pair_replay_lds(capA, n, false) > 160 * 1024) { orbx_set_error("feature counts %d / %d too large for the LDS tile of the replay", capA, n); return ORBX_ERR_CAPACITY; }
    ORBX_HIP_CHECK(hipSetDevice(m->device));
    int rc;
    hipStream_t st = m->stream;
    OrbxCallBox &bx = m->box;
    const size_t N = (size_t)n, KK = (size_t)K, CA = (size_t)capA;
    const int stride = std::max(capA, n);
    auto [pin, pout] = bx.plan();
    const auto sKpB = pin.add(b->keypoints, N);
    const auto sDescB = pin.add(b->descriptors, N * 32);
    const auto sGrB = pin.add(b->groups, b->groups ? N : 0);
    const auto sKpUn = pin.add(fr->keypoints_un, N);
    const auto sS2 = pin.add(fr->level_sigma2, (size_t)fr->nlevels);
    const auto sCnt = pin.add(cnt.data(), KK + 1);
    const auto sPairs = pin.add(iota.data(), 2 * KK);
    const auto sKpA = pin.hole<orbx_keypoint>(KK * CA);
    const auto sDescA = pin.hole<uint8_t>(KK * CA * 32);
    const auto sGrA = pin.hole<int32_t>(withGroups ? KK * CA : 0);
    const auto sValA = pin.hole<uint8_t>(withValid ? KK * CA : 0);
    const auto sPos = pin.hole<float>(KK * CA * 3);
    const auto rMat = pout.hole<int32_t>(KK * N), rKey = pout.hole<int32_t>(KK * N);
    const auto rP2 = pout.hole<float>(KK * N * 2), rS2 = pout.hole<float>(KK * N), rP3 = pout.hole<float>(KK * N * 3);
    const auto rInts = pout.hole<int32_t>(KK * 3);
    const OrbxStaged sg = bx.begin(st, &rc);
    if (rc != ORBX_OK) return rc;
    for (int k = 0; k < K; k++) {      // (a candidate staged with count 0 - bad, or without features - keeps its rows unwritten: nothing reads them)
        const size_t nA = (size_t)cnt[(size_t)k], at = (size_t)k * CA;
        if (!nA) continue;
        const orbx_feature_set *a = kfs[k].features;
        orbx_put_at(sg, sKpA, at, a->keypoints, nA); orbx_put_at(sg, sDescA, at * 32, a->descriptors, nA * 32); orbx_put_at(sg, sPos, at * 3, kfs[k].world_pos, nA * 3);
        if (withGroups) orbx_put_at(sg, sGrA, at, a->groups, nA);
        if (withValid) { if (a->valid) orbx_put_at(sg, sValA, at, a->valid, nA); else memset(sg.host(sValA) + at, 1, nA); }
    }
    if ((rc = orbx_match::track_mark(m, st, 0)) != ORBX_OK) return rc;
    uint8_t *ar;
    if ((rc = orbx_stage_to_arena(bx, m->arena, st, 512, &ar)) != ORBX_OK) return rc;
    ORBX_LAUNCH_CHECK();
    if ((rc = orbx_match::track_mark(m, st, 1)) != ORBX_OK) return rc;
    const int32_t *dCnt = sCnt.in(ar);
    FeatDev A, B;
    A.kp = sKpA.in(ar); A.desc = sDescA.in(ar); A.groups = withGroups ? sGrA.in(ar) : nullptr; A.valid = withValid ? sValA.in(ar) : nullptr; A.counts = dCnt; A.cap = capA;
    B.kp = sKpB.in(ar); B.desc = sDescB.in(ar); B.groups = b->groups ? sGrB.in(ar) : nullptr; B.valid = nullptr; B.counts = dCnt + K; B.cap = n;
    if ((rc = orbx_match::enqueue_bow_candidates(m, st, A, B, K, sPairs.in(ar), sPairs.in(ar) + K, nn_ratio, check_orientation, stride)) != ORBX_OK) return rc;
    if ((rc = orbx_match::track_mark(m, st, 2)) != ORBX_OK) return rc;
    const RelocMatchOut O = {sg.dev(rMat), sg.dev(rKey), sg.dev(rP2), sg.dev(rS2), sg.dev(rP3), sg.dev(rInts)};
    const unsigned long long seq = bx.arm();
    hipLaunchKernelGGL(k_reloc_pnp_gather, dim3((unsigned)K), dim3(RL_THREADS), 0, st, (const int32_t *)m->matches.p, (const int32_t *)m->nmatches.p, stride, n, sKpUn.in(ar),
                       sS2.in(ar), fr->nlevels, sPos.in(ar), capA, O, bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_CHECK();
    if ((rc = orbx_match::track_mark(m, st, 3)) != ORBX_OK) return rc;
    if ((rc = bx.wait(st)) != ORBX_OK) return rc;
    const int32_t *hi = sg.host(rInts);
    if (res->matches) memcpy(res->matches, sg.host(rMat), KK * N * 4);
    for (int k = 0; k < K; k++) {
        const size_t nk = (size_t)hi[3 * k], row = (size_t)k * N;
        if (res->n) res->n[k] = hi[3 * k];
        if (res->nmatches) res->nmatches[k] = hi[3 * k + 1];
        if (res->discarded) res->discarded[k] = (uint8_t)hi[3 * k + 2];
        if (res->key_index) memcpy(res->key_index + row, sg.host(rKey) + row, nk * 4);
        if (res->p2d) memcpy(res->p2d + 2 * row, sg.host(rP2) + 2 * row, nk * 8);
        if (res->sigma2) memcpy(res->sigma2 + row, sg.host(rS2) + row, nk * 4);
        if (res->p3dw) memcpy(res->p3dw + 3 * row, sg.host(rP3) + 3 * row, nk * 12);
    }
    return ORBX_OK;
}
