// orbx_loop_sim3.hip -- the refine step of LoopClosing::ComputeSim3 (src/LoopClosing.cc:435-480) for EVERY event of EVERY candidate as ONE launch chain
// with ONE host wait (include/orbx.h: orbx_loop_refine_sim3); the diagnostic arrays, when asked for, are copied behind it with a synchronisation of their own.
//
// The two numeric steps had kernels: the search of ORBmatcher::SearchBySim3 (k_fuse_best in orbx_match_proj.hip, chi2_gate = 0) and
// Optimizer::OptimizeSim3 (k_optsim3 in orbx_optimize_sim3.hip, here through orbx_optsim3_enqueue on device-resident problems).  This file adds what the
// reference does around them on the host:
//   k_ls_from_solver  (hypotheses named as iterations of a Sim3 solve) R12 / t12 / s12 and the inlier mask of each, read where orbx_sim3_solve left them
//   k_ls_seed         :437-443, src/ORBmatcher.cc:1333-1357  vpMapPointMatches from the mask, vbAlreadyMatched1 / 2, sR12, sR21, t21
//   k_ls_project      src/ORBmatcher.cc:1367-1411 / :1430-1474  both directions: the projection, z, IsInImage, dist3D, PredictScale, the radius per slot
//   k_ls_mutual       :1507-1521, src/Optimizer.cc:1429-1520  the mutual check, nFound, OptimizeSim3's pairs and its problem header
//   k_ls_finish       src/Optimizer.cc:1541 / :1578, :463-474  the removed pairs, nInliers >= 20, mg2oScw = gScm * gSmw, mScw; the LAST workgroup to arrive
//                     walks the status words in order, picks the winner, copies its matches out and raises the sequence word
// Launches of a call: k_stage_copy, [k_ls_from_solver,] k_ls_seed, k_ls_project, k_fuse_best, k_ls_mutual, k_optsim3, k_ls_finish = 7 (8 in form (b)).
// Every stage is enqueued unconditionally.  KF1 and the K candidates are staged once; the 2 H searches name their keyframe and their point list by index
// (ProjFrameDev::frameOf, FusePointsDev::descOf).  One workgroup per hypothesis where a stage compacts (rank from a ballot, orbx_wave.h): no atomics on
// global memory except the arrival counter.
#include "orbx_match_internal.h"
#include "orbx_optsim3.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace {

#define LS_THREADS 1024
#define LS_MAXP ORBX_SIM3_OPT_MAX_PAIRS
#define LI_STATUS 0
#define LI_NFOUND 1
#define LI_NPAIRS 2
#define LI_NIN 3
#define LI_NBAD 4
#define LI_WORDS 8

struct LsKf { float R[9], t[3], k[4]; int32_t n, nlevels; float ratioTh[ORBX_MAX_LEVELS], scale[ORBX_MAX_LEVELS], invS2[ORBX_MAX_LEVELS]; };
struct LsCam { float fx, fy, cx, cy, minX, maxX, minY, maxY; };      // KF1's intrinsics (both directions, as the reference) and the image bounds (statics of Frame)

struct LsDev {
    int H, NP, N1;
    // the keyframes: 0 = KF1, 1 + c = candidate c; slot s of keyframe f at f * NP + s
    const LsKf *kf; const orbx_keypoint *kp; const uint8_t *valid; const float *pos, *maxD, *minD; const int32_t *bow;      // bow: [K * N1]
    // the hypotheses
    const int32_t *hypCand; const float *hypR; const uint8_t *hypMask;      // hypR: [H * 13] R12 | t12 | s12
    // state
    float *xf;                  // [H * 24] sR12 | t12 | sR21 | t21
    int32_t *m12, *status, *ints, *vn1, *vn2, *bestIdx, *bestDist, *qLvl, *pairI1;
    uint8_t *alr1, *alr2, *qAct;
    float *qu, *qv, *qr;
    // OptimizeSim3's problems
    OsProb *prob; float *w1, *w2, *o1, *o2, *iv1, *iv2; uint8_t *optOut;
    unsigned *sync;             // [0] k_optsim3's arrival counter, [1] k_ls_finish's, [2..3] the word k_optsim3 publishes to
    float th2; int fixScale;
};

// form (b) of the hypotheses: model and mask of iteration rows[h] of a Sim3 solve, read where that chain left them, into the arrays form (a) stages
struct Sim3HypRow { const float *r12, *t12, *s12; const unsigned long long *mask; };
__global__ __launch_bounds__(LS_THREADS) void k_ls_from_solver(const Sim3HypRow *__restrict__ rows, const int32_t *__restrict__ hypCand, const int32_t *__restrict__ pairOf /* [K * N1] */,
                                                               int N1, float *__restrict__ hypR, uint8_t *__restrict__ mask)
{
    const int h = blockIdx.x, tid = threadIdx.x;
    const Sim3HypRow r = rows[h];
    if (tid < 9) hypR[h * 13 + tid] = r.r12[tid];
    else if (tid < 12) hypR[h * 13 + tid] = r.t12[tid - 9];
    else if (tid == 12) hypR[h * 13 + 12] = r.s12[0];
    const int32_t *po = pairOf + (size_t)hypCand[h] * N1;
    for (int j = tid; j < N1; j += LS_THREADS) {
        const int i = po[j];      // the compacted pair that sits on KF1 feature j (mvnIndices1 inverted), or -1
        mask[(size_t)h * N1 + j] = i >= 0 ? (uint8_t)((r.mask[i >> 6] >> (i & 63)) & 1ull) : 0;
    }
}

// :437-443 and src/ORBmatcher.cc:1333-1357
__global__ __launch_bounds__(LS_THREADS) void k_ls_seed(LsDev D)
{
    const int h = blockIdx.x, tid = threadIdx.x, N1 = D.N1, NP = D.NP, c = D.hypCand[h], N2 = D.kf[1 + c].n;
    for (int s = tid; s < NP; s += LS_THREADS) { D.alr1[(size_t)h * NP + s] = 0; D.alr2[(size_t)h * NP + s] = 0; }
    if (tid < LI_WORDS) D.ints[h * LI_WORDS + tid] = 0;
    if (h == 0 && tid < 4) D.sync[tid] = 0u;
    if (tid == 0) {
        D.status[h] = 0;
        const float *R = D.hypR + h * 13, *t = R + 9;
        const float s12 = R[12];
        float *X = D.xf + h * 24;
        const double inv = 1.0 / (double)s12;
        float sRinv[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) { X[3 * i + j] = s12 * R[3 * i + j]; sRinv[3 * i + j] = (float)(inv * (double)R[3 * j + i]); }      // :1333-1334
#pragma unroll
        for (int i = 0; i < 3; i++) {
            X[9 + i] = t[i];
            X[21 + i] = ((-sRinv[3 * i]) * t[0] + (-sRinv[3 * i + 1]) * t[1]) + (-sRinv[3 * i + 2]) * t[2];                                    // :1335
        }
#pragma unroll
        for (int k = 0; k < 9; k++) X[12 + k] = sRinv[k];
    }
    __syncthreads();
    for (int i = tid; i < N1; i += LS_THREADS) {
        const int b = D.hypMask[(size_t)h * N1 + i] ? D.bow[(size_t)c * N1 + i] : -1;
        D.m12[(size_t)h * N1 + i] = b;
        if (b >= 0) {
            D.alr1[(size_t)h * NP + i] = 1;
            if (b < N2) D.alr2[(size_t)h * NP + b] = 1;
        }
    }
}

// one thread per slot of list blockIdx.y = 2 h + direction.  Direction 0: KF1's points into the candidate (:1367-1411); 1: the candidate's into KF1 (:1430-1474)
__global__ __launch_bounds__(256) void k_ls_project(LsDev D, LsCam K, float th)
{
    const int p = blockIdx.y, h = p >> 1, dir = p & 1, i = blockIdx.x * 256 + threadIdx.x, NP = D.NP;
    if (i >= NP) return;
    const int c = D.hypCand[h], src = dir ? 1 + c : 0, dst = dir ? 0 : 1 + c;
    const LsKf *ks = D.kf + src, *kd = D.kf + dst;
    const size_t s = (size_t)src * NP + i, q = (size_t)p * NP + i;
    float u = 0.f, v = 0.f, radius = 0.f;
    int level = 0;
    bool ok = i < ks->n && D.valid[s] != 0 && (dir ? D.alr2 : D.alr1)[(size_t)h * NP + i] == 0;      // pMP && !vbAlreadyMatched && !isBad(), :1371-1375
    if (ok) {
        const float *X = D.pos + 3 * s, *M = D.xf + h * 24 + (dir ? 0 : 12), *tv = M + 9;
        float a[3], b[3];
#pragma unroll
        for (int r = 0; r < 3; r++) a[r] = ((ks->R[3 * r] * X[0] + ks->R[3 * r + 1] * X[1]) + ks->R[3 * r + 2] * X[2]) + ks->t[r];      // :1378
#pragma unroll
        for (int r = 0; r < 3; r++) b[r] = ((M[3 * r] * a[0] + M[3 * r + 1] * a[1]) + M[3 * r + 2] * a[2]) + tv[r];                      // :1379
        ok = !(b[2] < 0.0f);                                                                                                            // :1382
        if (ok) {
            const float invz = 1.0f / b[2];                                              // :1386 (a double quotient rounded to float: the float quotient)
            const float x = b[0] * invz, y = b[1] * invz;
            u = K.fx * x + K.cx; v = K.fy * y + K.cy;
            ok = u >= K.minX && u < K.maxX && v >= K.minY && v < K.maxY;                 // KeyFrame::IsInImage (a NaN leaves here)
        }
        if (ok) {
            const float dist = (float)sqrt((double)b[0] * (double)b[0] + (double)b[1] * (double)b[1] + (double)b[2] * (double)b[2]);   // cv::norm, :1399
            const float maxD = D.maxD[s], maxDistance = 1.2f * maxD, minDistance = 0.8f * D.minD[s];                                   // Get{Max,Min}DistanceInvariance
            ok = !(dist < minDistance || dist > maxDistance);                            // :1402
            if (ok) {
                const float ratio = maxD / dist;                                         // MapPoint::PredictScale(dist3D, pKF2), src/MapPoint.cc
                int lvl = kd->nlevels - 1;
                for (int k = kd->nlevels - 2; k >= 0; k--)
                    if (!(ratio > kd->ratioTh[k])) lvl = k;
                level = lvl;
                radius = th * kd->scale[lvl];                                            // :1411
            }
        }
    }
    D.qu[q] = ok ? u : 0.f; D.qv[q] = ok ? v : 0.f; D.qr[q] = ok ? radius : 0.f; D.qLvl[q] = ok ? level : 0; D.qAct[q] = ok ? 1 : 0;
}

// :1507-1521 and the loop of src/Optimizer.cc:1429-1520
__global__ __launch_bounds__(LS_THREADS) void k_ls_mutual(LsDev D)
{
    __shared__ int sh[LS_THREADS / 64];
    __shared__ int sFound;
    const int h = blockIdx.x, tid = threadIdx.x, N1 = D.N1, NP = D.NP, c = D.hypCand[h];
    const LsKf *k1 = D.kf, *k2 = D.kf + 1 + c;
    const int N2 = k2->n;
    const size_t l1 = (size_t)(2 * h) * NP, l2 = l1 + NP, hb = (size_t)h * NP;
    if (tid == 0) sFound = 0;
    for (int i = tid; i < NP; i += LS_THREADS) {
        D.vn1[hb + i] = (i < N1 && D.qAct[l1 + i] && D.bestDist[l1 + i] <= TH_HIGH) ? D.bestIdx[l1 + i] : -1;      // :1444
        D.vn2[hb + i] = (i < N2 && D.qAct[l2 + i] && D.bestDist[l2 + i] <= TH_HIGH) ? D.bestIdx[l2 + i] : -1;
    }
    __syncthreads();
    const size_t pb = (size_t)h * LS_MAXP;
    int base = 0, found = 0;
    for (int i0 = 0; i0 < N1; i0 += LS_THREADS) {
        const int i = i0 + tid;
        int mi = -1;
        if (i < N1) {
            mi = D.m12[(size_t)h * N1 + i];
            const int idx2 = D.vn1[hb + i];
            if (idx2 >= 0 && idx2 < N2 && D.vn2[hb + idx2] == i) { mi = idx2; D.m12[(size_t)h * N1 + i] = idx2; found++; }      // :1512-1517
        }
        const bool has = mi >= 0 && mi < N2 && D.valid[i] != 0 && D.valid[(size_t)(1 + c) * NP + mi] != 0;      // pMP1 && pMP2 && !isBad() && i2 >= 0, Optimizer.cc:1445-1447
        const int slot = block_ballot_rank<LS_THREADS>(has, &base, sh);
        if (has && slot < LS_MAXP) {
            const size_t e = pb + slot, s1 = (size_t)i, s2 = (size_t)(1 + c) * NP + mi;
            const orbx_keypoint a = D.kp[s1], b = D.kp[s2];
#pragma unroll
            for (int r = 0; r < 3; r++) { D.w1[3 * e + r] = D.pos[3 * s1 + r]; D.w2[3 * e + r] = D.pos[3 * s2 + r]; }
            D.o1[2 * e] = a.x; D.o1[2 * e + 1] = a.y; D.o2[2 * e] = b.x; D.o2[2 * e + 1] = b.y;
            D.iv1[e] = k1->invS2[min(max(a.octave, 0), k1->nlevels - 1)];
            D.iv2[e] = k2->invS2[min(max(b.octave, 0), k2->nlevels - 1)];
            D.pairI1[e] = i;
        }
    }
    found = wave_sum_dpp(found);
    if ((tid & 63) == 0 && found) atomicAdd(&sFound, found);
    __syncthreads();
    if (tid == 0) {
        const bool over = base > LS_MAXP;      // k_optsim3 holds LS_MAXP pairs: the hypothesis takes status 2 and its problem runs empty
        OsProb *P = D.prob + h;
        const float *R = D.hypR + h * 13;
#pragma unroll
        for (int j = 0; j < 9; j++) { P->rcw1[j] = k1->R[j]; P->rcw2[j] = k2->R[j]; P->r12[j] = (double)R[j]; }
#pragma unroll
        for (int j = 0; j < 3; j++) { P->tcw1[j] = k1->t[j]; P->tcw2[j] = k2->t[j]; P->t12[j] = (double)R[9 + j]; }
#pragma unroll
        for (int j = 0; j < 4; j++) { P->k1[j] = k1->k[j]; P->k2[j] = k2->k[j]; }
        P->s12 = (double)R[12];
        P->th2 = D.th2; P->n = over ? 0 : base; P->fixScale = D.fixScale; P->mb = (int32_t)pb;
        P->outOff = (unsigned long long)h * OsBlock(LS_MAXP).total;
        D.ints[h * LI_WORDS + LI_NFOUND] = sFound;
        D.ints[h * LI_WORDS + LI_NPAIRS] = base;
        if (over) D.status[h] = 2;
    }
}

struct LsOut { int32_t *ints; double *est; float *scw; int32_t *matches; int32_t *pick; };      // mapped host memory; pick: winner, candidate, overflow met

__global__ __launch_bounds__(256) void k_ls_finish(LsDev D, LsOut O, unsigned long long *pubFlag, unsigned long long pubSeq)
{
    __shared__ int sLast, sWin;
    const int h = blockIdx.x, tid = threadIdx.x, N1 = D.N1, c = D.hypCand[h];
    const OsProb *P = D.prob + h;
    const int n = P->n;
    const uint8_t *blk = D.optOut + P->outOff;
    const OsBlock L(n);
    const int32_t *head = (const int32_t *)blk;
    const uint8_t *remFirst = blk + L.remFirst, *remFinal = blk + L.remFinal;
    for (int k = tid; k < n; k += 256)
        if (remFirst[k] || remFinal[k]) D.m12[(size_t)h * N1 + D.pairI1[(size_t)h * LS_MAXP + k]] = -1;      // src/Optimizer.cc:1541 / :1578
    if (tid == 0) {
        const double *est = (const double *)(blk + L.est);
        const int over = D.status[h] == 2, nIn = over ? 0 : head[0], nBad = over ? 0 : head[1];
        OsSim3 gScm, gSmw, S;
#pragma unroll
        for (int j = 0; j < 4; j++) gScm.q[j] = est[j];
#pragma unroll
        for (int j = 0; j < 3; j++) gScm.t[j] = est[4 + j];
        gScm.s = est[7];
        const LsKf *k2 = D.kf + 1 + c;
        double Rm[9];
#pragma unroll
        for (int j = 0; j < 9; j++) Rm[j] = (double)k2->R[j];
        os_quat_from_R(Rm, gSmw.q);                                                    // g2o::Sim3(toMatrix3d(Rcw), toVector3d(tcw), 1.0), :469
#pragma unroll
        for (int j = 0; j < 3; j++) gSmw.t[j] = (double)k2->t[j];
        gSmw.s = 1.0;
        os_mul(gScm, gSmw, S);                                                         // :471
        double Rs[9];
        os_quat_to_R(S.q, Rs);
        float *scw = O.scw + 16 * h;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int j = 0; j < 3; j++) scw[4 * r + j] = (float)(S.s * Rs[3 * r + j]);     // Converter::toCvMat(g2o::Sim3): toCvSE3(s * R, t)
            scw[4 * r + 3] = (float)S.t[r];
            scw[12 + r] = 0.f;
        }
        scw[15] = 1.f;
        const int st = over ? 2 : (nIn >= 20 ? 1 : 0);                                 // :463
        D.status[h] = st;
        int32_t *I = O.ints + h * LI_WORDS;
        I[LI_STATUS] = st; I[LI_NFOUND] = D.ints[h * LI_WORDS + LI_NFOUND]; I[LI_NPAIRS] = D.ints[h * LI_WORDS + LI_NPAIRS]; I[LI_NIN] = nIn; I[LI_NBAD] = nBad;
#pragma unroll
        for (int j = 0; j < 8; j++) O.est[8 * h + j] = est[j];
    }
    // arrival: an agent-scope release per workgroup behind its stores, the last one acquires (the form of orbx_publish)
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        sLast = __hip_atomic_fetch_add(D.sync + 1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1 : 0;
    }
    __syncthreads();
    if (!sLast) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // every wave reads what the other workgroups stored
    if (tid == 0) {
        __hip_atomic_store(D.sync + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int win = -1, over = 0;
        for (int k = 0; k < D.H; k++) {                      // the walk of :403-482 over the events in the order given
            const int st = D.status[k];
            if (st == 1) { win = k; break; }
            if (st == 2) { over = 1; break; }
        }
        sWin = win;
        O.pick[0] = win; O.pick[1] = win >= 0 ? D.hypCand[win] : -1; O.pick[2] = over;
    }
    __syncthreads();
    const int win = sWin;
    for (int i = tid; i < N1; i += 256) O.matches[i] = win >= 0 ? D.m12[(size_t)win * N1 + i] : -1;      // mvpCurrentMatchedPoints, :474
    orbx_publish(nullptr, pubFlag, pubSeq, 1u);
}

struct LsSlots {      // the device working arrays of one call, planned once per call into m->lsWork
    OrbxSlot<int32_t, ORBX_STAGE_WORK> m12, status, ints, vn1, vn2, bestIdx, bestDist, qLvl, pairI1;
    OrbxSlot<uint8_t, ORBX_STAGE_WORK> alr1, alr2, qAct, solMask, optOut;
    OrbxSlot<float, ORBX_STAGE_WORK> xf, qu, qv, qr, solR, w1, w2, o1, o2, iv1, iv2;
    OrbxSlot<OsProb, ORBX_STAGE_WORK> prob;
    OrbxSlot<unsigned, ORBX_STAGE_WORK> sync;
    uint8_t *base = nullptr;
    int plan(orbx_matcher *m, size_t H, size_t N1, size_t NP, bool fromSolver)
    {
        OrbxWorkPlan &wp = m->lsPlan;
        wp.reset();
        m12 = wp.hole<int32_t>(H * N1); status = wp.hole<int32_t>(H); ints = wp.hole<int32_t>(H * LI_WORDS); vn1 = wp.hole<int32_t>(H * NP); vn2 = wp.hole<int32_t>(H * NP);
        bestIdx = wp.hole<int32_t>(2 * H * NP); bestDist = wp.hole<int32_t>(2 * H * NP); qLvl = wp.hole<int32_t>(2 * H * NP); pairI1 = wp.hole<int32_t>(H * LS_MAXP);
        alr1 = wp.hole<uint8_t>(H * NP); alr2 = wp.hole<uint8_t>(H * NP); qAct = wp.hole<uint8_t>(2 * H * NP);
        solMask = wp.hole<uint8_t>(fromSolver ? H * N1 : 0); optOut = wp.hole<uint8_t>(H * OsBlock(LS_MAXP).total);
        xf = wp.hole<float>(H * 24); qu = wp.hole<float>(2 * H * NP); qv = wp.hole<float>(2 * H * NP); qr = wp.hole<float>(2 * H * NP);
        solR = wp.hole<float>(fromSolver ? H * 13 : 0);
        w1 = wp.hole<float>(H * LS_MAXP * 3); w2 = wp.hole<float>(H * LS_MAXP * 3); o1 = wp.hole<float>(H * LS_MAXP * 2); o2 = wp.hole<float>(H * LS_MAXP * 2);
        iv1 = wp.hole<float>(H * LS_MAXP); iv2 = wp.hole<float>(H * LS_MAXP);
        prob = wp.hole<OsProb>(H); sync = wp.hole<unsigned>(4);
        const int rc = m->lsWork.ensure(wp.total());
        base = m->lsWork.p;
        return rc;
    }
};

int check_keyframe(const orbx_loop_sim3_keyframe *k, const char *what, int idx, bool needBow)
{
    if (!k->frame.counts) { orbx_set_error("NULL counts of %s %d", what, idx); return ORBX_ERR_ARG; }
    if (!k->scale_factors || !k->ratio_thresholds || !k->inv_level_sigma2 || k->nlevels < 1 || k->nlevels > ORBX_MAX_LEVELS) {
        orbx_set_error("bad scale tables of %s %d (%d levels, 1..%d)", what, idx, k->nlevels, ORBX_MAX_LEVELS);
        return ORBX_ERR_ARG;
    }
    if (k->frame.counts[0] < 1) { orbx_set_error("%s %d has no slots", what, idx); return ORBX_ERR_ARG; }
    if (!k->frame.keypoints_un || !k->frame.descriptors || !k->valid || !k->world_pos || !k->max_distance || !k->min_distance || !k->descriptors || (needBow && !k->bow_match)) {
        orbx_set_error("NULL array in %s %d", what, idx);
        return ORBX_ERR_ARG;
    }
    return ORBX_OK;
}

void fill_kf(LsKf &o, const orbx_loop_sim3_keyframe *k)
{
    memcpy(o.R, k->rcw, 36); memcpy(o.t, k->tcw, 12);
    o.k[0] = k->fx; o.k[1] = k->fy; o.k[2] = k->cx; o.k[3] = k->cy;
    o.n = k->frame.counts[0]; o.nlevels = k->nlevels;
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) {
        o.ratioTh[l] = l + 1 < k->nlevels ? k->ratio_thresholds[l] : 0.0f;
        o.scale[l] = l < k->nlevels ? k->scale_factors[l] : 0.0f;
        o.invS2[l] = l < k->nlevels ? k->inv_level_sigma2[l] : 0.0f;
    }
}

}  // namespace

extern "C" int orbx_loop_refine_sim3(orbx_matcher *m, const orbx_loop_sim3_keyframe *kf1, const orbx_loop_sim3_keyframe *cands, int ncands, const orbx_loop_sim3_hypotheses *hyp,
                                     float th, float th2, int fix_scale, orbx_loop_refine_result *res)
{
    if (!m || !kf1 || !cands || !hyp || !res) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = check_keyframe(kf1, "keyframe", 1, false)) != ORBX_OK) return rc;
    const int n1 = kf1->frame.counts[0], H = hyp->count, K = ncands;
    if (K < 1 || H < 1) { orbx_set_error("empty problem (candidates %d, hypotheses %d)", K, H); return ORBX_ERR_ARG; }
    if (!std::isfinite(th) || !std::isfinite(th2) || th2 < 0.f) { orbx_set_error("th = %g, th2 = %g", (double)th, (double)th2); return ORBX_ERR_ARG; }
    const bool fromSolver = hyp->solver != nullptr;
    if (!hyp->candidate || (fromSolver ? (!hyp->iteration || !hyp->index1 || !hyp->index1_count) : (!hyp->r12 || !hyp->t12 || !hyp->s12 || !hyp->inliers))) {
        orbx_set_error("NULL array in the hypotheses");
        return ORBX_ERR_ARG;
    }
    if (H > ORBX_LOOP_SIM3_MAX_HYPOTHESES) { orbx_set_error("%d hypotheses exceed %d", H, ORBX_LOOP_SIM3_MAX_HYPOTHESES); return ORBX_ERR_CAPACITY; }
    if (K > m->maxPairs) { orbx_set_error("%d candidates exceed the matcher's max_pairs %d", K, m->maxPairs); return ORBX_ERR_CAPACITY; }
    if (n1 > m->maxFeatures || n1 > 65535) { orbx_set_error("%d slots exceed the matcher's max_features %d", n1, m->maxFeatures); return ORBX_ERR_CAPACITY; }
    int maxN = n1;
    for (int c = 0; c < K; c++) {
        const orbx_loop_sim3_keyframe *k = cands + c;
        if ((rc = check_keyframe(k, "candidate", c, true)) != ORBX_OK) return rc;
        const int n2 = k->frame.counts[0];
        if (n2 > m->maxFeatures || n2 > 65535) { orbx_set_error("%d slots exceed the matcher's max_features %d", n2, m->maxFeatures); return ORBX_ERR_CAPACITY; }
        if (k->frame.min_x != kf1->frame.min_x || k->frame.min_y != kf1->frame.min_y || k->frame.grid_width_inv != kf1->frame.grid_width_inv ||
            k->frame.grid_height_inv != kf1->frame.grid_height_inv || k->min_x != kf1->min_x || k->max_x != kf1->max_x || k->min_y != kf1->min_y || k->max_y != kf1->max_y) {
            orbx_set_error("candidate %d: grid statics or image bounds differ from the keyframe's", c);
            return ORBX_ERR_ARG;
        }
        for (int j = 0; j < n1; j++)
            if (k->bow_match[j] < -1 || k->bow_match[j] >= n2) { orbx_set_error("bow_match[%d] = %d of candidate %d outside -1..%d", j, k->bow_match[j], c, n2 - 1); return ORBX_ERR_ARG; }
        maxN = std::max(maxN, n2);
    }
    const size_t N1 = (size_t)n1, NP = (size_t)maxN, HH = (size_t)H, KK = (size_t)K;
    for (int h = 0; h < H; h++)
        if (hyp->candidate[h] < 0 || hyp->candidate[h] >= K) { orbx_set_error("hypothesis %d names candidate %d of %d", h, hyp->candidate[h], K); return ORBX_ERR_ARG; }
    // form (b): where the Sim3 chain left each hypothesis' iteration, and per named candidate the compacted pair that sits on each KF1 feature
    std::vector<Sim3HypRow> rows;
    std::vector<int32_t> pairOf;
    if (fromSolver) {
        rows.resize(HH);
        pairOf.assign(KK * N1, -1);
        std::vector<char> done(KK, 0);
        for (int h = 0; h < H; h++) {
            const int c = hyp->candidate[h];
            OrbxSim3Rows sr;
            if ((rc = orbx_sim3_device_rows_internal(hyp->solver, c, m->device, &sr)) != ORBX_OK) return rc;
            const int it = hyp->iteration[h];
            if (it < 0 || it >= sr.iters) { orbx_set_error("hypothesis %d names iteration %d of candidate %d, which ran %d", h, it, c, sr.iters); return ORBX_ERR_ARG; }
            rows[(size_t)h] = Sim3HypRow{sr.r12 + 9 * (size_t)it, sr.t12 + 3 * (size_t)it, sr.s12 + it, sr.mask + (size_t)it * sr.words};
            if (done[(size_t)c]) continue;
            done[(size_t)c] = 1;
            if (hyp->index1_count[c] != sr.n || (sr.n > 0 && !hyp->index1[c])) {
                orbx_set_error("index1 of candidate %d has %d entries, the Sim3 solve had %d pairs", c, hyp->index1_count[c], sr.n);
                return ORBX_ERR_ARG;
            }
            for (int i = 0; i < sr.n; i++) {
                const int j = hyp->index1[c][i];
                if (j < 0 || j >= n1 || pairOf[(size_t)c * N1 + j] >= 0) { orbx_set_error("index1[%d][%d] = %d is outside 0..%d or names a feature twice", c, i, j, n1 - 1); return ORBX_ERR_ARG; }
                pairOf[(size_t)c * N1 + j] = i;
            }
        }
    }
    int nValid1 = 0;      // the pairs of a hypothesis sit on valid KF1 slots: the host's bound for k_optsim3's instantiation
    for (int j = 0; j < n1; j++) nValid1 += kf1->valid[j] ? 1 : 0;
    const int pairBound = std::max(1, std::min(nValid1, LS_MAXP));
    std::vector<LsKf> kfs(KK + 1);
    std::vector<int32_t> cnt(KK + 1), frameOf(2 * HH), descOf(2 * HH), pcnt(2 * HH);
    fill_kf(kfs[0], kf1);
    cnt[0] = n1;
    for (int c = 0; c < K; c++) { fill_kf(kfs[(size_t)c + 1], cands + c); cnt[(size_t)c + 1] = cands[c].frame.counts[0]; }
    for (int h = 0; h < H; h++) {
        const int c = hyp->candidate[h];
        frameOf[2 * (size_t)h] = 1 + c; descOf[2 * (size_t)h] = 0; pcnt[2 * (size_t)h] = n1;
        frameOf[2 * (size_t)h + 1] = 0; descOf[2 * (size_t)h + 1] = 1 + c; pcnt[2 * (size_t)h + 1] = cnt[(size_t)c + 1];
    }
    ORBX_HIP_CHECK(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    OrbxCallBox &bx = m->box;
    const size_t F = KK + 1;
    auto [pin, pout] = bx.plan();
    const auto sKf = pin.add(kfs.data(), F);
    const auto sCnt = pin.add(cnt.data(), F);
    const auto sFrameOf = pin.add(frameOf.data(), 2 * HH), sDescOf = pin.add(descOf.data(), 2 * HH), sPcnt = pin.add(pcnt.data(), 2 * HH);
    const auto sHc = pin.add(hyp->candidate, HH);
    const auto sKp = pin.hole<orbx_keypoint>(F * NP);
    const auto sDesc = pin.hole<uint8_t>(F * NP * 32), sPd = pin.hole<uint8_t>(F * NP * 32), sVal = pin.hole<uint8_t>(F * NP);
    const auto sPos = pin.hole<float>(F * NP * 3), sMax = pin.hole<float>(F * NP), sMin = pin.hole<float>(F * NP);
    const auto sBow = pin.hole<int32_t>(KK * N1);
    const auto sHr = pin.hole<float>(fromSolver ? 0 : HH * 13);
    const auto sMask = pin.add(hyp->inliers, fromSolver ? 0 : HH * N1);
    const auto sRows = pin.add(rows.data(), fromSolver ? HH : 0);
    const auto sPairOf = pin.add(pairOf.data(), fromSolver ? KK * N1 : 0);
    const auto rInts = pout.hole<int32_t>(HH * LI_WORDS);
    const auto rEst = pout.hole<double>(HH * 8);
    const auto rScw = pout.hole<float>(HH * 16);
    const auto rMat = pout.hole<int32_t>(N1);
    const auto rPick = pout.hole<int32_t>(4);
    const OrbxStaged sg = bx.begin(st, &rc);
    if (rc != ORBX_OK) return rc;
    for (size_t f = 0; f < F; f++) {
        const orbx_loop_sim3_keyframe *k = f ? cands + (f - 1) : kf1;
        const size_t b = f * NP, n = (size_t)cnt[f];
        orbx_put_at(sg, sKp, b, k->frame.keypoints_un, n); orbx_put_at(sg, sDesc, b * 32, k->frame.descriptors, n * 32); orbx_put_at(sg, sPd, b * 32, k->descriptors, n * 32);
        orbx_put_at(sg, sVal, b, k->valid, n); orbx_put_at(sg, sPos, b * 3, k->world_pos, n * 3); orbx_put_at(sg, sMax, b, k->max_distance, n); orbx_put_at(sg, sMin, b, k->min_distance, n);
        if (f) orbx_put_at(sg, sBow, (f - 1) * N1, k->bow_match, N1);
    }
    if (!fromSolver)
        for (int h = 0; h < H; h++) {
            float *r = sg.host(sHr) + 13 * (size_t)h;
            memcpy(r, hyp->r12 + 9 * (size_t)h, 36); memcpy(r + 9, hyp->t12 + 3 * (size_t)h, 12); r[12] = hyp->s12[h];
        }
    LsSlots w;
    if ((rc = w.plan(m, HH, N1, NP, fromSolver)) != ORBX_OK) return rc;
    if ((rc = m->lsTimer.create()) != ORBX_OK) return rc;
    if ((rc = orbx_match::track_mark(m, st, 0)) != ORBX_OK) return rc;
    if ((rc = m->lsTimer.begin(st)) != ORBX_OK) return rc;
    uint8_t *ar;
    if ((rc = orbx_stage_to_arena(bx, m->arena, st, 512, &ar)) != ORBX_OK) return rc;
    ORBX_LAUNCH_COUNT(m->lsTimer);
    if ((rc = orbx_match::track_mark(m, st, 1)) != ORBX_OK) return rc;
    uint8_t *wb = w.base;
    LsDev D;
    D.H = H; D.NP = maxN; D.N1 = n1;
    D.kf = sKf.in(ar); D.kp = sKp.in(ar); D.valid = sVal.in(ar); D.pos = sPos.in(ar); D.maxD = sMax.in(ar); D.minD = sMin.in(ar); D.bow = sBow.in(ar);
    D.hypCand = sHc.in(ar); D.hypR = sHr.in(ar); D.hypMask = sMask.in(ar);
    D.xf = w.xf.in(wb); D.m12 = w.m12.in(wb); D.status = w.status.in(wb); D.ints = w.ints.in(wb); D.vn1 = w.vn1.in(wb); D.vn2 = w.vn2.in(wb);
    D.bestIdx = w.bestIdx.in(wb); D.bestDist = w.bestDist.in(wb); D.qLvl = w.qLvl.in(wb); D.pairI1 = w.pairI1.in(wb);
    D.alr1 = w.alr1.in(wb); D.alr2 = w.alr2.in(wb); D.qAct = w.qAct.in(wb); D.qu = w.qu.in(wb); D.qv = w.qv.in(wb); D.qr = w.qr.in(wb);
    D.prob = w.prob.in(wb); D.w1 = w.w1.in(wb); D.w2 = w.w2.in(wb); D.o1 = w.o1.in(wb); D.o2 = w.o2.in(wb); D.iv1 = w.iv1.in(wb); D.iv2 = w.iv2.in(wb);
    D.optOut = w.optOut.in(wb); D.sync = w.sync.in(wb);
    D.th2 = th2; D.fixScale = fix_scale ? 1 : 0;
    const dim3 gH((unsigned)H);
    if (fromSolver) {
        D.hypR = w.solR.in(wb); D.hypMask = w.solMask.in(wb);
        hipLaunchKernelGGL(k_ls_from_solver, gH, dim3(LS_THREADS), 0, st, sRows.in(ar), D.hypCand, sPairOf.in(ar), n1, w.solR.in(wb), w.solMask.in(wb));
        ORBX_LAUNCH_COUNT(m->lsTimer);
    }
    hipLaunchKernelGGL(k_ls_seed, gH, dim3(LS_THREADS), 0, st, D);
    ORBX_LAUNCH_COUNT(m->lsTimer);
    if ((rc = orbx_match::track_mark(m, st, 2)) != ORBX_OK) return rc;
    const LsCam Kc = {kf1->fx, kf1->fy, kf1->cx, kf1->cy, kf1->min_x, kf1->max_x, kf1->min_y, kf1->max_y};
    hipLaunchKernelGGL(k_ls_project, dim3((unsigned)((maxN + 255) / 256), (unsigned)(2 * H)), dim3(256), 0, st, D, Kc, th);
    ORBX_LAUNCH_COUNT(m->lsTimer);
    if ((rc = orbx_match::track_mark(m, st, 3)) != ORBX_OK) return rc;
    {
        ProjFrameDev Fd = {sKp.in(ar), sDesc.in(ar), nullptr, nullptr, sCnt.in(ar), maxN, kf1->frame.min_x, kf1->frame.min_y, kf1->frame.grid_width_inv, kf1->frame.grid_height_inv,
                           sFrameOf.in(ar)};
        FusePointsDev Pd = {D.qu, D.qv, nullptr, D.qLvl, D.qr, D.qAct, sPd.in(ar), sPcnt.in(ar), maxN, kf1->min_x, kf1->min_y, sDescOf.in(ar)};
        FuseLevels LV;
        for (int l = 0; l < ORBX_MAX_LEVELS; l++) LV.invSigma2[l] = 0.0f;      // (read under chi2_gate only)
        orbx_match::launch_fuse_best_lists(st, Fd, Pd, LV, 2 * H, D.bestIdx, D.bestDist);
        ORBX_LAUNCH_COUNT(m->lsTimer);
    }
    if ((rc = orbx_match::track_mark(m, st, 4)) != ORBX_OK) return rc;
    hipLaunchKernelGGL(k_ls_mutual, gH, dim3(LS_THREADS), 0, st, D);
    ORBX_LAUNCH_COUNT(m->lsTimer);
    if ((rc = orbx_match::track_mark(m, st, 5)) != ORBX_OK) return rc;
    {
        OsIn I;
        I.prob = D.prob; I.world1 = D.w1; I.world2 = D.w2; I.obs1 = D.o1; I.obs2 = D.o2; I.inv1 = D.iv1; I.inv2 = D.iv2; I.active = nullptr;
        memset(&I.lin, 0, sizeof(I.lin));
        orbx_optsim3_enqueue(st, I, D.optOut, H, pairBound, D.sync, (unsigned long long *)(D.sync + 2), 1ull);
        ORBX_LAUNCH_COUNT(m->lsTimer);
    }
    if ((rc = orbx_match::track_mark(m, st, 6)) != ORBX_OK) return rc;
    const LsOut O = {sg.dev(rInts), sg.dev(rEst), sg.dev(rScw), sg.dev(rMat), sg.dev(rPick)};
    const unsigned long long seq = bx.arm();
    hipLaunchKernelGGL(k_ls_finish, gH, dim3(256), 0, st, D, O, bx.flagDev, seq);
    ORBX_LAUNCH_COUNT(m->lsTimer);
    if ((rc = orbx_match::track_mark(m, st, 7)) != ORBX_OK) return rc;
    if ((rc = m->lsTimer.end(st)) != ORBX_OK) return rc;
    if ((rc = bx.wait(st)) != ORBX_OK) return rc;      // the one synchronisation
    const int32_t *hi = sg.host(rInts), *pk = sg.host(rPick);
    const double *he = sg.host(rEst);
    for (int h = 0; h < H; h++) {
        const int32_t *I = hi + h * LI_WORDS;
        if (res->status) res->status[h] = I[LI_STATUS];
        if (res->n_found) res->n_found[h] = I[LI_NFOUND];
        if (res->n_pairs) res->n_pairs[h] = I[LI_NPAIRS];
        if (res->n_inliers) res->n_inliers[h] = I[LI_NIN];
        if (res->n_bad) res->n_bad[h] = I[LI_NBAD];
        if (res->quat) memcpy(res->quat + 4 * (size_t)h, he + 8 * (size_t)h, 32);
        if (res->t) memcpy(res->t + 3 * (size_t)h, he + 8 * (size_t)h + 4, 24);
        if (res->s) res->s[h] = he[8 * (size_t)h + 7];
    }
    if (res->scw) memcpy(res->scw, sg.host(rScw), HH * 64);
    if (res->matches12) memcpy(res->matches12, sg.host(rMat), N1 * 4);
    res->winner = pk[0]; res->hypothesis = pk[0]; res->candidate = pk[1];
    if (res->query_u || res->query_v || res->query_radius || res->query_level || res->query_active || res->match1 || res->match2) {
        // the per-slot arrays (tests, diagnostics): copies of their own
        ORBX_HIP_CHECK(hipStreamSynchronize(st));
#define LS_DL(dst, src, count) if (dst) ORBX_HIP_CHECK(hipMemcpy((dst), (src), (count) * sizeof(*(src)), hipMemcpyDeviceToHost))
        LS_DL(res->query_u, D.qu, 2 * HH * NP); LS_DL(res->query_v, D.qv, 2 * HH * NP); LS_DL(res->query_radius, D.qr, 2 * HH * NP);
        LS_DL(res->query_level, D.qLvl, 2 * HH * NP); LS_DL(res->query_active, D.qAct, 2 * HH * NP);
        LS_DL(res->match1, D.vn1, HH * NP); LS_DL(res->match2, D.vn2, HH * NP);
#undef LS_DL
    }
    if (pk[2]) {
        orbx_set_error("a hypothesis ahead of any winner gathered more than %d pairs (status 2)", LS_MAXP);
        return ORBX_ERR_CAPACITY;
    }
    return ORBX_OK;
}

extern "C" int orbx_loop_sim3_last_timing(orbx_matcher *m, float *device_ms, int *launches)
{
    if (!m) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    return m->lsTimer.read(m->device, device_ms, launches, "no orbx_loop_refine_sim3 call to report");
}
