// orbx_fuse_chain.hip -- steps 2 and 3 of LocalMapping::SearchInNeighbors (reference src/LocalMapping.cc:666-713): the T + 1 complete calls of
// ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:1020-1174) as one chain on the matcher's stream.  gfx950 only.
//
// What couples the calls lives on the device between them: isBad, mvpMapPoints of the searchable keyframes (kf_point, mutated inside the
// arena), Observations(), found / visible, the descriptor that Replace -> ComputeDistinctiveDescriptors rewrites, and the observation maps.
// An observation map is a singly linked list of nodes (keyframe slot, feature, next, stereo) kept in ascending rank: std::map<KeyFrame*, size_t>
// iterates that way, Replace walks it that way, and a node never moves - Replace relinks the loser's nodes into the winner's list, an added
// observation takes a node that a conflict erase freed, else a fresh one.  Nodes in use: at most the slice's observations + one per empty feature
// of a searchable keyframe (an add fills an empty feature, an erase empties one and frees its node).
//
//   k_fc_init      the lists from the CSR observations, Observations(), the counters
//   per Fuse call (keyframe k, list):
//     k_fc_prepare   a thread per list entry: skip -1 / bad / observed by k, the gates and values of :1040-1086, the entry's descriptor
//     k_fuse_best    (orbx_match_proj.hip) the search, chi2_gate = 1; the list's length is read on the device
//     k_fc_apply     ONE workgroup walks the list in order.  256 entries at a time are tested for bestDist <= TH_LOW and the walk jumps from
//                    decision to decision by ballot; per decision all lanes scan kf_point[k] for the re-check "entered k meanwhile", lane 0
//                    relinks the lists (a merge of two rank-ordered lists: the conflict "both observed by one keyframe" is an equal rank), and
//                    all lanes take the winner's new descriptor (row i per thread, the median by a 9-step bisection on the value, the
//                    arg-min by a workgroup minimum of median << 32 | i).  Sequential by definition: bounded by the decisions of a call
//                    times the length of the lists they touch; an entry without a decision costs 1/256 of a ballot round.
//   k_fc_mark / k_fc_gather   the candidates of the reverse pass: first occurrence of every held, good point over (target, feature) by an
//                    atomic minimum of the position, then an ordered compaction by one workgroup
//   k_fc_export    the final state into mapped host memory (observations back as CSR in ascending rank), then the sequence word
//
// Arithmetic of k_fc_prepare: the reference's on the project's OpenCV stand-in (oracle/cvshim): Rcw * p + tcw left to right in float, cv::norm
// and Mat::dot accumulated in double, the viewing gate a double comparison, PredictScale by the ratio thresholds of
// orbx_predict_scale_thresholds (no device logarithm).  -ffp-contract=off: every product and sum is its own operation.
#include <algorithm>
#include <climits>
#include <numeric>
#include <vector>

#include "orbx_match_internal.h"

#define FC_THREADS 256
#define FC_LDS_DESC 512      /* descriptors of a recomputed point held in LDS (16 KB); longer lists are read from memory */

namespace {

struct FcKf {
    unsigned long long kp, desc, ur, kfp;      // byte offsets inside the arena
    float tcw[12], ow[3];
    float fx, fy, cx, cy, mbf;
    float gMinX, gMinY, gwInv, ghInv;
    float minX, maxX, minY, maxY;              // (float) of the KeyFrame's int bounds
    float th;
    float sf[ORBX_MAX_LEVELS], invS2[ORBX_MAX_LEVELS], ratioTh[ORBX_MAX_LEVELS];
    int n, nlevels, slot, featBase;
};

struct FcDev {
    uint8_t *A;                                // the arena: the staged slice; kf_point, ptBad, ptDesc, visible and found are mutated in place
    const FcKf *kfs;
    const int32_t *pos, *sIndex;               // [NK] slot -> position in ascending rank; slot -> searchable index or -1
    const uint8_t *kfBad;
    int NK, S, P, T0, nodeCap;
    const float *ppos, *pnormal, *minD, *maxD, *rawMax;
    uint8_t *ptDesc, *ptBad;
    int32_t *visible, *found;
    const int32_t *obsOff, *obsKf, *obsIdx;
    const uint8_t *obsSt, *obsDesc;
    int4 *node;                                // x keyframe slot, y feature, z next, w bit 0 stereo, bit 1 added by this call (its descriptor is the keyframe's)
    int32_t *head, *nobs, *replaced, *firstPos, *listBuf, *counters, *cand;
    // results, mapped host memory
    orbx_fuse_decision *log;
    int32_t *oNfused, *oCounts, *oCand, *oKfp;
    uint8_t *oBad;
    int32_t *oReplaced, *oNobs, *oVisible, *oFound;
    uint8_t *oDesc;
    int32_t *oObsOff, *oObsKf, *oObsIdx;
    uint8_t *oObsSt;
};
enum { FC_NODES = 0, FC_LOG = 1, FC_CAND = 2, FC_FREE = 3 };      // counters: nodes handed out, decisions logged, candidates, head of the free nodes

struct FcCall { uint8_t *act; float *u, *v, *ur, *radius; int32_t *level, *bestIdx, *bestDist; uint8_t *desc; };

__device__ __forceinline__ int32_t *fc_kfp(const FcDev &D, const FcKf &K) { return (int32_t *)(D.A + K.kfp); }
__device__ __forceinline__ const uint32_t *fc_node_desc(const FcDev &D, int nd, const int4 &v)
{
    if (!(v.w & 2)) return (const uint32_t *)(D.obsDesc + (size_t)nd * 32);      // a node of the slice keeps its number: the observation's
    return (const uint32_t *)(D.A + D.kfs[D.sIndex[v.x]].desc + (size_t)v.y * 32);      // an added observation: always of a searchable keyframe
}

__global__ __launch_bounds__(FC_THREADS) void k_fc_init(FcDev D)
{
    const int p = blockIdx.x * FC_THREADS + threadIdx.x;
    if (p == 0) { D.counters[FC_NODES] = D.T0; D.counters[FC_LOG] = 0; D.counters[FC_CAND] = 0; D.counters[FC_FREE] = -1; }
    if (p >= D.P) return;
    const int o0 = D.obsOff[p], o1 = D.obsOff[p + 1];
    int s = 0;
    for (int o = o0; o < o1; o++) {
        const int st = D.obsSt[o] ? 1 : 0;
        D.node[o] = make_int4(D.obsKf[o], D.obsIdx[o], o + 1 < o1 ? o + 1 : -1, st);
        s += st ? 2 : 1;
    }
    D.head[p] = o1 > o0 ? o0 : -1;
    D.nobs[p] = s; D.replaced[p] = -1; D.firstPos[p] = INT_MAX;
}

// cv::Mat::dot / cv::norm of 3-vectors: products and sums in double
__device__ __forceinline__ double fc_dot3(const float (&a)[3], const float (&b)[3])
{
    double s = (double)a[0] * (double)b[0];
    s = s + (double)a[1] * (double)b[1];
    s = s + (double)a[2] * (double)b[2];
    return s;
}

__global__ __launch_bounds__(FC_THREADS) void k_fc_prepare(FcDev D, FcCall C, int s, const int32_t *list, const int32_t *lenPtr, int lenCap)
{
    const int i = blockIdx.x * FC_THREADS + threadIdx.x;
    const int L = min(*lenPtr, lenCap);
    if (i >= L) return;
    const FcKf &K = D.kfs[s];
    const int p = list[i];
    bool act = false;
    float u = 0.f, v = 0.f, ur = 0.f, radius = 0.f;
    int lvl = 0;
    if (p >= 0 && !D.ptBad[p]) {
        bool in = false;
        for (int nd = D.head[p]; nd >= 0;) { const int4 nv = D.node[nd]; in = in || nv.x == K.slot; nd = nv.z; }
        if (!in) {
            const float Pw[3] = {D.ppos[3 * (size_t)p], D.ppos[3 * (size_t)p + 1], D.ppos[3 * (size_t)p + 2]};
            const float Pn[3] = {D.pnormal[3 * (size_t)p], D.pnormal[3 * (size_t)p + 1], D.pnormal[3 * (size_t)p + 2]};
            float Pc[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                float t = K.tcw[4 * r] * Pw[0];
                t = t + K.tcw[4 * r + 1] * Pw[1];
                t = t + K.tcw[4 * r + 2] * Pw[2];
                Pc[r] = t + K.tcw[4 * r + 3];                                            // Rcw*p3Dw + tcw, :1049
            }
            if (!(Pc[2] < 0.0f)) {                                                       // :1052
                const float invz = 1.0f / Pc[2];
                const float x = Pc[0] * invz, y = Pc[1] * invz;
                u = K.fx * x + K.cx; v = K.fy * y + K.cy;
                if (u >= K.minX && u < K.maxX && v >= K.minY && v < K.maxY) {            // KeyFrame::IsInImage
                    ur = u - K.mbf * invz;
                    const float PO[3] = {Pw[0] - K.ow[0], Pw[1] - K.ow[1], Pw[2] - K.ow[2]};
                    const float dist3D = (float)sqrt(fc_dot3(PO, PO));                   // cv::norm, :1071
                    if (!(dist3D < D.minD[p] || dist3D > D.maxD[p]) && !(fc_dot3(PO, Pn) < 0.5 * (double)dist3D)) {      // :1074, :1080
                        const float ratio = D.rawMax[p] / dist3D;                        // MapPoint::PredictScale, src/MapPoint.cc:551-569
                        lvl = K.nlevels - 1;
                        for (int k = K.nlevels - 2; k >= 0; k--)
                            if (!(ratio > K.ratioTh[k])) lvl = k;
                        radius = K.th * K.sf[lvl];
                        act = true;
                    }
                }
            }
        }
    }
    C.act[i] = act ? 1 : 0;
    C.u[i] = u; C.v[i] = v; C.ur[i] = ur; C.level[i] = lvl; C.radius[i] = radius;
    uint4 *dst = (uint4 *)(C.desc + (size_t)i * 32);
    uint4 d0 = {0u, 0u, 0u, 0u}, d1 = d0;
    if (p >= 0) { const uint4 *src = (const uint4 *)(D.ptDesc + (size_t)p * 32); d0 = src[0]; d1 = src[1]; }
    dst[0] = d0; dst[1] = d1;
}

__device__ __forceinline__ int fc_dist(const uint32_t (&a)[8], const uint32_t *b)
{
    int d = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) d += __popc(a[w] ^ b[w]);
    return d;
}

// ONE workgroup.  Every branch below is uniform: its condition is read by all threads from the same words behind a barrier.
__global__ __launch_bounds__(FC_THREADS) void k_fc_apply(FcDev D, int call, int s, const int32_t *list, const int32_t *lenPtr, int lenCap, const uint8_t *act,
                                                         const int32_t *bestIdx, const int32_t *bestDist)
{
    __shared__ unsigned long long sMask[FC_THREADS / 64], sKey[FC_THREADS / 64];
    __shared__ int sN, sAny;
    __shared__ __attribute__((aligned(16))) uint32_t sDesc[FC_LDS_DESC * 8];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const FcKf &K = D.kfs[s];
    int32_t *kfp = fc_kfp(D, K);
    const int n = K.n, kslot = K.slot, kpos = D.pos[kslot];
    const float *uRight = (const float *)(D.A + K.ur);
    const int L = min(*lenPtr, lenCap);
    int nFused = 0;
    int logCount = 0, nodeCount = 0, freeHead = -1;      // thread 0's
    if (t == 0) { logCount = D.counters[FC_LOG]; nodeCount = D.counters[FC_NODES]; freeHead = D.counters[FC_FREE]; }
    for (int base = 0; base < L; base += FC_THREADS) {
        const int i = base + t;
        const bool candidate = i < L && act[i] && bestDist[i] <= TH_LOW && list[i] >= 0;
        const unsigned long long bm = __ballot(candidate);
        __syncthreads();      // (the previous round's masks have been consumed)
        if (lane == 0) sMask[w] = bm;
        __syncthreads();
        for (int w4 = 0; w4 < FC_THREADS / 64; w4++) {
            unsigned long long mask = sMask[w4];
            while (mask) {
                const int e = base + w4 * 64 + __builtin_ctzll(mask);
                mask &= mask - 1;
                const int p = list[e];
                // the re-check at the entry's turn (:1045): gone bad, or entered k (kf_point[k] holds it exactly then)
                __syncthreads();      // the previous decision's stores are visible; sAny may be reset
                if (D.ptBad[p]) continue;
                if (t == 0) sAny = 0;
                __syncthreads();
                bool in = false;
                for (int f = t; f < n; f += FC_THREADS) in = in || kfp[f] == p;
                if (in) sAny = 1;
                __syncthreads();
                if (sAny) continue;
                nFused++;
                const int bi = bestIdx[e], q = kfp[bi];
                int kind, a = -1, b = -1;
                if (q < 0) kind = ORBX_FUSE_ADDED;
                else if (D.ptBad[q]) kind = ORBX_FUSE_HOLDER_BAD;
                else if (D.nobs[q] > D.nobs[p]) { kind = ORBX_FUSE_REPLACED_BY_HOLDER; a = p; b = q; }      // pMP->Replace(pMPinKF), :1158
                else { kind = ORBX_FUSE_REPLACED_HOLDER; a = q; b = p; }
                __syncthreads();      // everybody has read the state this decision is taken on
                if (t == 0) {
                    orbx_fuse_decision d;
                    d.call = call; d.position = e; d.point = p; d.feature = bi; d.kind = kind; d.other = q;
                    D.log[logCount++] = d;
                    if (kind == ORBX_FUSE_ADDED) {      // AddObservation + AddMapPoint, :1166-1167
                        const int st = uRight[bi] >= 0 ? 1 : 0;
                        int prev = -1, cur = D.head[p];
                        while (cur >= 0) {
                            const int4 cv = D.node[cur];
                            if (D.pos[cv.x] > kpos) break;
                            prev = cur; cur = cv.z;
                        }
                        int fresh = freeHead;      // a node that an earlier Replace dropped, else a new one: the nodes in use never exceed the bound
                        if (fresh >= 0) freeHead = D.node[fresh].z; else fresh = nodeCount++;
                        D.node[fresh] = make_int4(kslot, bi, cur, st | 2);
                        if (prev < 0) D.head[p] = fresh; else D.node[prev].z = fresh;
                        D.nobs[p] += st ? 2 : 1;
                        kfp[bi] = p;
                    } else if (a >= 0) {      // a->Replace(b), src/MapPoint.cc:244-301: the two rank-ordered lists merged into b's
                        D.ptBad[a] = 1; D.replaced[a] = b;
                        int pa = D.head[a], pb = D.head[b], prev = -1, newHead = -1, N = 0, add = 0;
                        int4 va = make_int4(0, 0, -1, 0), vb = va;
                        if (pa >= 0) va = D.node[pa];
                        if (pb >= 0) vb = D.node[pb];
                        while (pa >= 0 || pb >= 0) {
                            const int ra = pa >= 0 ? D.pos[va.x] : INT_MAX, rb = pb >= 0 ? D.pos[vb.x] : INT_MAX;
                            int nd, kf;
                            if (ra == rb) {      // b is observed by that keyframe already: EraseMapPointMatch, a's observation is dropped
                                const int si = D.sIndex[va.x];
                                if (si >= 0) fc_kfp(D, D.kfs[si])[va.y] = -1;
                                D.node[pa].z = freeHead; freeHead = pa;
                                pa = va.z;
                                if (pa >= 0) va = D.node[pa];
                                continue;
                            }
                            if (ra < rb) {       // ReplaceMapPointMatch + AddObservation
                                nd = pa; kf = va.x;
                                const int si = D.sIndex[kf];
                                if (si >= 0) fc_kfp(D, D.kfs[si])[va.y] = b;
                                add += (va.w & 1) ? 2 : 1;
                                pa = va.z;
                                if (pa >= 0) va = D.node[pa];
                            } else {
                                nd = pb; kf = vb.x;
                                pb = vb.z;
                                if (pb >= 0) vb = D.node[pb];
                            }
                            if (prev < 0) newHead = nd; else D.node[prev].z = nd;
                            prev = nd;
                            if (!D.kfBad[kf]) D.listBuf[N++] = nd;      // ComputeDistinctiveDescriptors skips observers that are bad, :384
                        }
                        if (prev >= 0) D.node[prev].z = -1;
                        D.head[b] = newHead; D.head[a] = -1;
                        D.nobs[b] += add;
                        D.found[b] += D.found[a]; D.visible[b] += D.visible[a];
                        sN = N;
                    }
                }
                if (a < 0) continue;
                __syncthreads();
                // ComputeDistinctiveDescriptors(b), src/MapPoint.cc:359-439, over listBuf[0..N)
                const int N = sN;
                if (N == 0) continue;
                const bool lds = N <= FC_LDS_DESC;
                if (lds) {
                    for (int j = t; j < N; j += FC_THREADS) {
                        const int nd = D.listBuf[j];
                        const uint4 *g = (const uint4 *)fc_node_desc(D, nd, D.node[nd]);
                        uint4 *d4 = (uint4 *)(sDesc + j * 8);
                        d4[0] = g[0]; d4[1] = g[1];
                    }
                    __syncthreads();
                }
                const int need = ((N - 1) >> 1) + 1;
                unsigned long long key = ~0ull;
                for (int r = t; r < N; r += FC_THREADS) {
                    uint32_t mine[8];
                    {
                        const int nd = D.listBuf[r];
                        const uint32_t *g = lds ? sDesc + r * 8 : fc_node_desc(D, nd, D.node[nd]);
#pragma unroll
                        for (int x = 0; x < 8; x++) mine[x] = g[x];
                    }
                    int lo = 0, hi = 256;      // the smallest value v with count(d <= v) >= need: the element at sorted position (N - 1) / 2
                    for (int step = 0; step < 9; step++) {
                        const int mid = (lo + hi) >> 1;
                        int cnt = 0;
                        for (int j = 0; j < N; j++) {
                            const uint32_t *g;
                            if (lds) g = sDesc + j * 8;
                            else { const int nd = D.listBuf[j]; g = fc_node_desc(D, nd, D.node[nd]); }
                            cnt += fc_dist(mine, g) <= mid ? 1 : 0;
                        }
                        if (cnt >= need) hi = mid; else lo = mid + 1;
                    }
                    const unsigned long long k2 = (unsigned long long)(unsigned)lo << 32 | (unsigned)r;
                    key = k2 < key ? k2 : key;
                }
                key = wave_min(key);
                if (lane == 0) sKey[w] = key;
                __syncthreads();
                for (int j = 0; j < FC_THREADS / 64; j++) key = sKey[j] < key ? sKey[j] : key;
                if (t < 8) {
                    const int win = (int)(unsigned)(key & 0xffffffffu), nd = D.listBuf[win];
                    ((uint32_t *)(D.ptDesc + (size_t)b * 32))[t] = fc_node_desc(D, nd, D.node[nd])[t];
                }
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        D.counters[FC_LOG] = logCount; D.counters[FC_NODES] = nodeCount; D.counters[FC_FREE] = freeHead;
        D.oNfused[call] = nFused;
    }
}

// the first (target, feature) position at which a point is held, over all targets (a repeated target comes later: it lists nothing new)
__global__ __launch_bounds__(FC_THREADS) void k_fc_mark(FcDev D, const int32_t *targets, const int32_t *tOff, int T)
{
    const int e = blockIdx.x * FC_THREADS + threadIdx.x;
    if (e >= tOff[T]) return;
    int ti = 0;
    for (int hi = T - 1; ti < hi;) { const int mid = (ti + hi) >> 1; if (tOff[mid + 1] <= e) ti = mid + 1; else hi = mid; }
    const int p = fc_kfp(D, D.kfs[targets[ti]])[e - tOff[ti]];
    if (p >= 0 && !D.ptBad[p]) atomicMin(&D.firstPos[p], e);
}

// :690-711 in order: ONE workgroup compacts the first occurrences
__global__ __launch_bounds__(FC_THREADS) void k_fc_gather(FcDev D, const int32_t *targets, const int32_t *tOff, int T, int candCap)
{
    __shared__ int sh[FC_THREADS / 64];
    const int E = tOff[T];
    int base = 0, ti = 0;
    for (int e0 = 0; e0 < E; e0 += FC_THREADS) {
        const int e = e0 + (int)threadIdx.x;
        int p = -1;
        bool take = false;
        if (e < E) {
            while (tOff[ti + 1] <= e) ti++;
            p = fc_kfp(D, D.kfs[targets[ti]])[e - tOff[ti]];
            take = p >= 0 && !D.ptBad[p] && __hip_atomic_load(&D.firstPos[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == e;
        }
        const int at = block_ballot_rank<FC_THREADS>(take, &base, sh);
        if (take && at < candCap) D.cand[at] = p;
    }
    if (threadIdx.x == 0) D.counters[FC_CAND] = base < candCap ? base : candCap;
}

// the state after the chain -> mapped host memory.  ONE workgroup: the observations go back as CSR, which takes a scan over the points.
__global__ __launch_bounds__(FC_THREADS) void k_fc_export(FcDev D, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    __shared__ int sh[FC_THREADS / 64];
    __shared__ int sBase;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) sBase = 0;
    __syncthreads();
    for (int p0 = 0; p0 < D.P; p0 += FC_THREADS) {
        const int p = p0 + t;
        int len = 0;
        if (p < D.P) for (int nd = D.head[p]; nd >= 0; nd = D.node[nd].z) len++;
        const int incl = wave_incl_scan_dpp(len);
        if (lane == 63) sh[w] = incl;
        __syncthreads();
        int before = 0, all = 0;
        for (int j = 0; j < FC_THREADS / 64; j++) { before += j < w ? sh[j] : 0; all += sh[j]; }
        int at = sBase + before + incl - len;
        if (p < D.P) {
            D.oObsOff[p] = at;
            for (int nd = D.head[p]; nd >= 0;) {
                const int4 v = D.node[nd];
                D.oObsKf[at] = v.x; D.oObsIdx[at] = v.y; D.oObsSt[at] = (uint8_t)(v.w & 1);
                at++; nd = v.z;
            }
            D.oBad[p] = D.ptBad[p]; D.oReplaced[p] = D.replaced[p]; D.oNobs[p] = D.nobs[p]; D.oVisible[p] = D.visible[p]; D.oFound[p] = D.found[p];
        }
        __syncthreads();
        if (t == 0) sBase += all;
        __syncthreads();
    }
    for (size_t i = t; i < (size_t)D.P * 8; i += FC_THREADS) ((uint32_t *)D.oDesc)[i] = ((const uint32_t *)D.ptDesc)[i];
    for (int s = 0; s < D.S; s++) {
        const FcKf &K = D.kfs[s];
        const int32_t *kfp = fc_kfp(D, K);
        for (int f = t; f < K.n; f += FC_THREADS) D.oKfp[K.featBase + f] = kfp[f];
    }
    const int nc = D.counters[FC_CAND];
    for (int i = t; i < nc; i += FC_THREADS) D.oCand[i] = D.cand[i];
    if (t == 0) {
        D.oObsOff[D.P] = sBase;
        D.oCounts[0] = D.counters[FC_LOG]; D.oCounts[1] = nc; D.oCounts[2] = sBase;
    }
    orbx_publish(counter, flag, seq, 1);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------

// everything a kernel indexes with is checked here, before anything is launched (and before the handle is looked at)
int fc_validate(orbx_matcher *m, const orbx_fuse_slice *s, const char *who, std::vector<int32_t> &order, std::vector<int32_t> &pos, std::vector<int32_t> &sIndex)
{
    if (!s) { orbx_set_error("%s: NULL slice", who); return ORBX_ERR_ARG; }
    const int NK = s->num_keyframes, S = s->num_searchable, P = s->num_points, T0 = s->num_obs;
    if (NK < 1 || S < 1 || S > NK || P < 0 || T0 < 0) { orbx_set_error("%s: num_keyframes < 1, num_searchable outside 1..num_keyframes or a negative size", who); return ORBX_ERR_ARG; }
    if (!s->kf_rank || !s->kf_bad || !s->searchable || !s->obs_offset ||
        (P > 0 && (!s->pos || !s->normal || !s->min_distance || !s->max_distance || !s->raw_max_distance || !s->descriptors || !s->point_bad || !s->visible || !s->found)) ||
        (T0 > 0 && (!s->obs_kf || !s->obs_idx || !s->obs_stereo || !s->obs_descriptors))) {
        orbx_set_error("%s: NULL slice array", who);
        return ORBX_ERR_ARG;
    }
    if (s->obs_offset[0] != 0) { orbx_set_error("%s: obs_offset does not start at 0", who); return ORBX_ERR_ARG; }
    for (int p = 0; p < P; p++)
        if (s->obs_offset[p + 1] < s->obs_offset[p]) { orbx_set_error("%s: obs_offset decreases at point %d", who, p); return ORBX_ERR_ARG; }
    if (s->obs_offset[P] != T0) { orbx_set_error("%s: obs_offset[num_points] = %d, num_obs = %d", who, s->obs_offset[P], T0); return ORBX_ERR_ARG; }
    // the order of std::map<KeyFrame*, ...>
    order.resize((size_t)NK);
    std::iota(order.begin(), order.end(), 0);
    const int32_t *rk = s->kf_rank;
    std::sort(order.begin(), order.end(), [rk](int32_t a, int32_t b) { return rk[a] < rk[b]; });
    for (int i = 1; i < NK; i++)
        if (rk[order[(size_t)i]] == rk[order[(size_t)i - 1]]) {
            orbx_set_error("%s: keyframe slots %d and %d have the same rank %d", who, order[(size_t)i - 1], order[(size_t)i], rk[order[(size_t)i]]);
            return ORBX_ERR_ARG;
        }
    pos.resize((size_t)NK);
    for (int i = 0; i < NK; i++) pos[(size_t)order[(size_t)i]] = i;
    sIndex.assign((size_t)NK, -1);
    long long held = 0;
    for (int i = 0; i < S; i++) {
        const orbx_fuse_keyframe &k = s->searchable[i];
        if (k.slot < 0 || k.slot >= NK) { orbx_set_error("%s: searchable keyframe %d: slot %d is no keyframe slot (0..%d)", who, i, k.slot, NK - 1); return ORBX_ERR_ARG; }
        if (sIndex[(size_t)k.slot] >= 0) { orbx_set_error("%s: keyframe slot %d is searchable twice", who, k.slot); return ORBX_ERR_ARG; }
        sIndex[(size_t)k.slot] = i;
        if (k.num_features < 0) { orbx_set_error("%s: searchable keyframe %d: negative feature count", who, i); return ORBX_ERR_ARG; }
        if (k.num_features > 65535) { orbx_set_error("%s: searchable keyframe %d holds %d features, the limit is 65535", who, i, k.num_features); return ORBX_ERR_CAPACITY; }
        if (k.nlevels > ORBX_MAX_LEVELS) { orbx_set_error("%s: searchable keyframe %d has %d levels, the limit is %d", who, i, k.nlevels, ORBX_MAX_LEVELS); return ORBX_ERR_CAPACITY; }
        if (k.nlevels < 1 || !k.scale_factors || !k.inv_level_sigma2 || !(k.log_scale_factor > 0.0f)) { orbx_set_error("%s: searchable keyframe %d: bad scale tables", who, i); return ORBX_ERR_ARG; }
        if (k.num_features > 0 && (!k.keys_un || !k.descriptors || !k.u_right || !k.kf_point)) { orbx_set_error("%s: searchable keyframe %d: NULL feature array", who, i); return ORBX_ERR_ARG; }
        for (int f = 0; f < k.num_features; f++) {
            if (k.kf_point[f] < -1 || k.kf_point[f] >= P) { orbx_set_error("%s: searchable keyframe %d: kf_point[%d] = %d is no point (0..%d)", who, i, f, k.kf_point[f], P - 1); return ORBX_ERR_ARG; }
            held += k.kf_point[f] >= 0 ? 1 : 0;
            if (k.keys_un[f].octave < 0 || k.keys_un[f].octave >= k.nlevels) { orbx_set_error("%s: searchable keyframe %d: feature %d has octave %d", who, i, f, k.keys_un[f].octave); return ORBX_ERR_ARG; }
        }
    }
    long long seen = 0;
    for (int p = 0; p < P; p++)
        for (int o = s->obs_offset[p]; o < s->obs_offset[p + 1]; o++) {
            const int kf = s->obs_kf[o], idx = s->obs_idx[o];
            if (kf < 0 || kf >= NK) { orbx_set_error("%s: obs_kf[%d] = %d is no keyframe slot (0..%d)", who, o, kf, NK - 1); return ORBX_ERR_ARG; }
            if (idx < 0) { orbx_set_error("%s: obs_idx[%d] = %d is negative", who, o, idx); return ORBX_ERR_ARG; }
            if (o > s->obs_offset[p] && pos[(size_t)kf] <= pos[(size_t)s->obs_kf[o - 1]]) {
                orbx_set_error("%s: the observations of point %d are not in ascending rank at observation %d", who, p, o);
                return ORBX_ERR_ARG;
            }
            const int si = sIndex[(size_t)kf];
            if (si < 0) continue;
            const orbx_fuse_keyframe &k = s->searchable[si];
            if (idx >= k.num_features || k.kf_point[idx] != p) {
                orbx_set_error("%s: point %d is observed by keyframe slot %d at feature %d, whose kf_point does not hold it", who, p, kf, idx);
                return ORBX_ERR_ARG;
            }
            if ((s->obs_stereo[o] != 0) != (k.u_right[idx] >= 0)) { orbx_set_error("%s: obs_stereo[%d] disagrees with u_right of keyframe slot %d", who, o, kf); return ORBX_ERR_ARG; }
            seen++;
        }
    if (seen != held) { orbx_set_error("%s: the searchable keyframes hold %lld points, %lld of them observe their keyframe", who, held, seen); return ORBX_ERR_ARG; }
    if (!m) { orbx_set_error("%s: NULL handle", who); return ORBX_ERR_ARG; }
    return ORBX_OK;
}

struct FcSlots {
    OrbxSlot<int32_t, ORBX_STAGE_IN> pos, sIndex, obsOff, obsKf, obsIdx, visible, found, list, targets, tOff, lens;
    OrbxSlot<uint8_t, ORBX_STAGE_IN> kfBad, ptDesc, ptBad, obsSt, obsDesc, act;
    OrbxSlot<float, ORBX_STAGE_IN> ppos, pnormal, minD, maxD, rawMax;
    OrbxSlot<FcKf, ORBX_STAGE_IN> kfs;
    OrbxSlot<int32_t, ORBX_STAGE_IN> bestIdx, bestDist;
    std::vector<OrbxSlot<orbx_keypoint, ORBX_STAGE_IN>> kp;
    std::vector<OrbxSlot<uint8_t, ORBX_STAGE_IN>> desc;
    std::vector<OrbxSlot<float, ORBX_STAGE_IN>> ur;
    std::vector<OrbxSlot<int32_t, ORBX_STAGE_IN>> kfp;
};

struct FcOut {
    OrbxSlot<orbx_fuse_decision, ORBX_STAGE_OUT> log;
    OrbxSlot<int32_t, ORBX_STAGE_OUT> nfused, counts, cand, kfp, replaced, nobs, visible, found, obsOff, obsKf, obsIdx;
    OrbxSlot<uint8_t, ORBX_STAGE_OUT> bad, desc, obsSt;
};

// the common body.  list / act / bestIdx / bestDist non-NULL: orbx_fuse_apply (one call on keyframe searchable[sk]); else the chain.
int fc_run(orbx_matcher *m, const orbx_fuse_slice *s, int sk, const int32_t *targets, int T, const int32_t *list, const uint8_t *act, const int32_t *bestIdx,
           const int32_t *bestDist, int nList, const orbx_fuse_result *res, const char *who)
{
    const bool chain = list == nullptr;
    const int NK = s->num_keyframes, S = s->num_searchable, P = s->num_points, T0 = s->num_obs;
    const size_t nk = (size_t)NK, np = (size_t)P, t0 = (size_t)T0;
    const orbx_fuse_keyframe &cur = s->searchable[sk];
    int rc;
    // sizes: an add fills an empty feature, so the nodes are bounded by the observations plus the empty features
    size_t totalFeat = 0, empty = 0, candCap = 0;
    for (int i = 0; i < S; i++) {
        totalFeat += (size_t)s->searchable[i].num_features;
        for (int f = 0; f < s->searchable[i].num_features; f++) empty += s->searchable[i].kf_point[f] < 0 ? 1 : 0;
    }
    std::vector<int32_t> tIdx((size_t)T), tOff((size_t)T + 1, 0);
    for (int k = 0; k < T; k++) {
        tIdx[(size_t)k] = m->fcSIndex[(size_t)targets[k]];
        tOff[(size_t)k + 1] = tOff[(size_t)k] + s->searchable[tIdx[(size_t)k]].num_features;
        if (tOff[(size_t)k + 1] > (1 << 28)) { orbx_set_error("%s: more than 2^28 target features in one call", who); return ORBX_ERR_CAPACITY; }
    }
    candCap = chain ? std::min<size_t>(np, (size_t)tOff[(size_t)T]) : 0;
    const size_t nCur = chain ? (size_t)cur.num_features : (size_t)nList;
    const size_t lmax = std::max<size_t>(std::max(nCur, candCap), 1), nodeCap = t0 + empty;
    const size_t logCap = chain ? (size_t)T * nCur + candCap : nCur;
    const int calls = chain ? T + 1 : 1;
    const bool full = chain && (res->active || res->u || res->v || res->ur || res->level || res->radius || res->best_idx || res->best_dist);
    if (full && (size_t)res->full_stride < lmax) { orbx_set_error("%s: full_stride %d below the longest possible list (%zu)", who, res->full_stride, lmax); return ORBX_ERR_CAPACITY; }
    if (res->log_capacity < 0 || res->candidates_capacity < 0 || res->obs_capacity < 0) { orbx_set_error("%s: negative capacity", who); return ORBX_ERR_ARG; }
    ORBX_HIP_CHECK(hipSetDevice(m->device));

    // ---- the slice in the call box, copied once into the arena ----
    OrbxCallBox &bx = m->box;
    auto [pin, pout] = bx.plan();
    FcSlots I;
    I.pos = pin.add(m->fcPos.data(), nk); I.sIndex = pin.add(m->fcSIndex.data(), nk); I.kfBad = pin.add(s->kf_bad, nk);
    I.kfs = pin.hole<FcKf>((size_t)S);
    I.ppos = pin.add(s->pos, 3 * np); I.pnormal = pin.add(s->normal, 3 * np);
    I.minD = pin.add(s->min_distance, np); I.maxD = pin.add(s->max_distance, np); I.rawMax = pin.add(s->raw_max_distance, np);
    I.ptDesc = pin.add(s->descriptors, 32 * np); I.ptBad = pin.add(s->point_bad, np);
    I.visible = pin.add(s->visible, np); I.found = pin.add(s->found, np);
    I.obsOff = pin.add(s->obs_offset, np + 1); I.obsKf = pin.add(s->obs_kf, t0); I.obsIdx = pin.add(s->obs_idx, t0);
    I.obsSt = pin.add(s->obs_stereo, t0); I.obsDesc = pin.add(s->obs_descriptors, 32 * t0);
    I.list = pin.add(chain ? cur.kf_point : list, nCur);      // (the chain: its own copy - kf_point itself changes under the calls)
    I.targets = pin.add(tIdx.data(), (size_t)T); I.tOff = pin.add(tOff.data(), (size_t)T + 1);
    const int32_t lens[2] = {(int32_t)nCur, 0};
    I.lens = pin.add(lens, 2);
    I.act = pin.add(act, chain ? 0 : nCur); I.bestIdx = pin.add(bestIdx, chain ? 0 : nCur); I.bestDist = pin.add(bestDist, chain ? 0 : nCur);
    I.kp.resize((size_t)S); I.desc.resize((size_t)S); I.ur.resize((size_t)S); I.kfp.resize((size_t)S);
    for (int i = 0; i < S; i++) {
        const orbx_fuse_keyframe &k = s->searchable[i];
        const size_t n = (size_t)k.num_features;
        I.kp[(size_t)i] = pin.add(k.keys_un, n); I.desc[(size_t)i] = pin.add(k.descriptors, 32 * n);
        I.ur[(size_t)i] = pin.add(k.u_right, n); I.kfp[(size_t)i] = pin.add(k.kf_point, n);
    }
    FcOut O;
    O.log = pout.hole<orbx_fuse_decision>(logCap);
    O.nfused = pout.hole<int32_t>((size_t)calls); O.counts = pout.hole<int32_t>(4); O.cand = pout.hole<int32_t>(candCap); O.kfp = pout.hole<int32_t>(totalFeat);
    O.bad = pout.hole<uint8_t>(np); O.replaced = pout.hole<int32_t>(np); O.nobs = pout.hole<int32_t>(np); O.visible = pout.hole<int32_t>(np); O.found = pout.hole<int32_t>(np);
    O.desc = pout.hole<uint8_t>(32 * np); O.obsOff = pout.hole<int32_t>(np + 1); O.obsKf = pout.hole<int32_t>(nodeCap); O.obsIdx = pout.hole<int32_t>(nodeCap);
    O.obsSt = pout.hole<uint8_t>(nodeCap);

    // ---- the device state ----
    OrbxWorkPlan &wp = m->fcPlan;
    wp.reset();
    const auto wNode = wp.hole<int4>(nodeCap + 1);
    const auto wHead = wp.hole<int32_t>(np), wNobs = wp.hole<int32_t>(np), wRepl = wp.hole<int32_t>(np), wFirst = wp.hole<int32_t>(np);
    const auto wListBuf = wp.hole<int32_t>(nk), wCounters = wp.hole<int32_t>(8), wCand = wp.hole<int32_t>(candCap + 1);
    const size_t regions = full ? (size_t)calls : 1;
    const auto wAct = wp.hole<uint8_t>(regions * lmax), wDesc = wp.hole<uint8_t>(32 * lmax);
    const auto wU = wp.hole<float>(regions * lmax), wV = wp.hole<float>(regions * lmax), wUr = wp.hole<float>(regions * lmax), wRad = wp.hole<float>(regions * lmax);
    const auto wLvl = wp.hole<int32_t>(regions * lmax), wBi = wp.hole<int32_t>(regions * lmax), wBd = wp.hole<int32_t>(regions * lmax);
    if ((rc = m->fcWork.ensure(wp.total())) != ORBX_OK) return rc;
    if ((rc = m->fcTimer.create()) != ORBX_OK) return rc;
    const bool profile = s->profile_kernels != 0;
    if (profile)
        while (m->fcApplyEv.size() < 2 * (size_t)calls) { hipEvent_t e = nullptr; ORBX_HIP_CHECK(hipEventCreate(&e)); m->fcApplyEv.push_back(e); }
    m->fcTimer.timed = false; m->fcApplyTimed = 0;

    const OrbxStaged sg = bx.begin(m->stream, &rc);
    if (rc != ORBX_OK) return rc;
    // the keyframe table: offsets of the keyframe's arrays inside the arena, and the thresholds of PredictScale
    FcKf *tab = sg.host(I.kfs);
    size_t featBase = 0;
    for (int i = 0; i < S; i++) {
        const orbx_fuse_keyframe &k = s->searchable[i];
        FcKf &K = tab[i];
        memset(&K, 0, sizeof(K));
        K.kp = I.kp[(size_t)i].off; K.desc = I.desc[(size_t)i].off; K.ur = I.ur[(size_t)i].off; K.kfp = I.kfp[(size_t)i].off;
        memcpy(K.tcw, k.tcw, sizeof(K.tcw)); memcpy(K.ow, k.ow, sizeof(K.ow));
        K.fx = k.fx; K.fy = k.fy; K.cx = k.cx; K.cy = k.cy; K.mbf = k.mbf;
        K.gMinX = k.grid_min_x; K.gMinY = k.grid_min_y; K.gwInv = k.grid_width_inv; K.ghInv = k.grid_height_inv;
        K.minX = (float)k.min_x; K.maxX = (float)k.max_x; K.minY = (float)k.min_y; K.maxY = (float)k.max_y;
        K.th = s->th;
        for (int l = 0; l < ORBX_MAX_LEVELS; l++) { K.sf[l] = l < k.nlevels ? k.scale_factors[l] : 1.0f; K.invS2[l] = l < k.nlevels ? k.inv_level_sigma2[l] : 0.0f; }
        if ((rc = orbx_predict_scale_thresholds(k.log_scale_factor, k.nlevels, K.ratioTh)) != ORBX_OK) return rc;
        K.n = k.num_features; K.nlevels = k.nlevels; K.slot = k.slot; K.featBase = (int)featBase;
        featBase += (size_t)k.num_features;
    }
    if ((rc = m->fcTimer.begin(m->stream)) != ORBX_OK) return rc;
    uint8_t *A;
    if ((rc = orbx_stage_to_arena(bx, m->arena, m->stream, 256, &A)) != ORBX_OK) return rc;
    ORBX_LAUNCH_COUNT(m->fcTimer);
    FcDev D = {};
    D.A = A; D.kfs = I.kfs.in(A); D.pos = I.pos.in(A); D.sIndex = I.sIndex.in(A); D.kfBad = I.kfBad.in(A);
    D.NK = NK; D.S = S; D.P = P; D.T0 = T0; D.nodeCap = (int)nodeCap;
    D.ppos = I.ppos.in(A); D.pnormal = I.pnormal.in(A); D.minD = I.minD.in(A); D.maxD = I.maxD.in(A); D.rawMax = I.rawMax.in(A);
    D.ptDesc = I.ptDesc.in(A); D.ptBad = I.ptBad.in(A); D.visible = I.visible.in(A); D.found = I.found.in(A);
    D.obsOff = I.obsOff.in(A); D.obsKf = I.obsKf.in(A); D.obsIdx = I.obsIdx.in(A); D.obsSt = I.obsSt.in(A); D.obsDesc = I.obsDesc.in(A);
    void *W = m->fcWork.p;
    D.node = wNode.in(W); D.head = wHead.in(W); D.nobs = wNobs.in(W); D.replaced = wRepl.in(W); D.firstPos = wFirst.in(W);
    D.listBuf = wListBuf.in(W); D.counters = wCounters.in(W); D.cand = wCand.in(W);
    D.log = sg.dev(O.log); D.oNfused = sg.dev(O.nfused); D.oCounts = sg.dev(O.counts); D.oCand = sg.dev(O.cand); D.oKfp = sg.dev(O.kfp);
    D.oBad = sg.dev(O.bad); D.oReplaced = sg.dev(O.replaced); D.oNobs = sg.dev(O.nobs); D.oVisible = sg.dev(O.visible); D.oFound = sg.dev(O.found);
    D.oDesc = sg.dev(O.desc); D.oObsOff = sg.dev(O.obsOff); D.oObsKf = sg.dev(O.obsKf); D.oObsIdx = sg.dev(O.obsIdx); D.oObsSt = sg.dev(O.obsSt);
    const unsigned long long seq = bx.arm();      // before the first launch: an error below leaves the box pending and the next begin() drains the stream
    hipStream_t st = m->stream;
    const unsigned pointBlocks = (unsigned)((std::max(P, 1) + FC_THREADS - 1) / FC_THREADS);
    hipLaunchKernelGGL(k_fc_init, dim3(pointBlocks), dim3(FC_THREADS), 0, st, D);
    ORBX_LAUNCH_COUNT(m->fcTimer);

    auto region = [&](int c) {
        const size_t r = full ? (size_t)c * lmax : 0;
        FcCall C = {wAct.in(W) + r, wU.in(W) + r, wV.in(W) + r, wUr.in(W) + r, wRad.in(W) + r, wLvl.in(W) + r, wBi.in(W) + r, wBd.in(W) + r, wDesc.in(W)};
        return C;
    };
    // one Fuse call of searchable keyframe si on the list (device pointers; its length is read on the device, at most lenCap)
    auto fuse_call = [&](int c, int si, const int32_t *dList, const int32_t *dLen, size_t lenCap) -> int {
        const orbx_fuse_keyframe &k = s->searchable[si];
        const FcCall C = region(c);
        const uint8_t *dAct = C.act;
        const int32_t *dBi = C.bestIdx, *dBd = C.bestDist;
        if (chain) {
            if (lenCap > 0) {
                hipLaunchKernelGGL(k_fc_prepare, dim3((unsigned)((lenCap + FC_THREADS - 1) / FC_THREADS)), dim3(FC_THREADS), 0, st, D, C, si, dList, dLen, (int)lenCap);
                ORBX_LAUNCH_COUNT(m->fcTimer);
                const FcKf &K = tab[si];
                const ProjFrameDev F = {(const orbx_keypoint *)(A + K.kp), A + K.desc, (const float *)(A + K.ur), nullptr, &I.kfs.in(A)[si].n, std::max(k.num_features, 1),
                                        K.gMinX, K.gMinY, K.gwInv, K.ghInv};
                const FusePointsDev Pd = {C.u, C.v, C.ur, C.level, C.radius, C.act, C.desc, dLen, (int)lenCap, K.minX, K.minY};
                FuseLevels LV;
                for (int l = 0; l < ORBX_MAX_LEVELS; l++) LV.invSigma2[l] = K.invS2[l];
                orbx_match::launch_fuse_best(st, F, Pd, LV, C.bestIdx, C.bestDist);
                ORBX_LAUNCH_COUNT(m->fcTimer);
            }
        } else { dAct = I.act.in(A); dBi = I.bestIdx.in(A); dBd = I.bestDist.in(A); }
        if (profile) ORBX_HIP_CHECK(hipEventRecord(m->fcApplyEv[2 * (size_t)c], st));
        hipLaunchKernelGGL(k_fc_apply, dim3(1), dim3(FC_THREADS), 0, st, D, c, si, dList, dLen, (int)lenCap, dAct, dBi, dBd);
        ORBX_LAUNCH_COUNT(m->fcTimer);
        if (profile) ORBX_HIP_CHECK(hipEventRecord(m->fcApplyEv[2 * (size_t)c + 1], st));
        return ORBX_OK;
    };
    const int32_t *dLens = I.lens.in(A);
    if (chain) {
        for (int k = 0; k < T; k++)
            if ((rc = fuse_call(k, tIdx[(size_t)k], I.list.in(A), dLens, nCur)) != ORBX_OK) return rc;
        if (tOff[(size_t)T] > 0) {
            hipLaunchKernelGGL(k_fc_mark, dim3((unsigned)((tOff[(size_t)T] + FC_THREADS - 1) / FC_THREADS)), dim3(FC_THREADS), 0, st, D, I.targets.in(A), I.tOff.in(A), T);
            ORBX_LAUNCH_COUNT(m->fcTimer);
            hipLaunchKernelGGL(k_fc_gather, dim3(1), dim3(FC_THREADS), 0, st, D, I.targets.in(A), I.tOff.in(A), T, (int)candCap);
            ORBX_LAUNCH_COUNT(m->fcTimer);
        }
        if ((rc = fuse_call(T, sk, D.cand, D.counters + FC_CAND, candCap)) != ORBX_OK) return rc;
    } else if ((rc = fuse_call(0, sk, I.list.in(A), dLens, nCur)) != ORBX_OK) return rc;
    hipLaunchKernelGGL(k_fc_export, dim3(1), dim3(FC_THREADS), 0, st, D, bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_COUNT(m->fcTimer);
    if ((rc = m->fcTimer.end(st)) != ORBX_OK) return rc;
    m->fcApplyTimed = profile ? calls : 0;
    if ((rc = bx.wait(st)) != ORBX_OK) return rc;      // the one synchronisation

    // ---- results: the capacities first, nothing is written when one is too small ----
    const int32_t *cnt = sg.host(O.counts);
    const int nLog = cnt[0], nCand = cnt[1], nObs = cnt[2];
    if ((res->log && nLog > res->log_capacity) || (res->candidates && nCand > res->candidates_capacity) ||
        ((res->obs_kf || res->obs_idx || res->obs_stereo) && nObs > res->obs_capacity)) {
        orbx_set_error("%s: %d decisions, %d candidates and %d observations for capacities of %d, %d and %d", who, nLog, nCand, nObs, res->log_capacity, res->candidates_capacity,
                       res->obs_capacity);
        return ORBX_ERR_CAPACITY;
    }
    if (res->log && nLog) memcpy(res->log, sg.host(O.log), (size_t)nLog * sizeof(orbx_fuse_decision));
    if (res->log_count) *res->log_count = nLog;
    if (res->nfused) memcpy(res->nfused, sg.host(O.nfused), (size_t)calls * 4);
    if (res->candidates && nCand) memcpy(res->candidates, sg.host(O.cand), (size_t)nCand * 4);
    if (res->candidates_count) *res->candidates_count = nCand;
    if (res->kf_point && totalFeat) memcpy(res->kf_point, sg.host(O.kfp), totalFeat * 4);
    if (P) {
        if (res->point_bad) memcpy(res->point_bad, sg.host(O.bad), np);
        if (res->replaced) memcpy(res->replaced, sg.host(O.replaced), np * 4);
        if (res->point_obs) memcpy(res->point_obs, sg.host(O.nobs), np * 4);
        if (res->visible) memcpy(res->visible, sg.host(O.visible), np * 4);
        if (res->found) memcpy(res->found, sg.host(O.found), np * 4);
        if (res->descriptors) memcpy(res->descriptors, sg.host(O.desc), np * 32);
    }
    if (res->obs_offset) memcpy(res->obs_offset, sg.host(O.obsOff), (np + 1) * 4);
    if (nObs) {
        if (res->obs_kf) memcpy(res->obs_kf, sg.host(O.obsKf), (size_t)nObs * 4);
        if (res->obs_idx) memcpy(res->obs_idx, sg.host(O.obsIdx), (size_t)nObs * 4);
        if (res->obs_stereo) memcpy(res->obs_stereo, sg.host(O.obsSt), (size_t)nObs);
    }
    if (full) {      // the optional per-entry arrays (tests, diagnostics): copies of their own
        ORBX_HIP_CHECK(hipStreamSynchronize(st));
        for (int c = 0; c < calls; c++) {
            const size_t len = c < T ? nCur : (size_t)nCand, ho = (size_t)c * (size_t)res->full_stride;
            if (!len) continue;
            const FcCall C = region(c);
            if (res->active) ORBX_HIP_CHECK(hipMemcpy(res->active + ho, C.act, len, hipMemcpyDeviceToHost));
            if (res->u) ORBX_HIP_CHECK(hipMemcpy(res->u + ho, C.u, len * 4, hipMemcpyDeviceToHost));
            if (res->v) ORBX_HIP_CHECK(hipMemcpy(res->v + ho, C.v, len * 4, hipMemcpyDeviceToHost));
            if (res->ur) ORBX_HIP_CHECK(hipMemcpy(res->ur + ho, C.ur, len * 4, hipMemcpyDeviceToHost));
            if (res->level) ORBX_HIP_CHECK(hipMemcpy(res->level + ho, C.level, len * 4, hipMemcpyDeviceToHost));
            if (res->radius) ORBX_HIP_CHECK(hipMemcpy(res->radius + ho, C.radius, len * 4, hipMemcpyDeviceToHost));
            if (res->best_idx) ORBX_HIP_CHECK(hipMemcpy(res->best_idx + ho, C.bestIdx, len * 4, hipMemcpyDeviceToHost));
            if (res->best_dist) ORBX_HIP_CHECK(hipMemcpy(res->best_dist + ho, C.bestDist, len * 4, hipMemcpyDeviceToHost));
        }
    }
    return ORBX_OK;
}

}  // namespace

extern "C" int orbx_search_in_neighbors(orbx_matcher *m, const orbx_fuse_slice *s, int current, const int32_t *targets, int num_targets, const orbx_fuse_result *res)
{
    const char *who = "orbx_search_in_neighbors";
    if (!res) { orbx_set_error("%s: NULL result", who); return ORBX_ERR_ARG; }
    std::vector<int32_t> ownOrder, ownPos, ownS;
    int rc;
    if ((rc = fc_validate(m, s, who, m ? m->fcOrder : ownOrder, m ? m->fcPos : ownPos, m ? m->fcSIndex : ownS)) != ORBX_OK) return rc;
    if (num_targets < 0 || (num_targets > 0 && !targets)) { orbx_set_error("%s: NULL targets", who); return ORBX_ERR_ARG; }
    if (current < 0 || current >= s->num_keyframes || m->fcSIndex[(size_t)current] < 0) { orbx_set_error("%s: the current keyframe slot %d is not searchable", who, current); return ORBX_ERR_ARG; }
    for (int k = 0; k < num_targets; k++)
        if (targets[k] < 0 || targets[k] >= s->num_keyframes || m->fcSIndex[(size_t)targets[k]] < 0 || targets[k] == current) {
            orbx_set_error("%s: target %d (slot %d) is not a searchable keyframe other than the current one", who, k, targets[k]);
            return ORBX_ERR_ARG;
        }
    return fc_run(m, s, m->fcSIndex[(size_t)current], targets, num_targets, nullptr, nullptr, nullptr, nullptr, 0, res, who);
}

extern "C" int orbx_fuse_apply(orbx_matcher *m, const orbx_fuse_slice *s, int kf, const int32_t *list, const uint8_t *active, const int32_t *best_idx, const int32_t *best_dist, int n,
                               const orbx_fuse_result *res)
{
    const char *who = "orbx_fuse_apply";
    if (!res) { orbx_set_error("%s: NULL result", who); return ORBX_ERR_ARG; }
    std::vector<int32_t> ownOrder, ownPos, ownS;
    int rc;
    if ((rc = fc_validate(m, s, who, m ? m->fcOrder : ownOrder, m ? m->fcPos : ownPos, m ? m->fcSIndex : ownS)) != ORBX_OK) return rc;
    if (n < 0 || (n > 0 && (!list || !active || !best_idx || !best_dist))) { orbx_set_error("%s: NULL list array", who); return ORBX_ERR_ARG; }
    if (kf < 0 || kf >= s->num_keyframes || m->fcSIndex[(size_t)kf] < 0) { orbx_set_error("%s: keyframe slot %d is not searchable", who, kf); return ORBX_ERR_ARG; }
    const int nf = s->searchable[m->fcSIndex[(size_t)kf]].num_features;
    for (int i = 0; i < n; i++) {
        if (list[i] < -1 || list[i] >= s->num_points) { orbx_set_error("%s: list[%d] = %d is no point", who, i, list[i]); return ORBX_ERR_ARG; }
        if (list[i] >= 0 && active[i] && best_dist[i] <= TH_LOW && (best_idx[i] < 0 || best_idx[i] >= nf)) {
            orbx_set_error("%s: best_idx[%d] = %d is no feature of the keyframe (0..%d)", who, i, best_idx[i], nf - 1);
            return ORBX_ERR_ARG;
        }
    }
    static const int32_t dummyList = -1;
    static const uint8_t dummyAct = 0;
    if (n == 0) { list = &dummyList; active = &dummyAct; best_idx = &dummyList; best_dist = &dummyList; }
    return fc_run(m, s, m->fcSIndex[(size_t)kf], nullptr, 0, list, active, best_idx, best_dist, n, res, who);
}

extern "C" int orbx_search_in_neighbors_last_timing(orbx_matcher *m, float *device_ms, int *launches, float *apply_ms)
{
    if (!m) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (const int rc = m->fcTimer.read(m->device, device_ms, launches, "no orbx_search_in_neighbors call to report")) return rc;
    float ap = 0.f;
    for (int k = 0; k < m->fcApplyTimed; k++) {
        float t = 0.f;
        ORBX_HIP_CHECK(hipEventElapsedTime(&t, m->fcApplyEv[2 * (size_t)k], m->fcApplyEv[2 * (size_t)k + 1]));
        ap += t;
    }
    if (apply_ms) *apply_ms = ap;
    return ORBX_OK;
}
