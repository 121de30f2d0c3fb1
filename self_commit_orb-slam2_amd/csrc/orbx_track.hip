// orbx_track.hip -- a tracked frame on the device: Tracking::TrackWithMotionModel (src/Tracking.cc:1370-1421), Tracking::TrackLocalMap
// (:1454-1489) and Tracking::TrackReferenceKeyFrame (:1181-1239) as ONE launch chain each with ONE host wait (include/orbx.h:
// orbx_track_with_motion_model, orbx_track_local_map, orbx_track_reference_keyframe).
//
// Every numeric step already had a kernel: the two projection searches (orbx_match_proj.hip, chained here through orbx_match::enqueue_proj_last /
// enqueue_local_points), SearchByBoW for one pair (orbx_match.hip, enqueue_bow_pair) and Optimizer::PoseOptimization (k_pose_opt in orbx_lba.hip, through orbx_pose_opt_enqueue).  What was missing is what the
// reference does between them on the host, and that is all this file adds:
//   k_track_gather_last / _local / _ref          the features that hold a MapPoint after the search, compacted in ascending feature order into the
//                                                pose problem (world point, observation, information) in device memory, + the count the pose
//                                                kernel reads there and the words that gate it
//   k_track_discard                              :1403-1421 and :1215-1236  outliers leave mvpMapPoints, nmatches / nmatchesMap, every result + the
//                                                sequence word
//   k_track_local_stats                          :1464-1489  IncreaseFound / mnMatchesInliers / stereo outliers, every result + the sequence word
// All of them are one workgroup (a frame has a few thousand features and the chain is bound by latency, not by throughput): one coalesced pass, the order
// of the compaction from a scan (orbx_wave.h), no atomics on global memory.
#include "orbx_match_internal.h"
#include <algorithm>

namespace {

#define TRK_THREADS 1024
// control words the gather kernels leave for the links behind them
#define TC_COUNT 0      /* correspondences = edges of the pose problem (k_pose_opt's counts[0])                        */
#define TC_SKIP 1       /* 1 = the search ended below 20 matches (:1393; 15 for the reference keyframe, :1201): the discard falls through */
#define TC_WIDE 2       /* 1 = the 2 * th pass counted                                                                 */
#define TC_NMS 3        /* the search's return value                                                                   */
#define TC_GATE 4       /* k_pose_opt's gate: the count, or -1 = the optimisation does not run (:1393)                 */
#define TC_WORDS 8

// rank of a flagged element among the flagged ones of a TRK_THREADS-wide tile (ascending thread order) and the tile's total.  Every thread calls.
__device__ __forceinline__ int tile_rank(bool flag, int *sWave /* [TRK_THREADS / 64] */, int &total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int inc = wave_incl_scan_dpp(flag ? 1 : 0);
    if (lane == 63) sWave[wv] = inc;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TRK_THREADS / 64; w++) { const int c = sWave[w]; off += w < wv ? c : 0; tot += c; }
    __syncthreads();      // (sWave is the next tile's too)
    total = tot;
    return off + inc - (flag ? 1 : 0);
}

struct TrackProblem {      // the gathered pose problem (orbx_pose_problem's arrays for one frame) and the way back
    float *Xw, *obs, *is2;      // [cap*3], [cap*3], [cap]
    int32_t *featSlot;          // [n] slot of feature i in the problem, -1 = the feature has no edge (the discard walks the features)
    int32_t *ctl;               // [TC_WORDS]
};

// one edge: MapPoint::GetWorldPos, kpUn.pt, mvuRight, mvInvLevelSigma2[kpUn.octave] (src/Optimizer.cc:395-470)
__device__ __forceinline__ void put_edge(const TrackProblem &G, int slot, const float *X, const orbx_keypoint &k, float ur, const float *invS2, int nlevels)
{
    G.Xw[3 * slot + 0] = X[0]; G.Xw[3 * slot + 1] = X[1]; G.Xw[3 * slot + 2] = X[2];
    G.obs[3 * slot + 0] = k.x; G.obs[3 * slot + 1] = k.y; G.obs[3 * slot + 2] = ur;
    G.is2[slot] = invS2[min(max(k.octave, 0), nlevels - 1)];
}

// TrackWithMotionModel: which pass counts (:1386), whether the function goes on (:1393), and the pose problem of the matches that count.
// A -2 (assigned, then pruned by the rotation histogram) is a NULL in mvpMapPoints, as in the reference.
__global__ __launch_bounds__(TRK_THREADS) void k_track_gather_last(const int32_t *__restrict__ nm, const int32_t *__restrict__ mat1, const int32_t *__restrict__ mat2, int n,
                                                                   const orbx_keypoint *__restrict__ kp, const float *__restrict__ uRight,
                                                                   const float *__restrict__ lastPos, const float *__restrict__ invS2, int nlevels, TrackProblem G)
{
    __shared__ int sWave[TRK_THREADS / 64];
    const int tid = threadIdx.x;
    const int nm1 = nm[0];
    const bool wide = nm1 < 20;
    const int nms = wide ? nm[1] : nm1;
    const int32_t *mat = wide ? mat2 : mat1;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += TRK_THREADS) {
        const int i = i0 + tid;
        const int mi = i < n ? mat[i] : -1;
        const bool has = mi >= 0;
        orbx_keypoint k = {};
        float ur = 0.f, X[3] = {0.f, 0.f, 0.f};
        if (has) { k = kp[i]; ur = uRight[i]; X[0] = lastPos[3 * (size_t)mi]; X[1] = lastPos[3 * (size_t)mi + 1]; X[2] = lastPos[3 * (size_t)mi + 2]; }
        int tot;
        const int slot = base + tile_rank(has, sWave, tot);
        if (i < n) G.featSlot[i] = has ? slot : -1;
        if (has) put_edge(G, slot, X, k, ur, invS2, nlevels);
        base += tot;
    }
    if (tid == 0) { G.ctl[TC_COUNT] = base; G.ctl[TC_SKIP] = nms < 20 ? 1 : 0; G.ctl[TC_WIDE] = wide ? 1 : 0; G.ctl[TC_NMS] = nms; G.ctl[TC_GATE] = nms < 20 ? -1 : base; }
}

// TrackReferenceKeyFrame: the matches of SearchByBoW(pKF, F) (frame feature -> keyframe slot; a pruned match is already -1), whether the function goes
// on (:1201), and the pose problem: the keyframe's map point at the matched slot against the frame's feature.
__global__ __launch_bounds__(TRK_THREADS) void k_track_gather_ref(const int32_t *__restrict__ nm, const int32_t *__restrict__ mat, int n, const orbx_keypoint *__restrict__ kpUn,
                                                                  const float *__restrict__ uRight, const float *__restrict__ kfPos, const float *__restrict__ invS2, int nlevels,
                                                                  TrackProblem G)
{
    __shared__ int sWave[TRK_THREADS / 64];
    const int tid = threadIdx.x;
    const int nms = nm[0];
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += TRK_THREADS) {
        const int i = i0 + tid;
        const int mi = i < n ? mat[i] : -1;
        const bool has = mi >= 0;
        orbx_keypoint k = {};
        float ur = 0.f, X[3] = {0.f, 0.f, 0.f};
        if (has) { k = kpUn[i]; ur = uRight[i]; X[0] = kfPos[3 * (size_t)mi]; X[1] = kfPos[3 * (size_t)mi + 1]; X[2] = kfPos[3 * (size_t)mi + 2]; }
        int tot;
        const int slot = base + tile_rank(has, sWave, tot);
        if (i < n) G.featSlot[i] = has ? slot : -1;
        if (has) put_edge(G, slot, X, k, ur, invS2, nlevels);
        base += tot;
    }
    if (tid == 0) { G.ctl[TC_COUNT] = base; G.ctl[TC_SKIP] = nms < 15 ? 1 : 0; G.ctl[TC_WIDE] = 0; G.ctl[TC_NMS] = nms; G.ctl[TC_GATE] = nms < 15 ? -1 : base; }
}

// TrackLocalMap: the features that hold a MapPoint behind SearchLocalPoints - held on entry, or assigned by the search (which also overwrites a held point
// without observations, src/ORBmatcher.cc:110-112 / :169: the new point's position wins).  assigned == nullptr: no search ran (no local points).
__global__ __launch_bounds__(TRK_THREADS) void k_track_gather_local(const int32_t *__restrict__ assigned, int n, const uint8_t *__restrict__ held,
                                                                    const float *__restrict__ heldPos, const float *__restrict__ pointPos,
                                                                    const orbx_keypoint *__restrict__ kp, const float *__restrict__ uRight,
                                                                    const float *__restrict__ invS2, int nlevels, TrackProblem G)
{
    __shared__ int sWave[TRK_THREADS / 64];
    const int tid = threadIdx.x;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += TRK_THREADS) {
        const int i = i0 + tid;
        const int a = (i < n && assigned) ? assigned[i] : -1;
        const bool has = i < n && (a >= 0 || held[i] != 0);
        orbx_keypoint k = {};
        float ur = 0.f, X[3] = {0.f, 0.f, 0.f};
        if (has) {
            const float *src = a >= 0 ? pointPos + 3 * (size_t)a : heldPos + 3 * (size_t)i;
            k = kp[i]; ur = uRight[i]; X[0] = src[0]; X[1] = src[1]; X[2] = src[2];
        }
        int tot;
        const int slot = base + tile_rank(has, sWave, tot);
        if (i < n) G.featSlot[i] = has ? slot : -1;
        if (has) put_edge(G, slot, X, k, ur, invS2, nlevels);
        base += tot;
    }
    if (tid == 0) { G.ctl[TC_COUNT] = base; G.ctl[TC_SKIP] = 0; G.ctl[TC_WIDE] = 0; G.ctl[TC_NMS] = 0; G.ctl[TC_GATE] = base; }
}

// the workgroup's sums of two per-thread counts, in every thread
__device__ __forceinline__ void block_sum2(int &a, int &b, int *sAcc /* [2], zero on entry (behind a barrier) */)
{
    const int lane = threadIdx.x & 63;
    const int wa = wave_sum_dpp(a), wb = wave_sum_dpp(b);
    if (lane == 0) { if (wa) atomicAdd(&sAcc[0], wa); if (wb) atomicAdd(&sAcc[1], wb); }
    __syncthreads();
    a = sAcc[0]; b = sAcc[1];
}

struct MotionOut { int32_t *matches, *search; uint8_t *discarded; float *pose; int32_t *ints; double *stats; };      // mapped host memory
// ints: nmatches_search, wide, n_correspondences, pose_inliers, nmatches, nmatches_map, ran_pose

// :1403-1421.  The outlier flags come back to feature order through featSlot; every result of the call goes out here, the sequence word behind them.
__global__ __launch_bounds__(TRK_THREADS) void k_track_discard(const int32_t *__restrict__ ctl, const int32_t *__restrict__ mat1, const int32_t *__restrict__ mat2, int n,
                                                               const int32_t *__restrict__ featSlot, const uint8_t *__restrict__ outlier,
                                                               const uint8_t *__restrict__ lastHasObs, const float *__restrict__ tcwCur,
                                                               const float *__restrict__ poseOpt, const int32_t *__restrict__ ret, const double *__restrict__ stats,
                                                               MotionOut O, unsigned long long *pubFlag, unsigned long long pubSeq)
{
    __shared__ int sAcc[2];
    const int tid = threadIdx.x;
    const bool ran = ctl[TC_SKIP] == 0, wide = ctl[TC_WIDE] != 0;
    const int32_t *mat = wide ? mat2 : mat1;
    if (tid < 2) sAcc[tid] = 0;
    __syncthreads();
    int nDisc = 0, nMap = 0;
    for (int i = tid; i < n; i += TRK_THREADS) {
        const int mi = mat[i], s = featSlot[i];
        const bool d = ran && s >= 0 && outlier[s] != 0;                          // :1407
        const bool kept = mi >= 0 && !d;
        O.search[i] = mi;
        O.matches[i] = kept ? mi : -1;                                            // :1411
        O.discarded[i] = d ? 1 : 0;
        nDisc += d ? 1 : 0;                                                       // :1415
        nMap += (ran && kept && (!lastHasObs || lastHasObs[mi] != 0)) ? 1 : 0;    // :1417-1419
    }
    block_sum2(nDisc, nMap, sAcc);
    if (tid < 16) O.pose[tid] = ran ? poseOpt[tid] : tcwCur[tid];
    if (tid < 8) O.stats[tid] = ran ? stats[tid] : 0.0;
    if (tid == 0) {
        O.ints[0] = ctl[TC_NMS]; O.ints[1] = wide ? 1 : 0; O.ints[2] = ctl[TC_COUNT]; O.ints[3] = ran ? ret[0] : 0;
        O.ints[4] = ctl[TC_NMS] - nDisc; O.ints[5] = nMap; O.ints[6] = ran ? 1 : 0;
    }
    orbx_publish(nullptr, pubFlag, pubSeq, 1u);
}

struct LocalOut { int32_t *assigned; uint8_t *outlier, *found, *cleared; float *pose; int32_t *ints; double *stats; };      // mapped host memory
// ints: nmatches, n_correspondences, pose_inliers, inliers_map, inliers_all

// :1464-1489.  Observations() > 0 of the point a feature holds: the point's flag for a new assignment, `occupied` for a point held on entry.
__global__ __launch_bounds__(TRK_THREADS) void k_track_local_stats(const int32_t *__restrict__ ctl, const int32_t *__restrict__ assigned, const int32_t *__restrict__ nmSearch, int n,
                                                                   const int32_t *__restrict__ featSlot, const uint8_t *__restrict__ outlier,
                                                                   const uint8_t *__restrict__ occupied, const uint8_t *__restrict__ pointHasObs, int pointsAllObserved,
                                                                   int sensorStereo, const float *__restrict__ poseOpt, const int32_t *__restrict__ ret,
                                                                   const double *__restrict__ stats, LocalOut O, unsigned long long *pubFlag, unsigned long long pubSeq)
{
    __shared__ int sAcc[2];
    const int tid = threadIdx.x;
    if (tid < 2) sAcc[tid] = 0;
    __syncthreads();
    int nMap = 0, nAll = 0;
    for (int i = tid; i < n; i += TRK_THREADS) {
        const int a = assigned ? assigned[i] : -1, s = featSlot[i];
        const bool edge = s >= 0, out = edge && outlier[s] != 0;
        const bool in = edge && !out;                                                      // :1466-1469
        const bool observed = a >= 0 ? (pointsAllObserved || pointHasObs[a] != 0) : (occupied && occupied[i] != 0);
        O.assigned[i] = a;
        O.outlier[i] = out ? 1 : 0;
        O.found[i] = in ? 1 : 0;                                                           // :1471
        O.cleared[i] = (out && sensorStereo) ? 1 : 0;                                      // :1485-1486
        nAll += in ? 1 : 0;                                                                // :1483
        nMap += (in && observed) ? 1 : 0;                                                  // :1478-1479
    }
    block_sum2(nMap, nAll, sAcc);
    if (tid < 16) O.pose[tid] = poseOpt[tid];
    if (tid < 8) O.stats[tid] = stats[tid];
    if (tid == 0) { O.ints[0] = nmSearch ? nmSearch[0] : 0; O.ints[1] = ctl[TC_COUNT]; O.ints[2] = ret[0]; O.ints[3] = nMap; O.ints[4] = nAll; }
    orbx_publish(nullptr, pubFlag, pubSeq, 1u);
}

// the device working arrays of one chain call, planned once per call into m->trWork
struct TrackWork {
    OrbxSlot<int32_t, ORBX_STAGE_WORK> mat1, mat2, nm, ctl, featSlot, ret;
    OrbxSlot<float, ORBX_STAGE_WORK> Xw, obs, is2, pose;
    OrbxSlot<uint8_t, ORBX_STAGE_WORK> outl;
    OrbxSlot<double, ORBX_STAGE_WORK> stats;
    uint8_t *base = nullptr;
    int plan(orbx_matcher *m, size_t N)
    {
        OrbxWorkPlan &wp = m->trPlan;
        wp.reset();
        mat1 = wp.hole<int32_t>(N); mat2 = wp.hole<int32_t>(N); nm = wp.hole<int32_t>(4); ctl = wp.hole<int32_t>(TC_WORDS); featSlot = wp.hole<int32_t>(N); ret = wp.hole<int32_t>(4);
        Xw = wp.hole<float>(3 * N); obs = wp.hole<float>(3 * N); is2 = wp.hole<float>(N); pose = wp.hole<float>(16);
        outl = wp.hole<uint8_t>(N);
        stats = wp.hole<double>(8);
        const int rc = m->trWork.ensure(wp.total());
        base = m->trWork.p;
        return rc;
    }
    TrackProblem problem() const { return TrackProblem{Xw.in(base), obs.in(base), is2.in(base), featSlot.in(base), ctl.in(base)}; }
};

int pose_link(hipStream_t st, const TrackWork &w, const float *pose0, const float *cam, int cap, int maxCount)
{
    OrbxPoseOptArgs a;
    a.pose0 = pose0; a.cam = cam; a.Xw = w.Xw.in(w.base); a.obs = w.obs.in(w.base); a.invS2 = w.is2.in(w.base); a.counts = w.ctl.in(w.base) + TC_COUNT;
    a.cap = cap; a.maxCount = maxCount;
    a.poseOut = w.pose.in(w.base); a.outlier = w.outl.in(w.base); a.ret = w.ret.in(w.base); a.stats = w.stats.in(w.base);
    a.gate = w.ctl.in(w.base) + TC_GATE;
    return orbx_pose_opt_enqueue(st, a);
}

}  // namespace

#define TRK_MAX_MARKS 8
// profile_kernels: an event at boundary k of the chain
int orbx_match::track_mark(orbx_matcher *m, hipStream_t st, int k)
{
    if (!m->trProfile) return ORBX_OK;
    if (k < 0 || k >= TRK_MAX_MARKS) { orbx_set_error("chain boundary %d outside the %d events of the profiling tap", k, TRK_MAX_MARKS); return ORBX_ERR_ARG; }
    if (m->trEv.size() < TRK_MAX_MARKS) m->trEv.resize(TRK_MAX_MARKS, nullptr);
    if (!m->trEv[k]) { const int rc = orbx_event_create(&m->trEv[k]); if (rc != ORBX_OK) return rc; }
    ORBX_HIP_CHECK(hipEventRecord(m->trEv[k], st));
    m->trTimed = k + 1;
    return ORBX_OK;
}
using orbx_match::track_mark;

extern "C" int orbx_track_set_profiling(orbx_matcher *m, int on)
{
    if (!m) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    m->trProfile = on != 0;
    m->trTimed = 0;
    return ORBX_OK;
}

extern "C" int orbx_track_last_kernel_times(orbx_matcher *m, float *ms, int capacity, int *count)
{
    if (!m || !count) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    *count = 0;
    if (m->trTimed < 2) { orbx_set_error("no profiled tracking chain has run on this handle"); return ORBX_ERR_STATE; }
    ORBX_HIP_CHECK(hipSetDevice(m->device));
    ORBX_HIP_CHECK(hipEventSynchronize(m->trEv[m->trTimed - 1]));
    for (int k = 0; k + 1 < m->trTimed && k < capacity; k++) {
        float t = 0.f;
        ORBX_HIP_CHECK(hipEventElapsedTime(&t, m->trEv[k], m->trEv[k + 1]));
        if (ms) ms[k] = t;
        *count = k + 1;
    }
    return ORBX_OK;
}

extern "C" int orbx_track_with_motion_model(orbx_matcher *m, const orbx_projection_frame *fr, const orbx_projection_last *ls, const float *scale_factors, int nlevels,
                                            const float *inv_level_sigma2, float th, int b_mono, int check_orientation, orbx_track_motion_result *res)
{
    if (!m || !fr || !ls || !res || !inv_level_sigma2) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (!fr->counts || !ls->counts || !ls->tcw_current || !ls->tcw_last) { orbx_set_error("NULL counts or poses"); return ORBX_ERR_ARG; }
    if (!scale_factors || nlevels < 1 || nlevels > 64) { orbx_set_error("bad scale factor table (%d levels, 1..64)", nlevels); return ORBX_ERR_ARG; }
    const int n = fr->counts[0], nl = ls->counts[0];
    if (n > 0 && (!fr->keypoints_un || !fr->descriptors || !fr->u_right)) { orbx_set_error("NULL array in the frame arguments"); return ORBX_ERR_ARG; }
    if (nl > 0 && (!ls->valid || !ls->world_pos || !ls->descriptors || !ls->octave || !ls->angle)) { orbx_set_error("NULL array in the last-frame arguments"); return ORBX_ERR_ARG; }
    // what the function leaves when both searches find nothing (:1393): also the result for an empty side, without a launch
    res->nmatches_search = 0; res->wide = 1; res->n_correspondences = 0; res->pose_inliers = 0; res->nmatches = 0; res->nmatches_map = 0; res->ran_pose = 0;
    for (int k = 0; k < 8; k++) res->stats[k] = 0.0;
    if (n <= 0 || nl <= 0) {
        for (int i = 0; i < n; i++) { if (res->matches) res->matches[i] = -1; if (res->search_matches) res->search_matches[i] = -1; if (res->discarded) res->discarded[i] = 0; }
        if (res->pose) memcpy(res->pose, ls->tcw_current, 64);
        return ORBX_OK;
    }
    if (n > m->maxFeatures) { orbx_set_error("%d features exceed the matcher's max_features %d", n, m->maxFeatures); return ORBX_ERR_CAPACITY; }
    if (nl > 65535 || n > 65535) { orbx_set_error("bad capacities (features %d, last %d)", n, nl); return ORBX_ERR_CAPACITY; }
    int nvalid = 0;
    for (int i = 0; i < nl; i++) nvalid += ls->valid[i] == 1 ? 1 : 0;
    const int maxCount = std::min(n, nvalid);      // every correspondence takes a feature and a valid last-frame point of its own
    if (maxCount > ORBX_TRACK_MAX_CORRESPONDENCES) {
        orbx_set_error("%d possible correspondences exceed the pose kernel's limit %d", maxCount, ORBX_TRACK_MAX_CORRESPONDENCES);
        return ORBX_ERR_CAPACITY;
    }
    if ((size_t)n * 5 + 16 > 160 * 1024) { orbx_set_error("capacities too large for the LDS tile"); return ORBX_ERR_CAPACITY; }
    ORBX_HIP_CHECK(hipSetDevice(m->device));
    int rc;
    hipStream_t st = m->stream;
    OrbxCallBox &bx = m->box;
    const size_t N = (size_t)n, NL = (size_t)nl;
    const int32_t cnt[2] = {n, nl};
    const float cam[5] = {ls->fx, ls->fy, ls->cx, ls->cy, ls->mbf};
    auto [pin, pout] = bx.plan();
    const auto sKp = pin.add(fr->keypoints_un, N);
    const auto sDesc = pin.add(fr->descriptors, N * 32);
    const auto sUr = pin.add(fr->u_right, N);
    const auto sOcc = pin.add(fr->occupied, fr->occupied ? N : 0);
    const auto sCnt = pin.add(cnt, 2);
    const auto sPos = pin.add(ls->world_pos, NL * 3), sAng = pin.add(ls->angle, NL), sTc = pin.add(ls->tcw_current, 16), sTl = pin.add(ls->tcw_last, 16);
    const auto sOct = pin.add(ls->octave, NL);
    const auto sLd = pin.add(ls->descriptors, NL * 32), sVal = pin.add(ls->valid, NL), sObs = pin.add(ls->has_observations, ls->has_observations ? NL : 0);
    const auto sSc = pin.add(scale_factors, (size_t)nlevels), sIs = pin.add(inv_level_sigma2, (size_t)nlevels), sCam = pin.add(cam, 5);
    const auto rMat = pout.hole<int32_t>(N), rSearch = pout.hole<int32_t>(N);
    const auto rDisc = pout.hole<uint8_t>(N);
    const auto rPose = pout.hole<float>(16);
    const auto rInts = pout.hole<int32_t>(8);
    const auto rStats = pout.hole<double>(8);
    const OrbxStaged sg = bx.begin(st, &rc);
    if (rc != ORBX_OK) return rc;
    TrackWork w;
    if ((rc = w.plan(m, N)) != ORBX_OK) return rc;
    if ((rc = track_mark(m, st, 0)) != ORBX_OK) return rc;
    uint8_t *ar;
    if ((rc = orbx_stage_to_arena(bx, m->arena, st, 512, &ar)) != ORBX_OK) return rc;
    ORBX_LAUNCH_CHECK();
    if ((rc = track_mark(m, st, 1)) != ORBX_OK) return rc;
    const int32_t *dCnt = sCnt.in(ar);
    const float *dScales = sSc.in(ar);
    const uint8_t *dHasObs = ls->has_observations ? sObs.in(ar) : nullptr;
    ProjFrameDev F = {sKp.in(ar), sDesc.in(ar), sUr.in(ar), fr->occupied ? sOcc.in(ar) : nullptr, dCnt, n, fr->min_x, fr->min_y, fr->grid_width_inv, fr->grid_height_inv};
    ProjLastDev L = {sVal.in(ar), sPos.in(ar), sLd.in(ar), dHasObs, sOct.in(ar), sAng.in(ar), dCnt + 1, nl,
                     sTc.in(ar), sTl.in(ar), ls->fx, ls->fy, ls->cx, ls->cy, ls->mbf, ls->mb, ls->max_x, ls->max_y};
    int32_t *mat1 = w.mat1.in(w.base), *mat2 = w.mat2.in(w.base), *nm = w.nm.in(w.base);
    // pass 1 with th; pass 2 with 2 * th from cleared matches (its own array), decided on the device: its workgroups leave unless pass 1 counted < 20
    if ((rc = orbx_match::enqueue_proj_last(m, st, F, L, dScales, th, b_mono, check_orientation, mat1, nm, n, nullptr, nullptr, 0ull, ProjGate{nullptr, 0})) != ORBX_OK) return rc;
    if ((rc = track_mark(m, st, 2)) != ORBX_OK) return rc;
    if ((rc = orbx_match::enqueue_proj_last(m, st, F, L, dScales, 2.0f * th, b_mono, check_orientation, mat2, nm + 1, n, nullptr, nullptr, 0ull, ProjGate{nm, 20})) != ORBX_OK) return rc;
    if ((rc = track_mark(m, st, 3)) != ORBX_OK) return rc;
    hipLaunchKernelGGL(k_track_gather_last, dim3(1), dim3(TRK_THREADS), 0, st, nm, mat1, mat2, n, sKp.in(ar), sUr.in(ar), sPos.in(ar), sIs.in(ar), nlevels, w.problem());
    ORBX_LAUNCH_CHECK();
    if ((rc = track_mark(m, st, 4)) != ORBX_OK) return rc;
    // the count is known on the device only: one predicated launch per instantiation up to the host's upper bound (orbx_pose_opt_enqueue)
    if ((rc = pose_link(st, w, sTc.in(ar), sCam.in(ar), std::max(maxCount, 1), maxCount)) != ORBX_OK) return rc;
    if ((rc = track_mark(m, st, 5)) != ORBX_OK) return rc;
    const MotionOut O = {sg.dev(rMat), sg.dev(rSearch), sg.dev(rDisc), sg.dev(rPose), sg.dev(rInts), sg.dev(rStats)};
    const unsigned long long seq = bx.arm();
    hipLaunchKernelGGL(k_track_discard, dim3(1), dim3(TRK_THREADS), 0, st, w.ctl.in(w.base), mat1, mat2, n, w.featSlot.in(w.base), w.outl.in(w.base), dHasObs, sTc.in(ar),
                       w.pose.in(w.base), w.ret.in(w.base), w.stats.in(w.base), O, bx.flagDev, seq);
    ORBX_LAUNCH_CHECK();
    if ((rc = track_mark(m, st, 6)) != ORBX_OK) return rc;
    if ((rc = bx.wait(st)) != ORBX_OK) return rc;
    if (res->matches) memcpy(res->matches, sg.host(rMat), N * 4);
    if (res->search_matches) memcpy(res->search_matches, sg.host(rSearch), N * 4);
    if (res->discarded) memcpy(res->discarded, sg.host(rDisc), N);
    if (res->pose) memcpy(res->pose, sg.host(rPose), 64);
    const int32_t *hi = sg.host(rInts);
    res->nmatches_search = hi[0]; res->wide = hi[1]; res->n_correspondences = hi[2]; res->pose_inliers = hi[3]; res->nmatches = hi[4]; res->nmatches_map = hi[5];
    res->ran_pose = hi[6];
    memcpy(res->stats, sg.host(rStats), 64);
    return ORBX_OK;
}

extern "C" int orbx_track_reference_keyframe(orbx_matcher *m, const orbx_reference_keyframe *kf, const orbx_reference_frame *fr, float nn_ratio, int check_orientation,
                                             orbx_track_reference_result *res)
{
    if (!m || !kf || !fr || !res) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (!kf->features || !fr->features || !kf->features->counts || !fr->features->counts || !fr->tcw || !fr->inv_level_sigma2) { orbx_set_error("NULL counts, pose or level table"); return ORBX_ERR_ARG; }
    if (fr->nlevels < 1 || fr->nlevels > 64) { orbx_set_error("bad level table (%d levels, 1..64)", fr->nlevels); return ORBX_ERR_ARG; }
    const orbx_feature_set *a = kf->features, *b = fr->features;
    const int nA = a->counts[0], n = b->counts[0];
    if (nA > 0 && (!a->keypoints || !a->descriptors || !kf->world_pos)) { orbx_set_error("NULL array in the keyframe arguments"); return ORBX_ERR_ARG; }
    if (n > 0 && (!b->keypoints || !b->descriptors || !fr->keypoints_un || !fr->u_right)) { orbx_set_error("NULL array in the frame arguments"); return ORBX_ERR_ARG; }
    // what the function leaves when the search finds nothing (:1201): also the result for an empty side, without a launch
    res->nmatches_search = 0; res->n_correspondences = 0; res->pose_inliers = 0; res->nmatches = 0; res->nmatches_map = 0; res->ran_pose = 0;
    for (int k = 0; k < 8; k++) res->stats[k] = 0.0;
    if (n <= 0 || nA <= 0) {
        for (int i = 0; i < n; i++) { if (res->matches) res->matches[i] = -1; if (res->search_matches) res->search_matches[i] = -1; if (res->discarded) res->discarded[i] = 0; }
        if (res->pose) memcpy(res->pose, fr->tcw, 64);
        return ORBX_OK;
    }
    if (n > m->maxFeatures || nA > m->maxFeatures) { orbx_set_error("%d / %d features exceed the matcher's max_features %d", nA, n, m->maxFeatures); return ORBX_ERR_CAPACITY; }
    if (n > 4000) { orbx_set_error("%d frame features exceed the pair kernel's LDS bound 4000", n); return ORBX_ERR_CAPACITY; }
    if (nA > 65535 || orbx_match::bow_pair_replay_lds(nA, n, false) > 160 * 1024) { orbx_set_error("feature counts %d / %d too large for the LDS tile of the replay", nA, n); return ORBX_ERR_CAPACITY; }
    int nvalid = nA;
    if (a->valid) { nvalid = 0; for (int i = 0; i < nA; i++) nvalid += a->valid[i] ? 1 : 0; }
    const int maxCount = std::min(n, nvalid);      // every correspondence takes a feature and a valid keyframe slot of its own
    if (maxCount > ORBX_TRACK_MAX_CORRESPONDENCES) {
        orbx_set_error("%d possible correspondences exceed the pose kernel's limit %d", maxCount, ORBX_TRACK_MAX_CORRESPONDENCES);
        return ORBX_ERR_CAPACITY;
    }
    ORBX_HIP_CHECK(hipSetDevice(m->device));
    int rc;
    hipStream_t st = m->stream;
    OrbxCallBox &bx = m->box;
    const size_t N = (size_t)n, NA = (size_t)nA;
    const int32_t cnt[2] = {nA, n};
    const float cam[5] = {fr->fx, fr->fy, fr->cx, fr->cy, fr->mbf};
    auto [pin, pout] = bx.plan();
    const auto sKpA = pin.add(a->keypoints, NA);
    const auto sDescA = pin.add(a->descriptors, NA * 32);
    const auto sGrA = pin.add(a->groups, a->groups ? NA : 0);
    const auto sValA = pin.add(a->valid, a->valid ? NA : 0);
    const auto sKpB = pin.add(b->keypoints, N);
    const auto sDescB = pin.add(b->descriptors, N * 32);
    const auto sGrB = pin.add(b->groups, b->groups ? N : 0);
    const auto sCnt = pin.add(cnt, 2);
    const auto sPos = pin.add(kf->world_pos, NA * 3);
    const auto sObs = pin.add(kf->has_observations, kf->has_observations ? NA : 0);
    const auto sKpUn = pin.add(fr->keypoints_un, N);
    const auto sUr = pin.add(fr->u_right, N);
    const auto sTc = pin.add(fr->tcw, 16);
    const auto sIs = pin.add(fr->inv_level_sigma2, (size_t)fr->nlevels), sCam = pin.add(cam, 5);
    const auto rMat = pout.hole<int32_t>(N), rSearch = pout.hole<int32_t>(N);
    const auto rDisc = pout.hole<uint8_t>(N);
    const auto rPose = pout.hole<float>(16);
    const auto rInts = pout.hole<int32_t>(8);
    const auto rStats = pout.hole<double>(8);
    const OrbxStaged sg = bx.begin(st, &rc);
    if (rc != ORBX_OK) return rc;
    TrackWork w;
    if ((rc = w.plan(m, N)) != ORBX_OK) return rc;
    if ((rc = track_mark(m, st, 0)) != ORBX_OK) return rc;
    uint8_t *ar;
    if ((rc = orbx_stage_to_arena(bx, m->arena, st, 512, &ar)) != ORBX_OK) return rc;
    ORBX_LAUNCH_CHECK();
    if ((rc = track_mark(m, st, 1)) != ORBX_OK) return rc;
    const int32_t *dCnt = sCnt.in(ar);
    const uint8_t *dHasObs = kf->has_observations ? sObs.in(ar) : nullptr;
    FeatDev A, B;      // as orbx_search_by_bow's single-pair path builds them (the frame's valid flags play no part in mode 0)
    A.kp = sKpA.in(ar); A.desc = sDescA.in(ar); A.groups = a->groups ? sGrA.in(ar) : nullptr; A.valid = a->valid ? sValA.in(ar) : nullptr; A.counts = dCnt; A.cap = nA;
    B.kp = sKpB.in(ar); B.desc = sDescB.in(ar); B.groups = b->groups ? sGrB.in(ar) : nullptr; B.valid = nullptr; B.counts = dCnt + 1; B.cap = n;
    int32_t *mat = w.mat1.in(w.base), *nm = w.nm.in(w.base);
    if ((rc = orbx_match::enqueue_bow_pair(m, st, A, B, 0, nn_ratio, check_orientation, mat, m->dists.p, nm, n, nullptr, nullptr, 0ull)) != ORBX_OK) return rc;
    if ((rc = track_mark(m, st, 2)) != ORBX_OK) return rc;
    hipLaunchKernelGGL(k_track_gather_ref, dim3(1), dim3(TRK_THREADS), 0, st, nm, mat, n, sKpUn.in(ar), sUr.in(ar), sPos.in(ar), sIs.in(ar), fr->nlevels, w.problem());
    ORBX_LAUNCH_CHECK();
    if ((rc = track_mark(m, st, 3)) != ORBX_OK) return rc;
    if ((rc = pose_link(st, w, sTc.in(ar), sCam.in(ar), std::max(maxCount, 1), maxCount)) != ORBX_OK) return rc;
    if ((rc = track_mark(m, st, 4)) != ORBX_OK) return rc;
    // :1215-1236 is :1403-1421 with the keyframe's points in the last frame's place: the same kernel (one pass: both match arrays are the search's)
    const MotionOut O = {sg.dev(rMat), sg.dev(rSearch), sg.dev(rDisc), sg.dev(rPose), sg.dev(rInts), sg.dev(rStats)};
    const unsigned long long seq = bx.arm();
    hipLaunchKernelGGL(k_track_discard, dim3(1), dim3(TRK_THREADS), 0, st, w.ctl.in(w.base), mat, mat, n, w.featSlot.in(w.base), w.outl.in(w.base), dHasObs, sTc.in(ar),
                       w.pose.in(w.base), w.ret.in(w.base), w.stats.in(w.base), O, bx.flagDev, seq);
    ORBX_LAUNCH_CHECK();
    if ((rc = track_mark(m, st, 5)) != ORBX_OK) return rc;
    if ((rc = bx.wait(st)) != ORBX_OK) return rc;
    if (res->matches) memcpy(res->matches, sg.host(rMat), N * 4);
    if (res->search_matches) memcpy(res->search_matches, sg.host(rSearch), N * 4);
    if (res->discarded) memcpy(res->discarded, sg.host(rDisc), N);
    if (res->pose) memcpy(res->pose, sg.host(rPose), 64);
    const int32_t *hi = sg.host(rInts);
    res->nmatches_search = hi[0]; res->n_correspondences = hi[2]; res->pose_inliers = hi[3]; res->nmatches = hi[4]; res->nmatches_map = hi[5]; res->ran_pose = hi[6];
    memcpy(res->stats, sg.host(rStats), 64);
    return ORBX_OK;
}

extern "C" int orbx_track_local_map(orbx_matcher *m, const orbx_projection_frame *fr, const orbx_frustum_frame *pose, const orbx_local_points *pt, const float *scale_factors,
                                    int nlevels, float viewing_cos_limit, float th, float nn_ratio, const uint8_t *held, const float *held_world_pos,
                                    const float *inv_level_sigma2, int sensor_stereo, orbx_track_local_result *res)
{
    if (!m || !fr || !pose || !pt || !res || !inv_level_sigma2) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (!fr->counts || !pose->tcw || !pose->ratio_thresholds) { orbx_set_error("NULL array in the frame arguments"); return ORBX_ERR_ARG; }
    const int n = fr->counts[0], mm = pt->count;
    if (!scale_factors || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || pose->nlevels != nlevels) {
        orbx_set_error("scale_factors has %d levels, the frustum arguments name %d (must be equal, 1..%d)", nlevels, pose->nlevels, ORBX_MAX_LEVELS);
        return ORBX_ERR_ARG;
    }
    if (n > 0 && (!fr->keypoints_un || !fr->descriptors || !fr->u_right || !held || !held_world_pos)) { orbx_set_error("NULL array in the frame arguments"); return ORBX_ERR_ARG; }
    if (mm > 0 && (!pt->world_pos || !pt->normal || !pt->max_distance || !pt->min_distance || !pt->descriptors)) { orbx_set_error("NULL array in the point arguments"); return ORBX_ERR_ARG; }
    res->nmatches = 0; res->n_correspondences = 0; res->pose_inliers = 0; res->inliers_map = 0; res->inliers_all = 0;
    for (int k = 0; k < 8; k++) res->stats[k] = 0.0;
    if (n <= 0) {      // a frame without features: the reference still runs Frame::isInFrustum over the points; PoseOptimization returns at once (:509)
        if (res->pose) memcpy(res->pose, pose->tcw, 64);
        if (mm <= 0) return ORBX_OK;
        if (!res->in_view) { orbx_set_error("in_view is needed for a frame without features"); return ORBX_ERR_ARG; }
        const int32_t cm = mm;
        orbx_map_points mp = {pt->world_pos, pt->normal, pt->max_distance, pt->min_distance, &cm, mm};
        return orbx_is_in_frustum(m, pose, &mp, viewing_cos_limit, res->proj_x, res->proj_y, res->proj_xr, res->scale_level, res->view_cos, res->in_view);
    }
    if (n > m->maxFeatures) { orbx_set_error("%d features exceed the matcher's max_features %d", n, m->maxFeatures); return ORBX_ERR_CAPACITY; }
    if (n > 65535) { orbx_set_error("bad capacities (features %d)", n); return ORBX_ERR_CAPACITY; }
    int nheld = 0;
    for (int i = 0; i < n; i++) nheld += held[i] ? 1 : 0;
    const int maxCount = (int)std::min<long long>(n, (long long)nheld + std::max(mm, 0));
    if (maxCount > ORBX_TRACK_MAX_CORRESPONDENCES) {
        orbx_set_error("%d possible correspondences exceed the pose kernel's limit %d", maxCount, ORBX_TRACK_MAX_CORRESPONDENCES);
        return ORBX_ERR_CAPACITY;
    }
    if ((size_t)n * 6 + 16 > 160 * 1024) { orbx_set_error("feature count %d too large for the LDS tile of the projection replay", n); return ORBX_ERR_CAPACITY; }
    ORBX_HIP_CHECK(hipSetDevice(m->device));
    int rc;
    hipStream_t st = m->stream;
    OrbxCallBox &bx = m->box;
    const size_t N = (size_t)n, M = (size_t)std::max(mm, 0);
    const int32_t cnt[2] = {n, std::max(mm, 0)};
    const float cam[5] = {pose->fx, pose->fy, pose->cx, pose->cy, pose->mbf};
    auto [pin, pout] = bx.plan();
    const auto sKp = pin.add(fr->keypoints_un, N);
    const auto sDesc = pin.add(fr->descriptors, N * 32);
    const auto sUr = pin.add(fr->u_right, N);
    const auto sOcc = pin.add(fr->occupied, fr->occupied ? N : 0);
    const auto sCnt = pin.add(cnt, 2);
    const auto sTcw = pin.add(pose->tcw, 16);
    const auto sObs = pin.add(pt->has_observations, pt->has_observations ? M : 0);
    const auto sSc = pin.add(scale_factors, (size_t)nlevels), sIs = pin.add(inv_level_sigma2, (size_t)nlevels), sCam = pin.add(cam, 5);
    const auto sHeld = pin.add(held, N);
    const auto sHeldPos = pin.add(held_world_pos, N * 3);
    const auto sPos = pin.add(pt->world_pos, M * 3), sNrm = pin.add(pt->normal, M * 3), sMax = pin.add(pt->max_distance, M), sMin = pin.add(pt->min_distance, M);
    const auto sPd = pin.add(pt->descriptors, M * 32);
    const auto rPx = pout.hole<float>(M), rPy = pout.hole<float>(M), rPxr = pout.hole<float>(M), rVc = pout.hole<float>(M);
    const auto rLvl = pout.hole<int32_t>(M);
    const auto rIn = pout.hole<uint8_t>(M);
    const auto rAs = pout.hole<int32_t>(N);
    const auto rOutl = pout.hole<uint8_t>(N), rFound = pout.hole<uint8_t>(N), rCleared = pout.hole<uint8_t>(N);
    const auto rPose = pout.hole<float>(16);
    const auto rInts = pout.hole<int32_t>(8);
    const auto rStats = pout.hole<double>(8);
    const OrbxStaged sg = bx.begin(st, &rc);
    if (rc != ORBX_OK) return rc;
    TrackWork w;
    if ((rc = w.plan(m, N)) != ORBX_OK) return rc;
    if ((rc = track_mark(m, st, 0)) != ORBX_OK) return rc;
    uint8_t *ar;
    if ((rc = orbx_stage_to_arena(bx, m->arena, st, 512, &ar)) != ORBX_OK) return rc;
    ORBX_LAUNCH_CHECK();
    if ((rc = track_mark(m, st, 1)) != ORBX_OK) return rc;
    const int32_t *dCnt = sCnt.in(ar);
    const uint8_t *dOcc = fr->occupied ? sOcc.in(ar) : nullptr, *dObs = pt->has_observations ? sObs.in(ar) : nullptr;
    int32_t *as = nullptr, *nm = nullptr;
    if (mm > 0) {
        FrustumDev Fr;
        Fr.tcw = sTcw.in(ar); Fr.fx = pose->fx; Fr.fy = pose->fy; Fr.cx = pose->cx; Fr.cy = pose->cy; Fr.mbf = pose->mbf;
        Fr.minX = pose->min_x; Fr.maxX = pose->max_x; Fr.minY = pose->min_y; Fr.maxY = pose->max_y; Fr.cosLimit = viewing_cos_limit; Fr.nlevels = pose->nlevels;
        for (int k = 0; k < ORBX_MAX_LEVELS; k++) Fr.ratioTh[k] = k + 1 < pose->nlevels ? pose->ratio_thresholds[k] : 0.0f;
        MapPointsDev Mp = {sPos.in(ar), sNrm.in(ar), sMax.in(ar), sMin.in(ar), dCnt + 1, mm};
        ProjFrameDev F = {sKp.in(ar), sDesc.in(ar), sUr.in(ar), dOcc, dCnt, n, fr->min_x, fr->min_y, fr->grid_width_inv, fr->grid_height_inv};
        FrustumHostOut Ho = {sg.dev(rPx), sg.dev(rPy), sg.dev(rPxr), sg.dev(rVc), sg.dev(rLvl), sg.dev(rIn)};
        as = w.mat1.in(w.base); nm = w.nm.in(w.base);
        if ((rc = orbx_match::enqueue_local_points(m, st, Fr, Mp, F, sPd.in(ar), dObs, sSc.in(ar), th, nn_ratio, Ho, as, nm, n, nullptr, nullptr, 0ull)) != ORBX_OK) return rc;
    }
    if ((rc = track_mark(m, st, 2)) != ORBX_OK) return rc;
    hipLaunchKernelGGL(k_track_gather_local, dim3(1), dim3(TRK_THREADS), 0, st, as, n, sHeld.in(ar), sHeldPos.in(ar), sPos.in(ar), sKp.in(ar), sUr.in(ar), sIs.in(ar), nlevels,
                       w.problem());
    ORBX_LAUNCH_CHECK();
    if ((rc = track_mark(m, st, 3)) != ORBX_OK) return rc;
    if ((rc = pose_link(st, w, sTcw.in(ar), sCam.in(ar), std::max(maxCount, 1), maxCount)) != ORBX_OK) return rc;
    if ((rc = track_mark(m, st, 4)) != ORBX_OK) return rc;
    const LocalOut O = {sg.dev(rAs), sg.dev(rOutl), sg.dev(rFound), sg.dev(rCleared), sg.dev(rPose), sg.dev(rInts), sg.dev(rStats)};
    const unsigned long long seq = bx.arm();
    hipLaunchKernelGGL(k_track_local_stats, dim3(1), dim3(TRK_THREADS), 0, st, w.ctl.in(w.base), as, nm, n, w.featSlot.in(w.base), w.outl.in(w.base), dOcc, dObs,
                       pt->has_observations ? 0 : 1, sensor_stereo ? 1 : 0, w.pose.in(w.base), w.ret.in(w.base), w.stats.in(w.base), O, bx.flagDev, seq);
    ORBX_LAUNCH_CHECK();
    if ((rc = track_mark(m, st, 5)) != ORBX_OK) return rc;
    if ((rc = bx.wait(st)) != ORBX_OK) return rc;
    if (mm > 0) {
        const uint8_t *iv = sg.host(rIn);
        if (res->in_view) memcpy(res->in_view, iv, M);
        // (the mTrack* values of a point that is not in view are not written by the kernel: the caller's arrays keep what they held, as with the reference's members)
        const float *hx = sg.host(rPx), *hy = sg.host(rPy), *hxr = sg.host(rPxr), *hvc = sg.host(rVc);
        const int32_t *hl = sg.host(rLvl);
        for (int k = 0; k < mm; k++)
            if (iv[k]) {
                if (res->proj_x) res->proj_x[k] = hx[k];
                if (res->proj_y) res->proj_y[k] = hy[k];
                if (res->proj_xr) res->proj_xr[k] = hxr[k];
                if (res->view_cos) res->view_cos[k] = hvc[k];
                if (res->scale_level) res->scale_level[k] = hl[k];
            }
    }
    if (res->assigned) memcpy(res->assigned, sg.host(rAs), N * 4);
    if (res->outlier) memcpy(res->outlier, sg.host(rOutl), N);
    if (res->found) memcpy(res->found, sg.host(rFound), N);
    if (res->cleared) memcpy(res->cleared, sg.host(rCleared), N);
    if (res->pose) memcpy(res->pose, sg.host(rPose), 64);
    const int32_t *hi = sg.host(rInts);
    res->nmatches = hi[0]; res->n_correspondences = hi[1]; res->pose_inliers = hi[2]; res->inliers_map = hi[3]; res->inliers_all = hi[4];
    memcpy(res->stats, sg.host(rStats), 64);
    return ORBX_OK;
}
