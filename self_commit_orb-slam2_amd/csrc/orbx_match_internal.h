// orbx_match_internal.h -- shared by orbx_match.hip (SearchByBoW, SearchForTriangulation, stereo) and orbx_match_proj.hip
// (the projection / area searches): constants, device-side views and helpers, and the matcher handle.
#ifndef ORBX_MATCH_INTERNAL_H
#define ORBX_MATCH_INTERNAL_H

#include "orbx_handle.h"
#include <vector>

#define TH_HIGH 100       /* src/ORBmatcher.cc:49 */
#define TH_LOW 50         /* :50 */
#define HISTO_LENGTH 30   /* :51 */
#define KEY_EMPTY 0xffffffffu
#define TOPK 8            /* candidates kept per KeyFrame feature; the exact rescan handles overflow */
#define MATCH_PROF_RING 64

#define KEY64_EMPTY 0xffffffffffffffffull
#define GRID_COLS 64   /* include/Frame.h:60 */
#define GRID_ROWS 48   /* include/Frame.h:55 */

struct FeatDev {   // orbx_feature_set with device pointers
    const orbx_keypoint *kp;
    const uint8_t *desc;
    const int32_t *counts;
    const int32_t *groups;
    const uint8_t *valid;
    int cap;
};

__device__ __forceinline__ int hamming256(const unsigned long long a[4], unsigned long long b0, unsigned long long b1, unsigned long long b2,
                                          unsigned long long b3)
{
    return __popcll(a[0] ^ b0) + __popcll(a[1] ^ b1) + __popcll(a[2] ^ b2) + __popcll(a[3] ^ b3);
}

// ComputeThreeMaxima (src/ORBmatcher.cc:1866-1908) of a rotation histogram in LDS, by one wave with a bin per lane: the scan's strict comparisons in
// ascending bin order pick the three largest counts, equal counts in bin order, an empty bin never - i.e. the three largest keys count << 5 | (31 - bin)
// among the non-empty bins.  (Every thread walking the thirty bins itself is ~360 instructions; with sixteen waves on one CU that was 3.5 us of the
// replay kernels.)  Every wave of a workgroup may call it: same result.
__device__ __forceinline__ void three_maxima_wave(const int *hist, int lane, int &ind1, int &ind2, int &ind3)
{
    const int c = lane < HISTO_LENGTH ? hist[lane] : 0;
    uint32_t key = c > 0 ? ((uint32_t)c << 5) | (uint32_t)(31 - lane) : 0u;
    uint32_t top[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        uint32_t v = key;      // (wave_max written out: as a call k_search_init and k_proj_last_greedy come out with other instructions)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(v, o); v = u > v ? u : v; }
        top[k] = v;
        if (key == v) key = 0u;
    }
    const int max1 = (int)(top[0] >> 5), max2 = (int)(top[1] >> 5), max3 = (int)(top[2] >> 5);
    ind1 = top[0] ? 31 - (int)(top[0] & 31u) : -1; ind2 = top[1] ? 31 - (int)(top[1] & 31u) : -1; ind3 = top[2] ? 31 - (int)(top[2] & 31u) : -1;
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
}

struct ProjFrameDev { const orbx_keypoint *kp; const uint8_t *desc; const float *uRight; const uint8_t *occupied; const int32_t *counts; int cap;
                      float minX, minY, gwInv, ghInv;
                      const int32_t *frameOf; };      // k_fuse_best only: problem f searches the staged frame frameOf[f]; nullptr (what every other caller leaves) = frame f

// ORBmatcher::Fuse's search (k_fuse_best, orbx_match_proj.hip): the prepared points of one list per keyframe
struct FusePointsDev { const float *u, *v, *ur; const int32_t *level; const float *radius; const uint8_t *active, *desc; const int32_t *counts; int cap;
                       float kfMinX, kfMinY;
                       const int32_t *descOf; };      // list f's descriptors are row descOf[f] of `desc` (lists that share a keyframe's points); nullptr = row f
struct FuseLevels { float invSigma2[ORBX_MAX_LEVELS]; };

// The views of the two tracking searches (kernels in orbx_match_proj.hip; orbx_track.hip chains them through enqueue_proj_last / enqueue_local_points)
// SearchByProjection(CurrentFrame, LastFrame, th, bMono): the last frame's side
struct ProjLastDev { const uint8_t *valid; const float *pos; const uint8_t *desc, *hasObs; const int32_t *octave; const float *angle; const int32_t *counts;
                     int cap; const float *tcwCur, *tcwLast; float fx, fy, cx, cy, mbf, mb, maxX, maxY; };
// Frame::isInFrustum: the frame's side, the map points, and where k_frustum_topk leaves the mTrack* values for the caller (mapped host memory)
struct FrustumDev {
    const float *tcw;        // [16] per frame
    float fx, fy, cx, cy, mbf, minX, maxX, minY, maxY, cosLimit;
    int nlevels;
    float ratioTh[ORBX_MAX_LEVELS];   // ratioTh[k] = largest ratio with PredictScale <= k, k = 0 .. nlevels-2
};
struct MapPointsDev { const float *pos, *normal, *maxDist, *minDist; const int32_t *counts; int cap; };
struct FrustumHostOut { float *px, *py, *pxr, *vc; int32_t *lvl; uint8_t *inView; };
// "skip unless": a launch that is enqueued unconditionally and decided on the device - its workgroups leave at once, writing nothing, unless
// *word < below.  word == nullptr: run.
struct ProjGate { const int32_t *word; int below; };

// The greedy area search as a link of a chain (orbx_reloc.hip): H problems that share ONE frame.  status[f] != 0: problem f's workgroups leave at once;
// descBase[f]: first descriptor (32-byte units into the queries' descriptor array) of problem f's queries; blocked[f * F.cap + j]: feature j is taken
// from the start in problem f.
struct AreaChainDev { const int32_t *status, *descBase; const uint8_t *blocked; };
// ... its queries: problem f's query i at f * cap + i (descriptors: see descBase), counts[f] queries
struct AreaQueriesArgs { const float *u, *v, *radius; const int32_t *minLevel, *maxLevel; const uint8_t *active, *desc; const int32_t *counts; int cap;
                         float winMinX, winMinY; };

struct orbx_matcher : OrbxHandle {
    int maxFeatures = 0, maxPairs = 0;
    hipEvent_t evDep = nullptr;
    hipEvent_t ev0[MATCH_PROF_RING] = {}, ev1[MATCH_PROF_RING] = {};   // one pair per *_device call (ring)
    hipEvent_t evMid[MATCH_PROF_RING] = {};                             // SearchByBoW: between the distance kernel and the greedy replay
    bool midValid[MATCH_PROF_RING] = {};
    float lastDistanceMs = 0.f, lastReplayMs = 0.f;
    int profCount = 0;
    OrbxOwnedBuf<int32_t> pairsA, pairsB, order, matches, dists, nmatches;
    OrbxOwnedBuf<uint32_t> topk;
    OrbxOwnedBuf<float> scales, uright, depth, pf[2];          // pf: projection staging (floats)
    OrbxOwnedBuf<unsigned long long> topk64;
    OrbxOwnedBuf<uint8_t> pb[2];
    OrbxOwnedBuf<int32_t> pi32[2];
    OrbxOwnedBuf<orbx_keypoint> pkp;
    OrbxOwnedBuf<uint32_t> projDec, projQueue;   // k_proj_greedy: chosen feature per map point, rescan queue
    OrbxHostStage hostStage;     // host-array entry points: all inputs of a call in one pinned buffer, one copy
    OrbxCallBox box;             // single-call host entry points of the tracking thread: mapped pinned inputs / results + sequence word (no copy engine, no stream sync)
    OrbxOwnedBuf<uint8_t> arena;   // ... their inputs on the device, copied there once by k_stage_copy (same offsets as in box.in)
    OrbxOwnedBuf<int32_t> sad;
    OrbxOwnedBuf<int32_t> stRowStart, stRowList;   // ComputeStereoMatches: vRowIndices of the right frames (k_stereo_rows)
    hipEvent_t evDep2 = nullptr;
    int lastStereoPairs = 0;
    // orbx_stereo_frame (one stereo frame, host-synchronous): scale tables as last uploaded, a device zero for the pair arrays, pinned results
    float sfScales[128] = {};
    int sfLevels = 0;
    OrbxOwnedBuf<int32_t> sfZero;
    OrbxOwnedBuf<float> sfScalesDev;               // its own copy of the tables: the other calls overwrite `scales`
    float *sfHost = nullptr, *sfHostDev = nullptr;   // pinned: uright | depth, written by the kernels across PCIe
    size_t sfHostFloats = 0;
    int sfSeq = 0, sfFlagSeq = 0;                 // k_stereo_one: call counter; the value the kernel of the pending call writes into the pinned completion word (0: none)
    int sfPending = 0;                            // orbx_stereo_frame_begin .. _end: 0 none, 1 launched (results land in sfHost), 2 the general path ran (download at the end)
    // staging for the host-array convenience calls
    OrbxOwnedBuf<orbx_keypoint> hk[2];
    OrbxOwnedBuf<uint8_t> hd[2], hv[2];
    OrbxOwnedBuf<int32_t> hc[2], hg[2];
    OrbxOwnedBuf<uint8_t> hs[2];                               // SearchForTriangulation: stereo flags (host form)
    OrbxOwnedBuf<float> triGeom;                               // F12 + epipole per pair
    // Frame::isInFrustum results (proj_x | proj_y | proj_xr | view_cos, level, in_view), orbx_projection_points layout
    OrbxOwnedBuf<float> frProj;
    OrbxOwnedBuf<int32_t> frLevel;
    OrbxOwnedBuf<uint8_t> frInView;
    size_t frCount = 0;
    int lastPairs = 0, lastStride = 0;
    OrbxOwnedBuf<int> producerStatus;   // OR of the capacity words of the extractors this handle's calls were chained behind
    // new map points (orbx_triangulate.hip): KF1 + the K neighbours staged once (pinned buffer, one copy), per-slot results of every neighbour
    OrbxHostStage npStage;
    OrbxOwnedBuf<uint8_t> npStatus;     // [K * npStride]
    OrbxOwnedBuf<float> npX3d;          // [K * npStride * 3]
    OrbxOwnedBuf<int32_t> npMatches;    // [K * npStride]: the matches of each search (m->matches is overwritten by the next one)
    OrbxOwnedBuf<int32_t> npNm;         // [K]
    OrbxCallTimer npTimer;            // (its events are made by the first call)
    std::vector<hipEvent_t> npTriEv;  // profile_kernels: one pair per neighbour
    int npTriTimed = 0;
    // SearchInNeighbors (orbx_fuse_chain.hip): the mutable map state, the per-call prepare / search arrays and the rank tables
    OrbxOwnedBuf<uint8_t> fcWork;
    OrbxWorkPlan fcPlan;
    OrbxCallTimer fcTimer;            // (its events are made by the first call)
    std::vector<hipEvent_t> fcApplyEv;  // profile_kernels: one pair per Fuse call
    int fcApplyTimed = 0;
    std::vector<int32_t> fcOrder, fcPos, fcSIndex;      // slots in ascending rank, slot -> position, slot -> searchable index
    // TrackWithMotionModel / TrackLocalMap / TrackReferenceKeyFrame (orbx_track.hip): match arrays, the gathered pose problem and the optimisation's results, all device memory
    OrbxOwnedBuf<uint8_t> trWork;
    OrbxWorkPlan trPlan;
    std::vector<hipEvent_t> trEv;     // profile_kernels: one event per boundary between the chain's launches
    int trTimed = 0;
    bool trProfile = false;
    // Relocalization's refine loop (orbx_reloc.hip): the per-hypothesis state, queries, pose problems and results of one call, all device memory
    OrbxOwnedBuf<uint8_t> rlWork;
    OrbxWorkPlan rlPlan;
    // LoopClosing::ComputeSim3's refine step for every Sim3Solver event (orbx_loop_sim3.hip): seeds, query lists, search results, OptimizeSim3's problems and result blocks
    OrbxOwnedBuf<uint8_t> lsWork;
    OrbxWorkPlan lsPlan;
    OrbxCallTimer lsTimer;            // (its events are made by the first call)
    ~orbx_matcher()
    {
        hipEvent_t *const one[] = {&evDep, &evDep2};
        for (hipEvent_t *e : one) if (*e) (void)hipEventDestroy(*e);
        for (int r = 0; r < MATCH_PROF_RING; r++)
            for (hipEvent_t e : {ev0[r], ev1[r], evMid[r]}) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : npTriEv) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : fcApplyEv) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : trEv) if (e) (void)hipEventDestroy(e);
        if (sfHost) (void)hipHostFree(sfHost);
    }
};

// ---- shared by orbx_triangulate.hip (CreateNewMapPoints) and orbx_initializer.hip (Initializer::Triangulate) ----
// Sweeps of the one-sided Jacobi.  Chosen on the CPU with the same Jacobi restated in numpy float64 (tests/triangulate_ref.py::jacobi_null) over
// the test scenes (sideways 0.4 / forward 0.6 / sideways 0.05 baselines, depth 3-10, mono / mixed / stereo) and near-degenerate ones (parallax
// at the 0.9998 bound, motion along the optical axis, points 100 baselines away): against the float64 SVD the triangulated x3D was off by up to
// 1e-2 of its distance after 2 sweeps, 9.3e-8 after 3, and equal in every float32 bit after 4, 5, 6 and 8 (cyclic Jacobi converges
// quadratically; a 4x4 has six pairs).  The count after which nothing changes is 4; + 2 = 6.
// tests/test_new_map_points.py::test_jacobi_sweeps_settled asserts that 4 and 6 sweeps give the same bits on all of those scenes.
#define TRI_JACOBI_SWEEPS 6

#ifdef __HIPCC__
// Null vector of the 4x4 float matrix A (rows r0..r3): one-sided (Hestenes) Jacobi in FP64 on the columns of A, V accumulated alongside;
// the column of V under the smallest column norm is vt.row(3).  Everything is indexed by compile-time constants: registers, no scratch.
__device__ __forceinline__ void jacobi_null(const float (&r0)[4], const float (&r1)[4], const float (&r2)[4], const float (&r3)[4], double (&nv)[4])
{
    double a[4][4], v[4][4];      // [column][row]
#pragma unroll
    for (int c = 0; c < 4; c++) {
        a[c][0] = (double)r0[c]; a[c][1] = (double)r1[c]; a[c][2] = (double)r2[c]; a[c][3] = (double)r3[c];
#pragma unroll
        for (int r = 0; r < 4; r++) v[c][r] = r == c ? 1.0 : 0.0;
    }
#pragma unroll 1
    for (int sweep = 0; sweep < TRI_JACOBI_SWEEPS; sweep++) {
#pragma unroll
        for (int p = 0; p < 3; p++) {
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int r = 0; r < 4; r++) { alpha = alpha + a[p][r] * a[p][r]; beta = beta + a[q][r] * a[q][r]; gamma = gamma + a[p][r] * a[q][r]; }
                double c = 1.0, s = 0.0;
                if (gamma != 0.0) {
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = c * t;
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double ap = a[p][r], aq = a[q][r];
                    a[p][r] = c * ap - s * aq;
                    a[q][r] = s * ap + c * aq;
                    const double vp = v[p][r], vq = v[q][r];
                    v[p][r] = c * vp - s * vq;
                    v[q][r] = s * vp + c * vq;
                }
            }
        }
    }
    double best = 0.0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        double n2 = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) n2 = n2 + a[c][r] * a[c][r];
        const bool take = c == 0 || n2 < best;      // the first of equal norms
        best = take ? n2 : best;
#pragma unroll
        for (int r = 0; r < 4; r++) nv[r] = take ? v[c][r] : nv[r];
    }
}
#endif

// host helpers defined in orbx_match.hip
namespace orbx_match {
int prep_pairs(orbx_matcher *m, const orbx_feature_set *a, const orbx_feature_set *b, const int32_t *pa, const int32_t *pb, int npairs, orbx_extractor *after);
int chain_back(orbx_matcher *m, orbx_extractor *after);
int inherit_status(orbx_matcher *m, orbx_extractor *after, bool first = true);
int check_producer_status(orbx_matcher *m);
FeatDev to_dev(const orbx_feature_set *s);
/* stage one frame of host features per side (nsides = 1 or 2) into the matcher's staging buffer; d[side] receives the device view */
int stage_host(orbx_matcher *m, const orbx_feature_set *const *h, orbx_feature_set *const *d, int nsides);
/* k_fuse_best (orbx_match_proj.hip) for one keyframe with chi2_gate = 1: P.cap slots, the list's length read on the device from P.counts */
void launch_fuse_best(hipStream_t st, const ProjFrameDev &F, const FusePointsDev &P, const FuseLevels &LV, int32_t *bestIdx, int32_t *bestDist);
/* ... for nlists problems with chi2_gate = 0 in ONE launch: F.frameOf / P.descOf name each list's keyframe and descriptor row; results at [f * P.cap + i] */
void launch_fuse_best_lists(hipStream_t st, const ProjFrameDev &F, const FusePointsDev &P, const FuseLevels &LV, int nlists, int32_t *bestIdx, int32_t *bestDist);
/* k_proj_last_topk + k_proj_last_greedy for ONE frame (F.cap features, L.cap last-frame features; every pointer device memory) on `st`:
 * matches[0..stride) and nmatches[0] as orbx_search_by_projection_last_device leaves them.  pubFlag != nullptr: the replay also writes
 * pubAssigned[0..n] (mapped host memory) and raises the sequence word.  Both launches obey `gate`.  Grows the handle's candidate / replay buffers. */
int enqueue_proj_last(orbx_matcher *m, hipStream_t st, const ProjFrameDev &F, const ProjLastDev &L, const float *scalesDev, float th, int bMono, int checkOri,
                      int32_t *matches, int32_t *nmatches, int stride, int32_t *pubAssigned, unsigned long long *pubFlag, unsigned long long pubSeq, ProjGate gate);
/* k_frustum_topk + k_proj_greedy for ONE frame (Tracking::SearchLocalPoints): the mTrack* values go to the handle's frustum arrays and to H, the
 * matches as above.  hasObs may be nullptr (= all). */
int enqueue_local_points(orbx_matcher *m, hipStream_t st, const FrustumDev &Fr, const MapPointsDev &Mp, const ProjFrameDev &F, const uint8_t *pointDesc,
                         const uint8_t *hasObs, const float *scalesDev, float th, float nnRatio, const FrustumHostOut &H, int32_t *matches, int32_t *nmatches,
                         int stride, int32_t *pubAssigned, unsigned long long *pubFlag, unsigned long long pubSeq);
/* k_area_topk + k_area_greedy for the H problems of a chain on `st` (every pointer device memory): assigned / dists [f * A.cap + i] and nmatches[f] as
 * orbx_area_search_greedy leaves them, untouched where status[f] != 0.  F.counts[0] features, shared by all problems.  Grows the handle's candidate buffer. */
int enqueue_area_greedy(orbx_matcher *m, hipStream_t st, const ProjFrameDev &F, const AreaQueriesArgs &A, const AreaChainDev &C, int H, int maxDist,
                        int32_t *assigned, int32_t *dists, int32_t *nmatches);
/* k_bow_topk_pair + k_bow_greedy for ONE (KeyFrame A, Frame / KeyFrame B) pair on `st` (every pointer device memory; A.cap / B.cap = the two feature
 * counts, also at A.counts[0] / B.counts[0]): matches[0..stride), dists and nmatches[0] as orbx_search_by_bow_device leaves them for pair 0.
 * pubFlag != nullptr: the replay also writes the match list and the count behind it to pubMatches (mapped host memory) and raises the sequence word -
 * orbx_search_by_bow's single-pair path.  B.cap <= 4000 (B sits in the pair kernel's LDS); ORBX_ERR_CAPACITY if the replay's tile
 * (bow_pair_replay_lds) exceeds 160 KB.  Grows the handle's candidate / order buffers. */
size_t bow_pair_replay_lds(int nA, int nB, bool publish);
int enqueue_bow_pair(orbx_matcher *m, hipStream_t st, const FeatDev &A, const FeatDev &B, int mode, float nnRatio, int checkOri, int32_t *matches, int32_t *dists,
                     int32_t *nmatches, int stride, int32_t *pubMatches, unsigned long long *pubFlag, unsigned long long pubSeq);
/* The K-pair form: k_bow_topk_cands + k_bow_greedy (K workgroups) for K candidate KeyFrames (A: candidate c's features at c * A.cap, A.counts[c] of them -
 * 0 = its workgroups leave at once) against ONE Frame (B, B.cap features), mode 0.  pairsA / pairsB: device arrays 0..K-1 / K zeros.  Results in the
 * handle's buffers as orbx_search_by_bow_device leaves them: matches / dists at c * stride, nmatches[c]; K <= max_pairs, A.cap and B.cap <= stride <=
 * max_features, B.cap <= 4000. */
int enqueue_bow_candidates(orbx_matcher *m, hipStream_t st, const FeatDev &A, const FeatDev &B, int K, const int32_t *pairsA, const int32_t *pairsB, float nnRatio, int checkOri,
                           int stride);
/* profile_kernels of the tracking thread's chains (orbx_track.hip): an event at boundary k of the chain on `st` while orbx_track_set_profiling is on */
int track_mark(orbx_matcher *m, hipStream_t st, int k);
}  // namespace orbx_match

#endif
