// orbx_triangulate.hip -- new map points: the per-match geometry of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:423-596)
// and the chain over the neighbour keyframes around it (:350-624).  gfx950 only.
//
//   k_triangulate   one launch per neighbour, one lane per KF1 feature slot (or per listed match): rays, parallax, the three-way choice
//                   (4x4 null vector by a one-sided Jacobi SVD in FP64 registers / UnprojectStereo), depth, chi2 and scale tests; status
//                   byte, world point, and the byte store that takes an accepted KF1 feature out of the next neighbour's search.
//                   Latency bound: a few hundred matched lanes among a few thousand, every one a chain of dependent FP64 operations.
//   k_collect       one workgroup at the end of the chain: ordered compaction of the accepted slots (neighbour, then KF1 feature) by a
//                   block scan - DPP inside the wave, LDS across the waves, no atomics - into mapped pinned memory, then the sequence word.
//
// Arithmetic: float where the reference is float; Mat::dot and cv::norm accumulate in double and 1.0/z is a double quotient narrowed to
// float, as oracle/cvshim/cvshim.hpp computes them; 3-term matrix products left to right in float (cvshim.hpp:419-430).  The library is
// built with -ffp-contract=off: every product and sum below is its own operation.
#include <algorithm>
#include <vector>

#include "orbx_match_internal.h"

struct TriCam {
    float tcw[12], ow[3];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
    float sf[ORBX_MAX_LEVELS], sigma2[ORBX_MAX_LEVELS];
    const orbx_keypoint *kp;      // mvKeysUn
    const float *raw;             // mvKeys[i].pt (x, y) or NULL = kp
    const float *ur, *depth;      // mvuRight / mvDepth or NULL = monocular
    int n, nlevels;
};
struct TriArgs {
    TriCam c1, c2;
    float ratioFactor;            // 1.5f * mpCurrentKeyFrame->mfScaleFactor (:343)
};

// cv::Mat::dot / cv::norm of 3-vectors: products and sums in double, from 0 (cvshim.hpp:256-263, 480-491)
__device__ __forceinline__ double dot3d(float a0, float a1, float a2, float b0, float b1, float b2)
{
    double s = (double)a0 * (double)b0;
    s = s + (double)a1 * (double)b1;
    s = s + (double)a2 * (double)b2;
    return s;
}
__device__ __forceinline__ double norm3d(float a0, float a1, float a2) { return sqrt(dot3d(a0, a1, a2, a0, a1, a2)); }

// chi2 reprojection test of one keyframe (:516-542 / :546-570); mbf is ALWAYS the current keyframe's (:534, :562)
__device__ __forceinline__ bool reproj_fails(const TriCam &C, float x, float y, float invz, float kx, float ky, float ur, bool stereo, float sigma2, float mbf1)
{
    const float u = C.fx * x * invz + C.cx;
    const float v = C.fy * y * invz + C.cy;
    const float ex = u - kx, ey = v - ky;
    if (!stereo) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    const float u_r = u - mbf1 * invz;
    const float er = u_r - ur;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:805-827): the RAW keypoint, Twc.rowRange(0,3).colRange(0,3) * x3Dc + Twc.col(3)
__device__ __forceinline__ bool unproject_stereo(const TriCam &C, int idx, float kx, float ky, float (&X)[3])
{
    const float z = C.depth[idx];
    if (!(z > 0)) return false;
    const float u = C.raw ? C.raw[2 * idx] : kx, v = C.raw ? C.raw[2 * idx + 1] : ky;
    const float x = (u - C.cx) * z * C.invfx;
    const float y = (v - C.cy) * z * C.invfy;
#pragma unroll
    for (int i = 0; i < 3; i++) X[i] = (C.tcw[i] * x + C.tcw[4 + i] * y + C.tcw[8 + i] * z) + C.ow[i];      // Rwc = Rcw^T
    return true;
}

// nslots lanes; lane j handles KF1 feature idx1 = list1 ? list1[j] : j and KF2 feature matches[j]; lanes j >= nvalid and unmatched lanes
// write ORBX_NP_NONE.  mask (may be NULL): KF1's eligibility bytes, cleared for an accepted idx1.  nmSrc/nmDst: the search's return value
// is kept per neighbour (m->nmatches is overwritten by the next search).
__global__ __launch_bounds__(256) void k_triangulate(TriArgs T, const int32_t *__restrict__ matches, const int32_t *__restrict__ list1, int nvalid, int nslots,
                                                     uint8_t *__restrict__ mask, uint8_t *__restrict__ status, float *__restrict__ x3d, int32_t *__restrict__ matchCopy,
                                                     const int32_t *__restrict__ nmSrc, int32_t *__restrict__ nmDst)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0 && nmDst) *nmDst = *nmSrc;
    if (j >= nslots) return;
    int idx2 = j < nvalid ? matches[j] : -1;
    const int idx1 = (list1 && j < nvalid) ? list1[j] : j;
    if (idx2 >= T.c2.n || idx1 >= T.c1.n || idx1 < 0) idx2 = -1;
    if (matchCopy) matchCopy[j] = idx2;
    float X[3] = {0.f, 0.f, 0.f};
    int st = ORBX_NP_NONE;
    if (idx2 >= 0) {
        const TriCam &C1 = T.c1, &C2 = T.c2;
        const orbx_keypoint kp1 = C1.kp[idx1], kp2 = C2.kp[idx2];
        const float ur1 = C1.ur ? C1.ur[idx1] : -1.0f, ur2 = C2.ur ? C2.ur[idx2] : -1.0f;
        const bool bStereo1 = ur1 >= 0, bStereo2 = ur2 >= 0;
        const int o1 = min(max(kp1.octave, 0), C1.nlevels - 1), o2 = min(max(kp2.octave, 0), C2.nlevels - 1);
        // rays and their parallax (:437-444)
        const float xn1x = (kp1.x - C1.cx) * C1.invfx, xn1y = (kp1.y - C1.cy) * C1.invfy;
        const float xn2x = (kp2.x - C2.cx) * C2.invfx, xn2y = (kp2.y - C2.cy) * C2.invfy;
        float ray1[3], ray2[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            ray1[i] = C1.tcw[i] * xn1x + C1.tcw[4 + i] * xn1y + C1.tcw[8 + i] * 1.0f;
            ray2[i] = C2.tcw[i] * xn2x + C2.tcw[4 + i] * xn2y + C2.tcw[8 + i] * 1.0f;
        }
        const float cosRays = (float)(dot3d(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]) / (norm3d(ray1[0], ray1[1], ray1[2]) * norm3d(ray2[0], ray2[1], ray2[2])));
        float cosS1 = cosRays + 1, cosS2 = cosS1;
        if (bStereo1) cosS1 = cosf(2 * atan2f(C1.mb / 2, C1.depth[idx1]));
        else if (bStereo2) cosS2 = cosf(2 * atan2f(C2.mb / 2, C2.depth[idx2]));
        const float cosStereo = fminf(cosS1, cosS2);
        bool have = false;
        if (cosRays < cosStereo && cosRays > 0 && (bStereo1 || bStereo2 || cosRays < 0.9998)) {      // (float < double literal, :470)
            float r0[4], r1[4], r2[4], r3[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                r0[c] = xn1x * C1.tcw[8 + c] - C1.tcw[c];
                r1[c] = xn1y * C1.tcw[8 + c] - C1.tcw[4 + c];
                r2[c] = xn2x * C2.tcw[8 + c] - C2.tcw[c];
                r3[c] = xn2y * C2.tcw[8 + c] - C2.tcw[4 + c];
            }
            double nv[4];
            jacobi_null(r0, r1, r2, r3, nv);
            if (nv[3] == 0.0) st = ORBX_NP_W_ZERO;
            else {
#pragma unroll
                for (int i = 0; i < 3; i++) X[i] = (float)(nv[i] / nv[3]);
                have = true; st = ORBX_NP_TRIANGULATED;
            }
        } else if (bStereo1 && cosS1 < cosS2) {
            have = unproject_stereo(C1, idx1, kp1.x, kp1.y, X);
            st = have ? ORBX_NP_STEREO1 : ORBX_NP_DEPTH_INVALID;
        } else if (bStereo2 && cosS2 < cosS1) {
            have = unproject_stereo(C2, idx2, kp2.x, kp2.y, X);
            st = have ? ORBX_NP_STEREO2 : ORBX_NP_DEPTH_INVALID;
        } else
            st = ORBX_NP_LOW_PARALLAX;
        if (have) {
            const int path = st;
            // Rcw.row(i).dot(x3Dt) + tcw(i): a double dot plus a float, narrowed to float (:506-518)
            const float z1 = (float)(dot3d(C1.tcw[8], C1.tcw[9], C1.tcw[10], X[0], X[1], X[2]) + (double)C1.tcw[11]);
            const float z2 = (float)(dot3d(C2.tcw[8], C2.tcw[9], C2.tcw[10], X[0], X[1], X[2]) + (double)C2.tcw[11]);
            if (z1 <= 0) st = ORBX_NP_BEHIND1;
            else if (z2 <= 0) st = ORBX_NP_BEHIND2;
            else {
                const float x1 = (float)(dot3d(C1.tcw[0], C1.tcw[1], C1.tcw[2], X[0], X[1], X[2]) + (double)C1.tcw[3]);
                const float y1 = (float)(dot3d(C1.tcw[4], C1.tcw[5], C1.tcw[6], X[0], X[1], X[2]) + (double)C1.tcw[7]);
                const float invz1 = (float)(1.0 / (double)z1);
                const float x2 = (float)(dot3d(C2.tcw[0], C2.tcw[1], C2.tcw[2], X[0], X[1], X[2]) + (double)C2.tcw[3]);
                const float y2 = (float)(dot3d(C2.tcw[4], C2.tcw[5], C2.tcw[6], X[0], X[1], X[2]) + (double)C2.tcw[7]);
                const float invz2 = (float)(1.0 / (double)z2);
                if (reproj_fails(C1, x1, y1, invz1, kp1.x, kp1.y, ur1, bStereo1, C1.sigma2[o1], C1.mbf)) st = ORBX_NP_REPROJ1;
                else if (reproj_fails(C2, x2, y2, invz2, kp2.x, kp2.y, ur2, bStereo2, C2.sigma2[o2], C1.mbf)) st = ORBX_NP_REPROJ2;
                else {
                    const float dist1 = (float)norm3d(X[0] - C1.ow[0], X[1] - C1.ow[1], X[2] - C1.ow[2]);
                    const float dist2 = (float)norm3d(X[0] - C2.ow[0], X[1] - C2.ow[1], X[2] - C2.ow[2]);
                    if (dist1 == 0 || dist2 == 0) st = ORBX_NP_DIST_ZERO;
                    else {
                        const float ratioDist = dist2 / dist1;
                        const float ratioOctave = C1.sf[o1] / C2.sf[o2];
                        if (ratioDist * T.ratioFactor < ratioOctave || ratioDist > ratioOctave * T.ratioFactor) st = ORBX_NP_SCALE;
                        else st = path;
                    }
                }
            }
            if (st == path && mask) mask[idx1] = 0;      // the feature now holds a MapPoint: not eligible against the next neighbour
        }
    }
    status[j] = (uint8_t)st;
    x3d[3 * (size_t)j] = X[0]; x3d[3 * (size_t)j + 1] = X[1]; x3d[3 * (size_t)j + 2] = X[2];
}

#define COLLECT_THREADS 1024
#define COLLECT_PER 8      /* status bytes per thread and round: one 8-byte load */
// total = neighbours run * stride slots (stride a multiple of 8), slot s = neighbour * stride + idx1.  out: count | nmatches[K] | entries.
__global__ __launch_bounds__(COLLECT_THREADS) void k_collect(const uint8_t *__restrict__ status, const int32_t *__restrict__ matches, const float *__restrict__ x3d,
                                                              const int32_t *__restrict__ nm, int K, int done, int stride, int cap, int32_t *__restrict__ outHead,
                                                              orbx_new_point *__restrict__ outList, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    __shared__ int waveSum[COLLECT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t total = (size_t)done * stride;
    int base = 0;
    for (size_t s0 = 0; s0 < total; s0 += (size_t)COLLECT_THREADS * COLLECT_PER) {
        const size_t s = s0 + (size_t)tid * COLLECT_PER;
        unsigned long long w = 0;
        if (s < total) w = *(const unsigned long long *)(status + s);
        int mine = 0;
#pragma unroll
        for (int b = 0; b < COLLECT_PER; b++) { const unsigned st = (unsigned)(w >> (8 * b)) & 0xffu; mine += (st >= ORBX_NP_TRIANGULATED && st <= ORBX_NP_STEREO2) ? 1 : 0; }
        const int incl = wave_incl_scan_dpp(mine);
        if (lane == 63) waveSum[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int q = 0; q < COLLECT_THREADS / 64; q++) { const int t = waveSum[q]; before += q < wave ? t : 0; all += t; }
        int pos = base + before + incl - mine;
        if (mine) {
#pragma unroll
            for (int b = 0; b < COLLECT_PER; b++) {
                const unsigned st = (unsigned)(w >> (8 * b)) & 0xffu;
                if (st >= ORBX_NP_TRIANGULATED && st <= ORBX_NP_STEREO2) {
                    const size_t sl = s + b;
                    if (pos < cap) {
                        orbx_new_point e;
                        e.neighbour = (int32_t)(sl / (size_t)stride); e.idx1 = (int32_t)(sl % (size_t)stride); e.idx2 = matches[sl]; e.path = (int32_t)st;
                        e.x = x3d[3 * sl]; e.y = x3d[3 * sl + 1]; e.z = x3d[3 * sl + 2];
                        outList[pos] = e;
                    }
                    pos++;
                }
            }
        }
        base += all;
        __syncthreads();
    }
    if (tid == 0) outHead[0] = base < cap ? base : cap;
    for (int k = tid; k < K; k += COLLECT_THREADS) outHead[1 + k] = k < done ? nm[k] : 0;
    orbx_publish(counter, flag, seq, 1);
}

namespace orbx_tri {
static int check_geom(const orbx_keyframe_geom *g, const char *what, int idx)
{
    if (!g->scale_factors || !g->level_sigma2) { orbx_set_error("%s %d: NULL scale tables", what, idx); return ORBX_ERR_ARG; }
    if (g->nlevels < 1 || g->nlevels > ORBX_MAX_LEVELS) { orbx_set_error("%s %d: nlevels %d outside 1..%d", what, idx, g->nlevels, ORBX_MAX_LEVELS); return ORBX_ERR_ARG; }
    return ORBX_OK;
}

static void fill_cam(TriCam &C, const orbx_keyframe_geom *g)
{
    memcpy(C.tcw, g->tcw, sizeof(C.tcw)); memcpy(C.ow, g->center, sizeof(C.ow));
    C.fx = g->fx; C.fy = g->fy; C.cx = g->cx; C.cy = g->cy; C.invfx = g->invfx; C.invfy = g->invfy; C.mb = g->mb; C.mbf = g->mbf;
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) { C.sf[l] = l < g->nlevels ? g->scale_factors[l] : 1.0f; C.sigma2[l] = l < g->nlevels ? g->level_sigma2[l] : 1.0f; }
    C.nlevels = g->nlevels;
}

static int ensure_slots(orbx_matcher *m, size_t slots, size_t K)
{
    int rc;
    if ((rc = m->npStatus.ensure(slots + 8)) != ORBX_OK || (rc = m->npX3d.ensure(3 * slots + 8)) != ORBX_OK || (rc = m->npMatches.ensure(slots + 8)) != ORBX_OK ||
        (rc = m->npNm.ensure(K + 1)) != ORBX_OK)
        return rc;
    return ORBX_OK;
}
}  // namespace orbx_tri

using namespace orbx_tri;

extern "C" int orbx_triangulate_matches(orbx_matcher *m, const orbx_triangulate_pairs *P, uint8_t *status, float *x3d)
{
    if (!m || !P || !status || !x3d) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (P->npairs < 1 || !P->match_offset || !P->geom1 || !P->geom2 || !P->obs1 || !P->obs2) { orbx_set_error("bad triangulation pairs"); return ORBX_ERR_ARG; }
    const int K = P->npairs;
    if (P->match_offset[0] != 0) { orbx_set_error("match_offset[0] must be 0"); return ORBX_ERR_ARG; }
    const int M = P->match_offset[K];
    if (M > 0 && (!P->idx1 || !P->idx2)) { orbx_set_error("NULL match lists"); return ORBX_ERR_ARG; }
    int rc;
    for (int p = 0; p < K; p++) {
        if (P->match_offset[p + 1] < P->match_offset[p]) { orbx_set_error("match_offset decreases at pair %d", p); return ORBX_ERR_ARG; }
        if ((rc = check_geom(&P->geom1[p], "geom1 of pair", p)) != ORBX_OK || (rc = check_geom(&P->geom2[p], "geom2 of pair", p)) != ORBX_OK) return rc;
        const orbx_keyframe_obs *ob[2] = {&P->obs1[p], &P->obs2[p]};
        for (int sd = 0; sd < 2; sd++) {
            const int n = ob[sd]->count;
            if (n < 0) { orbx_set_error("pair %d: negative feature count %d", p, n); return ORBX_ERR_ARG; }      // (nothing here is sized by max_features)
            if (n > 0 && !ob[sd]->keys_un) { orbx_set_error("pair %d: NULL keys_un", p); return ORBX_ERR_ARG; }
            if ((ob[sd]->u_right == nullptr) != (ob[sd]->depth == nullptr)) { orbx_set_error("pair %d: u_right and depth go together", p); return ORBX_ERR_ARG; }
        }
        for (int j = P->match_offset[p]; j < P->match_offset[p + 1]; j++)
            if (P->idx1[j] < 0 || P->idx1[j] >= P->obs1[p].count || P->idx2[j] < 0 || P->idx2[j] >= P->obs2[p].count) {
                orbx_set_error("match %d of pair %d references a feature out of range", j, p); return ORBX_ERR_ARG;
            }
    }
    ORBX_HIP_CHECK(hipSetDevice(m->device));
    if (M == 0) return ORBX_OK;
    ORBX_HIP_CHECK(hipStreamSynchronize(m->stream));      // an earlier call's copy has left the pinned buffer
    OrbxHostStage &hs = m->npStage;
    OrbxInPlan &pl = hs.plan();
    const auto s1 = pl.add(P->idx1, (size_t)M), s2 = pl.add(P->idx2, (size_t)M);
    struct SideSlots { OrbxSlot<orbx_keypoint, ORBX_STAGE_IN> kp; OrbxSlot<float, ORBX_STAGE_IN> raw, ur, dp; };
    std::vector<SideSlots> slots(2 * (size_t)K);
    for (int p = 0; p < K; p++) {
        const orbx_keyframe_obs *ob[2] = {&P->obs1[p], &P->obs2[p]};
        for (int sd = 0; sd < 2; sd++) {
            const size_t n = (size_t)ob[sd]->count;
            SideSlots &S = slots[2 * (size_t)p + sd];
            S.kp = pl.add(ob[sd]->keys_un, n);
            S.raw = pl.add(ob[sd]->keys_raw, ob[sd]->keys_raw ? 2 * n : 0);
            S.ur = pl.add(ob[sd]->u_right, ob[sd]->u_right ? n : 0); S.dp = pl.add(ob[sd]->depth, ob[sd]->depth ? n : 0);
        }
    }
    const OrbxStaged sg = hs.begin(&rc);
    if (rc != ORBX_OK || (rc = ensure_slots(m, (size_t)M, 1)) != ORBX_OK) return rc;
    const int32_t *d1 = sg.dev(s1), *d2 = sg.dev(s2);
    std::vector<TriArgs> args((size_t)K);
    for (int p = 0; p < K; p++) {
        TriArgs &T = args[(size_t)p];
        fill_cam(T.c1, &P->geom1[p]); fill_cam(T.c2, &P->geom2[p]);
        T.ratioFactor = 1.5f * P->geom1[p].scale_factor;
        const orbx_keyframe_obs *ob[2] = {&P->obs1[p], &P->obs2[p]};
        TriCam *cam[2] = {&T.c1, &T.c2};
        for (int sd = 0; sd < 2; sd++) {
            const SideSlots &S = slots[2 * (size_t)p + sd];
            cam[sd]->kp = sg.dev(S.kp);
            cam[sd]->raw = ob[sd]->keys_raw ? sg.dev(S.raw) : nullptr; cam[sd]->ur = ob[sd]->u_right ? sg.dev(S.ur) : nullptr; cam[sd]->depth = ob[sd]->depth ? sg.dev(S.dp) : nullptr;
            cam[sd]->n = ob[sd]->count;
        }
    }
    if ((rc = hs.flush(m->stream)) != ORBX_OK) return rc;
    for (int p = 0; p < K; p++) {
        const int off = P->match_offset[p], n = P->match_offset[p + 1] - off;
        if (n == 0) continue;
        hipLaunchKernelGGL(k_triangulate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, args[(size_t)p], d2 + off, d1 + off, n, n, (uint8_t *)nullptr,
                           m->npStatus.p + off, m->npX3d.p + 3 * (size_t)off, (int32_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr);
        ORBX_LAUNCH_CHECK();
    }
    ORBX_HIP_CHECK(hipStreamSynchronize(m->stream));
    ORBX_HIP_CHECK(hipMemcpy(status, m->npStatus.p, (size_t)M, hipMemcpyDeviceToHost));
    ORBX_HIP_CHECK(hipMemcpy(x3d, m->npX3d.p, (size_t)M * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return ORBX_OK;
}

extern "C" int orbx_create_new_map_points(orbx_matcher *m, const orbx_feature_set *kf1, const orbx_feature_set *nb, const orbx_new_points_params *prm,
                                          const volatile uint8_t *stop_flag, const orbx_new_points_result *res)
{
    if (!m || !kf1 || !nb || !prm || !res) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (!res->created || !res->count || !res->nmatches || !res->pairs_done) { orbx_set_error("NULL result arrays"); return ORBX_ERR_ARG; }
    if (!kf1->keypoints || !kf1->descriptors || !kf1->counts || !nb->keypoints || !nb->descriptors || !nb->counts) { orbx_set_error("NULL feature arrays"); return ORBX_ERR_ARG; }
    if (!prm->geom1 || !prm->geom2 || !prm->f12 || !prm->epipole) { orbx_set_error("NULL geometry"); return ORBX_ERR_ARG; }
    if ((prm->u_right1 == nullptr) != (prm->depth1 == nullptr) || (prm->u_right2 == nullptr) != (prm->depth2 == nullptr)) { orbx_set_error("u_right and depth go together"); return ORBX_ERR_ARG; }
    const int K = nb->nframes, cap1 = kf1->capacity, cap2 = nb->capacity, n1 = kf1->counts[0];
    if (K < 1 || kf1->nframes != 1) { orbx_set_error("kf1 holds one frame, the neighbours at least one (got %d / %d)", kf1->nframes, K); return ORBX_ERR_ARG; }
    if (cap1 < 1 || cap2 < 1 || cap1 > m->maxFeatures || cap2 > m->maxFeatures) { orbx_set_error("feature capacity %d/%d exceeds the matcher's max_features %d", cap1, cap2, m->maxFeatures); return ORBX_ERR_CAPACITY; }
    if (n1 < 0 || n1 > cap1) { orbx_set_error("kf1 holds %d features, capacity %d", n1, cap1); return ORBX_ERR_CAPACITY; }
    for (int k = 0; k < K; k++)
        if (nb->counts[k] < 0 || nb->counts[k] > cap2) { orbx_set_error("neighbour %d holds %d features, capacity %d", k, nb->counts[k], cap2); return ORBX_ERR_CAPACITY; }
    if (res->created_capacity < n1) { orbx_set_error("created_capacity %d below the %d features of kf1", res->created_capacity, n1); return ORBX_ERR_CAPACITY; }
    int rc;
    if ((rc = check_geom(prm->geom1, "geom1", 0)) != ORBX_OK) return rc;
    for (int k = 0; k < K; k++) if ((rc = check_geom(&prm->geom2[k], "geom2", k)) != ORBX_OK) return rc;
    const size_t ldsGreedy = (size_t)cap2 * 4 + (size_t)cap1 * 4 + (size_t)((cap1 + 7) & ~7) * 2 * 2;      // k_bow_greedy's tile (orbx_search_for_triangulation_device)
    if (ldsGreedy > 160 * 1024) { orbx_set_error("feature capacity %d/%d too large for the LDS tile", cap1, cap2); return ORBX_ERR_CAPACITY; }
    ORBX_HIP_CHECK(hipSetDevice(m->device));

    // ---- stage KF1 and the K neighbours once: one pinned buffer, one copy ----
    OrbxHostStage &hs = m->npStage;
    const size_t C1 = (size_t)cap1, N1 = (size_t)n1, A2 = (size_t)K * cap2;
    const int stride = (cap1 + 7) & ~7;
    // KF1's arrays hold n1 elements on the host and capacity elements on the device
    OrbxInPlan &pl = hs.plan();
    const auto sKp1 = pl.add(kf1->keypoints, N1, C1);
    const auto sDesc1 = pl.add(kf1->descriptors, N1 * 32, C1 * 32);
    const int32_t heads[2] = {n1, 0};
    const auto sHeads = pl.add(heads, 2);
    const auto sG1 = pl.add(kf1->groups, kf1->groups ? N1 : 0, kf1->groups ? C1 : 0);
    const auto sMask = pl.add(kf1->valid, kf1->valid ? N1 : 0, C1);      // (no valid flags: a hole, all ones below)
    const auto sSt1 = pl.hole<uint8_t>(C1);
    const auto sRaw1 = pl.add(prm->keys_raw1, prm->keys_raw1 ? 2 * N1 : 0, prm->keys_raw1 ? 2 * C1 : 0);
    const auto sUr1 = pl.add(prm->u_right1, prm->u_right1 ? N1 : 0, prm->u_right1 ? C1 : 0), sDp1 = pl.add(prm->depth1, prm->depth1 ? N1 : 0, prm->depth1 ? C1 : 0);
    const auto sKp2 = pl.add(nb->keypoints, A2);
    const auto sDesc2 = pl.add(nb->descriptors, A2 * 32);
    const auto sCnt2 = pl.add(nb->counts, (size_t)K);
    const auto sG2 = pl.add(nb->groups, nb->groups ? A2 : 0);
    const auto sV2 = pl.add(nb->valid, nb->valid ? A2 : 0);
    const auto sSt2 = pl.hole<uint8_t>(A2);
    const auto sRaw2 = pl.add(prm->keys_raw2, prm->keys_raw2 ? 2 * A2 : 0), sUr2 = pl.add(prm->u_right2, prm->u_right2 ? A2 : 0), sDp2 = pl.add(prm->depth2, prm->depth2 ? A2 : 0);
    const auto sPair = pl.hole<int32_t>((size_t)K);
    const auto sF12 = pl.add(prm->f12, (size_t)K * 9), sEpi = pl.add(prm->epipole, (size_t)K * 2);
    OrbxCallBox &bx = m->box;
    auto [pin, pout] = bx.plan();
    (void)pin;
    const auto rHead = pout.hole<int32_t>((size_t)K + 1);
    const auto rList = pout.hole<orbx_new_point>((size_t)res->created_capacity);
    const OrbxStaged bg = bx.begin(m->stream, &rc);      // (waits for a call that was abandoned half way)
    if (rc != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipStreamSynchronize(m->stream));      // an earlier call's copy has left the pinned buffer
    const OrbxStaged sg = hs.begin(&rc);
    if (rc != ORBX_OK || (rc = ensure_slots(m, (size_t)K * stride, (size_t)K)) != ORBX_OK) return rc;
    if (prm->profile_kernels)
        while (m->npTriEv.size() < 2 * (size_t)K) { hipEvent_t e = nullptr; ORBX_HIP_CHECK(hipEventCreate(&e)); m->npTriEv.push_back(e); }
    if ((rc = m->npTimer.create()) != ORBX_OK) return rc;

    orbx_feature_set da = *kf1, db = *nb;
    TriCam cam1, cam2;
    fill_cam(cam1, prm->geom1);
    da.keypoints = sg.dev(sKp1);
    da.descriptors = sg.dev(sDesc1);
    da.counts = sg.dev(sHeads);
    da.groups = kf1->groups ? sg.dev(sG1) : nullptr;
    uint8_t *const mask = sg.dev(sMask);
    if (!kf1->valid) memset(sg.host(sMask), 1, N1);
    da.valid = mask;
    uint8_t *const st1 = sg.dev(sSt1);
    for (size_t i = 0; i < N1; i++) sg.host(sSt1)[i] = prm->u_right1 ? (prm->u_right1[i] >= 0 ? 1 : 0) : 0;
    cam1.kp = da.keypoints; cam1.raw = prm->keys_raw1 ? sg.dev(sRaw1) : nullptr; cam1.ur = prm->u_right1 ? sg.dev(sUr1) : nullptr; cam1.depth = prm->depth1 ? sg.dev(sDp1) : nullptr; cam1.n = n1;

    db.keypoints = sg.dev(sKp2); db.descriptors = sg.dev(sDesc2);
    db.counts = sg.dev(sCnt2);
    db.groups = nb->groups ? sg.dev(sG2) : nullptr; db.valid = nb->valid ? sg.dev(sV2) : nullptr;
    uint8_t *const st2 = sg.dev(sSt2);
    for (size_t i = 0; i < A2; i++) sg.host(sSt2)[i] = prm->u_right2 ? (prm->u_right2[i] >= 0 ? 1 : 0) : 0;
    const float *raw2 = sg.dev(sRaw2), *ur2 = sg.dev(sUr2), *dp2 = sg.dev(sDp2);
    for (int k = 0; k < K; k++) sg.host(sPair)[k] = k;
    m->npTimer.timed = false; m->npTriTimed = 0;
    if ((rc = m->npTimer.begin(m->stream)) != ORBX_OK) return rc;
    if ((rc = hs.flush(m->stream)) != ORBX_OK) return rc;

    // ---- the chain: search k, triangulate k, (mask), search k+1 ... all on m->stream ----
    const unsigned long long seq = bx.arm();      // before the first launch: an error below leaves the box pending and the next begin() drains the stream
    // the pair indices, F12 and the epipole are read by the search from the PINNED copy: its uploads stay asynchronous
    const int32_t *hostZero = sg.host(sHeads) + 1, *hostPair = sg.host(sPair);
    const float *hostF12 = sg.host(sF12), *hostEpi = sg.host(sEpi);
    int done = 0;
    for (int k = 0; k < K; k++) {
        if (k > 0 && stop_flag && *stop_flag) break;      // :353
        orbx_triangulation_params tp;
        tp.f12 = hostF12 + 9 * (size_t)k; tp.epipole = hostEpi + 2 * (size_t)k;
        tp.stereo_a = st1; tp.stereo_b = st2;
        tp.scale_factors = prm->geom2[k].scale_factors; tp.level_sigma2 = prm->geom2[k].level_sigma2; tp.nlevels = prm->geom2[k].nlevels;
        tp.check_orientation = prm->check_orientation;
        if ((rc = orbx_search_for_triangulation_device(m, &da, &db, hostZero, hostPair + k, 1, &tp, nullptr)) != ORBX_OK) return rc;
        fill_cam(cam2, &prm->geom2[k]);
        const size_t o2 = (size_t)k * cap2;
        cam2.kp = db.keypoints + o2; cam2.raw = prm->keys_raw2 ? raw2 + 2 * o2 : nullptr; cam2.ur = prm->u_right2 ? ur2 + o2 : nullptr; cam2.depth = prm->depth2 ? dp2 + o2 : nullptr;
        cam2.n = nb->counts[k];
        TriArgs T;
        T.c1 = cam1; T.c2 = cam2; T.ratioFactor = 1.5f * prm->geom1->scale_factor;
        const size_t so = (size_t)k * stride;
        if (prm->profile_kernels) ORBX_HIP_CHECK(hipEventRecord(m->npTriEv[2 * (size_t)k], m->stream));
        hipLaunchKernelGGL(k_triangulate, dim3((unsigned)((stride + 255) / 256)), dim3(256), 0, m->stream, T, (const int32_t *)m->matches.p, (const int32_t *)nullptr, n1, stride, mask,
                           m->npStatus.p + so, m->npX3d.p + 3 * so, m->npMatches.p + so, (const int32_t *)m->nmatches.p, m->npNm.p + k);
        ORBX_LAUNCH_CHECK();
        if (prm->profile_kernels) ORBX_HIP_CHECK(hipEventRecord(m->npTriEv[2 * (size_t)k + 1], m->stream));
        done++;
    }
    // Results: k_collect writes them into mapped pinned memory and raises the sequence word.  (A device list fetched with one copy behind a
    // stream synchronisation measured 9 - 17 us slower per call at every shape of profiles/new_points_latency.txt and was removed.)
    int32_t *outHead = bg.dev(rHead);
    orbx_new_point *outList = bg.dev(rList);
    hipLaunchKernelGGL(k_collect, dim3(1), dim3(COLLECT_THREADS), 0, m->stream, (const uint8_t *)m->npStatus.p, (const int32_t *)m->npMatches.p, (const float *)m->npX3d.p,
                       (const int32_t *)m->npNm.p, K, done, stride, res->created_capacity, outHead, outList, bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_CHECK();
    if ((rc = m->npTimer.end(m->stream)) != ORBX_OK) return rc;
    m->npTimer.launches = 4 * done + 1;      // k_bow_order, k_bow_topk, k_bow_greedy, k_triangulate per neighbour; k_collect
    m->npTriTimed = prm->profile_kernels ? done : 0;
    if ((rc = bx.wait(m->stream)) != ORBX_OK) return rc;      // the one synchronisation
    const int32_t *head = bg.host(rHead);
    const int cnt = head[0];
    *res->count = cnt; *res->pairs_done = done;
    memcpy(res->nmatches, head + 1, (size_t)K * 4);
    if (cnt > 0) memcpy(res->created, bg.host(rList), (size_t)cnt * sizeof(orbx_new_point));
    if (res->status || res->matches || res->x3d) {      // the optional per-slot arrays (tests, diagnostics): copies of their own
        ORBX_HIP_CHECK(hipStreamSynchronize(m->stream));
        for (int k = 0; k < K; k++) {
            const size_t so = (size_t)k * stride, ho = (size_t)k * cap1;
            if (k >= done) {
                if (res->status) memset(res->status + ho, 0, C1);
                if (res->matches) for (size_t i = 0; i < C1; i++) res->matches[ho + i] = -1;
                if (res->x3d) memset(res->x3d + 3 * ho, 0, 3 * C1 * sizeof(float));
                continue;
            }
            if (res->status) ORBX_HIP_CHECK(hipMemcpy(res->status + ho, m->npStatus.p + so, C1, hipMemcpyDeviceToHost));
            if (res->matches) ORBX_HIP_CHECK(hipMemcpy(res->matches + ho, m->npMatches.p + so, C1 * 4, hipMemcpyDeviceToHost));
            if (res->x3d) ORBX_HIP_CHECK(hipMemcpy(res->x3d + 3 * ho, m->npX3d.p + 3 * so, 3 * C1 * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    return ORBX_OK;
}

extern "C" int orbx_new_points_last_timing(orbx_matcher *m, float *device_ms, int *launches, float *triangulate_ms)
{
    if (!m) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (const int rc = m->npTimer.read(m->device, device_ms, launches, "no orbx_create_new_map_points call to report")) return rc;
    float tri = 0.f;
    for (int k = 0; k < m->npTriTimed; k++) {
        float t = 0.f;
        ORBX_HIP_CHECK(hipEventElapsedTime(&t, m->npTriEv[2 * (size_t)k], m->npTriEv[2 * (size_t)k + 1]));
        tri += t;
    }
    if (triangulate_ms) *triangulate_ms = tri;
    return ORBX_OK;
}
