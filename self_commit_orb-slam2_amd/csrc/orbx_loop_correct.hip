// orbx_loop_correct.hip -- the two passes of the loop closer that move the map (gfx950 only): the Sim3 propagation of LoopClosing::CorrectLoop
// and the map update after global bundle adjustment.
//
// Reference: src/LoopClosing.cc:617-716 and :930-1003.  Both are stateless, synchronous calls: host arrays go through mapped pinned memory
// (OrbxCallBox: no copy engine, no stream synchronisation), the results come back the same way behind a polled sequence word.  The pointer
// bookkeeping around them (Replace, AddObservation, UpdateConnections, the mutexes) stays with the caller (shim/LoopClosing_hip.cc).
//
// A. orbx_loop_correct_sim3.  The keyframe poses are float 3x4 rows, the Sim3 arithmetic is g2o's in double (orbx_sim3_group.h), the refresh of a
// moved point is MapPoint::UpdateNormalAndDepth on the OpenCV stand-in (orbx_normal_depth.h).  Twc of the current keyframe is DERIVED on the
// device from its tcw by KeyFrame::SetPose's own steps (Rwc = Rcw^T, Ow = (-Rwc) * tcw as a float 3-term product, last row 0 0 0 1); Tiw * Twc
// is the stand-in's 4x4 float product, accumulated left to right over all four terms (the fourth, t * 0 or t * 1, is not dropped).
//   k_stage_copy   the call's inputs from mapped memory into the arena (a point's flags and a keyframe's centre are read many times)
//   k_lc_sim3      a thread per group keyframe: NonCorrectedSim3, CorrectedSim3, its inverse, the SE3 pose and centre that SetPose derives,
//                  [sR | t]; a thread per point: the claim word = INT_MAX
//   k_lc_claim     a workgroup per group list: atomicMin of the group position on every point of the list that is neither bad nor done - the
//                  point is moved by the FIRST keyframe in group order that lists it, whatever the scheduling
//   k_lc_move      a 64-thread workgroup per point: the claimed point is mapped through the non-corrected and the inverse corrected Sim3 in double
//                  and narrowed; a thread per observer computes the unit vector - towards the NEW centre of a group keyframe at an earlier
//                  position than the corrector (it has had its SetPose), towards the old one otherwise - and lanes 0..3 do the ordered part
//                  (sequential float sum in list order, the distances through the reference keyframe's centre, picked by the same rule)
//   k_lc_results   the results, written by the kernels above into device memory, into the mapped result buffer in one coalesced pass
//
// B. orbx_loop_propagate_gba.  The breadth-first walk of :930-960 gives a keyframe the BA did not optimise the pose (Tchild * Twc_parent) *
// TcwGBA_parent, both factors of the first product from the poses before the update: the value depends only on the chain of non-optimised
// ancestors, top down.  The host walks the tree once (it has to anyway: it finds cycles and the reached set) and sorts the non-optimised reached
// keyframes by their depth in such chains; the products themselves are the device's:
//   k_stage_copy   the keyframe arrays into the arena (the point arrays are read once, in place, from mapped memory)
//   k_lg_chain     ONE workgroup, level by level behind a barrier: a thread per keyframe of the level, 4x4 float products left to right
//   k_lg_points    a thread per point: untouched / mPosGBA / Rwc * (Rcw_bef * X + tcw_bef) + twc with Rwc, twc as SetPose(TcwGBA) stores them
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "orbx_handle.h"
#include "orbx_normal_depth.h"
#include "orbx_sim3_group.h"

#define LC_THREADS 256
#define LC_POINT_THREADS 64
#define LC_CLAIM_BLOCKS 1024

namespace {

struct LcDev {
    int NK, G, M, cur;
    const float *tcw, *ow;                 // [NK][12], [NK][3]
    const int32_t *groupKf, *groupPos;     // [G] slot of position g, [NK] position of a slot or -1
    const double *scw;                     // [8]
    const int32_t *listOff, *listPt;       // [G + 1], [S]
    const float *pos;                      // [M][3]
    const uint8_t *bad, *done;             // [M]
    const int32_t *ref;                    // [M]
    const float *rsc, *tsc;                // [M]
    const int32_t *obsOff, *obsKf;         // [M + 1], [T]
    int32_t *claim;                        // work [M]
    double *wNonc, *wSwi;                  // work [G][8]
    float *wOwNew;                         // work [G][3]
    float *unit;                           // work [T][3]
    double *oNonc, *oCorr;                 // results (device memory, copied out by k_lc_results) [G][8]
    float *oTiw, *oOwNew, *oScwMat;        // results [G][12], [G][3], [G][12]
    float *oPos;                           // results [M][3]
    int32_t *oBy;                          // results [M]
    float *oNormal, *oMax, *oMin;          // results [M][3], [M], [M]
    uint8_t *oUpd;                         // results [M]
};

// KeyFrame::SetPose's own steps on a 3x4 float pose: Rwc = Rcw^T, Ow = (-Rwc) * tcw (inner dimension 3: a0 b0 + a1 b1 + a2 b2 in float, left to right)
__device__ __forceinline__ void lc_inverse_pose(const float *__restrict__ T, float (&Rwc)[9], float (&Ow)[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rwc[3 * i + j] = T[4 * j + i];
#pragma unroll
    for (int i = 0; i < 3; i++) Ow[i] = ((-Rwc[3 * i]) * T[3] + (-Rwc[3 * i + 1]) * T[7]) + (-Rwc[3 * i + 2]) * T[11];
}

// rows 0..2 of A * B for 4x4 float matrices kept as 3x4 rows over a last row 0 0 0 1: all FOUR terms, left to right (cvshim.hpp:419-435)
__device__ __forceinline__ void lc_mul44(const float *__restrict__ A, const float (&B)[12], float (&C)[12])
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float b3 = j == 3 ? 1.0f : 0.0f;
            C[4 * i + j] = ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * b3;
        }
}

__device__ __forceinline__ void lc_sim3_of_pose(const float *T, OsSim3 &S)      // g2o::Sim3(toMatrix3d(R), toVector3d(t), 1.0)
{
    const double R[9] = {(double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10]};
    os_quat_from_R(R, S.q);
    S.t[0] = (double)T[3]; S.t[1] = (double)T[7]; S.t[2] = (double)T[11];
    S.s = 1.0;
}

__device__ __forceinline__ void lc_store_sim3(double *o, const OsSim3 &S)
{
    o[0] = S.q[0]; o[1] = S.q[1]; o[2] = S.q[2]; o[3] = S.q[3]; o[4] = S.t[0]; o[5] = S.t[1]; o[6] = S.t[2]; o[7] = S.s;
}

__device__ __forceinline__ void lc_load_sim3(const double *o, OsSim3 &S)
{
    S.q[0] = o[0]; S.q[1] = o[1]; S.q[2] = o[2]; S.q[3] = o[3]; S.t[0] = o[4]; S.t[1] = o[5]; S.t[2] = o[6]; S.s = o[7];
}

__global__ __launch_bounds__(LC_THREADS) void k_lc_sim3(LcDev D)
{
    const int g = blockIdx.x * LC_THREADS + threadIdx.x;
    if (g < D.M) D.claim[g] = INT_MAX;
    if (g >= D.G) return;
    const float *Tiw = D.tcw + (size_t)D.groupKf[g] * 12;
    OsSim3 scw, nonc, corr, swi;
    lc_load_sim3(D.scw, scw);
    lc_sim3_of_pose(Tiw, nonc);
    if (g == D.cur) corr = scw;
    else {
        float Rwc[9], Ow[3], Twc[12], Tic[12];
        lc_inverse_pose(D.tcw + (size_t)D.groupKf[D.cur] * 12, Rwc, Ow);
#pragma unroll
        for (int i = 0; i < 3; i++) { Twc[4 * i] = Rwc[3 * i]; Twc[4 * i + 1] = Rwc[3 * i + 1]; Twc[4 * i + 2] = Rwc[3 * i + 2]; Twc[4 * i + 3] = Ow[i]; }
        lc_mul44(Tiw, Twc, Tic);
        OsSim3 sic;
        lc_sim3_of_pose(Tic, sic);
        os_mul(sic, scw, corr);
    }
    os_inverse(corr, swi);
    lc_store_sim3(D.wNonc + (size_t)g * 8, nonc); lc_store_sim3(D.oNonc + (size_t)g * 8, nonc);
    lc_store_sim3(D.wSwi + (size_t)g * 8, swi); lc_store_sim3(D.oCorr + (size_t)g * 8, corr);
    // :702-710: eigR = toRotationMatrix(), eigt *= (1. / s), toCvSE3; SetPose derives the centre
    double R[9];
    os_quat_to_R(corr.q, R);
    const double inv = 1.0 / corr.s;
    float P[12];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        P[4 * i] = (float)R[3 * i]; P[4 * i + 1] = (float)R[3 * i + 1]; P[4 * i + 2] = (float)R[3 * i + 2];
        P[4 * i + 3] = (float)(corr.t[i] * inv);
    }
    float Rn[9], On[3];
    lc_inverse_pose(P, Rn, On);
    float *oT = D.oTiw + (size_t)g * 12, *oS = D.oScwMat + (size_t)g * 12;
#pragma unroll
    for (int k = 0; k < 12; k++) oT[k] = P[k];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        D.wOwNew[(size_t)g * 3 + i] = On[i]; D.oOwNew[(size_t)g * 3 + i] = On[i];
        oS[4 * i] = (float)(corr.s * R[3 * i]); oS[4 * i + 1] = (float)(corr.s * R[3 * i + 1]); oS[4 * i + 2] = (float)(corr.s * R[3 * i + 2]);      // Converter::toCvMat(Sim3)
        oS[4 * i + 3] = (float)corr.t[i];
    }
}

__global__ __launch_bounds__(LC_THREADS) void k_lc_claim(LcDev D)
{
    for (int g = blockIdx.x; g < D.G; g += gridDim.x) {
        const int e1 = D.listOff[g + 1];
        for (int e = D.listOff[g] + threadIdx.x; e < e1; e += LC_THREADS) {
            const int p = D.listPt[e];
            if (p < 0 || D.bad[p] || D.done[p]) continue;      // :677-682
            atomicMin(&D.claim[p], g);
        }
    }
}

// the centre GetCameraCenter() returns for keyframe slot k while the keyframe at group position g is being processed
__device__ __forceinline__ const float *lc_centre(const LcDev &D, int k, int g)
{
    const int gp = D.groupPos[k];
    return gp >= 0 && gp < g ? D.wOwNew + (size_t)gp * 3 : D.ow + (size_t)k * 3;
}

__global__ __launch_bounds__(LC_POINT_THREADS) void k_lc_move(LcDev D)
{
    const int t = threadIdx.x;
    for (int p = blockIdx.x; p < D.M; p += gridDim.x) {
        const int g = D.claim[p];
        const float *P = D.pos + (size_t)p * 3;
        const int o0 = D.obsOff[p], n = D.obsOff[p + 1] - o0;
        float np[3] = {P[0], P[1], P[2]};
        const bool moved = g != INT_MAX;
        if (moved) {      // :687-692 (uniform over the workgroup)
            OsSim3 siw, swi;
            lc_load_sim3(D.wNonc + (size_t)g * 8, siw);
            lc_load_sim3(D.wSwi + (size_t)g * 8, swi);
            const double X[3] = {(double)P[0], (double)P[1], (double)P[2]};
            double a[3], b[3];
            os_map(siw, X, a);
            os_map(swi, a, b);
            np[0] = (float)b[0]; np[1] = (float)b[1]; np[2] = (float)b[2];
            float *unit = D.unit + (size_t)o0 * 3;
            for (int o = t; o < n; o += LC_POINT_THREADS) mp_unit(np, lc_centre(D, D.obsKf[o0 + o], g), unit + (size_t)o * 3);
        }
        __syncthreads();      // the unit vectors (global memory, this workgroup's own) are visible to lanes 0..2
        const bool upd = moved && n > 0;      // UpdateNormalAndDepth returns early without observations
        if (t < 3) {
            D.oPos[(size_t)p * 3 + t] = np[t];
            D.oNormal[(size_t)p * 3 + t] = upd ? mp_normal_component(D.unit + (size_t)o0 * 3, n, t) : 0.0f;
        } else if (t == 3) {
            float mx = 0.0f, mn = 0.0f;
            if (upd) mp_depth(np, lc_centre(D, D.ref[p], g), D.rsc[p], D.tsc[p], &mx, &mn);
            D.oMax[p] = mx; D.oMin[p] = mn;
            D.oBy[p] = moved ? g : -1;
            D.oUpd[p] = upd ? 1 : 0;
        }
    }
}

// the results, laid out in device memory as the call box's result buffer is, into that buffer in whole 16-byte units: a point's results are 37 bytes
// in six arrays, and six small stores per point across PCIe cost 40 ns a point
__global__ __launch_bounds__(LC_THREADS) void k_lc_results(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n16, unsigned *counter, unsigned long long *flag,
                                                           unsigned long long seq)
{
    for (size_t i = blockIdx.x * (size_t)LC_THREADS + threadIdx.x; i < n16; i += (size_t)gridDim.x * LC_THREADS) dst[i] = src[i];
    orbx_publish(counter, flag, seq, gridDim.x);
}

struct LgDev {
    int n, M, L;
    const float *tcw, *gbaIn;              // arena [n][12]
    const int32_t *parent;                 // arena [n]
    const uint8_t *reached;                // arena [n]
    const int32_t *order, *levelOff;       // arena: the non-optimised reached keyframes by chain depth, [L + 1]
    float *gba;                            // work [n][12]: TcwGBA, completed level by level
    const float *pos, *posGba;             // mapped, read in place [M][3]
    const uint8_t *ptIn, *ptBad;           // mapped [M]
    const int32_t *ref;                    // mapped [M]
    float *oGba;                           // mapped [n][12]
    float *oPos;                           // mapped [M][3]
    uint8_t *oMoved;                       // mapped [M]
};

__global__ __launch_bounds__(LC_THREADS) void k_lg_chain(LgDev D)
{
    const int t = threadIdx.x;
    const size_t n12 = (size_t)D.n * 12;
    for (size_t i = t; i < n12; i += LC_THREADS) D.gba[i] = D.gbaIn[i];
    __syncthreads();
    for (int l = 0; l < D.L; l++) {
        const int i1 = D.levelOff[l + 1];
        for (int i = D.levelOff[l] + t; i < i1; i += LC_THREADS) {
            const int c = D.order[i], p = D.parent[c];
            float Rwc[9], Ow[3], Twc[12], Tcp[12], Gp[12], Gc[12];
            lc_inverse_pose(D.tcw + (size_t)p * 12, Rwc, Ow);      // GetPoseInverse() of the parent BEFORE its update (:937)
#pragma unroll
            for (int r = 0; r < 3; r++) { Twc[4 * r] = Rwc[3 * r]; Twc[4 * r + 1] = Rwc[3 * r + 1]; Twc[4 * r + 2] = Rwc[3 * r + 2]; Twc[4 * r + 3] = Ow[r]; }
            lc_mul44(D.tcw + (size_t)c * 12, Twc, Tcp);          // Tchildc = pChild->GetPose() * Twc (:946)
#pragma unroll
            for (int k = 0; k < 12; k++) Gp[k] = D.gba[(size_t)p * 12 + k];
            lc_mul44(Tcp, Gp, Gc);                                 // mTcwGBA = Tchildc * pKF->mTcwGBA (:949)
#pragma unroll
            for (int k = 0; k < 12; k++) D.gba[(size_t)c * 12 + k] = Gc[k];
        }
        __syncthreads();      // the level's poses (global memory, this workgroup's own) are visible to the next level
    }
    for (size_t i = t; i < n12; i += LC_THREADS) D.oGba[i] = D.gba[i];
}

__global__ __launch_bounds__(LC_THREADS) void k_lg_points(LgDev D, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    const size_t p = (size_t)blockIdx.x * LC_THREADS + threadIdx.x;
    if (p < (size_t)D.M) {
        float X[3] = {D.pos[p * 3], D.pos[p * 3 + 1], D.pos[p * 3 + 2]};
        uint8_t moved = 0;
        if (!D.ptBad[p]) {
            const int r = D.ref[p];
            if (D.ptIn[p]) {      // :975-979
                X[0] = D.posGba[p * 3]; X[1] = D.posGba[p * 3 + 1]; X[2] = D.posGba[p * 3 + 2];
                moved = 1;
            } else if (r >= 0 && D.reached[r]) {      // :983-1002
                const float *B = D.tcw + (size_t)r * 12;
                float Xc[3], Rwc[9], twc[3];
#pragma unroll
                for (int i = 0; i < 3; i++) Xc[i] = ((B[4 * i] * X[0] + B[4 * i + 1] * X[1]) + B[4 * i + 2] * X[2]) + B[4 * i + 3];
                lc_inverse_pose(D.gba + (size_t)r * 12, Rwc, twc);      // what SetPose(mTcwGBA) stored
#pragma unroll
                for (int i = 0; i < 3; i++) X[i] = ((Rwc[3 * i] * Xc[0] + Rwc[3 * i + 1] * Xc[1]) + Rwc[3 * i + 2] * Xc[2]) + twc[i];
                moved = 2;
            }
        }
        D.oPos[p * 3] = X[0]; D.oPos[p * 3 + 1] = X[1]; D.oPos[p * 3 + 2] = X[2];
        D.oMoved[p] = moved;
    }
    orbx_publish(counter, flag, seq, gridDim.x);
}

}  // namespace

struct orbx_loop : OrbxHandle {
    OrbxCallTimer timer;
    OrbxCallBox box;
    OrbxOwnedBuf<uint8_t> arena;      // the staged inputs in device memory
    OrbxOwnedBuf<uint8_t> work;       // claim words, the group's Sim3s and centres, unit vectors | TcwGBA
    OrbxWorkPlan workPlan;            // ... their layout
    OrbxOwnedBuf<uint8_t> results;    // orbx_loop_correct_sim3: the results before they cross to the host in one piece
    std::vector<int32_t> groupPos, order, levelOff, level;
    std::vector<uint8_t> reached;
};

extern "C" int orbx_loop_create(int device, orbx_loop **out)
{
    if (!out) { orbx_set_error("orbx_loop_create: NULL argument"); return ORBX_ERR_ARG; }
    *out = nullptr;
    orbx_loop *h = new orbx_loop();
    int rc;
    if ((rc = h->open(device)) || (rc = h->timer.create())) { orbx_destroy_handle(h); return rc; }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_loop_destroy(orbx_loop *h) { orbx_destroy_handle(h); }

namespace {

bool lc_all_finite(const float *a, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(a[i])) return false;
    return true;
}

int lc_check_offsets(const int32_t *off, int count, int total, const char *name, const char *totalName, const char *who)
{
    if (off[0] != 0) { orbx_set_error("%s: %s does not start at 0", who, name); return ORBX_ERR_ARG; }
    for (int i = 0; i < count; i++)
        if (off[i + 1] < off[i]) { orbx_set_error("%s: %s decreases at %d", who, name, i); return ORBX_ERR_ARG; }
    if (off[count] != total) { orbx_set_error("%s: %s ends at %d, %s = %d", who, name, off[count], totalName, total); return ORBX_ERR_ARG; }
    return ORBX_OK;
}

// everything a kernel indexes with is checked here, before the handle is looked at and before anything is launched
int lc_validate_sim3(const orbx_loop_sim3_problem *p, std::vector<int32_t> &groupPos)
{
    const char *who = "orbx_loop_correct_sim3";
    if (!p) { orbx_set_error("%s: NULL problem", who); return ORBX_ERR_ARG; }
    const int NK = p->num_keyframes, G = p->num_group, M = p->num_points, S = p->num_entries, T = p->num_obs;
    if (NK < 1 || G < 1 || G > NK || M < 0 || S < 0 || T < 0) { orbx_set_error("%s: num_keyframes < 1, num_group < 1 or beyond num_keyframes, or a negative size", who); return ORBX_ERR_ARG; }
    if (!p->tcw || !p->ow || !p->group_kf || !p->scw || !p->list_offset || !p->obs_offset || (S > 0 && !p->list_point) || (T > 0 && !p->obs_kf) ||
        (M > 0 && (!p->pos || !p->point_bad || !p->point_done || !p->point_ref || !p->ref_scale || !p->top_scale))) {
        orbx_set_error("%s: NULL problem array", who);
        return ORBX_ERR_ARG;
    }
    if (p->current < 0 || p->current >= G) { orbx_set_error("%s: current = %d is no group position (0..%d)", who, p->current, G - 1); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = lc_check_offsets(p->list_offset, G, S, "list_offset", "num_entries", who)) != ORBX_OK) return rc;
    if ((rc = lc_check_offsets(p->obs_offset, M, T, "obs_offset", "num_obs", who)) != ORBX_OK) return rc;
    groupPos.assign((size_t)NK, -1);
    for (int g = 0; g < G; g++) {
        const int k = p->group_kf[g];
        if (k < 0 || k >= NK) { orbx_set_error("%s: group_kf[%d] = %d is no keyframe slot (0..%d)", who, g, k, NK - 1); return ORBX_ERR_ARG; }
        if (groupPos[(size_t)k] >= 0) { orbx_set_error("%s: two group entries (%d and %d) name keyframe slot %d", who, groupPos[(size_t)k], g, k); return ORBX_ERR_ARG; }
        groupPos[(size_t)k] = g;
    }
    for (int e = 0; e < S; e++)
        if (p->list_point[e] < -1 || p->list_point[e] >= M) { orbx_set_error("%s: list_point[%d] = %d is no point (-1..%d)", who, e, p->list_point[e], M - 1); return ORBX_ERR_ARG; }
    for (int o = 0; o < T; o++)
        if (p->obs_kf[o] < 0 || p->obs_kf[o] >= NK) { orbx_set_error("%s: obs_kf[%d] = %d is no keyframe slot (0..%d)", who, o, p->obs_kf[o], NK - 1); return ORBX_ERR_ARG; }
    for (int i = 0; i < M; i++)
        if (p->point_ref[i] < 0 || p->point_ref[i] >= NK) { orbx_set_error("%s: point_ref[%d] = %d is no keyframe slot (0..%d)", who, i, p->point_ref[i], NK - 1); return ORBX_ERR_ARG; }
    for (int i = 0; i < 8; i++)
        if (!std::isfinite(p->scw[i])) { orbx_set_error("%s: scw is not finite", who); return ORBX_ERR_ARG; }
    if (!(p->scw[7] > 0.0)) { orbx_set_error("%s: the scale of scw is %g, it must be positive", who, p->scw[7]); return ORBX_ERR_ARG; }
    if (!lc_all_finite(p->tcw, (size_t)NK * 12) || !lc_all_finite(p->ow, (size_t)NK * 3)) { orbx_set_error("%s: a keyframe pose or centre is not finite", who); return ORBX_ERR_ARG; }
    if (M > 0 && !lc_all_finite(p->pos, (size_t)M * 3)) { orbx_set_error("%s: a point position is not finite", who); return ORBX_ERR_ARG; }
    return ORBX_OK;
}

// the walk of :930-960 without its arithmetic: reached, and the non-optimised reached keyframes sorted by their depth below an optimised ancestor
// (or an origin).  A keyframe that is its own ancestor is an error; one whose chain ends at a -2 is merely never reached.
int lc_validate_gba(const orbx_loop_gba_problem *p, std::vector<uint8_t> &reached, std::vector<int32_t> &level, std::vector<int32_t> &order, std::vector<int32_t> &levelOff)
{
    const char *who = "orbx_loop_propagate_gba";
    if (!p) { orbx_set_error("%s: NULL problem", who); return ORBX_ERR_ARG; }
    const int n = p->num_keyframes, M = p->num_points;
    if (n < 1 || M < 0) { orbx_set_error("%s: num_keyframes < 1 or a negative size", who); return ORBX_ERR_ARG; }
    if (!p->parent || !p->tcw || !p->tcw_gba || !p->in_gba || (M > 0 && (!p->pos || !p->pos_gba || !p->point_in_gba || !p->point_bad || !p->point_ref))) {
        orbx_set_error("%s: NULL problem array", who);
        return ORBX_ERR_ARG;
    }
    int origins = 0;
    for (int i = 0; i < n; i++) {
        if (p->parent[i] < -2 || p->parent[i] >= n) { orbx_set_error("%s: parent[%d] = %d is no keyframe slot (-2..%d)", who, i, p->parent[i], n - 1); return ORBX_ERR_ARG; }
        origins += p->parent[i] == -1 ? 1 : 0;
    }
    if (!origins) { orbx_set_error("%s: no origin (no keyframe with parent -1)", who); return ORBX_ERR_ARG; }
    // state: 0 unknown, 1 on the path being walked, 2 reached, 3 not reached; level: depth in a chain of non-optimised keyframes
    reached.assign((size_t)n, 0);
    level.assign((size_t)n, 0);
    order.clear();      // (used as the path stack first)
    int L = 0;
    for (int i = 0; i < n; i++) {
        if (reached[(size_t)i]) continue;
        int k = i;
        while (k >= 0 && reached[(size_t)k] == 0) { reached[(size_t)k] = 1; order.push_back(k); k = p->parent[k]; }
        if (k >= 0 && reached[(size_t)k] == 1) { orbx_set_error("%s: keyframe slot %d is its own ancestor (a cycle in parent)", who, k); return ORBX_ERR_ARG; }
        uint8_t st = k == -1 ? 2 : k == -2 ? 3 : reached[(size_t)k];
        int lv = k >= 0 ? level[(size_t)k] : 0;
        while (!order.empty()) {      // top down
            const int c = order.back();
            order.pop_back();
            const bool given = p->parent[c] < 0 || p->in_gba[c];
            lv = given ? 0 : lv + 1;
            level[(size_t)c] = lv; reached[(size_t)c] = st;
            if (st == 2 && lv > L) L = lv;
        }
    }
    for (int i = 0; i < n; i++) reached[(size_t)i] = reached[(size_t)i] == 2 ? 1 : 0;
    for (int i = 0; i < M; i++)
        if (p->point_ref[i] < -1 || p->point_ref[i] >= n) { orbx_set_error("%s: point_ref[%d] = %d is no keyframe slot (-1..%d)", who, i, p->point_ref[i], n - 1); return ORBX_ERR_ARG; }
    if (!lc_all_finite(p->tcw, (size_t)n * 12) || !lc_all_finite(p->tcw_gba, (size_t)n * 12)) { orbx_set_error("%s: a keyframe pose is not finite", who); return ORBX_ERR_ARG; }
    if (M > 0 && (!lc_all_finite(p->pos, (size_t)M * 3) || !lc_all_finite(p->pos_gba, (size_t)M * 3))) { orbx_set_error("%s: a point position is not finite", who); return ORBX_ERR_ARG; }
    levelOff.assign((size_t)L + 1, 0);
    for (int i = 0; i < n; i++)
        if (reached[(size_t)i] && level[(size_t)i] > 0) levelOff[(size_t)level[(size_t)i]]++;      // count of level l at [l], shifted below
    int32_t run = 0;
    for (int l = 1; l <= L; l++) { const int32_t c = levelOff[(size_t)l]; levelOff[(size_t)l - 1] = run; run += c; }
    levelOff[(size_t)L] = run;
    order.assign((size_t)run, 0);
    std::vector<int32_t> at(levelOff.begin(), levelOff.end());
    for (int i = 0; i < n; i++)
        if (reached[(size_t)i] && level[(size_t)i] > 0) order[(size_t)at[(size_t)level[(size_t)i] - 1]++] = i;
    return ORBX_OK;
}

}  // namespace

extern "C" int orbx_loop_correct_sim3(orbx_loop *h, const orbx_loop_sim3_problem *p, const orbx_loop_sim3_result *r)
{
    int rc;
    std::vector<int32_t> ownPos;
    std::vector<int32_t> &groupPos = h ? h->groupPos : ownPos;
    if ((rc = lc_validate_sim3(p, groupPos)) != ORBX_OK) return rc;
    if (!h) { orbx_set_error("orbx_loop_correct_sim3: NULL handle"); return ORBX_ERR_ARG; }
    const size_t NK = (size_t)p->num_keyframes, G = (size_t)p->num_group, M = (size_t)p->num_points, S = (size_t)p->num_entries, T = (size_t)p->num_obs;
    h->timer.timed = false;
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    OrbxCallBox &bx = h->box;
    auto [pin, pout] = bx.plan();
    const auto sTcw = pin.add(p->tcw, 12 * NK), sOw = pin.add(p->ow, 3 * NK);
    const auto sGroupKf = pin.add(p->group_kf, G), sGroupPos = pin.add((const int32_t *)groupPos.data(), NK);
    const auto sScw = pin.add(p->scw, (size_t)8);
    const auto sListOff = pin.add(p->list_offset, G + 1), sListPt = pin.add(p->list_point, S);
    const auto sPos = pin.add(p->pos, 3 * M);
    const auto sBad = pin.add(p->point_bad, M), sDone = pin.add(p->point_done, M);
    const auto sRef = pin.add(p->point_ref, M);
    const auto sRsc = pin.add(p->ref_scale, M), sTsc = pin.add(p->top_scale, M);
    const auto sObsOff = pin.add(p->obs_offset, M + 1), sObsKf = pin.add(p->obs_kf, T);
    // the results: built in device memory (h->results) in this layout, then copied to the box in one pass
    const auto rNonc = pout.hole<double>(8 * G), rCorr = pout.hole<double>(8 * G);
    const auto rTiw = pout.hole<float>(12 * G), rOw = pout.hole<float>(3 * G), rScw = pout.hole<float>(12 * G), rPos = pout.hole<float>(3 * M);
    const auto rBy = pout.hole<int32_t>(M);
    const auto rNor = pout.hole<float>(3 * M), rMax = pout.hole<float>(M), rMin = pout.hole<float>(M);
    const auto rUpd = pout.hole<uint8_t>(M);
    const size_t outBytes = pout.total();
    OrbxWorkPlan &work = h->workPlan;
    work.reset();
    const auto wClaim = work.hole<int32_t>(M);
    const auto wNonc = work.hole<double>(8 * G), wSwi = work.hole<double>(8 * G);
    const auto wOw = work.hole<float>(3 * G), wUnit = work.hole<float>(3 * T);
    const OrbxStaged sg = bx.begin(h->stream, &rc);
    if (rc != ORBX_OK) return rc;
    if ((rc = h->work.ensure(work.total() ? work.total() : 256)) != ORBX_OK) return rc;
    if ((rc = h->results.ensure(outBytes)) != ORBX_OK) return rc;
    if ((rc = h->timer.begin(h->stream)) != ORBX_OK) return rc;
    uint8_t *A;
    if ((rc = orbx_stage_to_arena(bx, h->arena, h->stream, 256, &A)) != ORBX_OK) return rc;
    ORBX_LAUNCH_COUNT(h->timer);
    LcDev D = {};
    D.NK = (int)NK; D.G = (int)G; D.M = (int)M; D.cur = p->current;
    D.tcw = sTcw.in(A); D.ow = sOw.in(A); D.groupKf = sGroupKf.in(A); D.groupPos = sGroupPos.in(A); D.scw = sScw.in(A);
    D.listOff = sListOff.in(A); D.listPt = sListPt.in(A);
    D.pos = sPos.in(A); D.bad = sBad.in(A); D.done = sDone.in(A); D.ref = sRef.in(A); D.rsc = sRsc.in(A); D.tsc = sTsc.in(A);
    D.obsOff = sObsOff.in(A); D.obsKf = sObsKf.in(A);
    void *W = h->work.p;
    D.claim = wClaim.in(W); D.wNonc = wNonc.in(W); D.wSwi = wSwi.in(W); D.wOwNew = wOw.in(W); D.unit = wUnit.in(W);
    void *O = h->results.p;
    D.oNonc = rNonc.in(O); D.oCorr = rCorr.in(O); D.oTiw = rTiw.in(O); D.oOwNew = rOw.in(O); D.oScwMat = rScw.in(O);
    D.oPos = rPos.in(O); D.oBy = rBy.in(O); D.oNormal = rNor.in(O); D.oMax = rMax.in(O); D.oMin = rMin.in(O);
    D.oUpd = rUpd.in(O);
    hipLaunchKernelGGL(k_lc_sim3, dim3((unsigned)((std::max(G, M) + LC_THREADS - 1) / LC_THREADS)), dim3(LC_THREADS), 0, h->stream, D);
    ORBX_LAUNCH_COUNT(h->timer);
    if (S > 0 && M > 0) {
        hipLaunchKernelGGL(k_lc_claim, dim3((unsigned)std::min<size_t>(G, LC_CLAIM_BLOCKS)), dim3(LC_THREADS), 0, h->stream, D);
        ORBX_LAUNCH_COUNT(h->timer);
    }
    if (M > 0) {
        hipLaunchKernelGGL(k_lc_move, dim3((unsigned)std::min<size_t>(M, (size_t)1 << 20)), dim3(LC_POINT_THREADS), 0, h->stream, D);
        ORBX_LAUNCH_COUNT(h->timer);
    }
    const unsigned long long seq = bx.arm();
    const size_t o16 = outBytes / 16;
    hipLaunchKernelGGL(k_lc_results, dim3((unsigned)std::min<size_t>(256, (o16 + LC_THREADS - 1) / LC_THREADS)), dim3(LC_THREADS), 0, h->stream, (const uint4 *)h->results.p,
                       (uint4 *)sg.dev(rNonc), o16, bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_COUNT(h->timer);
    if ((rc = h->timer.end(h->stream)) != ORBX_OK) return rc;
    if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;
    if (r) {
        if (r->noncorrected) memcpy(r->noncorrected, sg.host(rNonc), 64 * G);
        if (r->corrected) memcpy(r->corrected, sg.host(rCorr), 64 * G);
        if (r->tiw) memcpy(r->tiw, sg.host(rTiw), 48 * G);
        if (r->ow_new) memcpy(r->ow_new, sg.host(rOw), 12 * G);
        if (r->scw_mat) memcpy(r->scw_mat, sg.host(rScw), 48 * G);
        if (M) {
            if (r->pos) memcpy(r->pos, sg.host(rPos), 12 * M);
            if (r->corrected_by) memcpy(r->corrected_by, sg.host(rBy), 4 * M);
            if (r->normal) memcpy(r->normal, sg.host(rNor), 12 * M);
            if (r->max_dist) memcpy(r->max_dist, sg.host(rMax), 4 * M);
            if (r->min_dist) memcpy(r->min_dist, sg.host(rMin), 4 * M);
            if (r->updated) memcpy(r->updated, sg.host(rUpd), M);
        }
    }
    return ORBX_OK;
}

extern "C" int orbx_loop_propagate_gba(orbx_loop *h, const orbx_loop_gba_problem *p, const orbx_loop_gba_result *r)
{
    int rc;
    std::vector<uint8_t> ownReached;
    std::vector<int32_t> ownLevel, ownOrder, ownOff;
    std::vector<uint8_t> &reached = h ? h->reached : ownReached;
    std::vector<int32_t> &level = h ? h->level : ownLevel, &order = h ? h->order : ownOrder, &levelOff = h ? h->levelOff : ownOff;
    if ((rc = lc_validate_gba(p, reached, level, order, levelOff)) != ORBX_OK) return rc;
    if (!h) { orbx_set_error("orbx_loop_propagate_gba: NULL handle"); return ORBX_ERR_ARG; }
    const size_t n = (size_t)p->num_keyframes, M = (size_t)p->num_points, L = levelOff.size() - 1, C = order.size();
    h->timer.timed = false;
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    OrbxCallBox &bx = h->box;
    auto [pin, pout] = bx.plan();
    // the keyframe arrays: staged to the arena; the point arrays behind them are read in place
    const auto sTcw = pin.add(p->tcw, 12 * n), sGba = pin.add(p->tcw_gba, 12 * n);
    const auto sParent = pin.add(p->parent, n);
    const auto sReached = pin.add((const uint8_t *)reached.data(), n);
    const auto sOrder = pin.add((const int32_t *)order.data(), C), sLevelOff = pin.add((const int32_t *)levelOff.data(), L + 1);
    const size_t kfBytes = pin.total();
    const auto sPos = pin.add(p->pos, 3 * M), sPosGba = pin.add(p->pos_gba, 3 * M);
    const auto sPtIn = pin.add(p->point_in_gba, M), sPtBad = pin.add(p->point_bad, M);
    const auto sRef = pin.add(p->point_ref, M);
    const auto rGba = pout.hole<float>(12 * n), rPos = pout.hole<float>(3 * M);
    const auto rMoved = pout.hole<uint8_t>(M);
    const OrbxStaged sg = bx.begin(h->stream, &rc);
    if (rc != ORBX_OK) return rc;
    OrbxWorkPlan &work = h->workPlan;
    work.reset();
    const auto wGba = work.hole<float>(12 * n);
    if ((rc = h->work.ensure(work.total())) != ORBX_OK) return rc;
    if ((rc = h->timer.begin(h->stream)) != ORBX_OK) return rc;
    uint8_t *A;
    if ((rc = orbx_stage_to_arena(bx, h->arena, h->stream, 256, &A, 0, kfBytes)) != ORBX_OK) return rc;
    ORBX_LAUNCH_COUNT(h->timer);
    LgDev D = {};
    D.n = (int)n; D.M = (int)M; D.L = (int)L;
    D.tcw = sTcw.in(A); D.gbaIn = sGba.in(A); D.parent = sParent.in(A); D.reached = sReached.in(A); D.order = sOrder.in(A); D.levelOff = sLevelOff.in(A);
    D.pos = sg.dev(sPos); D.posGba = sg.dev(sPosGba); D.ptIn = sg.dev(sPtIn); D.ptBad = sg.dev(sPtBad); D.ref = sg.dev(sRef);
    D.gba = wGba.in((void *)h->work.p);
    D.oGba = sg.dev(rGba); D.oPos = sg.dev(rPos); D.oMoved = sg.dev(rMoved);
    hipLaunchKernelGGL(k_lg_chain, dim3(1), dim3(LC_THREADS), 0, h->stream, D);
    ORBX_LAUNCH_COUNT(h->timer);
    const unsigned long long seq = bx.arm();
    hipLaunchKernelGGL(k_lg_points, dim3((unsigned)std::max<size_t>(1, (M + LC_THREADS - 1) / LC_THREADS)), dim3(LC_THREADS), 0, h->stream, D, bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_COUNT(h->timer);
    if ((rc = h->timer.end(h->stream)) != ORBX_OK) return rc;
    if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;
    if (r) {
        if (r->tcw_gba) memcpy(r->tcw_gba, sg.host(rGba), 48 * n);
        if (r->reached) memcpy(r->reached, reached.data(), n);
        if (M) {
            if (r->pos) memcpy(r->pos, sg.host(rPos), 12 * M);
            if (r->moved) memcpy(r->moved, sg.host(rMoved), M);
        }
    }
    return ORBX_OK;
}

extern "C" int orbx_loop_last_timing(orbx_loop *h, float *device_ms, int *launches)
{
    if (!h) { orbx_set_error("NULL loop correction handle"); return ORBX_ERR_ARG; }
    return h->timer.read(h->device, device_ms, launches, nullptr);
}
