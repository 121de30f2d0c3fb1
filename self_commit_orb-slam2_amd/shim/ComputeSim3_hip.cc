// shim/ComputeSim3_hip.cc -- see shim/ComputeSim3_hip.h.
#include "ComputeSim3_hip.h"

#include <map>
#include <stdint.h>
#include <string.h>

#include "Frame.h"
#include "KeyFrameArrays.h"
#include "MapPointAccess.h"
#include "orbx.h"
#include "shim_error.h"

namespace ORB_SLAM2
{
static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint must be the 28-byte layout of orbx_keypoint");

namespace
{
// one matcher handle per calling thread (a handle is not re-entrant); ComputeSim3 runs on the loop closing thread
struct LoopMatcher {
    orbx_matcher *h;
    int cap, pairs;
    LoopMatcher() : h(0), cap(0), pairs(0) {}
    ~LoopMatcher() { if (h) orbx_matcher_destroy(h); }
};
thread_local LoopMatcher tLoop;

orbx_matcher *Matcher(int need, int needPairs)
{
    if (tLoop.h && need <= tLoop.cap && needPairs <= tLoop.pairs) return tLoop.h;
    if (tLoop.h) { orbx_matcher_destroy(tLoop.h); tLoop.h = 0; }
    int cap = 4096, pairs = 8;
    while (cap < need) cap *= 2;
    while (pairs < needPairs) pairs *= 2;
    tLoop.pairs = pairs;
    if (orbx_matcher_create(orbx_shim::Device(), cap, pairs, &tLoop.h) != ORBX_OK) { tLoop.h = 0; tLoop.cap = 0; orbx_shim::Fail("LoopClosing::ComputeSim3"); return 0; }
    tLoop.cap = cap;
    return tLoop.h;
}

// a keyframe as the arrays of orbx_loop_sim3_keyframe: the gather of KeyFrameArrays.h (slots, valid, position, and from the same visit of each point its
// distance range and descriptor), the slot of every point, and the keyframe's own tables
struct LoopKeyFrame {
    KeyFrameArrays A;
    std::vector<int32_t> bow;
    std::map<MapPoint *, int> slotOf;      // a point's identity on the device is its (first) slot
    float ratioTh[64];
    orbx_loop_sim3_keyframe k;
    bool Gather(KeyFrame *pKF)
    {
        A.Gather(pKF, true);
        const int n = A.n;
        for (int i = 0; i < n; i++)
            if (A.vpMPs[(size_t)i]) slotOf.insert(std::make_pair(A.vpMPs[(size_t)i], i));
        if (orbx_predict_scale_thresholds(pKF->mfLogScaleFactor, pKF->mnScaleLevels, ratioTh) != ORBX_OK) return false;
        memset(&k, 0, sizeof k);
        const orbx_projection_frame pf = {A.set.keypoints, A.set.descriptors, NULL, NULL, &A.n, A.set.capacity, 1,
                                          Frame::mnMinX, Frame::mnMinY, pKF->mfGridElementWidthInv, pKF->mfGridElementHeightInv};      // what filed mGrid
        k.frame = pf;
        const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation();
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) k.rcw[3 * r + c] = R.at<float>(r, c);
            k.tcw[r] = t.at<float>(r);
        }
        k.fx = pKF->fx; k.fy = pKF->fy; k.cx = pKF->cx; k.cy = pKF->cy;
        k.min_x = (float)pKF->mnMinX; k.max_x = (float)pKF->mnMaxX; k.min_y = (float)pKF->mnMinY; k.max_y = (float)pKF->mnMaxY;      // KeyFrame::IsInImage
        k.scale_factors = &pKF->mvScaleFactors[0]; k.ratio_thresholds = ratioTh; k.inv_level_sigma2 = &pKF->mvInvLevelSigma2[0]; k.nlevels = pKF->mnScaleLevels;
        k.valid = &A.valid[0]; k.world_pos = &A.pos[0]; k.max_distance = &A.maxD[0]; k.min_distance = &A.minD[0]; k.descriptors = &A.desc[0];
        return true;
    }
};
}  // namespace

bool ComputeSim3Device(KeyFrame *pCurrentKF, const std::vector<KeyFrame *> &vpCandidates, const std::vector<std::vector<MapPoint *> > &vvpMapPointMatches,
                       const std::vector<LoopSim3Event> &events, bool bFixScale, int &matchedCandidate, g2o::Sim3 &g2oScw, cv::Mat &Scw,
                       std::vector<MapPoint *> &vpCurrentMatchedPoints)
{
    orbx_shim::Mark("ComputeSim3Device enters");
    matchedCandidate = -1;
    const int K = (int)vpCandidates.size(), H = (int)events.size();
    if (!pCurrentKF || K == 0 || H == 0) return false;
    // the gather: the current keyframe and the candidates an event names (the others keep one empty slot: nothing reads them)
    LoopKeyFrame A1;
    if (!A1.Gather(pCurrentKF)) { orbx_shim::Fail("LoopClosing::ComputeSim3"); return false; }
    const int N1 = A1.A.n;
    if (N1 == 0) return false;
    std::vector<LoopKeyFrame> A((size_t)K);
    std::vector<orbx_loop_sim3_keyframe> cands((size_t)K);
    std::vector<int32_t> remap((size_t)K, -1), hCand((size_t)H);
    int nUsed = 0, maxN = N1;
    for (int h = 0; h < H; h++) {
        const int c = events[(size_t)h].candidate;
        if (c < 0 || c >= K || !vpCandidates[(size_t)c]) { orbx_shim::Fail("LoopClosing::ComputeSim3"); return false; }
        if (remap[(size_t)c] < 0) {
            LoopKeyFrame &a = A[(size_t)nUsed];
            if (!a.Gather(vpCandidates[(size_t)c]) || a.A.n == 0) { orbx_shim::Fail("LoopClosing::ComputeSim3"); return false; }
            a.bow.assign((size_t)N1, -1);
            const std::vector<MapPoint *> &m = vvpMapPointMatches[(size_t)c];
            for (int j = 0; j < N1 && j < (int)m.size(); j++) {
                if (!m[(size_t)j]) continue;
                std::map<MapPoint *, int>::const_iterator it = a.slotOf.find(m[(size_t)j]);      // pMP->GetIndexInKeyFrame(pKF2), src/ORBmatcher.cc:1353
                if (it != a.slotOf.end()) a.bow[(size_t)j] = it->second;
            }
            a.k.bow_match = &a.bow[0];
            cands[(size_t)nUsed] = a.k;
            if (a.A.n > maxN) maxN = a.A.n;
            remap[(size_t)c] = nUsed++;
        }
        hCand[(size_t)h] = remap[(size_t)c];
    }
    std::vector<float> r12((size_t)H * 9), t12((size_t)H * 3), s12((size_t)H);
    std::vector<uint8_t> mask((size_t)H * (size_t)N1, 0);
    for (int h = 0; h < H; h++) {
        const LoopSim3Event &e = events[(size_t)h];
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) r12[9 * (size_t)h + 3 * (size_t)r + (size_t)c] = e.R12.at<float>(r, c);
            t12[3 * (size_t)h + (size_t)r] = e.t12.at<float>(r);
        }
        s12[(size_t)h] = e.s12;
        for (int j = 0; j < N1 && j < (int)e.vbInliers.size(); j++) mask[(size_t)h * (size_t)N1 + (size_t)j] = e.vbInliers[(size_t)j] ? 1 : 0;      // :437-443
    }
    std::vector<int32_t> matches((size_t)N1, -1);
    std::vector<double> quat((size_t)H * 4), tt((size_t)H * 3), ss((size_t)H);
    std::vector<float> scw((size_t)H * 16);
    orbx_shim::Mark("ComputeSim3Device marshalled");
    orbx_matcher *mt = Matcher(maxN, nUsed);
    if (!mt) return false;                                                                     // (reported and counted where the creation failed)
    // ORBX_LOOP_SIM3_MAX_HYPOTHESES events per device call, in walk order, until one is accepted: what the reference's `&& !bMatch` does
    int winner = -1, winnerSlot = -1;
    for (int h0 = 0; h0 < H && winner < 0; h0 += ORBX_LOOP_SIM3_MAX_HYPOTHESES) {
        const int Hc = H - h0 < ORBX_LOOP_SIM3_MAX_HYPOTHESES ? H - h0 : ORBX_LOOP_SIM3_MAX_HYPOTHESES;
        const size_t o = (size_t)h0;
        orbx_loop_sim3_hypotheses hy;
        memset(&hy, 0, sizeof hy);
        hy.count = Hc; hy.candidate = &hCand[o]; hy.r12 = &r12[9 * o]; hy.t12 = &t12[3 * o]; hy.s12 = &s12[o]; hy.inliers = &mask[o * (size_t)N1];
        orbx_loop_refine_result res;
        memset(&res, 0, sizeof res);
        res.quat = &quat[4 * o]; res.t = &tt[3 * o]; res.s = &ss[o]; res.scw = &scw[16 * o]; res.matches12 = &matches[0];
        // (an event with more than ORBX_SIM3_OPT_MAX_PAIRS pairs ahead of any winner comes back as ORBX_ERR_CAPACITY: an error, reported and counted)
        if (orbx_loop_refine_sim3(mt, &A1.k, &cands[0], nUsed, &hy, 7.5f, 10.f, bFixScale ? 1 : 0, &res) != ORBX_OK) { orbx_shim::Fail("LoopClosing::ComputeSim3"); return false; }
        if (res.winner >= 0) { winner = h0 + res.winner; winnerSlot = res.candidate; }
    }
    orbx_shim::Mark("ComputeSim3Device device calls returned");
    if (winner < 0) return false;
    // the write-back of :465-474
    const size_t w = (size_t)winner;
    matchedCandidate = events[w].candidate;
    const LoopKeyFrame &a = A[(size_t)winnerSlot];
    // gScm as the device left it, then mg2oScw = gScm * gSmw with the reference's own operator (the device's scw is the same product, narrowed)
    const g2o::Sim3 gScm(Eigen::Quaterniond(quat[4 * w + 3], quat[4 * w], quat[4 * w + 1], quat[4 * w + 2]), Eigen::Vector3d(tt[3 * w], tt[3 * w + 1], tt[3 * w + 2]), ss[w]);
    Eigen::Matrix3d R2;
    Eigen::Vector3d t2;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R2(r, c) = a.k.rcw[3 * r + c];
        t2(r) = a.k.tcw[r];
    }
    g2oScw = gScm * g2o::Sim3(R2, t2, 1.0);
    Scw = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) Scw.at<float>(r, c) = scw[16 * w + 4 * (size_t)r + (size_t)c];
    vpCurrentMatchedPoints.assign((size_t)N1, static_cast<MapPoint *>(NULL));
    for (int j = 0; j < N1; j++)
        if (matches[(size_t)j] >= 0) vpCurrentMatchedPoints[(size_t)j] = a.A.vpMPs[(size_t)matches[(size_t)j]];
    orbx_shim::Mark("ComputeSim3Device returns");
    return true;
}

}  // namespace ORB_SLAM2
