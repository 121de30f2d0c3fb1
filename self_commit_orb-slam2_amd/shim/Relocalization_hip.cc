// shim/Relocalization_hip.cc -- see shim/Relocalization_hip.h.
#include "Relocalization_hip.h"

#include <map>
#include <stdint.h>
#include <string.h>

#include "KeyFrameArrays.h"
#include "MapPointAccess.h"
#include "orbx.h"
#include "shim_error.h"

namespace ORB_SLAM2
{
static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint must be the 28-byte layout of orbx_keypoint");

namespace
{
// one matcher handle per calling thread (a handle is not re-entrant); relocalisation runs on the tracking thread
struct RelocMatcher {
    orbx_matcher *h;
    int cap, pairs;
    RelocMatcher() : h(0), cap(0), pairs(0) {}
    ~RelocMatcher() { if (h) orbx_matcher_destroy(h); }
};
thread_local RelocMatcher tReloc;

orbx_matcher *Matcher(int need, int needPairs = 1)
{
    if (tReloc.h && need <= tReloc.cap && needPairs <= tReloc.pairs) return tReloc.h;
    if (tReloc.h) { orbx_matcher_destroy(tReloc.h); tReloc.h = 0; }
    int cap = 4096, pairs = 8;
    while (cap < need) cap *= 2;
    while (pairs < needPairs) pairs *= 2;
    tReloc.pairs = pairs;
    if (orbx_matcher_create(orbx_shim::Device(), cap, pairs, &tReloc.h) != ORBX_OK) { tReloc.h = 0; tReloc.cap = 0; orbx_shim::Fail("Tracking::Relocalization"); return 0; }   // (the caller returns on the NULL handle)
    tReloc.cap = cap;
    return tReloc.h;
}

// a candidate's GetMapPointMatches() as the arrays of orbx_reloc_candidate
struct CandidateArrays {
    std::vector<MapPoint *> vpMPs;
    std::vector<uint8_t> valid, desc;
    std::vector<float> pos, maxD, minD, angle;
    std::vector<int32_t> bow;
};
}  // namespace

int AddRelocHypothesis(std::vector<RelocHypothesis> &hyps, int candidate, const cv::Mat &Tcw, const std::vector<bool> &vbInliers)
{
    for (size_t k = 0; k < hyps.size(); k++) {
        if (hyps[k].candidate != candidate || hyps[k].vbInliers != vbInliers) continue;
        bool same = true;
        for (int r = 0; r < 3 && same; r++)
            for (int c = 0; c < 4; c++) same = same && hyps[k].Tcw.at<float>(r, c) == Tcw.at<float>(r, c);
        if (same) return (int)k;
    }
    RelocHypothesis h;
    h.candidate = candidate; h.Tcw = Tcw.clone(); h.vbInliers = vbInliers;
    hyps.push_back(h);
    return (int)hyps.size() - 1;
}

int RelocalizationMatchHIP(Frame &F, const std::vector<KeyFrame *> &vpCandidateKFs, std::vector<std::vector<MapPoint *> > &vvpMapPointMatches, std::vector<bool> &vbDiscarded,
                           std::vector<RelocPnPProblem> &problems, float nnratio, bool checkOrientation)
{
    orbx_shim::Mark("RelocalizationMatch enters");
    const int N = F.N, nKFs = (int)vpCandidateKFs.size();
    vvpMapPointMatches.resize((size_t)nKFs);
    vbDiscarded.assign((size_t)nKFs, true);
    problems.assign((size_t)nKFs, RelocPnPProblem());
    if (N == 0 || nKFs == 0) return 0;
    // the gather: every candidate that is not bad, one visit per point (the arrays point into A: sized once, never copied)
    std::vector<KeyFrameArrays> A((size_t)nKFs);
    std::vector<orbx_reloc_match_keyframe> kfs((size_t)nKFs);
    int maxN = N;
    for (int c = 0; c < nKFs; c++) {
        KeyFrame *pKF = vpCandidateKFs[(size_t)c];
        const orbx_reloc_match_keyframe bad = {0, 0, 1};
        kfs[(size_t)c] = bad;
        if (pKF->isBad()) continue;                                                        // :2066
        A[(size_t)c].Gather(pKF);
        const orbx_reloc_match_keyframe k = {&A[(size_t)c].set, &A[(size_t)c].pos[0], 0};
        kfs[(size_t)c] = k;
        vvpMapPointMatches[(size_t)c] = std::vector<MapPoint *>((size_t)N, static_cast<MapPoint *>(NULL));      // src/ORBmatcher.cc:236
        if (A[(size_t)c].n > maxN) maxN = A[(size_t)c].n;
    }
    std::vector<int32_t> gF;
    FlatFeatureVector(F.mFeatVec, N, gF);
    const orbx_feature_set fs = {(const orbx_keypoint *)&F.mvKeys[0], F.mDescriptors.data, &N, &gF[0], NULL, N, 1};      // kp angle: src/ORBmatcher.cc:320
    const orbx_reloc_match_frame fr = {&fs, (const orbx_keypoint *)&F.mvKeysUn[0], &F.mvLevelSigma2[0], (int)F.mvLevelSigma2.size()};
    const size_t KN = (size_t)nKFs * (size_t)N;
    std::vector<int32_t> matches(KN, -1), keyIndex(KN), n((size_t)nKFs, 0), nm((size_t)nKFs, 0);
    std::vector<float> p2d(KN * 2), sigma2(KN), p3dw(KN * 3);
    std::vector<uint8_t> disc((size_t)nKFs, 1);
    const orbx_reloc_match_result res = {&matches[0], &keyIndex[0], &p2d[0], &sigma2[0], &p3dw[0], &n[0], &nm[0], &disc[0]};
    orbx_shim::Mark("RelocalizationMatch marshalled");
    orbx_matcher *m = Matcher(maxN, nKFs);
    if (!m) return 0;
    if (orbx_reloc_match_candidates(m, &fr, &kfs[0], nKFs, nnratio, checkOrientation ? 1 : 0, &res) != ORBX_OK) { orbx_shim::Fail("Tracking::Relocalization"); return 0; }
    orbx_shim::Mark("RelocalizationMatch device call returned");
    int nCandidates = 0;
    for (int c = 0; c < nKFs; c++) {
        const size_t row = (size_t)c * (size_t)N;
        if (!kfs[(size_t)c].is_bad)
            for (int j = 0; j < N; j++)
                if (matches[row + (size_t)j] >= 0) vvpMapPointMatches[(size_t)c][(size_t)j] = A[(size_t)c].vpMPs[(size_t)matches[row + (size_t)j]];      // :314
        vbDiscarded[(size_t)c] = disc[(size_t)c] != 0;                                     // :2069, :2077
        if (disc[(size_t)c]) continue;
        const size_t k = (size_t)n[(size_t)c];
        RelocPnPProblem &P = problems[(size_t)c];
        P.keyIndex.assign(keyIndex.begin() + (long)row, keyIndex.begin() + (long)(row + k));
        P.p2d.assign(p2d.begin() + (long)(2 * row), p2d.begin() + (long)(2 * (row + k)));
        P.sigma2.assign(sigma2.begin() + (long)row, sigma2.begin() + (long)(row + k));
        P.p3dw.assign(p3dw.begin() + (long)(3 * row), p3dw.begin() + (long)(3 * (row + k)));
        nCandidates++;                                                                     // :2092
    }
    orbx_shim::Mark("RelocalizationMatch returns");
    return nCandidates;
}

bool RelocalizationRefineHIP(Frame &CurrentFrame, const std::vector<KeyFrame *> &vpCandidateKFs, const std::vector<std::vector<MapPoint *> > &vvpMapPointMatches,
                             const std::vector<RelocHypothesis> &hyps, const std::vector<int> &sequence, int &winnerCandidate, bool checkOrientation)
{
    orbx_shim::Mark("RelocalizationRefine enters");
    winnerCandidate = -1;
    const int N = CurrentFrame.N, nKFs = (int)vpCandidateKFs.size(), H = (int)hyps.size();
    if (N == 0 || nKFs == 0 || H == 0 || sequence.empty()) return false;
    // the gather: only the candidates a hypothesis names are visited; the others stay empty (npoints 0)
    std::vector<char> named((size_t)nKFs, 0);
    for (int h = 0; h < H; h++)
        if (hyps[(size_t)h].candidate >= 0 && hyps[(size_t)h].candidate < nKFs) named[(size_t)hyps[(size_t)h].candidate] = 1;
    std::vector<CandidateArrays> A((size_t)nKFs);
    std::vector<orbx_reloc_candidate> cands((size_t)nKFs);
    int maxPoints = 0;
    for (int c = 0; c < nKFs; c++) {
        CandidateArrays &a = A[(size_t)c];
        a.bow.assign((size_t)N, -1);
        KeyFrame *pKF = vpCandidateKFs[(size_t)c];
        if (named[(size_t)c] && pKF) {
            a.vpMPs = pKF->GetMapPointMatches();                                           // src/ORBmatcher.cc:1745
            const size_t P = a.vpMPs.size();
            a.valid.assign(P + 1, 0); a.desc.assign(P * 32 + 32, 0); a.pos.assign(P * 3 + 3, 0.f); a.maxD.assign(P + 1, 0.f); a.minD.assign(P + 1, 0.f); a.angle.assign(P + 1, 0.f);
            std::map<MapPoint *, int> slotOf;                                              // a point's identity on the device is its (first) slot
            for (size_t i = 0; i < P; i++) {
                a.angle[i] = pKF->mvKeysUn[i].angle;                                       // :1826
                MapPoint *pMP = a.vpMPs[i];
                if (!pMP) continue;
                slotOf.insert(std::make_pair(pMP, (int)i));
                float nrm[3];
                uint8_t hasObs;
                if (MapPointAccess::Snapshot(pMP, &a.pos[3 * i], nrm, a.maxD[i], a.minD[i], hasObs, &a.desc[32 * i])) a.valid[i] = 1;      // pMP && !pMP->isBad(), :1752-1754
                else MapPointAccess::WorldPos(pMP, &a.pos[3 * i]);                         // (a bad seed is still an edge of PoseOptimization: position without the isBad gate)
            }
            const std::vector<MapPoint *> &m = vvpMapPointMatches[(size_t)c];
            for (int j = 0; j < N && j < (int)m.size(); j++) {
                if (!m[(size_t)j]) continue;
                std::map<MapPoint *, int>::const_iterator it = slotOf.find(m[(size_t)j]);
                if (it != slotOf.end()) a.bow[(size_t)j] = it->second;
            }
            if ((int)P > maxPoints) maxPoints = (int)P;
        }
        const bool any = !a.vpMPs.empty();
        orbx_reloc_candidate rc = {(int)a.vpMPs.size(), any ? &a.valid[0] : 0, any ? &a.pos[0] : 0, any ? &a.maxD[0] : 0, any ? &a.minD[0] : 0, any ? &a.desc[0] : 0,
                                   any ? &a.angle[0] : 0, &a.bow[0]};
        cands[(size_t)c] = rc;
    }
    std::vector<int32_t> hCand((size_t)H), seq(sequence.begin(), sequence.end());
    std::vector<float> hTcw((size_t)H * 12);
    std::vector<uint8_t> hMask((size_t)H * (size_t)N, 0);
    for (int h = 0; h < H; h++) {
        const RelocHypothesis &hy = hyps[(size_t)h];
        hCand[(size_t)h] = hy.candidate;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) hTcw[12 * (size_t)h + 4 * (size_t)r + (size_t)c] = hy.Tcw.at<float>(r, c);      // Tcw.copyTo(mCurrentFrame.mTcw), :2137
        for (int j = 0; j < N && j < (int)hy.vbInliers.size(); j++) hMask[(size_t)h * (size_t)N + (size_t)j] = hy.vbInliers[(size_t)j] ? 1 : 0;
    }
    float ratioTh[64];
    if (orbx_predict_scale_thresholds(CurrentFrame.mfLogScaleFactor, CurrentFrame.mnScaleLevels, ratioTh) != ORBX_OK) { orbx_shim::Fail("Tracking::Relocalization"); return false; }
    orbx_reloc_frame fr;
    memset(&fr, 0, sizeof fr);
    const orbx_projection_frame pf = {(const orbx_keypoint *)&CurrentFrame.mvKeysUn[0], CurrentFrame.mDescriptors.data, &CurrentFrame.mvuRight[0], NULL, &N, N, 1,
                                      Frame::mnMinX, Frame::mnMinY, Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv};
    fr.frame = pf;
    fr.fx = Frame::fx; fr.fy = Frame::fy; fr.cx = Frame::cx; fr.cy = Frame::cy; fr.mbf = CurrentFrame.mbf; fr.max_x = Frame::mnMaxX; fr.max_y = Frame::mnMaxY;
    fr.scale_factors = &CurrentFrame.mvScaleFactors[0]; fr.ratio_thresholds = ratioTh; fr.inv_level_sigma2 = &CurrentFrame.mvInvLevelSigma2[0];
    fr.nlevels = CurrentFrame.mnScaleLevels; fr.check_orientation = checkOrientation ? 1 : 0;
    const orbx_reloc_hypotheses hy = {H, &hCand[0], &hTcw[0], &hMask[0], &seq[0], (int)seq.size(), 0, 0, 0, 0};
    std::vector<int32_t> mapPoint((size_t)N, -1), success((size_t)H, 0);
    std::vector<uint8_t> outlier((size_t)N, 0);
    std::vector<float> pose((size_t)H * 16);
    orbx_reloc_result res;
    memset(&res, 0, sizeof res);
    res.success = &success[0]; res.pose = &pose[0]; res.map_point = &mapPoint[0]; res.outlier = &outlier[0];
    orbx_shim::Mark("RelocalizationRefine marshalled");
    orbx_matcher *mt = Matcher(N > maxPoints ? N : maxPoints);
    if (!mt) return false;                                                                 // (reported and counted where the creation failed)
    if (orbx_relocalize_refine(mt, &fr, &cands[0], nKFs, &hy, &res) != ORBX_OK) { orbx_shim::Fail("Tracking::Relocalization"); return false; }
    orbx_shim::Mark("RelocalizationRefine device call returned");
    // the write-back: what the accepted pose - or the last one processed - leaves in mCurrentFrame
    const CandidateArrays &a = A[(size_t)res.candidate];
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) T.at<float>(r, c) = pose[16 * (size_t)res.hypothesis + 4 * (size_t)r + (size_t)c];
    CurrentFrame.SetPose(T);                                                               // :2137, src/Optimizer.cc:600
    for (int j = 0; j < N; j++) {
        CurrentFrame.mvpMapPoints[(size_t)j] = mapPoint[(size_t)j] >= 0 ? a.vpMPs[(size_t)mapPoint[(size_t)j]] : static_cast<MapPoint *>(NULL);
        CurrentFrame.mvbOutlier[(size_t)j] = outlier[(size_t)j] != 0;
    }
    orbx_shim::Mark("RelocalizationRefine returns");
    if (res.winner < 0) return false;
    winnerCandidate = res.candidate;
    return true;
}

}  // namespace ORB_SLAM2
