// shim/Tracking_hip.cc -- see shim/Tracking_hip.h.
#include "Tracking_hip.h"

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
// one matcher handle per calling thread (a handle is not re-entrant); the functions run on the tracking thread
struct TrackMatcher {
    orbx_matcher *h;
    int cap;
    TrackMatcher() : h(0), cap(0) {}
    ~TrackMatcher() { if (h) orbx_matcher_destroy(h); }
};
thread_local TrackMatcher tTrack;

orbx_matcher *Matcher(int need)
{
    if (tTrack.h && need <= tTrack.cap) return tTrack.h;
    if (tTrack.h) { orbx_matcher_destroy(tTrack.h); tTrack.h = 0; }
    int cap = 4096;
    while (cap < need) cap *= 2;
    if (orbx_matcher_create(orbx_shim::Device(), cap, 1, &tTrack.h) != ORBX_OK) { tTrack.h = 0; tTrack.cap = 0; orbx_shim::Fail("Tracking"); return 0; }   // (the call that follows fails on the NULL handle)
    tTrack.cap = cap;
    return tTrack.h;
}

void PoseOf(const cv::Mat &T, float out[16])
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) out[4 * r + c] = T.at<float>(r, c);
}

void SetPoseFrom(Frame &F, const float p[16])
{
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) T.at<float>(r, c) = p[4 * r + c];
    F.SetPose(T);                                                                  // src/Optimizer.cc:600
}
}  // namespace

bool TrackWithMotionModelHIP(Frame &CurrentFrame, const Frame &LastFrame, int th, bool bMono, int &nmatches, int &nmatchesMap, bool checkOrientation)
{
    orbx_shim::Mark("TrackWithMotionModel enters");
    nmatches = 0; nmatchesMap = 0;
    std::fill(CurrentFrame.mvpMapPoints.begin(), CurrentFrame.mvpMapPoints.end(), static_cast<MapPoint *>(NULL));      // :1370
    const int N = CurrentFrame.N, NL = LastFrame.N;
    if (N == 0 || NL == 0) return false;
    // the gather: what SearchByProjection(CurrentFrame, LastFrame, ..) and PoseOptimization read of the last frame's points, one visit each
    std::vector<uint8_t> valid((size_t)NL, 0), hasObs((size_t)NL, 0), lastDesc((size_t)NL * 32, 0);
    std::vector<float> pos((size_t)NL * 3, 0.f), angle((size_t)NL);
    std::vector<int32_t> octave((size_t)NL);
    for (int i = 0; i < NL; i++) {
        octave[(size_t)i] = LastFrame.mvKeys[(size_t)i].octave;                            // src/ORBmatcher.cc:1628
        angle[(size_t)i] = LastFrame.mvKeysUn[(size_t)i].angle;                            // :1694
        MapPoint *pMP = LastFrame.mvpMapPoints[(size_t)i];
        if (!pMP || LastFrame.mvbOutlier[(size_t)i]) continue;                             // :1604-1608
        float nrm[3], mx, mn;
        if (!MapPointAccess::Snapshot(pMP, &pos[3 * (size_t)i], nrm, mx, mn, hasObs[(size_t)i], &lastDesc[32 * (size_t)i])) {
            // (a bad point is still projected by the reference, which never asks: position and descriptor without the isBad gate)
            MapPointAccess::WorldPos(pMP, &pos[3 * (size_t)i]);
            const cv::Mat d = pMP->GetDescriptor();
            if (d.data) memcpy(&lastDesc[32 * (size_t)i], d.ptr<unsigned char>(), 32);
            hasObs[(size_t)i] = pMP->Observations() > 0 ? 1 : 0;
        }
        valid[(size_t)i] = 1;
    }
    float tc[16], tl[16];
    PoseOf(CurrentFrame.mTcw, tc);
    PoseOf(LastFrame.mTcw, tl);
    orbx_projection_frame fr = {(const orbx_keypoint *)&CurrentFrame.mvKeysUn[0], CurrentFrame.mDescriptors.data, &CurrentFrame.mvuRight[0], NULL, &N, N, 1,
                                Frame::mnMinX, Frame::mnMinY, Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv};      // occupied: NULL, :1370 cleared every feature
    orbx_projection_last ls = {&valid[0], &pos[0], &lastDesc[0], &hasObs[0], &octave[0], &angle[0], &NL, NL, tc, tl,
                               Frame::fx, Frame::fy, Frame::cx, Frame::cy, CurrentFrame.mbf, CurrentFrame.mb, Frame::mnMaxX, Frame::mnMaxY};
    std::vector<int32_t> matches((size_t)N, -1), searched((size_t)N, -1);      // searched: which point a discarded feature held
    std::vector<uint8_t> discarded((size_t)N, 0);
    float pose[16];
    orbx_track_motion_result res;
    memset(&res, 0, sizeof res);
    res.matches = &matches[0]; res.search_matches = &searched[0]; res.discarded = &discarded[0]; res.pose = pose;
    orbx_shim::Mark("TrackWithMotionModel marshalled");
    if (orbx_track_with_motion_model(Matcher(N > NL ? N : NL), &fr, &ls, &CurrentFrame.mvScaleFactors[0], (int)CurrentFrame.mvScaleFactors.size(),
                                     &CurrentFrame.mvInvLevelSigma2[0], (float)th, bMono ? 1 : 0, checkOrientation ? 1 : 0, &res) != ORBX_OK)
        { orbx_shim::Fail("Tracking::TrackWithMotionModel"); return false; }
    orbx_shim::Mark("TrackWithMotionModel device call returned");
    // the write-back: mvpMapPoints as :1382-1390 and :1411 leave them, the discarded points' fields (:1413-1414), mvbOutlier (PoseOptimization
    // sets it for every feature with a point, :1412 clears the discarded ones: all false behind this function), the pose
    for (int i = 0; i < N; i++) {
        if (matches[(size_t)i] >= 0) { CurrentFrame.mvpMapPoints[(size_t)i] = LastFrame.mvpMapPoints[(size_t)matches[(size_t)i]]; CurrentFrame.mvbOutlier[(size_t)i] = false; }
        else if (discarded[(size_t)i]) {
            MapPoint *pMP = LastFrame.mvpMapPoints[(size_t)searched[(size_t)i]];
            CurrentFrame.mvbOutlier[(size_t)i] = false;                                    // :1412
            pMP->mbTrackInView = false;                                                    // :1413
            pMP->mnLastFrameSeen = CurrentFrame.mnId;                                      // :1414
        }
    }
    nmatches = res.nmatches; nmatchesMap = res.nmatches_map;
    if (!res.ran_pose) return false;                                                       // :1393
    SetPoseFrom(CurrentFrame, pose);
    orbx_shim::Mark("TrackWithMotionModel returns");
    return true;
}

bool TrackReferenceKeyFrameHIP(Frame &F, KeyFrame *pKF, const cv::Mat &TcwInit, int &nmatches, int &nmatchesMap, float nnratio, bool checkOrientation)
{
    orbx_shim::Mark("TrackReferenceKeyFrame enters");
    nmatches = 0; nmatchesMap = 0;
    const int N = F.N;
    if (N == 0) return false;
    // the gather: what SearchByBoW(pKF, F) and PoseOptimization read of the keyframe's points, one visit each
    KeyFrameArrays kfa;
    kfa.Gather(pKF);
    if (kfa.n == 0) return false;
    std::vector<int32_t> gF;
    FlatFeatureVector(F.mFeatVec, N, gF);
    const orbx_feature_set fs = {(const orbx_keypoint *)&F.mvKeys[0], F.mDescriptors.data, &N, &gF[0], NULL, N, 1};      // kp angle: src/ORBmatcher.cc:320
    float tc[16], pose[16];
    PoseOf(TcwInit, tc);
    const orbx_reference_keyframe kf = {&kfa.set, &kfa.pos[0], &kfa.hasObs[0]};
    const orbx_reference_frame fr = {&fs, (const orbx_keypoint *)&F.mvKeysUn[0], &F.mvuRight[0], tc, Frame::fx, Frame::fy, Frame::cx, Frame::cy, F.mbf,
                                     &F.mvInvLevelSigma2[0], (int)F.mvInvLevelSigma2.size()};
    std::vector<int32_t> matches((size_t)N, -1), searched((size_t)N, -1);      // searched: which point a discarded feature held
    std::vector<uint8_t> discarded((size_t)N, 0);
    orbx_track_reference_result res;
    memset(&res, 0, sizeof res);
    res.matches = &matches[0]; res.search_matches = &searched[0]; res.discarded = &discarded[0]; res.pose = pose;
    orbx_shim::Mark("TrackReferenceKeyFrame marshalled");
    if (orbx_track_reference_keyframe(Matcher(N > kfa.n ? N : kfa.n), &kf, &fr, nnratio, checkOrientation ? 1 : 0, &res) != ORBX_OK)
        { orbx_shim::Fail("Tracking::TrackReferenceKeyFrame"); return false; }
    orbx_shim::Mark("TrackReferenceKeyFrame device call returned");
    nmatches = res.nmatches; nmatchesMap = res.nmatches_map;
    if (!res.ran_pose) return false;                                                       // :1201 (vpMapPointMatches is a local of the reference's function)
    // the write-back: mvpMapPoints as :1205 and :1225 leave them, the discarded points' fields (:1227-1228), mvbOutlier (PoseOptimization sets it for
    // every feature with a point, :1226 clears the discarded ones: all false behind this function), the pose
    for (int i = 0; i < N; i++) {
        F.mvpMapPoints[(size_t)i] = matches[(size_t)i] >= 0 ? kfa.vpMPs[(size_t)matches[(size_t)i]] : static_cast<MapPoint *>(NULL);
        if (matches[(size_t)i] >= 0 || discarded[(size_t)i]) F.mvbOutlier[(size_t)i] = false;
        if (discarded[(size_t)i]) {
            MapPoint *pMP = kfa.vpMPs[(size_t)searched[(size_t)i]];
            pMP->mbTrackInView = false;                                                    // :1227
            pMP->mnLastFrameSeen = F.mnId;                                                 // :1228
        }
    }
    SetPoseFrom(F, pose);
    orbx_shim::Mark("TrackReferenceKeyFrame returns");
    return true;
}

int TrackLocalMapHIP(Frame &F, const std::vector<MapPoint *> &vpLocalMapPoints, int th, bool bStereo, bool bOnlyTracking, float nnratio, float viewingCosLimit)
{
    orbx_shim::Mark("TrackLocalMap enters");
    const int N = F.N, nFeat = N > 0 ? N : 1;
    // step 1 of SearchLocalPoints (:1765-1784) and the held side of the gather: position and "has observations" of every point a feature holds
    std::vector<uint8_t> held((size_t)nFeat, 0), occupied((size_t)nFeat, 0);
    std::vector<float> heldPos((size_t)nFeat * 3, 0.f);
    for (int i = 0; i < N; i++) {
        MapPoint *pMP = F.mvpMapPoints[(size_t)i];
        if (!pMP) continue;
        if (MapPointAccess::BadElseIncreaseVisible(pMP)) { F.mvpMapPoints[(size_t)i] = static_cast<MapPoint *>(NULL); continue; }
        pMP->mnLastFrameSeen = F.mnId; pMP->mbTrackInView = false;
        held[(size_t)i] = 1;
        MapPointAccess::WorldPos(pMP, &heldPos[3 * (size_t)i]);
        occupied[(size_t)i] = MapPointAccess::GoodAndObserved(pMP) == 2 ? 1 : 0;
    }
    // step 2 (:1791-1811): the local points Frame::isInFrustum would be asked about, one visit each
    const size_t L = vpLocalMapPoints.size();
    std::vector<int> idx;
    idx.reserve(L);
    std::vector<float> pos(L * 3 + 3), nrm(L * 3 + 3), mx(L + 1), mn(L + 1);
    std::vector<uint8_t> desc(L * 32 + 32), hasObs(L + 1);
    for (size_t i = 0; i < L; i++) {
        MapPoint *pMP = vpLocalMapPoints[i];
        if (pMP->mnLastFrameSeen == F.mnId) continue;
        const size_t k = idx.size();
        if (!MapPointAccess::Snapshot(pMP, &pos[3 * k], &nrm[3 * k], mx[k], mn[k], hasObs[k], &desc[32 * k])) continue;      // isBad()
        idx.push_back((int)i);
    }
    const int M = (int)idx.size(), mFeat = M > 0 ? M : 1;
    std::vector<uint8_t> inView((size_t)mFeat, 0), outlier((size_t)nFeat, 0), found((size_t)nFeat, 0), cleared((size_t)nFeat, 0);
    std::vector<float> px((size_t)mFeat), py((size_t)mFeat), pxr((size_t)mFeat), vc((size_t)mFeat);
    std::vector<int32_t> lvl((size_t)mFeat), assigned((size_t)nFeat, -1);
    float tcw[16], ratioTh[64], pose[16];
    PoseOf(F.mTcw, tcw);
    if (orbx_predict_scale_thresholds(F.mfLogScaleFactor, F.mnScaleLevels, ratioTh) != ORBX_OK) { orbx_shim::Fail("Tracking::TrackLocalMap"); return 0; }
    orbx_projection_frame fr = {N > 0 ? (const orbx_keypoint *)&F.mvKeysUn[0] : 0, N > 0 ? F.mDescriptors.data : 0, N > 0 ? &F.mvuRight[0] : 0, &occupied[0], &N, nFeat, 1,
                                Frame::mnMinX, Frame::mnMinY, Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv};
    orbx_frustum_frame fp = {tcw, Frame::fx, Frame::fy, Frame::cx, Frame::cy, F.mbf, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY, ratioTh, F.mnScaleLevels, 1};
    orbx_local_points pts = {&pos[0], &nrm[0], &mx[0], &mn[0], &desc[0], &hasObs[0], M};
    orbx_track_local_result res;
    memset(&res, 0, sizeof res);
    res.assigned = &assigned[0]; res.in_view = &inView[0]; res.proj_x = &px[0]; res.proj_y = &py[0]; res.proj_xr = &pxr[0]; res.scale_level = &lvl[0]; res.view_cos = &vc[0];
    res.pose = pose; res.outlier = &outlier[0]; res.found = &found[0]; res.cleared = &cleared[0];
    orbx_shim::Mark("TrackLocalMap marshalled");
    if (orbx_track_local_map(Matcher(N > M ? N : M), &fr, &fp, &pts, &F.mvScaleFactors[0], (int)F.mvScaleFactors.size(), viewingCosLimit, (float)th, nnratio, &held[0],
                             &heldPos[0], &F.mvInvLevelSigma2[0], bStereo ? 1 : 0, &res) != ORBX_OK)
        { orbx_shim::Fail("Tracking::TrackLocalMap"); return 0; }
    orbx_shim::Mark("TrackLocalMap device call returned");
    for (int k = 0; k < M; k++) {                                                   // what Frame::isInFrustum leaves in the MapPoint, src/Frame.cc:615, :721-731
        MapPoint *pMP = vpLocalMapPoints[(size_t)idx[(size_t)k]];
        pMP->mbTrackInView = inView[(size_t)k] != 0;
        if (!inView[(size_t)k]) continue;
        pMP->mTrackProjX = px[(size_t)k]; pMP->mTrackProjXR = pxr[(size_t)k]; pMP->mTrackProjY = py[(size_t)k];
        pMP->mnTrackScaleLevel = lvl[(size_t)k]; pMP->mTrackViewCos = vc[(size_t)k];
        pMP->IncreaseVisible();                                                     // src/Tracking.cc:1807
    }
    if (N > 0) SetPoseFrom(F, pose);
    for (int i = 0; i < N; i++) {
        if (assigned[(size_t)i] >= 0) F.mvpMapPoints[(size_t)i] = vpLocalMapPoints[(size_t)idx[(size_t)assigned[(size_t)i]]];     // src/ORBmatcher.cc:165
        MapPoint *pMP = F.mvpMapPoints[(size_t)i];
        if (!pMP) continue;
        F.mvbOutlier[(size_t)i] = outlier[(size_t)i] != 0;                          // src/Optimizer.cc:437 / :551-563
        if (found[(size_t)i]) pMP->IncreaseFound();                                 // src/Tracking.cc:1471
        if (cleared[(size_t)i]) F.mvpMapPoints[(size_t)i] = static_cast<MapPoint *>(NULL);      // :1485-1486
    }
    orbx_shim::Mark("TrackLocalMap returns");
    return bOnlyTracking ? res.inliers_all : res.inliers_map;                       // mnMatchesInliers, :1473-1483
}

}  // namespace ORB_SLAM2
