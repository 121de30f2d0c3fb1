// shim/LoopClosing_hip.cc -- the Sim3 propagation of LoopClosing::CorrectLoop (src/LoopClosing.cc:617-716) and the map update after global bundle
// adjustment (:930-1003) over orbx_loop_correct_sim3 / orbx_loop_propagate_gba.
//
// Compiled against the REFERENCE's own headers, like the other shim files.  A file of its own: the drop-in library of oracle/Makefile does not
// link it; it is compile-checked only.
//
// The gather.  Keyframes get slots in the order they are met.  The group's order is the order in which the reference iterates CorrectedSim3, a
// std::map<KeyFrame*, ...>: ascending POINTER, taken from a std::map of the group.  Every map point is visited ONCE, under its two mutexes
// (MapPointAccess::BadObservationsRefAndPos): isBad(), the observers in the map's order, mpRefKF and the position in one copy; the octave of the
// reference keyframe's keypoint and its scale factors are const members and need no lock.  A keyframe's list is GetMapPointMatches(), NULL entries
// kept as -1.  GetPose() and GetCameraCenter() are read once per slot.
// The write-back is the reference's: SetWorldPos, mnCorrectedByKF, mnCorrectedReference and the three stores of UpdateNormalAndDepth per moved
// point, SetPose per group keyframe, the two KeyFrameAndPose maps; mTcwGBA, mnBAGlobalForKF, mTcwBefGBA, SetPose and SetWorldPos after global BA.
// PARITY UNPINNED: the device sees the map as gathered (the caller holds mMutexMapUpdate, as the reference does; local mapping is stopped).  A
// point whose reference keyframe is no longer in the map is left where it is by PropagateGBA; the reference reads that keyframe's stale members.
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Map.h"
#include "LoopClosing.h"
#include "Converter.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
#include "MapPointAccess.h"
#include "orbx.h"
#include "shim_error.h"
#include "LoopClosing_hip.h"

namespace ORB_SLAM2
{
namespace
{
struct Slots {
    std::vector<KeyFrame *> kfs;
    std::map<KeyFrame *, int> slotOf;
    int Slot(KeyFrame *kf)
    {
        std::map<KeyFrame *, int>::iterator it = slotOf.find(kf);
        if (it != slotOf.end()) return it->second;
        const int s = (int)kfs.size();
        slotOf[kf] = s;
        kfs.push_back(kf);
        return s;
    }
    int Find(KeyFrame *kf) const
    {
        std::map<KeyFrame *, int>::const_iterator it = slotOf.find(kf);
        return it == slotOf.end() ? -1 : it->second;
    }
};

void PutPose(const cv::Mat &T, float *o)      // rows 0..2 of a 4x4 CV_32F
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) o[4 * r + c] = T.at<float>(r, c);
}

cv::Mat PoseMat(const float *p)
{
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) T.at<float>(r, c) = p[4 * r + c];
    return T;
}

cv::Mat PointMat(const float *p)
{
    cv::Mat X(3, 1, CV_32F);
    for (int c = 0; c < 3; c++) X.at<float>(c) = p[c];
    return X;
}

g2o::Sim3 GetSim3(const double *v) { return g2o::Sim3(Eigen::Quaterniond(v[3], v[0], v[1], v[2]), Eigen::Vector3d(v[4], v[5], v[6]), v[7]); }
}  // namespace

LoopCorrection_hip::LoopCorrection_hip() : mpOps(0)
{
    if (orbx_loop_create(orbx_shim::Device(), &mpOps) != ORBX_OK) {
        mpOps = 0;
        orbx_shim::Fail("LoopCorrection");
    }
}

LoopCorrection_hip::~LoopCorrection_hip()
{
    if (mpOps) orbx_loop_destroy(mpOps);
}

bool LoopCorrection_hip::CorrectLoopPropagate(KeyFrame *pCurrentKF, const std::vector<KeyFrame *> &vpCurrentConnectedKFs, const g2o::Sim3 &g2oScw,
                                              LoopClosing::KeyFrameAndPose &CorrectedSim3, LoopClosing::KeyFrameAndPose &NonCorrectedSim3)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpOps) return orbx_shim::Fail("LoopCorrection::CorrectLoopPropagate", "no device handle");
    // the group in the order of CorrectedSim3 (:664): ascending pointer, every keyframe once
    std::set<KeyFrame *> sGroup(vpCurrentConnectedKFs.begin(), vpCurrentConnectedKFs.end());
    sGroup.insert(pCurrentKF);
    Slots S;
    std::vector<KeyFrame *> group(sGroup.begin(), sGroup.end());
    std::vector<int32_t> groupKf, listOff(1, 0), listPoint, obsOff(1, 0), obsKf, pointRef;
    std::vector<uint8_t> pointBad, pointDone;
    std::vector<float> pos, refScale, topScale;
    std::vector<MapPoint *> points;
    std::map<MapPoint *, int> pointOf;
    std::vector<std::pair<KeyFrame *, size_t> > obs;
    int current = -1;
    for (size_t g = 0; g < group.size(); g++) {
        groupKf.push_back(S.Slot(group[g]));
        if (group[g] == pCurrentKF) current = (int)g;
    }
    for (size_t g = 0; g < group.size(); g++) {
        const std::vector<MapPoint *> vpMPsi = group[g]->GetMapPointMatches();
        for (size_t i = 0; i < vpMPsi.size(); i++) {
            MapPoint *pMP = vpMPsi[i];
            if (!pMP) { listPoint.push_back(-1); continue; }
            std::map<MapPoint *, int>::iterator it = pointOf.find(pMP);
            if (it != pointOf.end()) { listPoint.push_back(it->second); continue; }
            const int p = (int)points.size();
            pointOf[pMP] = p;
            points.push_back(pMP);
            listPoint.push_back(p);
            KeyFrame *pRef = 0;
            float X[3];
            const bool bad = MapPointAccess::BadObservationsRefAndPos(pMP, obs, pRef, X);
            pointBad.push_back(bad ? 1 : 0);
            pointDone.push_back(pMP->mnCorrectedByKF == pCurrentKF->mnId ? 1 : 0);
            pos.insert(pos.end(), X, X + 3);
            size_t idx = 0;      // observations[pRefKF] of :510 inserts 0 for a missing key
            for (size_t o = 0; o < obs.size(); o++) {
                obsKf.push_back(S.Slot(obs[o].first));
                if (obs[o].first == pRef) idx = obs[o].second;
            }
            obsOff.push_back((int32_t)obsKf.size());
            if (!bad && pRef) {
                pointRef.push_back(S.Slot(pRef));
                refScale.push_back(pRef->mvScaleFactors[pRef->mvKeysUn[idx].octave]);
                topScale.push_back(pRef->mvScaleFactors[pRef->mnScaleLevels - 1]);
            } else {      // never read: a bad point is not moved
                pointRef.push_back(0);
                refScale.push_back(1.0f);
                topScale.push_back(1.0f);
            }
        }
        listOff.push_back((int32_t)listPoint.size());
    }
    const size_t NK = S.kfs.size(), G = group.size(), M = points.size();
    std::vector<float> tcw(12 * NK), ow(3 * NK);
    for (size_t s = 0; s < NK; s++) {
        PutPose(S.kfs[s]->GetPose(), &tcw[12 * s]);
        const cv::Mat O = S.kfs[s]->GetCameraCenter();
        for (int c = 0; c < 3; c++) ow[3 * s + c] = O.at<float>(c);
    }
    const Eigen::Quaterniond &q = g2oScw.rotation();
    const Eigen::Vector3d t = g2oScw.translation();
    const double scw[8] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2), g2oScw.scale()};

    orbx_loop_sim3_problem P;
    P.num_keyframes = (int)NK; P.tcw = tcw.data(); P.ow = ow.data();
    P.num_group = (int)G; P.current = current; P.group_kf = groupKf.data(); P.scw = scw;
    P.num_entries = (int)listPoint.size(); P.list_offset = listOff.data(); P.list_point = listPoint.data();
    P.num_points = (int)M; P.num_obs = (int)obsKf.size();
    P.pos = pos.data(); P.point_bad = pointBad.data(); P.point_done = pointDone.data(); P.point_ref = pointRef.data();
    P.ref_scale = refScale.data(); P.top_scale = topScale.data(); P.obs_offset = obsOff.data(); P.obs_kf = obsKf.data();
    std::vector<double> nonc(8 * G), corr(8 * G);
    std::vector<float> tiw(12 * G), newPos(3 * M + 1), normal(3 * M + 1), maxD(M + 1), minD(M + 1);
    std::vector<int32_t> by(M + 1);
    std::vector<uint8_t> updated(M + 1);
    orbx_loop_sim3_result R;
    R.noncorrected = nonc.data(); R.corrected = corr.data(); R.tiw = tiw.data(); R.ow_new = 0; R.scw_mat = 0;
    R.pos = newPos.data(); R.corrected_by = by.data(); R.normal = normal.data(); R.max_dist = maxD.data(); R.min_dist = minD.data(); R.updated = updated.data();
    if (orbx_loop_correct_sim3(mpOps, &P, &R) != ORBX_OK) return orbx_shim::Fail("LoopCorrection::CorrectLoopPropagate");

    for (size_t p = 0; p < M; p++) {      // :692-696
        if (by[p] < 0) continue;
        MapPoint *pMP = points[p];
        pMP->SetWorldPos(PointMat(&newPos[3 * p]));
        pMP->mnCorrectedByKF = pCurrentKF->mnId;
        pMP->mnCorrectedReference = group[(size_t)by[p]]->mnId;
        if (updated[p]) MapPointAccess::StoreNormalAndDepth(pMP, &normal[3 * p], maxD[p], minD[p]);
    }
    for (size_t g = 0; g < G; g++) {      // :650, :658, :710
        CorrectedSim3[group[g]] = GetSim3(&corr[8 * g]);
        NonCorrectedSim3[group[g]] = GetSim3(&nonc[8 * g]);
        group[g]->SetPose(PoseMat(&tiw[12 * g]));
    }
    return true;
}

bool LoopCorrection_hip::PropagateGBA(Map *pMap, unsigned long nLoopKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpOps) return orbx_shim::Fail("LoopCorrection::PropagateGBA", "no device handle");
    Slots S;
    const std::vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    for (size_t i = 0; i < vpKFs.size(); i++) S.Slot(vpKFs[i]);
    const std::set<KeyFrame *> sOrigins(pMap->mvpKeyFrameOrigins.begin(), pMap->mvpKeyFrameOrigins.end());
    for (std::set<KeyFrame *>::const_iterator it = sOrigins.begin(); it != sOrigins.end(); ++it) S.Slot(*it);
    const size_t n = S.kfs.size();
    std::vector<int32_t> parent(n);
    std::vector<uint8_t> inGba(n);
    std::vector<float> tcw(12 * n), gba(12 * n, 0.0f);
    for (size_t s = 0; s < n; s++) {
        KeyFrame *pKF = S.kfs[s];
        KeyFrame *pParent = pKF->GetParent();
        // the walk follows GetChilds() from the origins: a keyframe is reached through its parent's child set
        parent[s] = sOrigins.count(pKF) ? -1 : (pParent && pParent->GetChilds().count(pKF) ? S.Find(pParent) : -2);
        if (parent[s] < -1 || (parent[s] == -1 && !sOrigins.count(pKF))) parent[s] = -2;
        inGba[s] = pKF->mnBAGlobalForKF == nLoopKF ? 1 : 0;
        PutPose(pKF->GetPose(), &tcw[12 * s]);
        if (!pKF->mTcwGBA.empty()) PutPose(pKF->mTcwGBA, &gba[12 * s]);
    }
    const std::vector<MapPoint *> vpMPs = pMap->GetAllMapPoints();
    const size_t M = vpMPs.size();
    std::vector<float> pos(3 * M + 1), posGba(3 * M + 1, 0.0f);
    std::vector<uint8_t> ptIn(M + 1), ptBad(M + 1);
    std::vector<int32_t> ptRef(M + 1);
    for (size_t i = 0; i < M; i++) {
        MapPoint *pMP = vpMPs[i];
        ptBad[i] = pMP->isBad() ? 1 : 0;
        ptIn[i] = pMP->mnBAGlobalForKF == nLoopKF ? 1 : 0;
        MapPointAccess::WorldPos(pMP, &pos[3 * i]);
        if (ptIn[i] && !pMP->mPosGBA.empty())
            for (int c = 0; c < 3; c++) posGba[3 * i + c] = pMP->mPosGBA.at<float>(c);
        KeyFrame *pRef = ptBad[i] ? 0 : pMP->GetReferenceKeyFrame();
        ptRef[i] = pRef ? S.Find(pRef) : -1;
    }
    orbx_loop_gba_problem P;
    P.num_keyframes = (int)n; P.parent = parent.data(); P.tcw = tcw.data(); P.tcw_gba = gba.data(); P.in_gba = inGba.data();
    P.num_points = (int)M; P.pos = pos.data(); P.pos_gba = posGba.data(); P.point_in_gba = ptIn.data(); P.point_bad = ptBad.data(); P.point_ref = ptRef.data();
    std::vector<float> gbaOut(12 * n), posOut(3 * M + 1);
    std::vector<uint8_t> reached(n), moved(M + 1);
    orbx_loop_gba_result R;
    R.tcw_gba = gbaOut.data(); R.reached = reached.data(); R.pos = posOut.data(); R.moved = moved.data();
    if (orbx_loop_propagate_gba(mpOps, &P, &R) != ORBX_OK) return orbx_shim::Fail("LoopCorrection::PropagateGBA");

    for (size_t s = 0; s < n; s++) {      // :943-957
        if (!reached[s]) continue;
        KeyFrame *pKF = S.kfs[s];
        if (!inGba[s] && parent[s] >= 0) {
            pKF->mTcwGBA = PoseMat(&gbaOut[12 * s]);
            pKF->mnBAGlobalForKF = nLoopKF;
        }
        pKF->mTcwBefGBA = pKF->GetPose();
        pKF->SetPose(pKF->mTcwGBA);
    }
    for (size_t i = 0; i < M; i++)      // :978, :1002
        if (moved[i]) vpMPs[i]->SetWorldPos(PointMat(&posOut[3 * i]));
    return true;
}
}  // namespace ORB_SLAM2
