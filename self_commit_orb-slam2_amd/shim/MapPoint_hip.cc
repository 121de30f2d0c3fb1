// shim/MapPoint_hip.cc -- MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth for a whole list of points in ONE device call.
//
// Compiled against the REFERENCE's own include/MapPoint.h / KeyFrame.h, like the other shim files.  It replaces no member function: the loops
//     for (each pMP) { pMP->ComputeDistinctiveDescriptors(); pMP->UpdateNormalAndDepth(); }
// of LocalMapping (src/LocalMapping.cc:233-235, 612-614, 726-729), Tracking::CreateNewKeyFrame (src/Tracking.cc:1720-1721), the bundle adjustments
// (src/Optimizer.cc:331, 995, 1337) and loop correction (src/LoopClosing.cc:696, 737) become one call of
//     ORB_SLAM2::orbx_shim::RefreshMapPoints(points, descriptor, normalAndDepth)
// ("MapPoint refresh").  A file of its own: the drop-in library of oracle/Makefile does not link it; it is compile-checked only.
//
// Per point, through an accessor derived from MapPoint (as in shim/MapPointAccess.h): the observations IN THE MAP'S ORDER, mpRefKF and mWorldPos are
// copied under mMutexFeatures, then mMutexPos - the order MapPoint::UpdateNormalAndDepth takes them (src/MapPoint.cc:483-484) -, the keyframes
// are asked (isBad, GetCameraCenter, mDescriptors.row, mvKeysUn[...].octave) after the point's mutexes are released, as the reference does.
// Results are written back under the mutex the reference holds for each: mDescriptor under mMutexFeatures (:432), mfMaxDistance / mfMinDistance /
// mNormalVector under mMutexPos (:515); a point that went bad meanwhile is skipped.  On a device error nothing is written (shim_error.h).
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbx.h"
#include "shim_error.h"

static unsigned long gRefreshCalls = 0;
extern "C" __attribute__((visibility("default"))) unsigned long orbx_shim_refresh_map_points_calls(void) { return gRefreshCalls; }

namespace ORB_SLAM2
{
namespace
{
struct MapPointRefreshAccess : public MapPoint {
    // what both reference functions copy before they work (src/MapPoint.cc:367-372, 482-491); false = bad
    static bool Gather(MapPoint *p, std::vector<std::pair<KeyFrame *, size_t> > &obs, KeyFrame *&ref, float pos[3])
    {
        MapPointRefreshAccess *q = static_cast<MapPointRefreshAccess *>(p);
        std::unique_lock<std::mutex> lock1(q->mMutexFeatures);
        std::unique_lock<std::mutex> lock2(q->mMutexPos);
        if (q->mbBad) return false;
        obs.assign(q->mObservations.begin(), q->mObservations.end());      // the map's order
        ref = q->mpRefKF;
        for (int c = 0; c < 3; c++) pos[c] = q->mWorldPos.at<float>(c);
        return true;
    }
    static void StoreDescriptor(MapPoint *p, const cv::Mat &row)
    {
        MapPointRefreshAccess *q = static_cast<MapPointRefreshAccess *>(p);
        std::unique_lock<std::mutex> lock(q->mMutexFeatures);
        if (q->mbBad) return;
        q->mDescriptor = row.clone();
    }
    static void StoreNormalAndDepth(MapPoint *p, const float nrm[3], float maxD, float minD)
    {
        MapPointRefreshAccess *q = static_cast<MapPointRefreshAccess *>(p);
        cv::Mat n(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) n.at<float>(c) = nrm[c];
        std::unique_lock<std::mutex> lock3(q->mMutexPos);      // (SetBadFlag writes mbBad under both mutexes: either one makes the read safe)
        if (q->mbBad) return;
        q->mfMaxDistance = maxD;
        q->mfMinDistance = minD;
        q->mNormalVector = n;
    }
};

// one handle per calling thread (local mapper, tracker, loop closer), grown when a call needs more
struct ThreadMapPointOps {
    orbx_mappoint_ops *h;
    int capPoints, capObs;
    ThreadMapPointOps() : h(0), capPoints(0), capObs(0) {}
    ~ThreadMapPointOps() { if (h) orbx_mappoint_ops_destroy(h); }
};
thread_local ThreadMapPointOps tOps;

// isBad() / GetCameraCenter() once per keyframe and call
struct KfState { bool bad; float ow[3]; };
const KfState &StateOf(std::map<KeyFrame *, KfState> &kfs, KeyFrame *kf)
{
    std::map<KeyFrame *, KfState>::iterator it = kfs.find(kf);
    if (it != kfs.end()) return it->second;
    KfState s;
    s.bad = kf->isBad();
    const cv::Mat ow = kf->GetCameraCenter();
    for (int c = 0; c < 3; c++) s.ow[c] = ow.at<float>(c);
    return kfs[kf] = s;
}
}  // namespace

namespace orbx_shim
{
void RefreshMapPoints(const std::vector<MapPoint *> &pts, bool descriptor, bool normalAndDepth)
{
    __atomic_add_fetch(&gRefreshCalls, 1, __ATOMIC_RELAXED);
    if (pts.empty() || (!descriptor && !normalAndDepth)) return;
    std::vector<MapPoint *> live;
    std::vector<int32_t> off(1, 0);
    std::vector<std::pair<KeyFrame *, size_t> > all, obs;
    std::vector<float> pos, refc, rsc, tsc;
    std::map<KeyFrame *, KfState> kfs;
    for (size_t i = 0; i < pts.size(); i++) {
        MapPoint *p = pts[i];
        KeyFrame *ref = 0;
        float x[3];
        if (!p || !MapPointRefreshAccess::Gather(p, obs, ref, x)) continue;      // (!p: the callers' vectors hold NULLs; bad: both functions return)
        if (obs.empty() || !ref) continue;                                         // :374, :493
        size_t refIdx = 0;                                                         // observations[pRefKF] (:510): 0 when the map has no such key
        for (size_t k = 0; k < obs.size(); k++) {
            KeyFrame *kf = obs[k].first;
            if (kf == ref) refIdx = obs[k].second;
            (void)StateOf(kfs, kf);
        }
        live.push_back(p);
        all.insert(all.end(), obs.begin(), obs.end());
        off.push_back((int32_t)all.size());
        const KfState &rs = StateOf(kfs, ref);
        for (int c = 0; c < 3; c++) { pos.push_back(x[c]); refc.push_back(rs.ow[c]); }
        rsc.push_back(ref->mvScaleFactors[ref->mvKeysUn[refIdx].octave]);
        tsc.push_back(ref->mvScaleFactors[ref->mnScaleLevels - 1]);
    }
    const int M = (int)live.size(), T = (int)all.size();
    if (M == 0) return;
    std::vector<unsigned char> desc((size_t)T * 32), valid((size_t)T);
    std::vector<float> cam((size_t)T * 3);
    for (int t = 0; t < T; t++) {
        const KfState &s = kfs[all[t].first];
        valid[t] = s.bad ? 0 : 1;
        memcpy(&desc[(size_t)t * 32], all[t].first->mDescriptors.ptr<unsigned char>((int)all[t].second), 32);
        for (int c = 0; c < 3; c++) cam[(size_t)t * 3 + c] = s.ow[c];
    }

    ThreadMapPointOps &O = tOps;
    if (!O.h || M > O.capPoints || T > O.capObs) {
        if (O.h) { orbx_mappoint_ops_destroy(O.h); O.h = 0; }
        O.capPoints = std::max(2 * M, 4096); O.capObs = std::max(2 * T, 65536);
        if (orbx_mappoint_ops_create(::orbx_shim::Device(), O.capPoints, O.capObs, &O.h) != ORBX_OK) { O.h = 0; ::orbx_shim::Fail("RefreshMapPoints"); return; }
    }
    orbx_mappoint_batch b;
    b.num_points = M; b.num_obs = T; b.obs_offset = &off[0]; b.desc = &desc[0]; b.desc_valid = &valid[0]; b.cam_center = &cam[0];
    b.pos = &pos[0]; b.ref_center = &refc[0]; b.ref_scale = &rsc[0]; b.top_scale = &tsc[0];
    std::vector<int32_t> best(M);
    std::vector<float> nrm((size_t)M * 3), maxD(M), minD(M);
    orbx_mappoint_result r;
    r.best_obs = &best[0]; r.best_median = 0; r.normal = &nrm[0]; r.max_dist = &maxD[0]; r.min_dist = &minD[0]; r.updated = 0;
    if (orbx_mappoint_refresh(O.h, &b, &r) != ORBX_OK) { ::orbx_shim::Fail("RefreshMapPoints"); return; }      // the points stay as they were

    for (int i = 0; i < M; i++) {      // (every gathered point has observations: updated == 1)
        if (descriptor && best[i] >= 0) {      // -1: every observer is bad, the reference returns before it writes (:388)
            const std::pair<KeyFrame *, size_t> &o = all[(size_t)off[i] + best[i]];
            MapPointRefreshAccess::StoreDescriptor(live[i], o.first->mDescriptors.row((int)o.second));
        }
        if (normalAndDepth) MapPointRefreshAccess::StoreNormalAndDepth(live[i], &nrm[(size_t)i * 3], maxD[i], minD[i]);
    }
}
}  // namespace orbx_shim
}  // namespace ORB_SLAM2
