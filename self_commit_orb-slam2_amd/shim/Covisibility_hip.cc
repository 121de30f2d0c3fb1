// shim/Covisibility_hip.cc -- KeyFrame::UpdateConnections (src/KeyFrame.cc:386-507), LocalMapping::KeyFrameCulling (src/LocalMapping.cc:873-956) and the
// vote of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1897-1950) over orbx_covis_*.
//
// Compiled against the REFERENCE's own headers, like the other shim files.  A file of its own: the drop-in library of oracle/Makefile does not
// link it; it is compile-checked only.
//
// The gather.  Keyframes get slots in the order they are met; their ranks are the ranks of the KeyFrame POINTERS (std::map<KeyFrame*, ...> orders by
// them), taken from a std::map of the slots.  Every map point is visited ONCE, under its two mutexes (MapPointAccess::BadAndObservations): isBad()
// and the observers in one copy; the observers' octave and mvuRight are const members of the keyframes and need no lock.  A keyframe's list is its
// mvpMapPoints copied under mMutexFeatures, as the reference copies it.
// The write-back is the reference's, in the reference's order: AddConnection on the connected keyframes, then mConnectedKeyFrameWeights /
// mvpOrderedConnectedKeyFrames / mvOrderedWeights under mMutexConnections, the first-connection parent, and RefreshCovisibles for the device keyframe
// database.  The spanning-tree repair of SetBadFlag stays KeyFrame::SetBadFlag(): the culling calls it on the culled keyframes in list order.
// PARITY UNPINNED: the device sees the map as gathered; the reference's loop reads every point as of its own visit (another thread may change a
// point between two keyframes of one culling pass).
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "MapPointAccess.h"
#include "orbx.h"
#include "shim_error.h"
#include "KeyFrameDatabase_hip.h"
#include "Covisibility_hip.h"

namespace ORB_SLAM2
{
namespace
{
struct KeyFrameCovisAccess : public KeyFrame {
    static void Points(KeyFrame *kf, std::vector<MapPoint *> &out)
    {
        KeyFrameCovisAccess *q = static_cast<KeyFrameCovisAccess *>(kf);
        std::unique_lock<std::mutex> lock(q->mMutexFeatures);
        out = q->mvpMapPoints;
    }
    static bool NotErase(KeyFrame *kf)
    {
        KeyFrameCovisAccess *q = static_cast<KeyFrameCovisAccess *>(kf);
        std::unique_lock<std::mutex> lock(q->mMutexConnections);
        return q->mbNotErase;
    }
    // step 3 of UpdateConnections (:487-506); -> this was the first connection of a keyframe other than the first: the caller sets the parent
    static bool Store(KeyFrame *kf, const std::map<KeyFrame *, int> &counter, const std::vector<KeyFrame *> &ordered, const std::vector<int> &weights)
    {
        KeyFrameCovisAccess *q = static_cast<KeyFrameCovisAccess *>(kf);
        std::unique_lock<std::mutex> lock(q->mMutexConnections);
        q->mConnectedKeyFrameWeights = counter;
        q->mvpOrderedConnectedKeyFrames = ordered;
        q->mvOrderedWeights = weights;
        if (q->mbFirstConnection && q->mnId != 0) {
            q->mbFirstConnection = false;
            return true;
        }
        return false;
    }
};

// the arrays of orbx_covis_slice and the objects behind the slots
struct Slice {
    std::vector<KeyFrame *> kfs;                  // slot -> keyframe
    std::map<KeyFrame *, int> slotOf;
    std::map<MapPoint *, int> pointOf;
    std::vector<int32_t> rank, obsOff, obsKf, listOff, listKf, listPoint;
    std::vector<uint8_t> flags, obsOct, obsStereo, pointBad, listOct, listClose;
    std::vector<std::pair<KeyFrame *, size_t> > obs;      // reused

    Slice() { obsOff.push_back(0); listOff.push_back(0); }
    int Slot(KeyFrame *kf)
    {
        std::map<KeyFrame *, int>::iterator it = slotOf.find(kf);
        if (it != slotOf.end()) return it->second;
        const int s = (int)kfs.size();
        slotOf[kf] = s;
        kfs.push_back(kf);
        return s;
    }
    // one visit per point; -> its index
    int Point(MapPoint *pMP)
    {
        std::map<MapPoint *, int>::iterator it = pointOf.find(pMP);
        if (it != pointOf.end()) return it->second;
        const int p = (int)pointBad.size();
        pointOf[pMP] = p;
        pointBad.push_back(MapPointAccess::BadAndObservations(pMP, obs) ? 1 : 0);
        for (size_t i = 0; i < obs.size(); i++) {
            KeyFrame *pKFi = obs[i].first;
            obsKf.push_back(Slot(pKFi));
            obsOct.push_back((uint8_t)pKFi->mvKeysUn[obs[i].second].octave);
            obsStereo.push_back(pKFi->mvuRight[obs[i].second] >= 0 ? 1 : 0);
        }
        obsOff.push_back((int32_t)obsKf.size());
        return p;
    }
    void AddList(KeyFrame *owner, const std::vector<MapPoint *> &pts, bool bMonocular)
    {
        listKf.push_back(owner ? Slot(owner) : -1);
        for (size_t i = 0; i < pts.size(); i++) {
            if (!pts[i]) continue;
            listPoint.push_back(Point(pts[i]));
            listOct.push_back(owner ? (uint8_t)owner->mvKeysUn[i].octave : 0);
            listClose.push_back(!owner || bMonocular || !(owner->mvDepth[i] > owner->mThDepth || owner->mvDepth[i] < 0) ? 1 : 0);
        }
        listOff.push_back((int32_t)listPoint.size());
    }
    // ranks and flags of the slots, then the C struct (the vectors must stay as they are while it is used)
    orbx_covis_slice Finish(bool culling)
    {
        rank.resize(kfs.size());
        flags.resize(kfs.size());
        int r = 0;
        for (std::map<KeyFrame *, int>::const_iterator it = slotOf.begin(); it != slotOf.end(); ++it) rank[(size_t)it->second] = r++;      // pointer order
        for (size_t s = 0; s < kfs.size(); s++)
            flags[s] = (uint8_t)((kfs[s]->mnId == 0 ? 1 : 0) | (culling && KeyFrameCovisAccess::NotErase(kfs[s]) ? 2 : 0) | (kfs[s]->isBad() ? 4 : 0));
        orbx_covis_slice S;
        S.num_keyframes = (int)kfs.size(); S.kf_rank = rank.data(); S.kf_flags = flags.data();
        S.num_points = (int)pointBad.size(); S.num_obs = (int)obsKf.size();
        S.obs_offset = obsOff.data(); S.obs_kf = obsKf.data(); S.obs_octave = obsOct.data(); S.obs_stereo = obsStereo.data(); S.point_bad = pointBad.data();
        S.num_lists = (int)listKf.size(); S.num_entries = (int)listPoint.size();
        S.list_offset = listOff.data(); S.list_kf = listKf.data(); S.list_point = listPoint.data(); S.list_octave = listOct.data(); S.list_close = listClose.data();
        return S;
    }
};
}  // namespace

Covisibility_hip::Covisibility_hip(KeyFrameDatabase_hip *pKFDB) : mpOps(0), mpKFDB(pKFDB)
{
    if (orbx_covis_create(orbx_shim::Device(), &mpOps) != ORBX_OK) {
        mpOps = 0;
        orbx_shim::Fail("Covisibility");
    }
}

Covisibility_hip::~Covisibility_hip()
{
    if (mpOps) orbx_covis_destroy(mpOps);
}

void Covisibility_hip::UpdateConnections(KeyFrame *pKF)
{
    UpdateConnections(std::vector<KeyFrame *>(1, pKF));
}

void Covisibility_hip::UpdateConnections(const std::vector<KeyFrame *> &vpKFs)
{
    if (!mpOps || vpKFs.empty()) return;
    Slice sl;
    std::vector<MapPoint *> vpMP;
    for (size_t q = 0; q < vpKFs.size(); q++) {
        KeyFrameCovisAccess::Points(vpKFs[q], vpMP);
        sl.AddList(vpKFs[q], vpMP, true);
    }
    const orbx_covis_slice S = sl.Finish(false);
    const size_t Q = vpKFs.size();
    // a counter holds at most every slot, and at most one entry per observation under the list
    size_t cap = 0;
    for (size_t q = 0; q < Q; q++) {
        size_t n = 0;
        for (int32_t e = sl.listOff[q]; e < sl.listOff[q + 1] && n < sl.kfs.size(); e++) n += (size_t)(sl.obsOff[(size_t)sl.listPoint[(size_t)e] + 1] - sl.obsOff[(size_t)sl.listPoint[(size_t)e]]);
        cap += std::min(n, sl.kfs.size()) + 1;
    }
    std::vector<int32_t> cOff(Q + 1), cKf(cap), cW(cap), nMax(Q), kfMax(Q), nOff(Q + 1), nKf(cap), nW(cap);
    orbx_covis_connections R;
    R.counter_offset = cOff.data(); R.counter_kf = cKf.data(); R.counter_weight = cW.data(); R.counter_capacity = (int)cap;
    R.n_max = nMax.data(); R.kf_max = kfMax.data();
    R.conn_offset = nOff.data(); R.conn_kf = nKf.data(); R.conn_weight = nW.data(); R.conn_capacity = (int)cap;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (orbx_covis_update_connections(mpOps, &S, 15, &R) != ORBX_OK) { orbx_shim::Fail("KeyFrame::UpdateConnections"); return; }
    }
    for (size_t q = 0; q < Q; q++) {
        if (cOff[q + 1] == cOff[q]) continue;      // "This should not happen": the reference returns
        KeyFrame *pKF = vpKFs[q];
        std::map<KeyFrame *, int> KFcounter;
        for (int32_t i = cOff[q]; i < cOff[q + 1]; i++) KFcounter[sl.kfs[(size_t)cKf[(size_t)i]]] = cW[(size_t)i];
        std::vector<KeyFrame *> ordered;
        std::vector<int> weights;
        for (int32_t i = nOff[q]; i < nOff[q + 1]; i++) {
            KeyFrame *other = sl.kfs[(size_t)nKf[(size_t)i]];
            other->AddConnection(pKF, nW[(size_t)i]);
            ordered.push_back(other);
            weights.push_back(nW[(size_t)i]);
        }
        if (KeyFrameCovisAccess::Store(pKF, KFcounter, ordered, weights)) pKF->ChangeParent(ordered.front());      // mpParent = front; mpParent->AddChild(this)
        if (mpKFDB) mpKFDB->RefreshCovisibles(pKF);
    }
}

void Covisibility_hip::KeyFrameCulling(KeyFrame *pKF, bool bMonocular)
{
    if (!mpOps) return;
    const std::vector<KeyFrame *> vpLocalKeyFrames = pKF->GetVectorCovisibleKeyFrames();
    if (vpLocalKeyFrames.empty()) return;
    Slice sl;
    for (size_t q = 0; q < vpLocalKeyFrames.size(); q++) sl.AddList(vpLocalKeyFrames[q], vpLocalKeyFrames[q]->GetMapPointMatches(), bMonocular);
    const orbx_covis_slice S = sl.Finish(true);
    std::vector<uint8_t> culled(vpLocalKeyFrames.size(), 0);
    orbx_covis_culling R;
    R.n_mps = 0; R.n_redundant = 0; R.culled = culled.data(); R.point_bad = 0; R.point_obs = 0;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (orbx_covis_keyframe_culling(mpOps, &S, &R) != ORBX_OK) { orbx_shim::Fail("LocalMapping::KeyFrameCulling"); return; }
    }
    for (size_t q = 0; q < vpLocalKeyFrames.size(); q++)
        if (culled[q]) vpLocalKeyFrames[q]->SetBadFlag();      // the erases the device has applied, the connections and the spanning tree
}

bool Covisibility_hip::UpdateLocalKeyFrames(Frame &F, std::map<KeyFrame *, int> &keyframeCounter, KeyFrame *&pKFmax, int &nmax)
{
    keyframeCounter.clear();
    pKFmax = static_cast<KeyFrame *>(NULL);
    nmax = 0;
    if (!mpOps) return false;
    Slice sl;
    sl.AddList(0, F.mvpMapPoints, true);
    for (int i = 0; i < F.N; i++) {      // :1912-1915
        MapPoint *pMP = F.mvpMapPoints[i];
        if (pMP && sl.pointBad[(size_t)sl.pointOf[pMP]]) F.mvpMapPoints[i] = static_cast<MapPoint *>(NULL);
    }
    if (sl.kfs.empty()) return false;
    const orbx_covis_slice S = sl.Finish(false);
    const size_t cap = sl.kfs.size() + 1;
    std::vector<int32_t> cOff(2), cKf(cap), cW(cap), n1(1), k1(1);
    orbx_covis_connections R;
    R.counter_offset = cOff.data(); R.counter_kf = cKf.data(); R.counter_weight = cW.data(); R.counter_capacity = (int)cap;
    R.n_max = n1.data(); R.kf_max = k1.data();
    R.conn_offset = 0; R.conn_kf = 0; R.conn_weight = 0; R.conn_capacity = 0;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (orbx_covis_update_connections(mpOps, &S, 15, &R) != ORBX_OK) { orbx_shim::Fail("Tracking::UpdateLocalKeyFrames"); return false; }
    }
    for (int32_t i = 0; i < cOff[1]; i++) keyframeCounter[sl.kfs[(size_t)cKf[(size_t)i]]] = cW[(size_t)i];
    if (k1[0] >= 0) { pKFmax = sl.kfs[(size_t)k1[0]]; nmax = n1[0]; }
    return !keyframeCounter.empty();
}
}  // namespace ORB_SLAM2
