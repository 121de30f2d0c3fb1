// shim/SearchInNeighbors_hip.cc -- steps 2 and 3 of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:666-713) over orbx_search_in_neighbors.
//
// Compiled against the REFERENCE's own headers, like the other shim files.  A file of its own: the drop-in library of oracle/Makefile does not
// link it; it is compile-checked only.
//
// The gather.  Slot 0 is the current keyframe, the targets follow (each once, however often vpTargetKFs names it), then every other keyframe that
// observes a point as it is met; the ranks are the ranks of the KeyFrame POINTERS (std::map<KeyFrame*, size_t> orders by them).  The points are the
// mvpMapPoints of the current keyframe and of the targets; every point is visited ONCE under its two mutexes (features, then position): isBad, the
// observers in the map's order, position, normal, the distance range, the descriptor, mnVisible and mnFound.  An observer's descriptor, octave and
// mvuRight are const members of its keyframe and need no lock.
// The write-back.  The device's decisions come back as a log in execution order; each is replayed through the reference's own functions on the real
// objects - AddObservation + AddMapPoint, pMP->Replace(pMPinKF) or pMPinKF->Replace(pMP) - so Replace's bookkeeping (mpReplaced, IncreaseFound /
// IncreaseVisible, ComputeDistinctiveDescriptors, Map::EraseMapPoint) is the reference's.  mnFuseCandidateForKF is set on the candidates as :708 does.
// PARITY UNPINNED: the device sees the map as gathered; another thread may change a point between the gather and the replay (the reference's loop
// reads every point as of its own visit).  The local mapper holds no map-wide lock here either.
#include <map>
#include <mutex>
#include <string.h>
#include <utility>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbx.h"
#include "shim_error.h"
#include "SearchInNeighbors_hip.h"

namespace ORB_SLAM2
{
namespace
{
struct MapPointFuseAccess : public MapPoint {
    // everything the chain reads of a point, in one visit; -> isBad
    static bool Snapshot(MapPoint *p, std::vector<std::pair<KeyFrame *, size_t> > &obs, float pos[3], float nrm[3], float &rawMax, float &rawMin, unsigned char desc[32],
                         int &visible, int &found)
    {
        MapPointFuseAccess *q = static_cast<MapPointFuseAccess *>(p);
        obs.clear();
        std::unique_lock<std::mutex> lock(q->mMutexFeatures);
        std::unique_lock<std::mutex> lock2(q->mMutexPos);
        for (std::map<KeyFrame *, size_t>::const_iterator it = q->mObservations.begin(); it != q->mObservations.end(); ++it) obs.push_back(*it);
        for (int c = 0; c < 3; c++) { pos[c] = q->mWorldPos.at<float>(c); nrm[c] = q->mNormalVector.empty() ? 0.f : q->mNormalVector.at<float>(c); }
        rawMax = q->mfMaxDistance; rawMin = q->mfMinDistance;
        if (q->mDescriptor.data) memcpy(desc, q->mDescriptor.data, 32); else memset(desc, 0, 32);
        visible = q->mnVisible; found = q->mnFound;
        return q->mbBad;
    }
};

struct Slice {
    std::vector<KeyFrame *> kfs;                  // slot -> keyframe
    std::map<KeyFrame *, int> slotOf;
    std::vector<MapPoint *> pts;                  // point id -> point
    std::map<MapPoint *, int> pointOf;
    std::vector<float> pos, nrm, minD, maxD, rawMax;
    std::vector<uint8_t> desc, bad, obsStereo, obsDesc, kfBad;
    std::vector<int32_t> visible, found, obsOff, obsKf, obsIdx, rank;
    std::vector<std::pair<KeyFrame *, size_t> > obs;      // reused

    Slice() { obsOff.push_back(0); }
    int Slot(KeyFrame *kf)
    {
        std::map<KeyFrame *, int>::iterator it = slotOf.find(kf);
        if (it != slotOf.end()) return it->second;
        const int s = (int)kfs.size();
        slotOf[kf] = s;
        kfs.push_back(kf);
        return s;
    }
    int Point(MapPoint *pMP)
    {
        std::map<MapPoint *, int>::iterator it = pointOf.find(pMP);
        if (it != pointOf.end()) return it->second;
        const int p = (int)pts.size();
        pointOf[pMP] = p;
        pts.push_back(pMP);
        float x[3], n[3], rmax, rmin;
        unsigned char d[32];
        int vis, fnd;
        bad.push_back(MapPointFuseAccess::Snapshot(pMP, obs, x, n, rmax, rmin, d, vis, fnd) ? 1 : 0);
        for (int c = 0; c < 3; c++) { pos.push_back(x[c]); nrm.push_back(n[c]); }
        rawMax.push_back(rmax); maxD.push_back(1.2f * rmax); minD.push_back(0.8f * rmin);      // the getters' values (src/MapPoint.cc:523-533)
        desc.insert(desc.end(), d, d + 32);
        visible.push_back(vis); found.push_back(fnd);
        for (size_t i = 0; i < obs.size(); i++) {      // the map's order: ascending pointer = ascending rank
            KeyFrame *pKFi = obs[i].first;
            obsKf.push_back(Slot(pKFi));
            obsIdx.push_back((int32_t)obs[i].second);
            obsStereo.push_back(pKFi->mvuRight[obs[i].second] >= 0 ? 1 : 0);
            const unsigned char *row = pKFi->mDescriptors.ptr<unsigned char>((int)obs[i].second);
            obsDesc.insert(obsDesc.end(), row, row + 32);
        }
        obsOff.push_back((int32_t)obsKf.size());
        return p;
    }
};
}  // namespace

SearchInNeighbors_hip::SearchInNeighbors_hip() : mpMatcher(0)
{
    if (orbx_matcher_create(orbx_shim::Device(), 4096, 1, &mpMatcher) != ORBX_OK) {
        mpMatcher = 0;
        orbx_shim::Fail("SearchInNeighbors");
    }
}

SearchInNeighbors_hip::~SearchInNeighbors_hip()
{
    if (mpMatcher) orbx_matcher_destroy(mpMatcher);
}

int SearchInNeighbors_hip::Fuse(KeyFrame *pCurrentKF, const std::vector<KeyFrame *> &vpTargetKFs, std::vector<int> *pnFused)
{
    if (!mpMatcher || !pCurrentKF) return -1;
    std::unique_lock<std::mutex> lockCall(mMutex);
    Slice sl;
    sl.Slot(pCurrentKF);
    std::vector<int32_t> targets;
    for (size_t t = 0; t < vpTargetKFs.size(); t++) targets.push_back(sl.Slot(vpTargetKFs[t]));
    const size_t S = sl.kfs.size();      // the searchable keyframes: slots 0 .. S-1
    std::vector<std::vector<int32_t> > kfPoint(S);
    std::vector<cv::Mat> Tcw(S), Ow(S);
    for (size_t s = 0; s < S; s++) {
        const std::vector<MapPoint *> vpMP = sl.kfs[s]->GetMapPointMatches();
        kfPoint[s].resize(vpMP.size());
        for (size_t i = 0; i < vpMP.size(); i++) kfPoint[s][i] = vpMP[i] ? sl.Point(vpMP[i]) : -1;
        Tcw[s] = sl.kfs[s]->GetPose();
        Ow[s] = sl.kfs[s]->GetCameraCenter();
    }
    // (a point met through two keyframes was snapshot at its first visit; kf_point and the observations of a searchable keyframe agree unless another
    //  thread changed the point in between: the call then refuses the slice and nothing is changed)
    std::vector<orbx_fuse_keyframe> tab(S);
    for (size_t s = 0; s < S; s++) {
        KeyFrame *kf = sl.kfs[s];
        orbx_fuse_keyframe &K = tab[s];
        memset(&K, 0, sizeof(K));
        K.slot = (int)s; K.num_features = kf->N;
        K.keys_un = kf->N ? (const orbx_keypoint *)&kf->mvKeysUn[0] : 0;
        K.descriptors = kf->mDescriptors.data;
        K.u_right = kf->N ? &kf->mvuRight[0] : 0;
        K.kf_point = kfPoint[s].empty() ? 0 : &kfPoint[s][0];
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 4; c++) K.tcw[4 * r + c] = Tcw[s].at<float>(r, c);
            K.ow[r] = Ow[s].at<float>(r);
        }
        K.fx = kf->fx; K.fy = kf->fy; K.cx = kf->cx; K.cy = kf->cy; K.mbf = kf->mbf;
        K.grid_min_x = Frame::mnMinX; K.grid_min_y = Frame::mnMinY;      // what filed mGrid
        K.grid_width_inv = kf->mfGridElementWidthInv; K.grid_height_inv = kf->mfGridElementHeightInv;
        K.min_x = kf->mnMinX; K.max_x = kf->mnMaxX; K.min_y = kf->mnMinY; K.max_y = kf->mnMaxY;
        K.scale_factors = &kf->mvScaleFactors[0]; K.inv_level_sigma2 = &kf->mvInvLevelSigma2[0];
        K.log_scale_factor = kf->mfLogScaleFactor; K.nlevels = kf->mnScaleLevels;
    }
    sl.rank.resize(sl.kfs.size());
    sl.kfBad.resize(sl.kfs.size());
    int r = 0;
    for (std::map<KeyFrame *, int>::const_iterator it = sl.slotOf.begin(); it != sl.slotOf.end(); ++it) sl.rank[(size_t)it->second] = r++;      // pointer order
    for (size_t s = 0; s < sl.kfs.size(); s++) sl.kfBad[s] = sl.kfs[s]->isBad() ? 1 : 0;
    orbx_fuse_slice F;
    memset(&F, 0, sizeof(F));
    F.num_keyframes = (int)sl.kfs.size(); F.kf_rank = &sl.rank[0]; F.kf_bad = &sl.kfBad[0];
    F.num_searchable = (int)S; F.searchable = &tab[0];
    F.num_points = (int)sl.pts.size(); F.num_obs = (int)sl.obsKf.size();
    F.pos = sl.pos.data(); F.normal = sl.nrm.data(); F.min_distance = sl.minD.data(); F.max_distance = sl.maxD.data(); F.raw_max_distance = sl.rawMax.data();
    F.descriptors = sl.desc.data(); F.point_bad = sl.bad.data(); F.visible = sl.visible.data(); F.found = sl.found.data();
    F.obs_offset = sl.obsOff.data(); F.obs_kf = sl.obsKf.data(); F.obs_idx = sl.obsIdx.data(); F.obs_stereo = sl.obsStereo.data(); F.obs_descriptors = sl.obsDesc.data();
    F.th = 3.0f;

    const size_t T = targets.size();
    size_t worst = sl.pts.size();
    for (size_t t = 0; t < T; t++) worst += kfPoint[0].size();
    std::vector<orbx_fuse_decision> log(worst ? worst : 1);
    std::vector<int32_t> nFused(T + 1, 0), cand(sl.pts.size() ? sl.pts.size() : 1);
    int32_t nLog = 0, nCand = 0;
    orbx_fuse_result R;
    memset(&R, 0, sizeof(R));
    R.log = &log[0]; R.log_capacity = (int)worst; R.log_count = &nLog;
    R.nfused = &nFused[0];
    R.candidates = &cand[0]; R.candidates_capacity = (int)sl.pts.size(); R.candidates_count = &nCand;
    if (orbx_search_in_neighbors(mpMatcher, &F, 0, T ? &targets[0] : 0, (int)T, &R) != ORBX_OK) { orbx_shim::Fail("SearchInNeighbors"); return -1; }

    // the replay, in execution order, through the reference's own functions
    for (int c = 0; c < nCand; c++) sl.pts[(size_t)cand[(size_t)c]]->mnFuseCandidateForKF = pCurrentKF->mnId;      // :708
    for (int i = 0; i < nLog; i++) {
        const orbx_fuse_decision &d = log[(size_t)i];
        KeyFrame *pKF = d.call < (int)T ? vpTargetKFs[(size_t)d.call] : pCurrentKF;
        MapPoint *pMP = sl.pts[(size_t)d.point];
        if (d.kind == ORBX_FUSE_ADDED) {
            pMP->AddObservation(pKF, (size_t)d.feature);
            pKF->AddMapPoint(pMP, (size_t)d.feature);
        } else if (d.kind == ORBX_FUSE_REPLACED_BY_HOLDER) pMP->Replace(sl.pts[(size_t)d.other]);
        else if (d.kind == ORBX_FUSE_REPLACED_HOLDER) sl.pts[(size_t)d.other]->Replace(pMP);
    }
    if (pnFused) pnFused->assign(nFused.begin(), nFused.end());
    return nLog;
}
}  // namespace ORB_SLAM2
