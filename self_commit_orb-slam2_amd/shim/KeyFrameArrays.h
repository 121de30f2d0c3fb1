// shim/KeyFrameArrays.h -- a KeyFrame as the arrays SearchByBoW(pKF, F) and the pose problems behind it read: one gather, one visit per MapPoint.
//
// Shared by TrackReferenceKeyFrameHIP (shim/Tracking_hip.cc), RelocalizationMatchHIP (shim/Relocalization_hip.cc) and ComputeSim3Device
// (shim/ComputeSim3_hip.cc: with the points' distance range and descriptor kept from the same visit).
#ifndef ORBX_SHIM_KEYFRAME_ARRAYS_H
#define ORBX_SHIM_KEYFRAME_ARRAYS_H

#include <stdint.h>
#include <vector>

#include "KeyFrame.h"
#include "MapPointAccess.h"
#include "orbx.h"

namespace ORB_SLAM2
{
// DBoW2::FeatureVector (node id -> feature indices) as one node id per feature; -1 = not filed (never matched)
inline void FlatFeatureVector(const DBoW2::FeatureVector &fv, int N, std::vector<int32_t> &g)
{
    g.assign((size_t)(N > 0 ? N : 1), -1);
    for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it)
        for (size_t k = 0; k < it->second.size(); k++)
            if ((int)it->second[k] < N) g[it->second[k]] = (int32_t)it->first;
}

struct KeyFrameArrays {
    std::vector<MapPoint *> vpMPs;          // GetMapPointMatches()
    std::vector<int32_t> groups;            // mFeatVec, flat
    std::vector<uint8_t> valid, hasObs;     // pMP && !pMP->isBad() (src/ORBmatcher.cc:268-274); Observations() > 0
    std::vector<float> pos;                 // GetWorldPos() of the valid slots
    std::vector<float> maxD, minD;          // withPointData: mfMaxDistance / mfMinDistance of the valid slots
    std::vector<uint8_t> desc;              // withPointData: GetDescriptor() of the valid slots, 32 bytes each
    int n;
    orbx_feature_set set;
    // fills the arrays and `set` (which points into them and into pKF: both must outlive the call that reads it)
    void Gather(KeyFrame *pKF, bool withPointData = false)
    {
        vpMPs = pKF->GetMapPointMatches();
        n = (int)vpMPs.size();
        const size_t cap = (size_t)(n > 0 ? n : 1);
        FlatFeatureVector(pKF->mFeatVec, n, groups);
        valid.assign(cap, 0); hasObs.assign(cap, 0); pos.assign(cap * 3, 0.f);
        if (withPointData) { maxD.assign(cap, 0.f); minD.assign(cap, 0.f); desc.assign(cap * 32, 0); }
        for (int i = 0; i < n; i++) {
            MapPoint *pMP = vpMPs[(size_t)i];
            if (!pMP) continue;
            float nrm[3], mx, mn;
            unsigned char d[32];
            float &rmx = withPointData ? maxD[(size_t)i] : mx, &rmn = withPointData ? minD[(size_t)i] : mn;
            if (MapPointAccess::Snapshot(pMP, &pos[3 * (size_t)i], nrm, rmx, rmn, hasObs[(size_t)i], withPointData ? &desc[32 * (size_t)i] : d)) valid[(size_t)i] = 1;
        }
        const orbx_feature_set s = {n > 0 ? (const orbx_keypoint *)&pKF->mvKeysUn[0] : 0, n > 0 ? pKF->mDescriptors.data : 0, &n, &groups[0], &valid[0], (int)cap, 1};   // kp angle: :318
        set = s;
    }
};
}  // namespace ORB_SLAM2

#endif
