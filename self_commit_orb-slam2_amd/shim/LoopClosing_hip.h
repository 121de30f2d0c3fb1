// shim/LoopClosing_hip.h -- the two passes of the loop closer that move the map, on the device (shim/LoopClosing_hip.cc).
#ifndef ORBX_SHIM_LOOP_CLOSING_HIP_H
#define ORBX_SHIM_LOOP_CLOSING_HIP_H

#include <mutex>
#include <vector>

#include "KeyFrame.h"
#include "LoopClosing.h"
#include "Map.h"
#include "orbx.h"

namespace ORB_SLAM2
{
// One handle of orbx_loop_* behind LoopClosing::CorrectLoop's Sim3 propagation (src/LoopClosing.cc:617-716) and the map update that ends
// RunGlobalBundleAdjustment (:930-1003).  Everything is gathered from the real KeyFrame / MapPoint objects (one visit per point under its
// mutexes, shim/MapPointAccess.h) and everything the reference's loops write is written back here.  The caller holds mpMap->mMutexMapUpdate, as the
// reference does around both loops, and keeps the bookkeeping: UpdateConnections of the group, Replace / AddObservation, LoopConnections.
// A class of its own: the drop-in library keeps the reference's bodies.  On a device error (shim_error.h) nothing is changed and false comes back.
class LoopCorrection_hip
{
public:
    LoopCorrection_hip();
    ~LoopCorrection_hip();

    // :620-711 for mpCurrentKF = pCurrentKF, mvpCurrentConnectedKFs (the current keyframe included) and mg2oScw: fills CorrectedSim3 and
    // NonCorrectedSim3, moves every map point of the group once (SetWorldPos, mnCorrectedByKF, mnCorrectedReference, the normal and the distance
    // range of UpdateNormalAndDepth) and gives every keyframe of the group its corrected pose (SetPose).  UpdateConnections (:715) is the caller's.
    bool CorrectLoopPropagate(KeyFrame *pCurrentKF, const std::vector<KeyFrame *> &vpCurrentConnectedKFs, const g2o::Sim3 &g2oScw,
                              LoopClosing::KeyFrameAndPose &CorrectedSim3, LoopClosing::KeyFrameAndPose &NonCorrectedSim3);
    // :930-1003: mTcwGBA / mnBAGlobalForKF of the keyframes the BA did not see, mTcwBefGBA and SetPose of every keyframe the walk reaches,
    // SetWorldPos of every map point
    bool PropagateGBA(Map *pMap, unsigned long nLoopKF);

private:
    orbx_loop *mpOps;
    std::mutex mMutex;      // one call at a time on the handle
};
}  // namespace ORB_SLAM2

#endif
