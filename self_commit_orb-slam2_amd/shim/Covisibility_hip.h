// shim/Covisibility_hip.h -- the counting of KeyFrame::UpdateConnections, LocalMapping::KeyFrameCulling and Tracking::UpdateLocalKeyFrames on the
// device (shim/Covisibility_hip.cc).
#ifndef ORBX_SHIM_COVISIBILITY_HIP_H
#define ORBX_SHIM_COVISIBILITY_HIP_H

#include <map>
#include <mutex>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "orbx.h"

namespace ORB_SLAM2
{
class KeyFrameDatabase_hip;

// One handle of orbx_covis_* behind the three loops.  The slice is gathered from the real KeyFrame / MapPoint objects (one visit per point under
// its mutexes, shim/MapPointAccess.h), the ranks are the ranks of the KeyFrame pointers, and everything the reference's bodies write is written
// back here.  A class of its own: the drop-in library keeps the reference's bodies.  On a device error (shim_error.h) nothing is changed.
class Covisibility_hip
{
public:
    // pKFDB (may be NULL): the device keyframe database whose covisibles are pushed again after every UpdateConnections
    explicit Covisibility_hip(KeyFrameDatabase_hip *pKFDB = 0);
    ~Covisibility_hip();

    // KeyFrame::UpdateConnections() of pKF / of every keyframe of the list in ONE call, written back in the list's order (src/KeyFrame.cc:386-507)
    void UpdateConnections(KeyFrame *pKF);
    void UpdateConnections(const std::vector<KeyFrame *> &vpKFs);
    // LocalMapping::KeyFrameCulling() for mpCurrentKeyFrame = pKF: SetBadFlag() on the culled keyframes, in order (src/LocalMapping.cc:873-956)
    void KeyFrameCulling(KeyFrame *pKF, bool bMonocular);
    // the vote that opens Tracking::UpdateLocalKeyFrames() (src/Tracking.cc:1897-1950): bad points of F are set to NULL, keyframeCounter holds every
    // observer (bad ones included, as there), pKFmax / nmax the best one that is not bad; false = an empty counter (the reference returns)
    bool UpdateLocalKeyFrames(Frame &F, std::map<KeyFrame *, int> &keyframeCounter, KeyFrame *&pKFmax, int &nmax);

private:
    orbx_covis *mpOps;
    KeyFrameDatabase_hip *mpKFDB;
    std::mutex mMutex;      // one call at a time on the handle
};
}  // namespace ORB_SLAM2

#endif
