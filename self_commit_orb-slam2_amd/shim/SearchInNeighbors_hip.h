// shim/SearchInNeighbors_hip.h -- steps 2 and 3 of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:666-713) as ONE device call
// (shim/SearchInNeighbors_hip.cc).
#ifndef ORBX_SHIM_SEARCH_IN_NEIGHBORS_HIP_H
#define ORBX_SHIM_SEARCH_IN_NEIGHBORS_HIP_H

#include <mutex>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbx.h"

namespace ORB_SLAM2
{
// One matcher handle behind the T + 1 ORBmatcher::Fuse calls.  The slice is gathered from the real KeyFrame / MapPoint objects (one visit per point
// under its mutexes), the ranks are the ranks of the KeyFrame pointers, and the decisions the device took are replayed in their order through the
// reference's own Replace / AddObservation / AddMapPoint: the map ends as the reference's loop leaves it.  Steps 1, 4 and 5 stay with the caller.
// A class of its own: the drop-in library keeps the reference's body.  On a device error (shim_error.h) nothing is changed.
class SearchInNeighbors_hip
{
public:
    SearchInNeighbors_hip();
    ~SearchInNeighbors_hip();
    // vpTargetKFs as LocalMapping::SearchInNeighbors builds it (:640-664; a keyframe may repeat).  Returns the decisions replayed, -1 on an error;
    // pnFused (may be NULL) receives the T + 1 return values of ORBmatcher::Fuse.
    int Fuse(KeyFrame *pCurrentKF, const std::vector<KeyFrame *> &vpTargetKFs, std::vector<int> *pnFused = 0);

private:
    orbx_matcher *mpMatcher;
    std::mutex mMutex;      // one call at a time on the handle
};
}  // namespace ORB_SLAM2

#endif
