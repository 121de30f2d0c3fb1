// shim/EssentialGraph_hip.h -- Optimizer::OptimizeEssentialGraph on the device (shim/EssentialGraph_hip.cc).
#ifndef ORBX_SHIM_ESSENTIALGRAPH_HIP_H
#define ORBX_SHIM_ESSENTIALGRAPH_HIP_H

#include <map>
#include <set>

#include "KeyFrame.h"
#include "LoopClosing.h"
#include "Map.h"

namespace ORB_SLAM2
{
// Optimizer::OptimizeEssentialGraph's signature and effects (src/Optimizer.cc:1017-1339): every keyframe's pose is set to the optimised
// [R | t / s], every map point is moved with its reference keyframe.  A free function: the drop-in library keeps the reference's
// Optimizer::OptimizeEssentialGraph, and a build that wants this one forwards to it.  On a device error (shim_error.h) nothing is touched.
void OptimizeEssentialGraph_hip(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                const LoopClosing::KeyFrameAndPose &CorrectedSim3, const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections,
                                const bool &bFixScale);
}  // namespace ORB_SLAM2

// orbx_optimize_essential_graph calls served so far (every thread)
extern "C" unsigned long orbx_shim_essential_graph_calls(void);

#endif
