// shim/OptimizeSim3_hip.h -- Optimizer::OptimizeSim3 on the device (shim/OptimizeSim3_hip.cc).
#ifndef ORBX_SHIM_OPTIMIZESIM3_HIP_H
#define ORBX_SHIM_OPTIMIZESIM3_HIP_H

#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"

namespace ORB_SLAM2
{
// Optimizer::OptimizeSim3's signature and effects (src/Optimizer.cc:1364-1590): the return value is nIn, the removed pairs are nulled in
// vpMatches1, g2oS12 is written on success and left alone on a return 0.  A free function: the drop-in library keeps the reference's
// Optimizer::OptimizeSim3, and a build that wants this one forwards to it.
int OptimizeSim3_hip(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2, const bool bFixScale);
}  // namespace ORB_SLAM2

namespace orbx_shim
{
struct Sim3Refinement {              // one (candidate, matches, Sim3) triple of LoopClosing::ComputeSim3
    ORB_SLAM2::KeyFrame *pKF1, *pKF2;
    std::vector<ORB_SLAM2::MapPoint *> *vpMatches1;
    g2o::Sim3 *g2oS12;
    int nInliers;                    // out: what OptimizeSim3 returns
};
// Every triple of the list in ONE device call.  false on a device error (shim_error.h): every nInliers is then 0 and nothing else is touched.
bool OptimizeSim3All(std::vector<Sim3Refinement> &items, float th2, bool bFixScale);
}  // namespace orbx_shim

// orbx_optimize_sim3 calls served so far / problems they served (every thread)
extern "C" unsigned long orbx_shim_optsim3_calls(void);
extern "C" unsigned long orbx_shim_optsim3_problems(void);

#endif
