// shim/MapPoint_hip.h -- the batched MapPoint refresh of shim/MapPoint_hip.cc ("MapPoint refresh").
#ifndef ORBX_SHIM_MAP_POINT_HIP_H
#define ORBX_SHIM_MAP_POINT_HIP_H

#include <vector>

namespace ORB_SLAM2
{
class MapPoint;
namespace orbx_shim
{
// ComputeDistinctiveDescriptors (descriptor) and / or UpdateNormalAndDepth (normalAndDepth) of every point of `pts` that is neither NULL nor bad,
// in one device call.  On a device error (counted, std::cerr: shim_error.h) the points are left as they were.
void RefreshMapPoints(const std::vector<MapPoint *> &pts, bool descriptor, bool normalAndDepth);
}  // namespace orbx_shim
}  // namespace ORB_SLAM2

#endif
