// shim/LocalMapping_hip.h -- the body of LocalMapping::CreateNewMapPoints in one device call (shim/LocalMapping_hip.cc; INTEGRATION.md, "New map points").
#ifndef ORBX_SHIM_LOCAL_MAPPING_HIP_H
#define ORBX_SHIM_LOCAL_MAPPING_HIP_H

namespace ORB_SLAM2
{
class LocalMapping;
namespace orbx_shim
{
// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:312-625) of `lm` on its current keyframe: the baseline / median-depth gate and ComputeF12 per
// neighbour on the host, ONE orbx_create_new_map_points, then the reference's bookkeeping (:600-622) per created point in creation order.  Returns the
// number of points created (nnew); on a device error (counted, std::cerr: shim_error.h) nothing is created.
int CreateNewMapPoints(LocalMapping *lm);
}  // namespace orbx_shim
}  // namespace ORB_SLAM2

#endif
