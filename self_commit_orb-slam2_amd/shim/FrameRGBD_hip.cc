// shim/FrameRGBD_hip.cc -- HIP body for ORB_SLAM2::Frame::ComputeStereoFromRGBD.
//
// Compiled against the REFERENCE's own include/Frame.h with shim/ORBextractor.h in place of include/ORBextractor.h, like
// shim/Frame_hip.cc.  Replaces the body of
//     void Frame::ComputeStereoFromRGBD(const cv::Mat &imDepth)                src/Frame.cc:1423-1461
// (called from the RGB-D constructor, src/Frame.cc:302, after ExtractORB and UndistortKeyPoints).  The left extractor still holds this
// frame's keypoints - on the device and in its pinned result arena -, so the call is orbx_frame_rgbd_begin / _end on them: the depth values
// under the keypoints are looked up on the host, the kernel returns mvDepth / mvuRight (and the depth order, the camera-frame points and the
// close-point count, which Tracking can take from orbx_shim_rgbd_last instead of recomputing them).
// A file of its own: the drop-in library of oracle/Makefile does not link it ("RGB-D": one more objcopy -W line).
//
// imDepth is the CV_32F image the reference's Tracking::GrabImageRGBD passes (src/Tracking.cc:334-338).  A GrabImageRGBD that skips its
// whole-image convertTo may pass the raw CV_16U image after telling the shim mDepthMapFactor once (orbx_shim_rgbd_depth_factor): only the
// N looked-up pixels are converted, d = (float)raw * factor.
#include <cstring>
#include <mutex>
#include <vector>

#include "Frame.h"
#include "orbx.h"
#include "shim_error.h"

static float gDepthFactor = 1.0f;
extern "C" __attribute__((visibility("default"))) void orbx_shim_rgbd_depth_factor(float factor) { gDepthFactor = factor; }
static unsigned long gRgbdCalls = 0;
extern "C" __attribute__((visibility("default"))) unsigned long orbx_shim_compute_stereo_from_rgbd_calls(void) { return gRgbdCalls; }

namespace
{
// one device handle for the camera in use (mK, mDistCoef); frames are built by one thread at a time in the reference
std::mutex gMutex;
orbx_frame_ops *gOps = 0;
orbx_camera gCam;
orbx_rgbd_frame gLast;
int gLastN = 0;
long gLastId = -1;

orbx_frame_ops *OpsFor(const cv::Mat &K, const cv::Mat &D)
{
    orbx_camera cam;
    memset(&cam, 0, sizeof(cam));
    cam.fx = K.at<float>(0, 0); cam.fy = K.at<float>(1, 1); cam.cx = K.at<float>(0, 2); cam.cy = K.at<float>(1, 2);
    cam.ndist = D.rows * D.cols;
    if (cam.ndist != 4 && cam.ndist != 5) { orbx_shim::Fail("Frame::ComputeStereoFromRGBD", "mDistCoef must hold 4 or 5 coefficients"); return 0; }
    for (int i = 0; i < cam.ndist; i++) cam.dist[i] = D.at<float>(i);
    if (gOps && memcmp(&cam, &gCam, sizeof(cam)) == 0) return gOps;
    if (gOps) { orbx_frame_ops_destroy(gOps); gOps = 0; }
    if (orbx_frame_ops_create(orbx_shim::Device(), &cam, &gOps) != ORBX_OK) { gOps = 0; orbx_shim::Fail("Frame::ComputeStereoFromRGBD"); return 0; }
    gCam = cam;
    return gOps;
}
}  // namespace

// What Tracking derives from mvDepth on every RGB-D frame (UpdateLastFrame, CreateNewKeyFrame, NeedNewKeyFrame), for the frame with id
// `frameId` if it is the last one ComputeStereoFromRGBD ran on: views into the handle's pinned memory, valid until the next frame.
extern "C" __attribute__((visibility("default"))) int orbx_shim_rgbd_last(long frameId, orbx_rgbd_frame *out, int *n)
{
    std::lock_guard<std::mutex> lock(gMutex);
    if (gLastId < 0 || gLastId != frameId || !out) return -1;
    *out = gLast;
    if (n) *n = gLastN;
    return 0;
}

namespace ORB_SLAM2
{

void Frame::ComputeStereoFromRGBD(const cv::Mat &imDepth)
{
    __atomic_add_fetch(&gRgbdCalls, 1, __ATOMIC_RELAXED);
    mvuRight = std::vector<float>(N, -1);   // :1428-1429
    mvDepth = std::vector<float>(N, -1);
    std::lock_guard<std::mutex> lock(gMutex);
    gLastId = -1;
    if (N == 0) return;
    orbx_extractor *ext = mpORBextractorLeft ? mpORBextractorLeft->Handle() : 0;
    orbx_frame_ops *ops = OpsFor(mK, mDistCoef);
    if (!ext || !ops) { if (!ext) orbx_shim::Fail("Frame::ComputeStereoFromRGBD", "no extractor handle"); return; }
    orbx_depth_desc dd;
    dd.data = imDepth.data; dd.cols = imDepth.cols; dd.rows = imDepth.rows; dd.stride_bytes = (int)imDepth.step; dd.factor = gDepthFactor;
    if (imDepth.type() == CV_32F) dd.format = ORBX_DEPTH_F32;
    else if (imDepth.type() == CV_16U) dd.format = ORBX_DEPTH_U16;
    else { orbx_shim::Fail("Frame::ComputeStereoFromRGBD", "imDepth must be CV_32F or CV_16U"); return; }
    const orbx_rgbd_params prm = {mbf, mThDepth};
    orbx_rgbd_frame r;
    int n = 0;
    // (no grid here: the constructor assigns features to the grid after this call, src/Frame.cc:347; mvKeysUn is already filled)
    if (orbx_frame_rgbd_begin(ops, ext, 0, &dd, &prm) != ORBX_OK || orbx_frame_rgbd_end(ops, 0, 0, 0, &n, &r) != ORBX_OK) {
        orbx_shim::Fail("Frame::ComputeStereoFromRGBD");      // no depth: mvuRight / mvDepth stay -1
        return;
    }
    if (n != N) { orbx_shim::Fail("Frame::ComputeStereoFromRGBD", "the extractor's last call is not this frame's"); return; }
    memcpy(&mvDepth[0], r.depth, (size_t)N * sizeof(float));
    memcpy(&mvuRight[0], r.u_right, (size_t)N * sizeof(float));
    gLast = r; gLastN = N; gLastId = (long)mnId;
}

}  // namespace ORB_SLAM2
