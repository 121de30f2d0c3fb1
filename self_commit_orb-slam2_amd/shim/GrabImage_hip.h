// shim/GrabImage_hip.h -- what happens to a camera image in front of ORBextractor::operator(), on the device (shim/GrabImage_hip.cc).
#ifndef ORBX_SHIM_GRAB_IMAGE_HIP_H
#define ORBX_SHIM_GRAB_IMAGE_HIP_H

#include <mutex>

#include <opencv2/core/core.hpp>

#include "orbx.h"

namespace ORB_SLAM2
{
// The three cvtColor ladders of Tracking::GrabImageMonocular / GrabImageStereo / GrabImageRGBD (src/Tracking.cc:250-278, 311-326, 369-384):
// a CV_8UC3 / CV_8UC4 image comes back as a new CV_8UC1 image (RGB2GRAY / RGBA2GRAY with bRGB, BGR2GRAY / BGRA2GRAY without), a one-channel
// image is returned as it is (no copy).  One handle per calling thread, grown to the largest image seen.  On a device error (shim_error.h)
// an empty cv::Mat comes back: the Frame constructors extract nothing from it.
cv::Mat ToGray(const cv::Mat &im, bool bRGB);

// Examples/Stereo/stereo_euroc.cc:124-134 (the two cv::initUndistortRectifyMap calls, here orbx_rectify_maps) and :181-188 (the two cv::remap
// calls per pair).  P is the 3 x 4 (or 3 x 3) projection matrix of the settings file: its left 3 x 3 block is used, as rowRange(0,3).colRange(0,3)
// there.  Colour input is converted to grey FIRST and the grey image is rectified (bRGB as Camera.RGB); the outputs are CV_8UC1.
class StereoRectifier
{
public:
    StereoRectifier(const cv::Mat &K_l, const cv::Mat &D_l, const cv::Mat &R_l, const cv::Mat &P_l, const cv::Mat &K_r, const cv::Mat &D_r, const cv::Mat &R_r,
                    const cv::Mat &P_r, int cols, int rows, bool bRGB = true);
    ~StereoRectifier();
    bool ok() const { return mpPrep != 0; }      // false: a matrix of the wrong shape or a device error (reported through shim_error.h)

    // imLeftRect / imRightRect = cv::remap(imLeft / imRight, M1, M2, cv::INTER_LINEAR); false (and empty outputs) on a device error or a size other than cols x rows
    bool operator()(const cv::Mat &imLeft, const cv::Mat &imRight, cv::Mat &imLeftRect, cv::Mat &imRightRect);

private:
    StereoRectifier(const StereoRectifier &);
    StereoRectifier &operator=(const StereoRectifier &);
    orbx_image_prep *mpPrep;
    int mCols, mRows;
    bool mbRGB;
    std::mutex mMutex;      // one call at a time on the handle
};
}  // namespace ORB_SLAM2

#endif
