// shim/GrabImage_hip.cc -- colour to grey and stereo rectification through orbx_image_prep_* (csrc/orbx_image.hip).
//
// Replaces, in a build with -DORBSLAM_HIP:
//   src/Tracking.cc:250-278, 311-326, 369-384   the cvtColor ladders                 -> mImGray = ToGray(im, mbRGB)
//   Examples/Stereo/stereo_euroc.cc:124-134     the two cv::initUndistortRectifyMap  -> StereoRectifier rectify(K_l, D_l, R_l, P_l, K_r, ..., cols_l, rows_l)
//   Examples/Stereo/stereo_euroc.cc:181-188     the two cv::remap per pair           -> rectify(imLeft, imRight, imLeftRect, imRightRect)
// The arithmetic is the project's pinned one (include/orbx.h); parity with the OpenCV build the reference is linked to is unpinned.
// Not part of the drop-in library: a file to add to the reference's build next to the lines above.  Host images in, host images out: a
// caller that keeps its frames on the device uses orbx_image_prep_batch_device in front of orbx_extract_batch_device instead.
#include "GrabImage_hip.h"

#include <vector>

#include "shim_error.h"

namespace ORB_SLAM2
{
namespace
{
orbx_image_prep *CreatePrep(int cols, int rows, const char *where)
{
    orbx_image_prep_config cfg;
    memset(&cfg, 0, sizeof(cfg));      // all-zero grey weights: OpenCV 4.x's
    cfg.device = orbx_shim::Device();
    cfg.max_width = cols;
    cfg.max_height = rows;
    cfg.max_batch = 1;
    orbx_image_prep *h = 0;
    if (orbx_image_prep_create(&cfg, &h) != ORBX_OK) { orbx_shim::Fail(where); return 0; }
    return h;
}

// a thread's own handle for ToGray, replaced by a larger one when a larger image arrives
struct GrayHandle {
    orbx_image_prep *h;
    int cols, rows;
    GrayHandle() : h(0), cols(0), rows(0) {}
    ~GrayHandle() { orbx_image_prep_destroy(h); }
    orbx_image_prep *For(int c, int r)
    {
        if (h && c <= cols && r <= rows) return h;
        orbx_image_prep_destroy(h);
        cols = c > cols ? c : cols;
        rows = r > rows ? r : rows;
        h = CreatePrep(cols, rows, "ToGray");
        if (!h) cols = rows = 0;
        return h;
    }
};

bool Run(orbx_image_prep *h, const cv::Mat &im, bool bRGB, int side, cv::Mat &out, const char *where)
{
    if (im.depth() != CV_8U || (im.channels() != 1 && im.channels() != 3 && im.channels() != 4)) return orbx_shim::Fail(where, "the image must be CV_8UC1, CV_8UC3 or CV_8UC4");
    out.create(im.rows, im.cols, CV_8UC1);
    const uint8_t *one[1] = {im.data};
    if (orbx_image_prep_run(h, one, 1, im.cols, im.rows, im.channels(), bRGB ? 1 : 0, (int)im.step, side, out.data, (int)out.step) != ORBX_OK) {
        out = cv::Mat();
        return orbx_shim::Fail(where);
    }
    return true;
}

bool Doubles(const cv::Mat &m, int count, std::vector<double> &v)
{
    if (m.empty() || m.channels() != 1) return false;
    cv::Mat d;
    m.convertTo(d, CV_64F);
    v.clear();
    for (int i = 0; i < d.rows; i++)
        for (int j = 0; j < d.cols; j++) v.push_back(d.at<double>(i, j));
    return count < 0 || (int)v.size() == count;
}
}  // namespace

cv::Mat ToGray(const cv::Mat &im, bool bRGB)
{
    if (im.empty() || im.channels() == 1) return im;
    static thread_local GrayHandle g;
    orbx_image_prep *h = g.For(im.cols, im.rows);
    cv::Mat out;
    if (!h || !Run(h, im, bRGB, -1, out, "ToGray")) return cv::Mat();
    return out;
}

StereoRectifier::StereoRectifier(const cv::Mat &K_l, const cv::Mat &D_l, const cv::Mat &R_l, const cv::Mat &P_l, const cv::Mat &K_r, const cv::Mat &D_r, const cv::Mat &R_r,
                                 const cv::Mat &P_r, int cols, int rows, bool bRGB)
    : mpPrep(0), mCols(cols), mRows(rows), mbRGB(bRGB)
{
    if (cols < 1 || rows < 1) { orbx_shim::Fail("StereoRectifier", "empty image size"); return; }
    orbx_image_prep *h = CreatePrep(cols, rows, "StereoRectifier");
    if (!h) return;
    const cv::Mat *Ks[2] = {&K_l, &K_r}, *Ds[2] = {&D_l, &D_r}, *Rs[2] = {&R_l, &R_r}, *Ps[2] = {&P_l, &P_r};
    std::vector<float> m1((size_t)cols * rows), m2((size_t)cols * rows);
    for (int side = 0; side < 2; side++) {
        std::vector<double> K, D, R, P;
        if (!Doubles(*Ks[side], 9, K) || !Doubles(*Rs[side], 9, R) || !Doubles(*Ds[side], -1, D) || (D.size() != 4 && D.size() != 5) || !Doubles(*Ps[side], -1, P) ||
            (P.size() != 9 && P.size() != 12)) {
            orbx_shim::Fail("StereoRectifier", "K and R must be 3 x 3, D 4 or 5 coefficients, P 3 x 3 or 3 x 4");
            orbx_image_prep_destroy(h);
            return;
        }
        const int pc = (int)P.size() / 3;
        const double Pnew[9] = {P[0], P[1], P[2], P[pc], P[pc + 1], P[pc + 2], P[2 * pc], P[2 * pc + 1], P[2 * pc + 2]};      // P.rowRange(0,3).colRange(0,3)
        if (orbx_rectify_maps(&K[0], &D[0], (int)D.size(), &R[0], Pnew, cols, rows, &m1[0], &m2[0]) != ORBX_OK ||
            orbx_image_prep_set_maps(h, side, &m1[0], &m2[0], cols, cols, rows) != ORBX_OK) {
            orbx_shim::Fail("StereoRectifier");
            orbx_image_prep_destroy(h);
            return;
        }
    }
    mpPrep = h;
}

StereoRectifier::~StereoRectifier() { orbx_image_prep_destroy(mpPrep); }

bool StereoRectifier::operator()(const cv::Mat &imLeft, const cv::Mat &imRight, cv::Mat &imLeftRect, cv::Mat &imRightRect)
{
    imLeftRect = cv::Mat();
    imRightRect = cv::Mat();
    if (!mpPrep) return orbx_shim::Fail("StereoRectifier", "not constructed");
    if (imLeft.cols != mCols || imLeft.rows != mRows || imRight.cols != mCols || imRight.rows != mRows) return orbx_shim::Fail("StereoRectifier", "the images do not have the size of the maps");
    std::lock_guard<std::mutex> lock(mMutex);
    cv::Mat l, r;
    if (!Run(mpPrep, imLeft, mbRGB, 0, l, "StereoRectifier") || !Run(mpPrep, imRight, mbRGB, 1, r, "StereoRectifier")) return false;
    imLeftRect = l;
    imRightRect = r;
    return true;
}
}  // namespace ORB_SLAM2
