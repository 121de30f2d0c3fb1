// shim/Initializer_hip.cc -- a body for Initializer::Initialize (src/Initializer.cc:68-230) with everything behind the random draws on the device.
//
// Compiled against the REFERENCE's own include/Initializer.h, like the other shim files: this file defines the member function itself, so the
// private members are its own.  A file of its own: the drop-in library of oracle/Makefile does not link it; it is compile-checked only.
//
// What stays on the host: mvKeys2 / mvMatches12 / mvbMatched1 (:82-109) and the RANSAC sets, drawn with DUtils::Random::RandomInt exactly as
// :139-168 draws them (the generator's state is the process's).  ONE orbx_initialize then runs FindHomography, FindFundamental, the choice on RH,
// the twelve motion hypotheses, CheckRT and the selection.  On a device error (counted, std::cerr: shim_error.h) the body returns false with
// R21 / t21 empty, the reference's "no initialisation yet".
#include <vector>

#include "Initializer.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "orbx.h"
#include "shim_error.h"
#include "Initializer_hip.h"

static unsigned long gInitializeCalls = 0;
extern "C" __attribute__((visibility("default"))) unsigned long orbx_shim_initialize_calls(void) { return gInitializeCalls; }

namespace ORB_SLAM2
{
namespace
{
struct ThreadInitializer {
    orbx_initializer *h;
    int matches, iterations;
    ThreadInitializer() : h(0), matches(0), iterations(0) {}
    ~ThreadInitializer() { if (h) orbx_initializer_destroy(h); }
};
thread_local ThreadInitializer tInit;
}  // namespace

bool Initializer::Initialize(const Frame &CurrentFrame, const vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21, vector<cv::Point3f> &vP3D, vector<bool> &vbTriangulated)
{
    __sync_fetch_and_add(&gInitializeCalls, 1ul);
    // :82-109
    mvKeys2 = CurrentFrame.mvKeysUn;
    mvMatches12.clear();
    mvMatches12.reserve(mvKeys2.size());
    mvbMatched1.resize(mvKeys1.size());
    for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
        if (vMatches12[i] >= 0) {
            mvMatches12.push_back(make_pair(i, vMatches12[i]));
            mvbMatched1[i] = true;
        } else
            mvbMatched1[i] = false;
    }
    const int N = mvMatches12.size();
    R21 = cv::Mat();
    t21 = cv::Mat();
    if (N < 8 || mMaxIterations < 1 || mvKeys1.empty() || mvKeys2.empty()) return false;      // (the reference's RandomInt(0, -1) has no answer either)

    // :111-168, the same draws in the same order
    vector<size_t> vAllIndices;
    vAllIndices.reserve(N);
    vector<size_t> vAvailableIndices;
    for (int i = 0; i < N; i++) vAllIndices.push_back(i);
    mvSets = vector<vector<size_t> >(mMaxIterations, vector<size_t>(8, 0));
    DUtils::Random::SeedRandOnce(0);
    std::vector<int32_t> sets((size_t)mMaxIterations * 8);
    for (int it = 0; it < mMaxIterations; it++) {
        vAvailableIndices = vAllIndices;
        for (size_t j = 0; j < 8; j++) {
            int randi = DUtils::Random::RandomInt(0, vAvailableIndices.size() - 1);
            int idx = vAvailableIndices[randi];
            mvSets[it][j] = idx;
            sets[(size_t)it * 8 + j] = idx;
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }

    ThreadInitializer &T = tInit;
    if (!T.h || T.matches < N || T.iterations < mMaxIterations) {
        if (T.h) orbx_initializer_destroy(T.h);
        T.h = 0;
        int cap = 2048;
        while (cap < N) cap *= 2;
        if (cap > ORBX_INIT_MAX_MATCHES) cap = ORBX_INIT_MAX_MATCHES;
        if (orbx_initializer_create(orbx_shim::Device(), cap, mMaxIterations, &T.h) != ORBX_OK) { T.h = 0; orbx_shim::Fail("Initializer::Initialize"); return false; }
        T.matches = cap; T.iterations = mMaxIterations;
    }
    const size_t n1 = mvKeys1.size(), n2 = mvKeys2.size();
    std::vector<float> k1(2 * n1), k2(2 * n2);
    for (size_t i = 0; i < n1; i++) { k1[2 * i] = mvKeys1[i].pt.x; k1[2 * i + 1] = mvKeys1[i].pt.y; }
    for (size_t i = 0; i < n2; i++) { k2[2 * i] = mvKeys2[i].pt.x; k2[2 * i + 1] = mvKeys2[i].pt.y; }
    std::vector<int32_t> m12(n1, -1);
    for (size_t i = 0; i < vMatches12.size() && i < n1; i++) m12[i] = vMatches12[i];
    orbx_init_problem P;
    memset(&P, 0, sizeof(P));
    P.keys1_xy = &k1[0]; P.keys2_xy = &k2[0]; P.n1 = (int)n1; P.n2 = (int)n2; P.matches12 = &m12[0];
    P.sets = &sets[0]; P.iterations = mMaxIterations; P.sigma = mSigma;
    P.fx = mK.at<float>(0, 0); P.fy = mK.at<float>(1, 1); P.cx = mK.at<float>(0, 2); P.cy = mK.at<float>(1, 2);
    P.min_parallax = 1.0f; P.min_triangulated = 50;      // :221, :226
    int32_t success = 0;
    float r[9], t[3];
    std::vector<float> p3d(3 * n1);
    std::vector<uint8_t> tri(n1);
    orbx_init_result Rs;
    memset(&Rs, 0, sizeof(Rs));
    Rs.success = &success; Rs.r21 = r; Rs.t21 = t; Rs.p3d = &p3d[0]; Rs.triangulated = &tri[0];
    if (orbx_initialize(T.h, &P, &Rs) != ORBX_OK) { orbx_shim::Fail("Initializer::Initialize"); return false; }
    if (!success) return false;
    R21 = cv::Mat(3, 3, CV_32F);
    t21 = cv::Mat(3, 1, CV_32F);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R21.at<float>(i, j) = r[3 * i + j];
        t21.at<float>(i) = t[i];
    }
    vP3D.resize(n1);
    vbTriangulated.assign(n1, false);
    for (size_t i = 0; i < n1; i++) {
        vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
        vbTriangulated[i] = tri[i] != 0;
    }
    return true;
}
}  // namespace ORB_SLAM2
