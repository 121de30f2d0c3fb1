// shim/OptimizeSim3_hip.cc -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1364-1590) with both optimize() rounds on the device.
//
// Compiled against the REFERENCE's own headers, like the other shim files.  A file of its own: the drop-in library of oracle/Makefile does not
// link it; it is compile-checked only.
//
// What stays on the host is the reference's pointer walk (:1429-1520): pairs whose vpMatches1 entry is null are skipped, and so are pairs with a
// missing or bad map point or GetIndexInKeyFrame < 0; for the kept pairs the two world positions, mvKeysUn[i].pt / mvKeysUn[i2].pt and
// mvInvLevelSigma2[octave] are gathered.  ONE orbx_optimize_sim3 then runs the camera points, both rounds and both chi2 tests of every triple
// handed to orbx_shim::OptimizeSim3All.  The effects are the reference's: removed pairs are nulled in vpMatches1 (those of the first test also
// on a return 0), g2oS12 is written on success and stays as passed in on a return 0.
// The C ABI takes the estimate as a rotation matrix: g2oS12's quaternion goes through toRotationMatrix() and Quaterniond(R) on its way in (the
// same quaternion up to rounding for the unit quaternion LoopClosing::ComputeSim3 passes).
// On a device error (counted, std::cerr: shim_error.h) the function returns 0 and touches nothing: the candidate is discarded.
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Converter.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
#include "orbx.h"
#include "shim_error.h"
#include "OptimizeSim3_hip.h"

static unsigned long gOptSim3Calls = 0, gOptSim3Problems = 0;
extern "C" __attribute__((visibility("default"))) unsigned long orbx_shim_optsim3_calls(void) { return gOptSim3Calls; }
extern "C" __attribute__((visibility("default"))) unsigned long orbx_shim_optsim3_problems(void) { return gOptSim3Problems; }

namespace
{
struct ThreadOptimizer {
    orbx_sim3_optimizer *h;
    int problems, pairs;
    ThreadOptimizer() : h(0), problems(0), pairs(0) {}
    ~ThreadOptimizer() { if (h) orbx_sim3_optimizer_destroy(h); }
};
thread_local ThreadOptimizer tOptimizer;

struct Gathered {
    std::vector<size_t> vnIndexEdge;                         // slot of vpMatches1 per kept pair
    std::vector<float> world1, world2, obs1, obs2, inv1, inv2;
    std::vector<uint8_t> removedFirst, removedFinal;
    int32_t nInliers, nBad;
    double quat[4], t[3], s;
    Gathered() : nInliers(0), nBad(0), s(1.0) {}
};
}  // namespace

namespace orbx_shim
{
bool OptimizeSim3All(std::vector<Sim3Refinement> &items, float th2, bool bFixScale)
{
    using namespace ORB_SLAM2;
    const int C = (int)items.size();
    for (int c = 0; c < C; c++) items[c].nInliers = 0;
    if (!C) return true;
    std::vector<Gathered> G(C);
    std::vector<orbx_sim3_opt_problem> probs(C);
    std::vector<orbx_sim3_opt_result> results(C);
    int maxN = 1;
    for (int c = 0; c < C; c++) {
        Sim3Refinement &I = items[c];
        KeyFrame *pKF1 = I.pKF1, *pKF2 = I.pKF2;
        std::vector<MapPoint *> &vpMatches1 = *I.vpMatches1;
        Gathered &g = G[c];
        orbx_sim3_opt_problem &P = probs[c];
        memset(&P, 0, sizeof(P));
        const cv::Mat &K1 = pKF1->mK;
        const cv::Mat &K2 = pKF2->mK;
        const cv::Mat R1w = pKF1->GetRotation();
        const cv::Mat t1w = pKF1->GetTranslation();
        const cv::Mat R2w = pKF2->GetRotation();
        const cv::Mat t2w = pKF2->GetTranslation();
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) { P.rcw1[3 * i + j] = R1w.at<float>(i, j); P.rcw2[3 * i + j] = R2w.at<float>(i, j); }
            P.tcw1[i] = t1w.at<float>(i); P.tcw2[i] = t2w.at<float>(i);
        }
        P.fx1 = K1.at<float>(0, 0); P.fy1 = K1.at<float>(1, 1); P.cx1 = K1.at<float>(0, 2); P.cy1 = K1.at<float>(1, 2);
        P.fx2 = K2.at<float>(0, 0); P.fy2 = K2.at<float>(1, 1); P.cx2 = K2.at<float>(0, 2); P.cy2 = K2.at<float>(1, 2);
        // :1411-1520
        const int N = vpMatches1.size();
        const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches();
        for (int i = 0; i < N; i++) {
            if (!vpMatches1[i]) continue;
            MapPoint *pMP1 = vpMapPoints1[i];
            MapPoint *pMP2 = vpMatches1[i];
            const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (!pMP1 || !pMP2) continue;
            if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
            const cv::Mat P3D1w = pMP1->GetWorldPos();
            const cv::Mat P3D2w = pMP2->GetWorldPos();
            for (int k = 0; k < 3; k++) { g.world1.push_back(P3D1w.at<float>(k)); g.world2.push_back(P3D2w.at<float>(k)); }
            const cv::KeyPoint &kpUn1 = pKF1->mvKeysUn[i];
            const cv::KeyPoint &kpUn2 = pKF2->mvKeysUn[i2];
            g.obs1.push_back(kpUn1.pt.x); g.obs1.push_back(kpUn1.pt.y);
            g.obs2.push_back(kpUn2.pt.x); g.obs2.push_back(kpUn2.pt.y);
            g.inv1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]);
            g.inv2.push_back(pKF2->mvInvLevelSigma2[kpUn2.octave]);
            g.vnIndexEdge.push_back(i);
        }
        const int n = (int)g.vnIndexEdge.size();
        P.n = n;
        if (n) {
            P.world1 = &g.world1[0]; P.world2 = &g.world2[0]; P.obs1 = &g.obs1[0]; P.obs2 = &g.obs2[0]; P.inv_sigma2_1 = &g.inv1[0]; P.inv_sigma2_2 = &g.inv2[0];
        }
        const Eigen::Matrix3d R = I.g2oS12->rotation().toRotationMatrix();
        const Eigen::Vector3d t = I.g2oS12->translation();
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) P.r12[3 * i + j] = R(i, j);
            P.t12[i] = t[i];
        }
        P.s12 = I.g2oS12->scale();
        P.th2 = th2; P.fix_scale = bFixScale ? 1 : 0;
        g.removedFirst.assign(n ? n : 1, 0); g.removedFinal.assign(n ? n : 1, 0);
        orbx_sim3_opt_result &R_ = results[c];
        memset(&R_, 0, sizeof(R_));
        R_.n_inliers = &g.nInliers; R_.n_bad = &g.nBad; R_.quat = g.quat; R_.t = g.t; R_.s = &g.s;
        R_.removed_first = &g.removedFirst[0]; R_.removed_final = &g.removedFinal[0];
        if (n > maxN) maxN = n;
    }
    if (maxN > ORBX_SIM3_OPT_MAX_PAIRS) return Fail("OptimizeSim3", "more pairs than ORBX_SIM3_OPT_MAX_PAIRS");
    ThreadOptimizer &T = tOptimizer;
    if (!T.h || T.problems < C || T.pairs < maxN) {
        if (T.h) orbx_sim3_optimizer_destroy(T.h);
        T.h = 0;
        const int problems = C > 8 ? C : 8, pairs = maxN > 512 ? ORBX_SIM3_OPT_MAX_PAIRS : 512;
        if (orbx_sim3_optimizer_create(Device(), problems, pairs, &T.h) != ORBX_OK) { T.h = 0; return Fail("OptimizeSim3"); }
        T.problems = problems; T.pairs = pairs;
    }
    if (orbx_optimize_sim3(T.h, &probs[0], C, &results[0]) != ORBX_OK) return Fail("OptimizeSim3");
    gOptSim3Calls++; gOptSim3Problems += (unsigned long)C;
    for (int c = 0; c < C; c++) {
        Sim3Refinement &I = items[c];
        Gathered &g = G[c];
        std::vector<MapPoint *> &vpMatches1 = *I.vpMatches1;
        const int n = (int)g.vnIndexEdge.size();
        // :1531-1548, :1568-1582
        for (int k = 0; k < n; k++)
            if (g.removedFirst[k] || g.removedFinal[k]) vpMatches1[g.vnIndexEdge[k]] = static_cast<MapPoint *>(NULL);
        if (n - g.nBad < 10) { I.nInliers = 0; continue; }      // :1558-1559, g2oS12 stays as passed in
        *I.g2oS12 = g2o::Sim3(Eigen::Quaterniond(g.quat[3], g.quat[0], g.quat[1], g.quat[2]), Eigen::Vector3d(g.t[0], g.t[1], g.t[2]), g.s);
        I.nInliers = g.nInliers;
    }
    return true;
}
}  // namespace orbx_shim

namespace ORB_SLAM2
{
int OptimizeSim3_hip(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2, const bool bFixScale)
{
    std::vector<orbx_shim::Sim3Refinement> one(1);
    one[0].pKF1 = pKF1; one[0].pKF2 = pKF2; one[0].vpMatches1 = &vpMatches1; one[0].g2oS12 = &g2oS12; one[0].nInliers = 0;
    if (!orbx_shim::OptimizeSim3All(one, th2, bFixScale)) return 0;
    return one[0].nInliers;
}
}  // namespace ORB_SLAM2
