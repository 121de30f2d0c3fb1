// shim/LocalMapping_hip.cc -- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:312-625) on real objects with the neighbour loop on the device.
//
// Compiled against the REFERENCE's own include/LocalMapping.h / KeyFrame.h / MapPoint.h, like the other shim files.  It replaces no member function:
// the call `CreateNewMapPoints();` of LocalMapping::Run (src/LocalMapping.cc:96) becomes
//     ORB_SLAM2::orbx_shim::CreateNewMapPoints(this)
// ("New map points").  A file of its own: the drop-in library of oracle/Makefile does not link it; it is compile-checked only.
//
// What stays on the host, per neighbour: the baseline / ComputeSceneMedianDepth gate (:358-384, it walks MapPoints), ComputeF12 (:388) and the epipole
// (src/ORBmatcher.cc:817-826) - K tiny computations.  The neighbours that pass go to ONE orbx_create_new_map_points: per neighbour, in order,
// SearchForTriangulation on the current eligibility of KF1's features, the per-match geometry (:423-596) and the eligibility update, without a
// host synchronisation in between.  CheckNewKeyFrames() (:353): the call reads a byte before it enqueues every neighbour but the first; the body
// sets the exported byte orbx_shim_new_keyframe_pending from CheckNewKeyFrames() right before the call, and an integrator who wants the abort
// to take effect while the chain is being enqueued raises it in LocalMapping::InsertKeyFrame.  The bookkeeping of :600-622 then
// runs per created entry, in the list's order = the reference's creation order.
#include <cstring>
#include <mutex>
#include <vector>

#include "KeyFrame.h"
#include "LocalMapping.h"
#include "Map.h"
#include "MapPoint.h"
#include "orbx.h"
#include "shim_error.h"
#include "LocalMapping_hip.h"

static unsigned long gCreateCalls = 0;
extern "C" __attribute__((visibility("default"))) unsigned long orbx_shim_create_new_map_points_calls(void) { return gCreateCalls; }
// raised by the integrator's InsertKeyFrame (optional): the device call reads it before every neighbour but the first
extern "C" __attribute__((visibility("default"))) volatile unsigned char orbx_shim_new_keyframe_pending = 0;

namespace ORB_SLAM2
{
namespace
{
struct ThreadMatcher {
    orbx_matcher *h;
    int cap;
    ThreadMatcher() : h(0), cap(0) {}
    ~ThreadMatcher() { if (h) orbx_matcher_destroy(h); }
};
thread_local ThreadMatcher tMatcher;

void FlatGroups(const DBoW2::FeatureVector &fv, int N, int32_t *g)
{
    for (int i = 0; i < N; i++) g[i] = -1;
    for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it)
        for (size_t k = 0; k < it->second.size(); k++)
            if ((int)it->second[k] < N) g[it->second[k]] = (int32_t)it->first;
}

void FillGeom(KeyFrame *kf, orbx_keyframe_geom &g)
{
    const cv::Mat R = kf->GetRotation(), t = kf->GetTranslation(), ow = kf->GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) g.tcw[4 * r + c] = R.at<float>(r, c);
        g.tcw[4 * r + 3] = t.at<float>(r);
        g.center[r] = ow.at<float>(r);
    }
    g.fx = kf->fx; g.fy = kf->fy; g.cx = kf->cx; g.cy = kf->cy; g.invfx = kf->invfx; g.invfy = kf->invfy; g.mb = kf->mb; g.mbf = kf->mbf;
    g.scale_factor = kf->mfScaleFactor;
    g.scale_factors = &kf->mvScaleFactors[0]; g.level_sigma2 = &kf->mvLevelSigma2[0]; g.nlevels = (int)kf->mvScaleFactors.size();
}

struct LocalMappingAccess : public LocalMapping {
    static int Create(LocalMapping *lm)
    {
        LocalMappingAccess *q = static_cast<LocalMappingAccess *>(lm);
        KeyFrame *kf1 = q->mpCurrentKeyFrame;
        int nn = 10;                                                                          // :316-318
        if (q->mbMonocular) nn = 20;
        const std::vector<KeyFrame *> vpNeighKFs = kf1->GetBestCovisibilityKeyFrames(nn);    // :321
        const cv::Mat Ow1 = kf1->GetCameraCenter();
        // the gate of :358-384 and F12 (:388): the neighbours that pass, in order
        std::vector<KeyFrame *> nbs;
        std::vector<float> f12, epi;
        for (size_t i = 0; i < vpNeighKFs.size(); i++) {
            KeyFrame *kf2 = vpNeighKFs[i];
            const cv::Mat Ow2 = kf2->GetCameraCenter();
            const cv::Mat vBaseline = Ow2 - Ow1;
            const float baseline = cv::norm(vBaseline);
            if (!q->mbMonocular) {
                if (baseline < kf2->mb) continue;
            } else {
                const float medianDepthKF2 = kf2->ComputeSceneMedianDepth(2);
                const float ratioBaselineDepth = baseline / medianDepthKF2;
                if (ratioBaselineDepth < 0.01) continue;
            }
            const cv::Mat F12 = q->ComputeF12(kf1, kf2);
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) f12.push_back(F12.at<float>(r, c));
            const cv::Mat C2 = kf2->GetRotation() * Ow1 + kf2->GetTranslation();             // src/ORBmatcher.cc:817-826
            const float invz = 1.0f / C2.at<float>(2);
            epi.push_back(kf2->fx * C2.at<float>(0) * invz + kf2->cx);
            epi.push_back(kf2->fy * C2.at<float>(1) * invz + kf2->cy);
            nbs.push_back(kf2);
        }
        const int K = (int)nbs.size(), N1 = kf1->N;
        if (K == 0 || N1 == 0) return 0;

        // KF1 and the neighbours as flat arrays
        int cap2 = 1;
        for (int k = 0; k < K; k++) cap2 = nbs[k]->N > cap2 ? nbs[k]->N : cap2;
        std::vector<int32_t> g1((size_t)N1), cnt2((size_t)K), g2((size_t)K * cap2, -1);
        std::vector<uint8_t> ok1((size_t)N1), ok2((size_t)K * cap2, 0), d2((size_t)K * cap2 * 32, 0);
        std::vector<orbx_keypoint> kp2((size_t)K * cap2);
        std::vector<float> raw1((size_t)N1 * 2), raw2((size_t)K * cap2 * 2, 0.f), ur2((size_t)K * cap2, -1.f), dp2((size_t)K * cap2, -1.f);
        std::vector<orbx_keyframe_geom> geom2((size_t)K);
        FlatGroups(kf1->mFeatVec, N1, &g1[0]);
        for (int i = 0; i < N1; i++) {
            ok1[(size_t)i] = kf1->GetMapPoint((size_t)i) ? 0 : 1;                            // src/ORBmatcher.cc:845-849
            raw1[2 * (size_t)i] = kf1->mvKeys[(size_t)i].pt.x; raw1[2 * (size_t)i + 1] = kf1->mvKeys[(size_t)i].pt.y;
        }
        for (int k = 0; k < K; k++) {
            KeyFrame *kf2 = nbs[k];
            const int N2 = kf2->N;
            const size_t o = (size_t)k * cap2;
            cnt2[(size_t)k] = N2;
            FillGeom(kf2, geom2[(size_t)k]);
            if (N2 == 0) continue;
            memcpy(&kp2[o], &kf2->mvKeysUn[0], (size_t)N2 * sizeof(orbx_keypoint));
            memcpy(&d2[o * 32], kf2->mDescriptors.data, (size_t)N2 * 32);
            FlatGroups(kf2->mFeatVec, N2, &g2[o]);
            for (int i = 0; i < N2; i++) {
                ok2[o + i] = kf2->GetMapPoint((size_t)i) ? 0 : 1;                            // :867-871
                raw2[2 * (o + i)] = kf2->mvKeys[(size_t)i].pt.x; raw2[2 * (o + i) + 1] = kf2->mvKeys[(size_t)i].pt.y;
                ur2[o + i] = kf2->mvuRight[(size_t)i]; dp2[o + i] = kf2->mvDepth[(size_t)i];
            }
        }
        orbx_keyframe_geom geom1;
        FillGeom(kf1, geom1);
        const orbx_feature_set a = {(const orbx_keypoint *)&kf1->mvKeysUn[0], kf1->mDescriptors.data, &N1, &g1[0], &ok1[0], N1, 1};
        const orbx_feature_set b = {&kp2[0], &d2[0], &cnt2[0], &g2[0], &ok2[0], cap2, K};
        orbx_new_points_params prm;
        memset(&prm, 0, sizeof(prm));
        prm.geom1 = &geom1; prm.geom2 = &geom2[0]; prm.f12 = &f12[0]; prm.epipole = &epi[0];
        prm.keys_raw1 = &raw1[0]; prm.u_right1 = &kf1->mvuRight[0]; prm.depth1 = &kf1->mvDepth[0];
        prm.keys_raw2 = &raw2[0]; prm.u_right2 = &ur2[0]; prm.depth2 = &dp2[0];
        prm.check_orientation = 0;                                                           // ORBmatcher matcher(0.6,false), :323

        const int need = N1 > cap2 ? N1 : cap2;
        ThreadMatcher &M = tMatcher;
        if (!M.h || need > M.cap) {
            if (M.h) { orbx_matcher_destroy(M.h); M.h = 0; }
            M.cap = need > 4096 ? need : 4096;
            if (orbx_matcher_create(::orbx_shim::Device(), M.cap, 1, &M.h) != ORBX_OK) { M.h = 0; ::orbx_shim::Fail("CreateNewMapPoints"); return 0; }
        }
        std::vector<orbx_new_point> created((size_t)N1);
        std::vector<int32_t> nm((size_t)K);
        int32_t count = 0, done = 0;
        orbx_new_points_result res;
        memset(&res, 0, sizeof(res));
        res.created = &created[0]; res.created_capacity = N1; res.count = &count; res.nmatches = &nm[0]; res.pairs_done = &done;
        orbx_shim_new_keyframe_pending = q->CheckNewKeyFrames() ? 1 : 0;                     // :353, read by the call before neighbour k > 0
        if (orbx_create_new_map_points(M.h, &a, &b, &prm, &orbx_shim_new_keyframe_pending, &res) != ORBX_OK) { ::orbx_shim::Fail("CreateNewMapPoints"); return 0; }

        // :600-622 per created point, in creation order
        int nnew = 0;
        for (int e = 0; e < count; e++) {
            const orbx_new_point &p = created[(size_t)e];
            KeyFrame *kf2 = nbs[(size_t)p.neighbour];
            cv::Mat x3D(3, 1, CV_32F);
            x3D.at<float>(0) = p.x; x3D.at<float>(1) = p.y; x3D.at<float>(2) = p.z;
            MapPoint *pMP = new MapPoint(x3D, kf1, q->mpMap);
            pMP->AddObservation(kf1, (size_t)p.idx1);
            pMP->AddObservation(kf2, (size_t)p.idx2);
            kf1->AddMapPoint(pMP, (size_t)p.idx1);
            kf2->AddMapPoint(pMP, (size_t)p.idx2);
            pMP->ComputeDistinctiveDescriptors();
            pMP->UpdateNormalAndDepth();
            q->mpMap->AddMapPoint(pMP);
            q->mlpRecentAddedMapPoints.push_back(pMP);
            nnew++;
        }
        return nnew;
    }
};
}  // namespace

namespace orbx_shim
{
int CreateNewMapPoints(LocalMapping *lm)
{
    __atomic_add_fetch(&gCreateCalls, 1, __ATOMIC_RELAXED);
    if (!lm) return 0;
    return LocalMappingAccess::Create(lm);
}
}  // namespace orbx_shim
}  // namespace ORB_SLAM2
