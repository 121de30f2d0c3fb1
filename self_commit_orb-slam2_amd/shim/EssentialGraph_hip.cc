// shim/EssentialGraph_hip.cc -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1017-1339) with the Sim3 pose graph on the device.
//
// Compiled against the REFERENCE's own headers, like the other shim files.  A file of its own: the drop-in library of oracle/Makefile does not
// link it; it is compile-checked only.
//
// What stays on the host is the reference's pointer walk: the keyframes that are not bad become the vertices, in ascending mnId (:1059-1098;
// CorrectedSim3 where present, else Sim3(Rcw, tcw, 1) through Quaterniond(R)); the edges are chosen by the reference's rules (:1106-1262:
// LoopConnections pairs below minFeat are skipped unless they are the (current, loop) pair, and fill sInsertedEdges, which dedupes covisibility
// edges only; loop and covisibility edges go towards the smaller id; covisibility edges skip the parent, the children, the loop edges and bad
// keyframes; GetCovisiblesByWeight's order is kept); every map point that is not bad gets the vertex of mnCorrectedReference or of its reference
// keyframe (:1311-1322).  ONE orbx_optimize_essential_graph (repeated once with the dense fill bound when the factor outgrows the handle's fill budget) then forms the measurements, runs the Levenberg iterations and corrects poses and
// points.  Under mMutexMapUpdate the host calls SetPose, SetWorldPos and UpdateNormalAndDepth, as the reference does (:1274-1338).
// On a device error (counted, std::cerr: shim_error.h) the function returns and touches nothing.
#include <algorithm>
#include <map>
#include <set>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Map.h"
#include "LoopClosing.h"
#include "Converter.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
#include "orbx.h"
#include "shim_error.h"
#include "EssentialGraph_hip.h"

static unsigned long gEssentialGraphCalls = 0;
extern "C" __attribute__((visibility("default"))) unsigned long orbx_shim_essential_graph_calls(void) { return gEssentialGraphCalls; }

namespace
{
struct ThreadGraph {
    orbx_essential_graph *h;
    int keyframes, edges, points;
    long long fill;
    ThreadGraph() : h(0), keyframes(0), edges(0), points(0), fill(0) {}
    ~ThreadGraph() { if (h) orbx_essential_graph_destroy(h); }
    bool Create(int nk, int ne, int np, long long nfill)
    {
        if (h) orbx_essential_graph_destroy(h);
        h = 0;
        nfill = std::min<long long>(std::max<long long>(nfill, 1), 2147483647LL);
        if (orbx_essential_graph_create(orbx_shim::Device(), nk, ne, np, (int)nfill, &h) != ORBX_OK) { h = 0; return orbx_shim::Fail("OptimizeEssentialGraph"); }
        keyframes = nk; edges = ne; points = np; fill = nfill;
        return true;
    }
};
thread_local ThreadGraph tGraph;

void PutSim3(std::vector<double> &v, size_t i, const g2o::Sim3 &S)
{
    const Eigen::Quaterniond &q = S.rotation();
    const Eigen::Vector3d &t = S.translation();
    double *o = &v[8 * i];
    o[0] = q.x(); o[1] = q.y(); o[2] = q.z(); o[3] = q.w(); o[4] = t[0]; o[5] = t[1]; o[6] = t[2]; o[7] = S.scale();
}
bool ById(ORB_SLAM2::KeyFrame *a, ORB_SLAM2::KeyFrame *b) { return a->mnId < b->mnId; }
}  // namespace

namespace ORB_SLAM2
{
void OptimizeEssentialGraph_hip(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                const LoopClosing::KeyFrameAndPose &CorrectedSim3, const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections,
                                const bool &bFixScale)
{
    const std::vector<KeyFrame *> vpAll = pMap->GetAllKeyFrames();
    const std::vector<MapPoint *> vpMPs = pMap->GetAllMapPoints();
    const unsigned int nMaxKFid = pMap->GetMaxKFid();
    const int minFeat = 100;

    // :1059-1098 the vertices
    std::vector<KeyFrame *> vpKFs;
    for (size_t i = 0; i < vpAll.size(); i++)
        if (!vpAll[i]->isBad()) vpKFs.push_back(vpAll[i]);
    std::sort(vpKFs.begin(), vpKFs.end(), ById);
    const int N = (int)vpKFs.size();
    std::vector<int> vnIndex(nMaxKFid + 1, -1);
    std::vector<double> est(8 * (size_t)(N ? N : 1)), meas(8 * (size_t)(N ? N : 1));
    int fixed = -1;
    for (int i = 0; i < N; i++) {
        KeyFrame *pKF = vpKFs[i];
        if (pKF->mnId > nMaxKFid) { orbx_shim::Fail("OptimizeEssentialGraph", "a keyframe id beyond GetMaxKFid"); return; }
        vnIndex[pKF->mnId] = i;
        LoopClosing::KeyFrameAndPose::const_iterator it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) PutSim3(est, i, it->second);
        else {
            Eigen::Matrix<double, 3, 3> Rcw = Converter::toMatrix3d(pKF->GetRotation());
            Eigen::Matrix<double, 3, 1> tcw = Converter::toVector3d(pKF->GetTranslation());
            PutSim3(est, i, g2o::Sim3(Rcw, tcw, 1.0));
        }
        LoopClosing::KeyFrameAndPose::const_iterator itn = NonCorrectedSim3.find(pKF);
        if (itn != NonCorrectedSim3.end()) PutSim3(meas, i, itn->second);
        else std::copy(est.begin() + 8 * i, est.begin() + 8 * i + 8, meas.begin() + 8 * i);
        if (pKF == pLoopKF) fixed = i;
    }
    if (fixed < 0) { orbx_shim::Fail("OptimizeEssentialGraph", "the loop keyframe is not in the map"); return; }
#define ORBX_EG_INDEX(pKF) ((pKF) && (pKF)->mnId <= nMaxKFid ? vnIndex[(pKF)->mnId] : -1)

    // :1106-1143 LoopConnections
    std::vector<int32_t> edges;
    std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;
    for (std::map<KeyFrame *, std::set<KeyFrame *> >::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        KeyFrame *pKF = mit->first;
        const long unsigned int nIDi = pKF->mnId;
        const std::set<KeyFrame *> &spConnections = mit->second;
        for (std::set<KeyFrame *>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            const long unsigned int nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            const int vi = ORBX_EG_INDEX(pKF), vj = ORBX_EG_INDEX(*sit);
            if (vi >= 0 && vj >= 0 && vi != vj) { edges.push_back(vi); edges.push_back(vj); edges.push_back(0); }
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    // :1147-1262 spanning tree, loop edges, covisibility graph
    for (int i = 0; i < N; i++) {
        KeyFrame *pKF = vpKFs[i];
        KeyFrame *pParentKF = pKF->GetParent();
        const int vp = ORBX_EG_INDEX(pParentKF);
        if (pParentKF && vp >= 0 && vp != i) { edges.push_back(i); edges.push_back(vp); edges.push_back(1); }
        const std::set<KeyFrame *> sLoopEdges = pKF->GetLoopEdges();
        for (std::set<KeyFrame *>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
            KeyFrame *pLKF = *sit;
            const int vl = ORBX_EG_INDEX(pLKF);
            if (pLKF->mnId < pKF->mnId && vl >= 0) { edges.push_back(i); edges.push_back(vl); edges.push_back(1); }
        }
        const std::vector<KeyFrame *> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (std::vector<KeyFrame *>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            KeyFrame *pKFn = *vit;
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    const int vn = ORBX_EG_INDEX(pKFn);
                    if (vn >= 0) { edges.push_back(i); edges.push_back(vn); edges.push_back(1); }
                }
            }
        }
    }
    // :1304-1322 the map points and their reference vertices
    std::vector<MapPoint *> vpKept;
    std::vector<float> points;
    std::vector<int32_t> ref;
    for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
        MapPoint *pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        long unsigned int nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
        else nIDr = pMP->GetReferenceKeyFrame()->mnId;
        const cv::Mat P3Dw = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) points.push_back(P3Dw.at<float>(k));
        ref.push_back(nIDr <= nMaxKFid ? vnIndex[nIDr] : -1);      // a reference without a vertex: the table's default entries, two identities
        vpKept.push_back(pMP);
    }
#undef ORBX_EG_INDEX
    const int E = (int)(edges.size() / 3), M = (int)vpKept.size();

    ThreadGraph &T = tGraph;
    const long long dense = (long long)N * (N + 1) / 2;
    if (!T.h || T.keyframes < N || T.edges < E || T.points < M) {
        const long long fill = std::min<long long>(std::max<long long>(dense, 1), 96LL * std::max(2 * N, 256));
        if (!T.Create(std::max(2 * N, 256), std::max(2 * E, 4096), std::max(2 * M, 1 << 16), fill)) return;
    }
    orbx_essential_graph_problem P;
    memset(&P, 0, sizeof(P));
    P.n = N; P.est = &est[0]; P.meas = &meas[0]; P.fixed = fixed; P.fix_scale = bFixScale ? 1 : 0;
    P.n_edges = E; P.edges = E ? &edges[0] : 0;
    P.n_points = M; P.points = M ? &points[0] : 0; P.point_ref = M ? &ref[0] : 0;
    P.iterations = 20; P.lambda_init = 1e-16;
    std::vector<float> tiw(12 * (size_t)N), corrected(3 * (size_t)(M ? M : 1));
    orbx_essential_graph_result R;
    memset(&R, 0, sizeof(R));
    R.tiw = &tiw[0]; R.points = &corrected[0];
    int rc = orbx_optimize_essential_graph(T.h, &P, &R);
    if (rc == ORBX_ERR_CAPACITY && T.fill < dense) {      // the keyframes, edges and points fit: the factor outgrew the fill budget.  Once more with the dense bound.
        if (!T.Create(T.keyframes, T.edges, T.points, (long long)T.keyframes * (T.keyframes + 1) / 2)) return;
        rc = orbx_optimize_essential_graph(T.h, &P, &R);
    }
    if (rc != ORBX_OK) { orbx_shim::Fail("OptimizeEssentialGraph"); return; }
    gEssentialGraphCalls++;

    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    // :1279-1299 [R | t / s]
    for (int i = 0; i < N; i++) {
        cv::Mat Tiw = cv::Mat::eye(4, 4, CV_32F);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) Tiw.at<float>(r, c) = tiw[12 * (size_t)i + 4 * r + c];
        vpKFs[i]->SetPose(Tiw);
    }
    // :1304-1338
    for (int i = 0; i < M; i++) {
        cv::Mat cvCorrectedP3Dw(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) cvCorrectedP3Dw.at<float>(k) = corrected[3 * (size_t)i + k];
        vpKept[i]->SetWorldPos(cvCorrectedP3Dw);
        vpKept[i]->UpdateNormalAndDepth();
    }
}
}  // namespace ORB_SLAM2
