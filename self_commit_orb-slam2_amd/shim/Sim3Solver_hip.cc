// shim/Sim3Solver_hip.cc -- bodies for Sim3Solver (src/Sim3Solver.cc) with ComputeSim3 and CheckInliers of EVERY iteration on the device.
//
// Compiled against the REFERENCE's own include/Sim3Solver.h, like the other shim files: this file defines the member functions themselves, so
// the protected members are its own.  A file of its own: the drop-in library of oracle/Makefile does not link it; it is compile-checked only.
//
// What stays on the host: the pointer walk of the constructor (:78-127: vpMatched12 compacted in i1 order, pairs with a missing or bad point or
// an index < 0 skipped), SetRansacParameters' libm calls (orbx_sim3_ransac_iterations) and the RANSAC sets, drawn with
// DUtils::Random::RandomInt by the reference's draw, overwrite-with-back, pop scheme (:228-249).  The reference draws lazily, three numbers per
// iteration, interleaved between the candidates of LoopClosing's round-robin loop; here all mRansacMaxIts sets of a solver are drawn ahead,
// solver after solver, so the process's rand() sequence is consumed in ANOTHER ORDER: same scheme, same distribution, no parity of the draws.
// ONE orbx_sim3_solve then runs the constructor's arithmetic, ComputeSim3 and CheckInliers of every iteration of every solver handed to
// orbx_shim::SolveAll, and derives the return events; iterate replays them.  The first event's inliers come with the call; later events read
// their row of the device's masks (orbx_sim3_inliers), and a solver whose masks another call has overwritten since is solved again, alone, with
// the sets it drew.  What the reference's class cannot hold (it is not changed) lives in a table beside it, keyed by the solver's address.
// On a device error (counted, std::cerr: shim_error.h) iterate returns an empty matrix with bNoMore = true: the candidate is discarded.
#include <map>
#include <mutex>
#include <vector>

#include "Sim3Solver.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "orbx.h"
#include "shim_error.h"
#include "Sim3Solver_hip.h"

static unsigned long gSim3Calls = 0, gSim3Solvers = 0;
extern "C" __attribute__((visibility("default"))) unsigned long orbx_shim_sim3_calls(void) { return gSim3Calls; }
extern "C" __attribute__((visibility("default"))) unsigned long orbx_shim_sim3_solvers(void) { return gSim3Solvers; }

namespace ORB_SLAM2
{
namespace
{
struct Sim3State {
    std::vector<float> world1, world2, sigma1, sigma2;      // per kept pair
    float rcw1[9], tcw1[3], rcw2[9], tcw2[3];
    std::vector<int32_t> sets;                              // [mRansacMaxIts][3], drawn once
    bool solved;
    unsigned long generation;                               // of the device call that holds this solver's masks
    int candidate;                                          // ... and its place in that call
    std::vector<int32_t> count;
    std::vector<float> r12, t12, s12;
    std::vector<uint8_t> inliersFirst;
    int firstEvent;
    Sim3State() : solved(false), generation(0), candidate(0), firstEvent(-1) {}
};
std::mutex gTableMutex;
std::map<const Sim3Solver *, Sim3State> gTable;

struct ThreadSolver {
    orbx_sim3_solver *h;
    int candidates, matches, iterations;
    unsigned long generation;
    ThreadSolver() : h(0), candidates(0), matches(0), iterations(0), generation(0) {}
    ~ThreadSolver() { if (h) orbx_sim3_solver_destroy(h); }
};
thread_local ThreadSolver tSolver;

Sim3State &StateOf(const Sim3Solver *s)
{
    std::lock_guard<std::mutex> lock(gTableMutex);
    return gTable[s];
}
}  // namespace

// the reference's members from outside its member functions (SolveAll): a derived type, as shim/MapPointAccess.h does for MapPoint
struct Sim3Access : public Sim3Solver {
    static Sim3Access *Of(Sim3Solver *s) { return static_cast<Sim3Access *>(s); }
    int Pairs() const { return N; }
    int MaxIts() const { return mRansacMaxIts; }
    int MinInliers() const { return mRansacMinInliers; }
    bool FixScale() const { return mbFixScale; }
    const cv::Mat &K1() const { return mK1; }
    const cv::Mat &K2() const { return mK2; }
};

namespace
{
bool SolveList(const std::vector<Sim3Solver *> &list)
{
    const int C = (int)list.size();
    if (!C) return true;
    std::vector<orbx_sim3_problem> probs(C);
    std::vector<orbx_sim3_result> results(C);
    std::vector<Sim3State *> states(C);
    std::vector<int32_t> first(C, -1);
    int maxN = 3, maxIt = 1;
    for (int c = 0; c < C; c++) {
        Sim3Access *A = Sim3Access::Of(list[c]);
        Sim3State &S = StateOf(list[c]);
        states[c] = &S;
        const int n = A->Pairs(), its = n < A->MinInliers() ? 0 : A->MaxIts();
        if ((int)S.sets.size() != 3 * its) {
            // :228-249, all iterations ahead
            S.sets.resize((size_t)3 * its);
            std::vector<size_t> vAvailableIndices;
            for (int it = 0; it < its; it++) {
                vAvailableIndices.resize(n);
                for (int i = 0; i < n; i++) vAvailableIndices[i] = i;
                for (short i = 0; i < 3; ++i) {
                    int randi = DUtils::Random::RandomInt(0, vAvailableIndices.size() - 1);
                    S.sets[(size_t)3 * it + i] = (int32_t)vAvailableIndices[randi];
                    vAvailableIndices[randi] = vAvailableIndices.back();
                    vAvailableIndices.pop_back();
                }
            }
        }
        orbx_sim3_problem &P = probs[c];
        memset(&P, 0, sizeof(P));
        memcpy(P.rcw1, S.rcw1, sizeof(P.rcw1)); memcpy(P.tcw1, S.tcw1, sizeof(P.tcw1)); memcpy(P.rcw2, S.rcw2, sizeof(P.rcw2)); memcpy(P.tcw2, S.tcw2, sizeof(P.tcw2));
        P.fx1 = A->K1().at<float>(0, 0); P.fy1 = A->K1().at<float>(1, 1); P.cx1 = A->K1().at<float>(0, 2); P.cy1 = A->K1().at<float>(1, 2);
        P.fx2 = A->K2().at<float>(0, 0); P.fy2 = A->K2().at<float>(1, 1); P.cx2 = A->K2().at<float>(0, 2); P.cy2 = A->K2().at<float>(1, 2);
        P.n = n;
        P.world1 = n ? &S.world1[0] : 0; P.world2 = n ? &S.world2[0] : 0; P.sigma2_1 = n ? &S.sigma1[0] : 0; P.sigma2_2 = n ? &S.sigma2[0] : 0;
        P.sets = its ? &S.sets[0] : 0; P.iterations = its; P.min_inliers = A->MinInliers(); P.fix_scale = A->FixScale() ? 1 : 0;
        S.count.assign(its, 0); S.r12.assign((size_t)9 * its, 0.0f); S.t12.assign((size_t)3 * its, 0.0f); S.s12.assign(its, 0.0f); S.inliersFirst.assign(n, 0);
        orbx_sim3_result &R = results[c];
        memset(&R, 0, sizeof(R));
        if (its) { R.count = &S.count[0]; R.r12 = &S.r12[0]; R.t12 = &S.t12[0]; R.s12 = &S.s12[0]; }
        if (n) R.inliers_first = &S.inliersFirst[0];
        R.first_event = &first[c];
        if (n > maxN) maxN = n;
        if (its > maxIt) maxIt = its;
    }
    ThreadSolver &T = tSolver;
    if (!T.h || T.candidates < C || T.matches < maxN || T.iterations < maxIt) {
        if (T.h) orbx_sim3_solver_destroy(T.h);
        T.h = 0;
        int capC = 8, capN = 2048;
        while (capC < C) capC *= 2;
        while (capN < maxN) capN *= 2;
        if (capN > ORBX_SIM3_MAX_MATCHES) capN = ORBX_SIM3_MAX_MATCHES;
        const int capI = maxIt > 300 ? maxIt : 300;
        if (orbx_sim3_solver_create(orbx_shim::Device(), capC, capN, capI, &T.h) != ORBX_OK) { T.h = 0; return orbx_shim::Fail("Sim3Solver::iterate"); }
        T.candidates = capC; T.matches = capN; T.iterations = capI;
    }
    __sync_fetch_and_add(&gSim3Calls, 1ul);
    __sync_fetch_and_add(&gSim3Solvers, (unsigned long)C);
    T.generation++;
    if (orbx_sim3_solve(T.h, &probs[0], C, &results[0]) != ORBX_OK) return orbx_shim::Fail("Sim3Solver::iterate");
    for (int c = 0; c < C; c++) {
        states[c]->solved = true; states[c]->generation = T.generation; states[c]->candidate = c; states[c]->firstEvent = first[c];
    }
    return true;
}
}  // namespace

Sim3Solver::Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const vector<MapPoint *> &vpMatched12, const bool bFixScale) : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale)
{
    mpKF1 = pKF1;
    mpKF2 = pKF2;
    vector<MapPoint *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    mN1 = vpMatched12.size();
    mvpMapPoints1.reserve(mN1);
    mvpMapPoints2.reserve(mN1);
    mvpMatches12 = vpMatched12;
    mvnIndices1.reserve(mN1);
    mvAllIndices.reserve(mN1);

    Sim3State &S = StateOf(this);
    S = Sim3State();      // an earlier solver at this address
    cv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation(), Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) { S.rcw1[3 * i + j] = Rcw1.at<float>(i, j); S.rcw2[3 * i + j] = Rcw2.at<float>(i, j); }
        S.tcw1[i] = tcw1.at<float>(i); S.tcw2[i] = tcw2.at<float>(i);
    }
    size_t idx = 0;
    for (int i1 = 0; i1 < mN1; i1++) {
        if (!vpMatched12[i1]) continue;
        MapPoint *pMP1 = vpKeyFrameMP1[i1];
        MapPoint *pMP2 = vpMatched12[i1];
        if (!pMP1) continue;
        if (pMP1->isBad() || pMP2->isBad()) continue;
        int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
        int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (indexKF1 < 0 || indexKF2 < 0) continue;
        const cv::KeyPoint &kp1 = pKF1->mvKeysUn[indexKF1];
        const cv::KeyPoint &kp2 = pKF2->mvKeysUn[indexKF2];
        S.sigma1.push_back(pKF1->mvLevelSigma2[kp1.octave]);      // the device makes mvnMaxError1 / 2 of them (9.210 * sigma2, truncated)
        S.sigma2.push_back(pKF2->mvLevelSigma2[kp2.octave]);
        mvpMapPoints1.push_back(pMP1);
        mvpMapPoints2.push_back(pMP2);
        mvnIndices1.push_back(i1);
        cv::Mat X3D1w = pMP1->GetWorldPos(), X3D2w = pMP2->GetWorldPos();
        for (int c = 0; c < 3; c++) { S.world1.push_back(X3D1w.at<float>(c)); S.world2.push_back(X3D2w.at<float>(c)); }
        mvAllIndices.push_back(idx);
        idx++;
    }
    mK1 = pKF1->mK;
    mK2 = pKF2->mK;
    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations)
{
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    N = mvpMapPoints1.size();
    mvbInliersi.resize(N);
    mRansacMaxIts = orbx_sim3_ransac_iterations(probability, minInliers, maxIterations, N);
    mnIterations = 0;
    Sim3State &S = StateOf(this);
    S.solved = false;      // min_inliers decides the events, mRansacMaxIts the sets
    S.sets.clear();
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    bNoMore = false;
    vbInliers = vector<bool>(mN1, false);
    nInliers = 0;
    if (N < mRansacMinInliers) {
        bNoMore = true;
        return cv::Mat();
    }
    Sim3State &S = StateOf(this);
    if (!S.solved && !SolveList(std::vector<Sim3Solver *>(1, this))) {
        bNoMore = true;
        return cv::Mat();
    }
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
        nCurrentIterations++;
        const int it = mnIterations++;
        mnInliersi = S.count[it];
        if (mnInliersi < mnBestInliers) continue;
        // :258-276
        mnBestInliers = mnInliersi;
        ms12i = S.s12[it];
        mR12i = cv::Mat(3, 3, CV_32F);
        mt12i = cv::Mat(3, 1, CV_32F);
        mT12i = cv::Mat::eye(4, 4, CV_32F);
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) { mR12i.at<float>(i, j) = S.r12[9 * it + 3 * i + j]; mT12i.at<float>(i, j) = ms12i * S.r12[9 * it + 3 * i + j]; }
            mt12i.at<float>(i) = S.t12[3 * it + i];
            mT12i.at<float>(i, 3) = S.t12[3 * it + i];
        }
        mBestT12 = mT12i.clone();
        mBestRotation = mR12i.clone();
        mBestTranslation = mt12i.clone();
        mBestScale = ms12i;
        if (mnInliersi <= mRansacMinInliers) continue;      // mvbBestInliers is only read on a return: filled there
        std::vector<uint8_t> row;
        const uint8_t *inl = 0;
        if (it == S.firstEvent) inl = N ? &S.inliersFirst[0] : 0;
        else {
            if (S.generation != tSolver.generation && !SolveList(std::vector<Sim3Solver *>(1, this))) { bNoMore = true; return cv::Mat(); }
            row.resize(N);
            if (orbx_sim3_inliers(tSolver.h, S.candidate, it, &row[0]) != ORBX_OK) { orbx_shim::Fail("Sim3Solver::iterate"); bNoMore = true; return cv::Mat(); }
            inl = &row[0];
        }
        nInliers = mnInliersi;
        for (int i = 0; i < N; i++) {
            mvbInliersi[i] = inl[i] != 0;
            if (inl[i]) vbInliers[mvnIndices1[i]] = true;
        }
        mvbBestInliers = mvbInliersi;
        return mBestT12;
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;
    return cv::Mat();
}

cv::Mat Sim3Solver::find(vector<bool> &vbInliers12, int &nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation() { return mBestRotation.clone(); }

cv::Mat Sim3Solver::GetEstimatedTranslation() { return mBestTranslation.clone(); }

float Sim3Solver::GetEstimatedScale() { return mBestScale; }
}  // namespace ORB_SLAM2

namespace orbx_shim
{
bool SolveAll(const std::vector<ORB_SLAM2::Sim3Solver *> &solvers)
{
    std::vector<ORB_SLAM2::Sim3Solver *> todo;
    for (size_t i = 0; i < solvers.size(); i++)
        if (solvers[i] && !ORB_SLAM2::StateOf(solvers[i]).solved) todo.push_back(solvers[i]);
    return ORB_SLAM2::SolveList(todo);
}

void Release(ORB_SLAM2::Sim3Solver *solver)
{
    std::lock_guard<std::mutex> lock(ORB_SLAM2::gTableMutex);
    ORB_SLAM2::gTable.erase(solver);
}
}  // namespace orbx_shim
