// shim/PnPsolver_hip.cc -- bodies for PnPsolver (src/PnPsolver.cc) with compute_pose, CheckInliers and Refine of EVERY iteration on the device.
//
// Compiled against the REFERENCE's own include/PnPsolver.h, like the other shim files: this file defines the member functions themselves, so
// the private members are its own.  A file of its own: the drop-in library of oracle/Makefile does not link it; it is compile-checked only.
//
// What stays on the host: the pointer walk of the constructor (:120-168: matches with a missing or bad point skipped), SetRansacParameters'
// libm calls (orbx_pnp_ransac_parameters) and the RANSAC sets, drawn with DUtils::Random::RandomInt by the reference's draw,
// overwrite-with-back, pop scheme (:274-290).  The reference draws lazily, four numbers per iteration, interleaved between the candidates of
// Tracking::Relocalization's round-robin loop; here all mRansacMaxIts sets of a solver are drawn ahead, solver after solver, so the process's
// rand() sequence is consumed in ANOTHER ORDER: same scheme, same distribution, no parity of the draws.  ONE orbx_pnp_solve then runs
// compute_pose and CheckInliers of every iteration and Refine of every record of every solver handed to orbx_shim::SolveAll, and derives the
// return events; iterate replays them, loop condition (:266) included: a call behind mRansacMaxIts runs nIterations further iterations, on
// further sets solved by a further device call.  The first event's refined inliers come with the call; other rows are read from the device's
// masks (orbx_pnp_inliers), and a solver whose masks another call has overwritten since is solved again, alone, with the sets it drew.
// What the reference's class cannot hold (it is not changed) lives in a table beside it, keyed by the solver's address.
// On a device error (counted, std::cerr: shim_error.h) iterate returns an empty matrix with bNoMore = true: the candidate is discarded.
#include <map>
#include <mutex>
#include <vector>

#include "PnPsolver.h"
#include "Frame.h"
#include "MapPoint.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "orbx.h"
#include "shim_error.h"
#include "PnPsolver_hip.h"

static unsigned long gPnPCalls = 0, gPnPSolvers = 0;
extern "C" __attribute__((visibility("default"))) unsigned long orbx_shim_pnp_calls(void) { return gPnPCalls; }
extern "C" __attribute__((visibility("default"))) unsigned long orbx_shim_pnp_solvers(void) { return gPnPSolvers; }

namespace ORB_SLAM2
{
namespace
{
struct PnPState {
    std::vector<float> p2d, sigma2, p3d;                    // per kept match
    double probability;                                     // the SetRansacParameters arguments as given
    int minInliers, maxIterations, minSet;
    float epsilon, th2;
    std::vector<int32_t> sets;                              // [iterations][4], drawn once, extended behind mRansacMaxIts
    bool solved;
    unsigned long generation;                               // of the device call that holds this solver's masks
    int candidate;                                          // ... and its place in that call
    int iterations, nrecords, firstEvent;
    std::vector<int32_t> count, recordOf, recordIteration, refinedCount;
    std::vector<double> r, t;
    std::vector<float> refinedTcw;
    std::vector<uint8_t> inliersFirst;
    PnPState() : probability(0.99), minInliers(8), maxIterations(300), minSet(4), epsilon(0.4f), th2(5.991f), solved(false), generation(0), candidate(0), iterations(0),
                 nrecords(0), firstEvent(-1) {}
};
std::mutex gTableMutex;
std::map<const PnPsolver *, PnPState> gTable;

struct ThreadSolver {
    orbx_pnp_solver *h;
    int candidates, matches, iterations;
    unsigned long generation;
    ThreadSolver() : h(0), candidates(0), matches(0), iterations(0), generation(0) {}
    ~ThreadSolver() { if (h) orbx_pnp_solver_destroy(h); }
};
thread_local ThreadSolver tSolver;

PnPState &StateOf(const PnPsolver *s)
{
    std::lock_guard<std::mutex> lock(gTableMutex);
    return gTable[s];
}

struct Entry { PnPsolver *solver; int n, maxIts, minInliers; float fx, fy, cx, cy; };

// draws the sets a solver still lacks (:274-290, ahead) and solves the list in one device call
bool SolveList(const std::vector<Entry> &list, int wantIterations = 0)
{
    const int C = (int)list.size();
    if (!C) return true;
    std::vector<orbx_pnp_problem> probs(C);
    std::vector<orbx_pnp_result> results(C);
    std::vector<PnPState *> states(C);
    std::vector<int32_t> first(C, -1), nrec(C, 0);
    int maxN = 4, maxIt = 1;
    for (int c = 0; c < C; c++) {
        const Entry &E = list[c];
        PnPState &S = StateOf(E.solver);
        states[c] = &S;
        const int n = E.n;
        int its = n < E.minInliers ? 0 : (wantIterations > E.maxIts ? wantIterations : E.maxIts);
        if ((int)S.sets.size() > 4 * its) its = (int)S.sets.size() / 4;
        std::vector<size_t> vAvailableIndices;
        for (int it = (int)S.sets.size() / 4; it < its; it++) {
            vAvailableIndices.resize(n);
            for (int i = 0; i < n; i++) vAvailableIndices[i] = i;
            for (short i = 0; i < 4; ++i) {
                int randi = DUtils::Random::RandomInt(0, vAvailableIndices.size() - 1);
                S.sets.push_back((int32_t)vAvailableIndices[randi]);
                vAvailableIndices[randi] = vAvailableIndices.back();
                vAvailableIndices.pop_back();
            }
        }
        orbx_pnp_problem &P = probs[c];
        memset(&P, 0, sizeof(P));
        P.fx = E.fx; P.fy = E.fy; P.cx = E.cx; P.cy = E.cy;
        P.n = n;
        P.p2d = n ? &S.p2d[0] : 0; P.sigma2 = n ? &S.sigma2[0] : 0; P.p3dw = n ? &S.p3d[0] : 0;
        P.probability = S.probability; P.min_inliers = S.minInliers; P.max_iterations = S.maxIterations; P.min_set = S.minSet; P.epsilon = S.epsilon; P.th2 = S.th2;
        P.sets = its ? &S.sets[0] : 0; P.iterations = its;
        S.iterations = its;
        S.count.assign(its, 0); S.recordOf.assign(its, -1); S.recordIteration.assign(its, -1); S.refinedCount.assign(its, 0);
        S.r.assign((size_t)9 * its, 0.0); S.t.assign((size_t)3 * its, 0.0); S.refinedTcw.assign((size_t)12 * its, 0.0f); S.inliersFirst.assign(n, 0);
        orbx_pnp_result &R = results[c];
        memset(&R, 0, sizeof(R));
        if (its) {
            R.count = &S.count[0]; R.record_of = &S.recordOf[0]; R.record_iteration = &S.recordIteration[0]; R.refined_count = &S.refinedCount[0];
            R.r = &S.r[0]; R.t = &S.t[0]; R.refined_tcw = &S.refinedTcw[0];
        }
        if (n) R.inliers_first = &S.inliersFirst[0];
        R.first_event = &first[c];
        R.nrecords = &nrec[c];
        if (n > maxN) maxN = n;
        if (its > maxIt) maxIt = its;
    }
    ThreadSolver &T = tSolver;
    if (!T.h || T.candidates < C || T.matches < maxN || T.iterations < maxIt) {
        if (T.h) orbx_pnp_solver_destroy(T.h);
        T.h = 0;
        int capC = 8, capN = 2048;
        while (capC < C) capC *= 2;
        while (capN < maxN) capN *= 2;
        if (capN > ORBX_PNP_MAX_MATCHES) capN = ORBX_PNP_MAX_MATCHES;
        const int capI = maxIt > 320 ? maxIt + 64 : 320;
        if (orbx_pnp_solver_create(orbx_shim::Device(), capC, capN, capI, &T.h) != ORBX_OK) { T.h = 0; return orbx_shim::Fail("PnPsolver::iterate"); }
        T.candidates = capC; T.matches = capN; T.iterations = capI;
    }
    __sync_fetch_and_add(&gPnPCalls, 1ul);
    __sync_fetch_and_add(&gPnPSolvers, (unsigned long)C);
    T.generation++;
    if (orbx_pnp_solve(T.h, &probs[0], C, &results[0]) != ORBX_OK) return orbx_shim::Fail("PnPsolver::iterate");
    for (int c = 0; c < C; c++) {
        states[c]->solved = true; states[c]->generation = T.generation; states[c]->candidate = c; states[c]->firstEvent = first[c]; states[c]->nrecords = nrec[c];
    }
    return true;
}
}  // namespace

// PnPsolver's members are private (Sim3Solver's are protected, so its shim reads them through a derived type): SolveAll asks each solver for
// its entry through a probing iterate call, which reports them and runs nothing.
namespace
{
thread_local Entry *tEntryOut = 0;      // set by SolveAll around a probing iterate(0) call
}

PnPsolver::PnPsolver(const Frame &F, const vector<MapPoint *> &vpMapPointMatches)
    : pws(0), us(0), alphas(0), pcs(0), maximum_number_of_correspondences(0), number_of_correspondences(0), mnInliersi(0), mnIterations(0), mnBestInliers(0), N(0)
{
    mvpMapPointMatches = vpMapPointMatches;
    mvP2D.reserve(F.mvpMapPoints.size());
    mvSigma2.reserve(F.mvpMapPoints.size());
    mvP3Dw.reserve(F.mvpMapPoints.size());
    mvKeyPointIndices.reserve(F.mvpMapPoints.size());
    mvAllIndices.reserve(F.mvpMapPoints.size());

    PnPState &S = StateOf(this);
    S = PnPState();      // an earlier solver at this address
    int idx = 0;
    for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
        MapPoint *pMP = vpMapPointMatches[i];
        if (!pMP) continue;
        if (pMP->isBad()) continue;
        const cv::KeyPoint &kp = F.mvKeysUn[i];
        mvP2D.push_back(kp.pt);
        mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
        cv::Mat Pos = pMP->GetWorldPos();
        mvP3Dw.push_back(cv::Point3f(Pos.at<float>(0), Pos.at<float>(1), Pos.at<float>(2)));
        mvKeyPointIndices.push_back(i);
        mvAllIndices.push_back(idx);
        S.p2d.push_back(kp.pt.x); S.p2d.push_back(kp.pt.y);
        S.sigma2.push_back(F.mvLevelSigma2[kp.octave]);
        for (int c = 0; c < 3; c++) S.p3d.push_back(Pos.at<float>(c));
        idx++;
    }
    fu = F.fx;
    fv = F.fy;
    uc = F.cx;
    vc = F.cy;
    SetRansacParameters();
}

PnPsolver::~PnPsolver()
{
    delete[] pws;
    delete[] us;
    delete[] alphas;
    delete[] pcs;
    orbx_shim::Release(this);
}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2)
{
    mRansacProb = probability;
    mRansacMinSet = minSet;
    N = mvP2D.size();
    mvbInliersi.resize(N);
    int adjusted = minInliers, its = 1;
    float eps = epsilon;
    orbx_pnp_ransac_parameters(probability, minInliers, maxIterations, minSet, epsilon, th2, N, &adjusted, &its, &eps);
    mRansacMinInliers = adjusted;
    mRansacEpsilon = eps;
    mRansacMaxIts = its;
    mvMaxError.resize(mvSigma2.size());
    for (size_t i = 0; i < mvSigma2.size(); i++) mvMaxError[i] = mvSigma2[i] * th2;      // (the device forms its own from sigma2 and th2)
    PnPState &S = StateOf(this);
    S.probability = probability; S.minInliers = minInliers; S.maxIterations = maxIterations; S.minSet = minSet; S.epsilon = epsilon; S.th2 = th2;
    S.solved = false;      // minInliers decides the records and the events, mRansacMaxIts the sets
    S.sets.clear();
}

cv::Mat PnPsolver::find(vector<bool> &vbInliers, int &nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
}

cv::Mat PnPsolver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    if (tEntryOut) {      // SolveAll's probe: hand out what only a member function can read, run nothing
        Entry &E = *tEntryOut;
        E.solver = this; E.n = N; E.maxIts = mRansacMaxIts; E.minInliers = mRansacMinInliers;
        E.fx = (float)fu; E.fy = (float)fv; E.cx = (float)uc; E.cy = (float)vc;
        return cv::Mat();
    }
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    if (N < mRansacMinInliers) {
        bNoMore = true;
        return cv::Mat();
    }
    PnPState &S = StateOf(this);
    Entry self;
    self.solver = this; self.n = N; self.maxIts = mRansacMaxIts; self.minInliers = mRansacMinInliers;
    self.fx = (float)fu; self.fy = (float)fv; self.cx = (float)uc; self.cy = (float)vc;
    const std::vector<Entry> alone(1, self);
    // one row of the device's masks into mvbInliersi and vbInliers; a solver whose masks another call has overwritten is solved again first
    struct Rows {
        static bool Read(PnPsolver *, PnPState &S, const std::vector<Entry> &alone, int index, int refined, std::vector<uint8_t> &row, int n)
        {
            if (S.generation != tSolver.generation && !SolveList(alone, S.iterations)) return false;
            row.resize(n);
            if (orbx_pnp_inliers(tSolver.h, S.candidate, index, refined, &row[0]) != ORBX_OK) return orbx_shim::Fail("PnPsolver::iterate");
            return true;
        }
    };
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {      // :266, an OR
        nCurrentIterations++;
        const int it = mnIterations++;
        if (!S.solved || it >= S.iterations) {
            // further sets for the iterations this call can still run, solved by a further device call
            const int want = it + 1 + (nIterations > nCurrentIterations ? nIterations - nCurrentIterations : 0);
            if (!SolveList(alone, want)) { bNoMore = true; return cv::Mat(); }
        }
        mnInliersi = S.count[it];
        if (mnInliersi < mRansacMinInliers) continue;
        const int rec = S.recordOf[it];
        if (mnInliersi > mnBestInliers) {      // :305-317; mvbBestInliers is only read on a return: filled there
            mnBestInliers = mnInliersi;
            mBestTcw = cv::Mat::eye(4, 4, CV_32F);
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) { mRi[i][j] = S.r[9 * it + 3 * i + j]; mBestTcw.at<float>(i, j) = (float)mRi[i][j]; }
                mti[i] = S.t[3 * it + i];
                mBestTcw.at<float>(i, 3) = (float)mti[i];
            }
        }
        if (rec < 0 || S.refinedCount[rec] <= mRansacMinInliers) continue;      // Refine (:366-418) of the running best failed
        std::vector<uint8_t> row;
        const uint8_t *inl = 0;
        if (it == S.firstEvent) inl = N ? &S.inliersFirst[0] : 0;
        else {
            if (!Rows::Read(this, S, alone, rec, 1, row, N)) { bNoMore = true; return cv::Mat(); }
            inl = &row[0];
        }
        mnRefinedInliers = S.refinedCount[rec];
        nInliers = mnRefinedInliers;
        vbInliers = vector<bool>(mvpMapPointMatches.size(), false);
        mvbRefinedInliers.resize(N);
        for (int i = 0; i < N; i++) {
            mvbRefinedInliers[i] = inl[i] != 0;
            if (inl[i]) vbInliers[mvKeyPointIndices[i]] = true;
        }
        mRefinedTcw = cv::Mat::eye(4, 4, CV_32F);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 4; j++) mRefinedTcw.at<float>(i, j) = S.refinedTcw[12 * rec + 4 * i + j];
        return mRefinedTcw.clone();
    }
    if (mnIterations >= mRansacMaxIts) {
        bNoMore = true;
        if (mnBestInliers >= mRansacMinInliers) {
            const int rec = S.recordOf[mnIterations - 1];
            std::vector<uint8_t> row;
            if (rec < 0 || !Rows::Read(this, S, alone, S.recordIteration[rec], 0, row, N)) return cv::Mat();
            nInliers = mnBestInliers;
            vbInliers = vector<bool>(mvpMapPointMatches.size(), false);
            mvbBestInliers.resize(N);
            for (int i = 0; i < N; i++) {
                mvbBestInliers[i] = row[i] != 0;
                if (row[i]) vbInliers[mvKeyPointIndices[i]] = true;
            }
            return mBestTcw.clone();
        }
    }
    return cv::Mat();
}
}  // namespace ORB_SLAM2

namespace orbx_shim
{
bool SolveAll(const std::vector<ORB_SLAM2::PnPsolver *> &solvers)
{
    std::vector<ORB_SLAM2::Entry> todo;
    for (size_t i = 0; i < solvers.size(); i++) {
        if (!solvers[i] || ORB_SLAM2::StateOf(solvers[i]).solved) continue;
        ORB_SLAM2::Entry E;
        bool flag;
        std::vector<bool> none;
        int k;
        ORB_SLAM2::tEntryOut = &E;      // PnPsolver's members are private: the solver reports them itself
        solvers[i]->iterate(0, flag, none, k);
        ORB_SLAM2::tEntryOut = 0;
        todo.push_back(E);
    }
    return ORB_SLAM2::SolveList(todo);
}

void Release(ORB_SLAM2::PnPsolver *solver)
{
    std::lock_guard<std::mutex> lock(ORB_SLAM2::gTableMutex);
    ORB_SLAM2::gTable.erase(solver);
}
}  // namespace orbx_shim
