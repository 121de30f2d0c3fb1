// shim/ComputeSim3_hip.h -- device body for the refine step of LoopClosing::ComputeSim3 (src/LoopClosing.cc:435-480), every Sim3Solver event at once.
//
// LoopClosing.cc itself is outside this repository's scope; this is the binding a maintainer adds to it.  The round-robin loop
// (:403-482) keeps asking its solvers for estimates; what it does with each one - seed vpMapPointMatches, SearchBySim3, OptimizeSim3, nInliers >= 20 -
// depends only on the estimate, so the events are collected first and refined together:
//
//     std::vector<ORB_SLAM2::LoopSim3Event> events;                      // in the order the loop meets them; every event once
//     while (nCandidates > 0) {                                          // :403, without `&& !bMatch`
//         for (int i = 0; i < nInitialCandidates; i++) {
//             if (vbDiscarded[i]) continue;
//             ...
//             cv::Mat Scm = vpSim3Solvers[i]->iterate(5, bNoMore, vbInliers, nInliers);                    // :423, unchanged
//             if (bNoMore) { vbDiscarded[i] = true; nCandidates--; }                                       // :428-432, unchanged
//             if (!Scm.empty()) events.push_back(ORB_SLAM2::LoopSim3Event(i, vpSim3Solvers[i], vbInliers));
//         }
//     }
//     int matched = -1;
//     bMatch = ORB_SLAM2::ComputeSim3Device(mpCurrentKF, mvpEnoughConsistentCandidates, vvpMapPointMatches, events, mbFixScale, matched, mg2oScw, mScw,
//                                           mvpCurrentMatchedPoints);
//     if (bMatch) mpMatchedKF = mvpEnoughConsistentCandidates[matched];
//
// ONE gather over the real KeyFrame / MapPoint objects (shim/KeyFrameArrays.h with the points' distance range and descriptor: one visit per point), ONE
// device call with one host wait per ORBX_LOOP_SIM3_MAX_HYPOTHESES (64) events (orbx_loop_refine_sim3: every event through SearchBySim3, OptimizeSim3
// and the decision as one launch chain) - the events go in walk order, 64 at a time, and the calls stop at the first accepted one - and the write-back
// of :465-474.
// The identity of a map point is its slot in the keyframe (the same MapPoint in two slots of one keyframe counts as two points).
// Errors follow shim/shim_error.h: reported, counted (orbx_shim::Fail), and false is returned - also for an event that gathers more than 1024 pairs ahead of any
// accepted one (ORBX_ERR_CAPACITY): that is an error in the count, not the reference's "nothing found".
// Not linked into the drop-in library of oracle/: switching its LoopClosing over is a later step.
#ifndef ORBX_SHIM_COMPUTE_SIM3_HIP_H
#define ORBX_SHIM_COMPUTE_SIM3_HIP_H

#include <vector>

#include "KeyFrame.h"
#include "LoopClosing.h"
#include "MapPoint.h"
#include "Sim3Solver.h"

namespace ORB_SLAM2
{
struct LoopSim3Event {
    int candidate;                  // index into the candidate keyframes
    cv::Mat R12, t12;               // GetEstimatedRotation / GetEstimatedTranslation when iterate returned (3x3, 3x1 CV_32F)
    float s12;                      // GetEstimatedScale
    std::vector<bool> vbInliers;    // over the current keyframe's features
    LoopSim3Event() : candidate(-1), s12(1.f) {}
    LoopSim3Event(int c, Sim3Solver *pSolver, const std::vector<bool> &inl)
        : candidate(c), R12(pSolver->GetEstimatedRotation().clone()), t12(pSolver->GetEstimatedTranslation().clone()), s12(pSolver->GetEstimatedScale()), vbInliers(inl) {}
};
// :435-480 for every event, in order.  true = an event was accepted (bMatch): matchedCandidate, g2oScw (mg2oScw), Scw (mScw) and vpCurrentMatchedPoints
// (mvpCurrentMatchedPoints) are those of the first accepted event; otherwise they are left as they were.
bool ComputeSim3Device(KeyFrame *pCurrentKF, const std::vector<KeyFrame *> &vpCandidates, const std::vector<std::vector<MapPoint *> > &vvpMapPointMatches,
                       const std::vector<LoopSim3Event> &events, bool bFixScale, int &matchedCandidate, g2o::Sim3 &g2oScw, cv::Mat &Scw,
                       std::vector<MapPoint *> &vpCurrentMatchedPoints);
}

#endif
