// shim/Relocalization_hip.h -- device bodies for the head (src/Tracking.cc:2063-2095) and the refine loop (:2135-2223) of Tracking::Relocalization.
//
// The head - SearchByBoW against every candidate keyframe, the < 15 decision, the arrays each PnPsolver collects - is ONE call:
//
//     std::vector<ORB_SLAM2::RelocPnPProblem> problems;                   // per candidate: mvKeyPointIndices, mvP2D, mvSigma2, mvP3Dw
//     int nCandidates = ORB_SLAM2::RelocalizationMatchHIP(mCurrentFrame, vpCandidateKFs, vvpMapPointMatches, vbDiscarded, problems);   // replaces :2063-2095
//     for (int i = 0; i < nKFs; i++)                                      // the solvers, from the rows the call left (or from problems[i] directly)
//         if (!vbDiscarded[i]) { vpPnPsolvers[i] = new PnPsolver(mCurrentFrame, vvpMapPointMatches[i]); vpPnPsolvers[i]->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991); }
//
// Tracking.cc itself is outside this repository's scope; this is the binding a maintainer adds to it.  The round-robin loop
// (:2105-2226) keeps asking its solvers for poses; what it does with each pose - seed mvpMapPoints, PoseOptimization, two SearchByProjection calls, two
// more PoseOptimization calls - depends only on the pose, so the poses are collected first and refined together:
//
//     std::vector<ORB_SLAM2::RelocHypothesis> hyps;                       // the DISTINCT poses, in order of first appearance
//     std::vector<int> sequence;                                          // every returned pose as an index into hyps
//     while (nCandidates > 0) {                                           // :2105, without `&& !bMatch`
//         for (int i = 0; i < nKFs; i++) {
//             if (vbDiscarded[i]) continue;
//             ...
//             cv::Mat Tcw = vpPnPsolvers[i]->iterate(5, bNoMore, vbInliers, nInliers);                      // :2124, unchanged
//             if (bNoMore) { vbDiscarded[i] = true; nCandidates--; }                                        // :2128-2132, unchanged
//             if (!Tcw.empty()) sequence.push_back(ORB_SLAM2::AddRelocHypothesis(hyps, i, Tcw, vbInliers));
//         }
//     }
//     int winner = -1;                                                    // the candidate of the first pose that is accepted, :2218
//     bMatch = ORB_SLAM2::RelocalizationRefineHIP(mCurrentFrame, vpCandidateKFs, vvpMapPointMatches, hyps, sequence, winner);
//
// Each function makes ONE gather over the real KeyFrame / MapPoint objects (shim/MapPointAccess.h: one visit per point), ONE device call with one host
// wait (orbx_reloc_match_candidates; orbx_relocalize_refine: every hypothesis through the whole loop as one launch chain) and the write-back the reference's lines do: mTcw,
// mvpMapPoints, mvbOutlier - of the accepted pose, or, when none is accepted, of the last one (what the reference leaves in mCurrentFrame).
// The identity of a map point is its slot in the keyframe (a MapPoint held by two slots of one keyframe counts as two points for sFound).
// Errors follow shim/shim_error.h: reported, counted, and the reference's "nothing found" value is returned (false).
// Not linked into the drop-in library of oracle/: switching its Tracking over is a later step.
#ifndef ORBX_SHIM_RELOCALIZATION_HIP_H
#define ORBX_SHIM_RELOCALIZATION_HIP_H

#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"

namespace ORB_SLAM2
{
struct RelocHypothesis {
    int candidate;                  // index into vpCandidateKFs
    cv::Mat Tcw;                    // 4x4 CV_32F as PnPsolver::iterate returned it
    std::vector<bool> vbInliers;    // over the frame's features
};
// What the PnPsolver constructor collects for one candidate (src/PnPsolver.cc:136-158), in the layout of orbx_pnp_problem; empty for a discarded candidate
struct RelocPnPProblem {
    std::vector<int> keyIndex;      // mvKeyPointIndices
    std::vector<float> p2d, sigma2, p3dw;      // [n][2], [n], [n][3]
};
// :2063-2095 without the `new PnPsolver`: vvpMapPointMatches[i] as SearchByBoW(vpCandidateKFs[i], F, ..) leaves it (untouched for a bad keyframe),
// vbDiscarded[i] (bad, or fewer than 15 matches), problems[i].  F.mBowVec / mFeatVec are computed (:2032).  Returns nCandidates.
int RelocalizationMatchHIP(Frame &F, const std::vector<KeyFrame *> &vpCandidateKFs, std::vector<std::vector<MapPoint *> > &vvpMapPointMatches, std::vector<bool> &vbDiscarded,
                           std::vector<RelocPnPProblem> &problems, float nnratio = 0.75f, bool checkOrientation = true);
// The index of (candidate, Tcw, vbInliers) in hyps, appended when no equal entry is there (a record returned by several iterate calls is refined once).
int AddRelocHypothesis(std::vector<RelocHypothesis> &hyps, int candidate, const cv::Mat &Tcw, const std::vector<bool> &vbInliers);
// :2135-2223 for every entry of `sequence`.  true = a pose was accepted (bMatch); winnerCandidate = its candidate, or -1.
bool RelocalizationRefineHIP(Frame &CurrentFrame, const std::vector<KeyFrame *> &vpCandidateKFs, const std::vector<std::vector<MapPoint *> > &vvpMapPointMatches,
                             const std::vector<RelocHypothesis> &hyps, const std::vector<int> &sequence, int &winnerCandidate, bool checkOrientation = true);
}

#endif
