// shim/Tracking_hip.h -- device bodies for Tracking::TrackWithMotionModel (src/Tracking.cc:1353-1431), Tracking::TrackLocalMap (:1443-1503) and
// Tracking::TrackReferenceKeyFrame (:1181-1239).
//
// Tracking.cc itself is outside this repository's scope; this is the binding a maintainer adds to it:
//
//     bool Tracking::TrackWithMotionModel()
//     {
//         UpdateLastFrame();                                              // :1365, unchanged
//         mCurrentFrame.SetPose(mVelocity * mLastFrame.mTcw);             // :1368, unchanged
//         const int th = mSensor != System::STEREO ? 15 : 7;              // :1374-1378
//         int nmatches = 0, nmatchesMap = 0;
//         if (!ORB_SLAM2::TrackWithMotionModelHIP(mCurrentFrame, mLastFrame, th, mSensor == System::MONOCULAR, nmatches, nmatchesMap))
//             return false;                                               // :1393
//         if (mbOnlyTracking) { mbVO = nmatchesMap < 10; return nmatches > 20; }   // :1423-1430, unchanged
//         return nmatchesMap >= 10;
//     }
//
//     bool Tracking::TrackLocalMap()
//     {
//         UpdateLocalMap();                                               // :1450, unchanged
//         int th = 1;                                                     // :1818-1825 (SearchLocalPoints' own choice)
//         if (mSensor == System::RGBD) th = 3;
//         if (mCurrentFrame.mnId < mnLastRelocFrameId + 2) th = 5;
//         mnMatchesInliers = ORB_SLAM2::TrackLocalMapHIP(mCurrentFrame, mvpLocalMapPoints, th, mSensor == System::STEREO, mbOnlyTracking);
//         ...                                                             // :1495-1502, unchanged
//     }
//
//     bool Tracking::TrackReferenceKeyFrame()
//     {
//         mCurrentFrame.ComputeBoW();                                     // :1185, unchanged
//         int nmatches = 0, nmatchesMap = 0;
//         if (!ORB_SLAM2::TrackReferenceKeyFrameHIP(mCurrentFrame, mpReferenceKF, mLastFrame.mTcw, nmatches, nmatchesMap))
//             return false;                                               // :1201
//         return nmatchesMap >= 10;                                       // :1238, unchanged
//     }
//
// Each function makes ONE gather over the real Frame / MapPoint objects (shim/MapPointAccess.h: one visit per point), ONE device call with one
// host wait (orbx_track_with_motion_model / orbx_track_local_map / orbx_track_reference_keyframe: search, pose optimisation and the outlier pass as one launch chain) and the
// write-back the reference's lines do: mvpMapPoints, mvbOutlier, SetPose, mbTrackInView, mnLastFrameSeen, IncreaseFound, the mTrack* fields.
// Errors follow shim/shim_error.h: reported, counted, and the reference's "nothing found" value is returned (false / 0).
// Not linked into the drop-in library of oracle/: switching its Tracking over is a later step.
#ifndef ORBX_SHIM_TRACKING_HIP_H
#define ORBX_SHIM_TRACKING_HIP_H

#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"

namespace ORB_SLAM2
{
// :1370-1421.  CurrentFrame.mTcw is the predicted pose on entry.  false = fewer than 20 matches after both searches (:1393).
bool TrackWithMotionModelHIP(Frame &CurrentFrame, const Frame &LastFrame, int th, bool bMono, int &nmatches, int &nmatchesMap, bool checkOrientation = true);
// :1454-1489 (SearchLocalPoints, PoseOptimization, the statistics loop).  Returns mnMatchesInliers.
// :1189-1236.  TcwInit = the pose handed to SetPose (:1206, mLastFrame.mTcw); F.mBowVec / mFeatVec are computed (:1185).  false = the search found fewer
// than 15 matches (:1201): F.mvpMapPoints and F.mTcw are left as they were, as the reference leaves them.
bool TrackReferenceKeyFrameHIP(Frame &F, KeyFrame *pKF, const cv::Mat &TcwInit, int &nmatches, int &nmatchesMap, float nnratio = 0.7f, bool checkOrientation = true);
int TrackLocalMapHIP(Frame &F, const std::vector<MapPoint *> &vpLocalMapPoints, int th, bool bStereo, bool bOnlyTracking, float nnratio = 0.8f, float viewingCosLimit = 0.5f);
}

#endif
