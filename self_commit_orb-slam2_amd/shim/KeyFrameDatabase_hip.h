// shim/KeyFrameDatabase_hip.h -- KeyFrameDatabase on the device (shim/KeyFrameDatabase_hip.cc).
#ifndef ORBX_SHIM_KEYFRAMEDATABASE_HIP_H
#define ORBX_SHIM_KEYFRAMEDATABASE_HIP_H

#include <map>
#include <mutex>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "ORBVocabulary.h"
#include "orbx.h"

namespace ORB_SLAM2
{
// KeyFrameDatabase's surface (include/KeyFrameDatabase.h:53-85) over orbx_kfdb_*: mnId is the id, mBowVec is flattened in map order, the
// candidates come back as the reference's pointers in the reference's order, and the scored keyframes get mnLoopQuery / mnLoopWords /
// mLoopScore (mnRelocQuery / mnRelocWords / mRelocScore) written back.  A class of its own: the drop-in library keeps the reference's
// KeyFrameDatabase, and a build that wants this one forwards to it.  On a device error (shim_error.h) a query returns no candidates.
class KeyFrameDatabase_hip
{
public:
    // max_keyframes / max_entries size the device pool (entries: the sum of the BowVector lengths of the keyframes held at one time)
    KeyFrameDatabase_hip(const ORBVocabulary &voc, int max_keyframes = 20000, int max_entries = 20000 * 1200);
    ~KeyFrameDatabase_hip();

    void add(KeyFrame *pKF);       // pushes GetBestCovisibilityKeyFrames(10) of pKF with it
    void erase(KeyFrame *pKF);
    void clear();
    // KeyFrame::UpdateConnections / UpdateBestCovisibles changed pKF's covisibles: push them again (a query reads them as last pushed)
    void RefreshCovisibles(KeyFrame *pKF);

    std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame *pKF, float minScore);
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *F);
    // LoopClosing.cc:160-176: the lowest score of pKF to a connected keyframe that is not bad (1 without one); no candidates are computed
    float DetectLoopMinScore(KeyFrame *pKF);

private:
    bool Query(int mode, const DBoW2::BowVector &bow, KeyFrame *pKF, float minScoreIn, bool minScoreOnly, float *minScoreOut, unsigned long queryId,
               std::vector<KeyFrame *> *out);
    const ORBVocabulary *mpVoc;
    orbx_kf_database *mpDb;
    std::map<long unsigned int, KeyFrame *> mmKeyFrames;      // the keyframes in the database by mnId
    std::mutex mMutex;
};
}  // namespace ORB_SLAM2

#endif
