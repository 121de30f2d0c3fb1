// shim/KeyFrameDatabase_hip.cc -- KeyFrameDatabase::add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates
// (src/KeyFrameDatabase.cc:53-374) and the minimum-score loop of LoopClosing::DetectLoop (src/LoopClosing.cc:160-176) over orbx_kfdb_*.
//
// Compiled against the REFERENCE's own headers, like the other shim files.  A file of its own: the drop-in library of oracle/Makefile does not
// link it; it is compile-checked only.
//
// What stays on the host is the pointer bookkeeping: a map mnId -> KeyFrame* of the keyframes in the database, the flattening of mBowVec (a
// std::map: ascending word ids) and of GetConnectedKeyFrames() (isBad() ones with count 0: they stay out of the sharers as the reference's set keeps
// them out, and out of the minimum score), and the write-back of mnLoopQuery / mnLoopWords / mLoopScore (mnRelocQuery / mnRelocWords / mRelocScore)
// for the keyframes the query scored.  The device keeps GetBestCovisibilityKeyFrames(10) of a keyframe as pushed by add() and RefreshCovisibles():
// a query reads the covisibles as last pushed, not as of the query (PARITY UNPINNED, like mRelocScore of a keyframe that no query has scored).
// On a device error (counted, std::cerr: shim_error.h) a query returns no candidates and touches nothing.
#include <algorithm>
#include <vector>

#include "KeyFrame.h"
#include "Frame.h"
#include "ORBVocabulary.h"
#include "orbx.h"
#include "shim_error.h"
#include "KeyFrameDatabase_hip.h"

namespace
{
void Flatten(const DBoW2::BowVector &bow, std::vector<int32_t> &words, std::vector<double> &values)
{
    words.clear();
    values.clear();
    for (DBoW2::BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) {      // map order: ascending word id
        words.push_back((int32_t)it->first);
        values.push_back((double)it->second);
    }
}
}  // namespace

namespace ORB_SLAM2
{
KeyFrameDatabase_hip::KeyFrameDatabase_hip(const ORBVocabulary &voc, int max_keyframes, int max_entries) : mpVoc(&voc), mpDb(0)
{
    if (orbx_kfdb_create(orbx_shim::Device(), (int)voc.size(), max_keyframes, max_entries, 1, ORBX_KFDB_MAX_QUERY_WORDS, &mpDb) != ORBX_OK) {
        mpDb = 0;
        orbx_shim::Fail("KeyFrameDatabase");
    }
}

KeyFrameDatabase_hip::~KeyFrameDatabase_hip()
{
    if (mpDb) orbx_kfdb_destroy(mpDb);
}

void KeyFrameDatabase_hip::add(KeyFrame *pKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpDb) return;
    std::vector<int32_t> words;
    std::vector<double> values;
    Flatten(pKF->mBowVec, words, values);
    if (orbx_kfdb_add(mpDb, (int64_t)pKF->mnId, words.data(), values.data(), (int)words.size()) != ORBX_OK) { orbx_shim::Fail("KeyFrameDatabase::add"); return; }
    mmKeyFrames[pKF->mnId] = pKF;
    lock.unlock();
    RefreshCovisibles(pKF);
}

void KeyFrameDatabase_hip::RefreshCovisibles(KeyFrame *pKF)
{
    const std::vector<KeyFrame *> vpNeighs = pKF->GetBestCovisibilityKeyFrames(10);
    std::vector<int64_t> ids;
    for (size_t i = 0; i < vpNeighs.size() && i < 10; i++) ids.push_back((int64_t)vpNeighs[i]->mnId);
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpDb || !mmKeyFrames.count(pKF->mnId)) return;
    if (orbx_kfdb_set_covisibles(mpDb, (int64_t)pKF->mnId, ids.data(), (int)ids.size()) != ORBX_OK) orbx_shim::Fail("KeyFrameDatabase::RefreshCovisibles");
}

void KeyFrameDatabase_hip::erase(KeyFrame *pKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpDb) return;
    if (orbx_kfdb_erase(mpDb, (int64_t)pKF->mnId) != ORBX_OK) { orbx_shim::Fail("KeyFrameDatabase::erase"); return; }
    mmKeyFrames.erase(pKF->mnId);
}

void KeyFrameDatabase_hip::clear()
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpDb) return;
    if (orbx_kfdb_clear(mpDb) != ORBX_OK) { orbx_shim::Fail("KeyFrameDatabase::clear"); return; }
    mmKeyFrames.clear();
}

// one query; pKF != 0: loop mode with pKF's connected keyframes
bool KeyFrameDatabase_hip::Query(int mode, const DBoW2::BowVector &bow, KeyFrame *pKF, float minScoreIn, bool minScoreOnly, float *minScoreOut,
                                 unsigned long queryId, std::vector<KeyFrame *> *out)
{
    std::vector<int32_t> words;
    std::vector<double> values;
    Flatten(bow, words, values);
    std::vector<int64_t> connected;
    std::vector<int32_t> counts;
    if (pKF) {
        const std::set<KeyFrame *> spConnected = pKF->GetConnectedKeyFrames();
        for (std::set<KeyFrame *>::const_iterator it = spConnected.begin(); it != spConnected.end(); ++it) {
            connected.push_back((int64_t)(*it)->mnId);
            counts.push_back((*it)->isBad() ? 0 : std::max(1, pKF->GetWeight(*it)));
        }
    }
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpDb) return false;
    const int cap = (int)mmKeyFrames.size();
    std::vector<int64_t> scoredId((size_t)cap + 1), candidates((size_t)cap + 1);
    std::vector<int32_t> scoredWords((size_t)cap + 1);
    std::vector<float> scoredScore((size_t)cap + 1);
    int32_t nScored = 0, nCandidates = 0;
    float minScore = 0.f;
    orbx_kfdb_query_t Q;
    Q.mode = mode; Q.words = words.data(); Q.values = values.data(); Q.n = (int)words.size();
    Q.connected = connected.data(); Q.connected_counts = counts.data(); Q.n_connected = (int)connected.size();
    Q.min_score_in = minScoreIn; Q.capacity = cap;
    orbx_kfdb_result R;
    memset(&R, 0, sizeof(R));
    R.min_score = &minScore;
    if (!minScoreOnly) {
        R.scored_id = scoredId.data(); R.scored_words = scoredWords.data(); R.scored_score = scoredScore.data(); R.n_scored = &nScored;
        R.candidates = candidates.data(); R.n_candidates = &nCandidates;
    }
    if (orbx_kfdb_query(mpDb, &Q, 1, &R) != ORBX_OK) return orbx_shim::Fail(pKF ? "KeyFrameDatabase::DetectLoopCandidates" : "KeyFrameDatabase::DetectRelocalizationCandidates");
    if (minScoreOut) *minScoreOut = minScore;
    for (int i = 0; i < nScored; i++) {      // what the reference leaves behind in the keyframes it scored
        KeyFrame *pKFi = mmKeyFrames[(long unsigned int)scoredId[i]];
        if (mode == ORBX_KFDB_LOOP) { pKFi->mnLoopQuery = queryId; pKFi->mnLoopWords = scoredWords[i]; pKFi->mLoopScore = scoredScore[i]; }
        else { pKFi->mnRelocQuery = queryId; pKFi->mnRelocWords = scoredWords[i]; pKFi->mRelocScore = scoredScore[i]; }
    }
    if (out) {
        out->reserve((size_t)nCandidates);
        for (int i = 0; i < nCandidates; i++) out->push_back(mmKeyFrames[(long unsigned int)candidates[i]]);
    }
    return true;
}

std::vector<KeyFrame *> KeyFrameDatabase_hip::DetectLoopCandidates(KeyFrame *pKF, float minScore)
{
    std::vector<KeyFrame *> vpLoopCandidates;
    Query(ORBX_KFDB_LOOP, pKF->mBowVec, pKF, minScore, false, 0, pKF->mnId, &vpLoopCandidates);
    return vpLoopCandidates;
}

std::vector<KeyFrame *> KeyFrameDatabase_hip::DetectRelocalizationCandidates(Frame *F)
{
    std::vector<KeyFrame *> vpRelocCandidates;
    Query(ORBX_KFDB_RELOC, F->mBowVec, 0, 0.f, false, 0, F->mnId, &vpRelocCandidates);
    return vpRelocCandidates;
}

float KeyFrameDatabase_hip::DetectLoopMinScore(KeyFrame *pKF)
{
    // the connected keyframes that LoopClosing has not added to the database yet are scored on the host (a handful), the rest on the device
    float minScore = 1;
    {
        const std::vector<KeyFrame *> vpConnectedKeyFrames = pKF->GetVectorCovisibleKeyFrames();
        std::unique_lock<std::mutex> lock(mMutex);
        for (size_t i = 0; i < vpConnectedKeyFrames.size(); i++) {
            KeyFrame *pKFi = vpConnectedKeyFrames[i];
            if (pKFi->isBad() || mmKeyFrames.count(pKFi->mnId)) continue;
            const float score = mpVoc->score(pKF->mBowVec, pKFi->mBowVec);
            if (score < minScore) minScore = score;
        }
    }
    float out = minScore;
    if (!Query(ORBX_KFDB_LOOP, pKF->mBowVec, pKF, minScore, true, &out, pKF->mnId, 0)) return minScore;
    return out;
}
}  // namespace ORB_SLAM2
