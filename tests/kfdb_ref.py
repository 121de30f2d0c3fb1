"""A literal restatement of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cc:53-374), of L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) and of the minimum-score loop of LoopClosing::DetectLoop (src/LoopClosing.cc:160-176).

It is written from the reference's text line by line: an inverted file of lists per word walked in the query's word order, keyframe objects with the
persistent members mnLoopQuery / mnLoopWords / mLoopScore and the Reloc three, np.float32 wherever the reference computes in float, and the score as a
sequential Python-float loop over the two merged iterators.  It does NOT know the (first shared word, add sequence) key of csrc/orbx_kfdb.hip:
tests/test_kfdb.py proves that key against the order this walk produces.

Where the restatement has to decide what the reference leaves open:
  * mRelocScore starts at 0 (uninitialised in the reference: parity is not defined there);
  * mnLoopQuery / mnRelocQuery start at -1 and every query carries a fresh id (the reference starts them at 0, which keyframe 0's own query would match);
  * a keyframe that is erased and added again is a new object;
  * a covisible id that names no keyframe of the database is skipped (the reference's object would carry another query's mark);
  * `batch` mode (query_batch): every relocalisation query of a call starts from the mRelocScore values of before the call, and after the call a keyframe
    holds the score of the highest-numbered query that scored it.  With one query this is the reference exactly.
The scene generator at the end draws keyframes of P places over n_words words.
"""
import bisect

import numpy as np

f32 = np.float32
LOOP, RELOC = 0, 1


def l1_score(v1, v2):
    """L1Scoring::score(v1, v2): v1, v2 lists of (word, value) in ascending word order (a std::map's order) -> Python float (double)"""
    k1 = [w for w, _ in v1]
    k2 = [w for w, _ in v2]
    i1, i2 = 0, 0
    score = 0.0
    while i1 != len(v1) and i2 != len(v2):
        vi = v1[i1][1]
        wi = v2[i2][1]
        if v1[i1][0] == v2[i2][0]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i1 += 1
            i2 += 1
        elif v1[i1][0] < v2[i2][0]:
            i1 = bisect.bisect_left(k1, v2[i2][0])      # v1.lower_bound(v2_it->first)
        else:
            i2 = bisect.bisect_left(k2, v1[i1][0])
    score = -score / 2.0
    return score


class KeyFrame:
    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = bow                   # [(word, value)] ascending
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = -1, 0, f32(0)
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = -1, 0, f32(0)
        self.covisibles = []                 # ids, GetBestCovisibilityKeyFrames(10) order, as last pushed


def as_bow(words, values):
    return [(int(w), float(v)) for w, v in zip(words, values)]


class KeyFrameDatabaseRef:
    def __init__(self, n_words):
        self.n_words = n_words
        self.mvInvertedFile = {}             # word -> list of keyframes in insertion order (the vector of lists, sparse)
        self.kfs = {}                        # id -> KeyFrame, the keyframes in the database
        self.next_query = 1 << 40            # fresh query ids
        self.stale_reads = 0                 # instrumentation: relocalisation neighbours read although this query did not score them, value != 0

    def __len__(self):
        return len(self.kfs)

    # ---- :53-91
    def add(self, mnId, words, values):
        assert mnId not in self.kfs
        pKF = KeyFrame(mnId, as_bow(words, values))
        self.kfs[mnId] = pKF
        for w, _ in pKF.mBowVec:
            self.mvInvertedFile.setdefault(w, []).append(pKF)

    def erase(self, mnId):
        pKF = self.kfs.pop(mnId, None)
        if pKF is None:
            return
        for w, _ in pKF.mBowVec:
            lKFs = self.mvInvertedFile[w]
            for i, kf in enumerate(lKFs):
                if kf is pKF:
                    del lKFs[i]
                    break

    def clear(self):
        self.mvInvertedFile = {}
        self.kfs = {}

    def set_covisibles(self, mnId, ids):
        assert len(ids) <= 10
        self.kfs[mnId].covisibles = [int(i) for i in ids]

    def _neighs(self, pKFi):
        return [self.kfs[i] for i in pKFi.covisibles if i in self.kfs]

    # ---- LoopClosing.cc:160-176 over the connected keyframes the database holds
    def min_score(self, bow, connected, counts, min_score_in):
        minScore = f32(min_score_in)
        connected_score = []
        for i, c in zip(connected, counts):
            pKF = self.kfs.get(i)
            if pKF is None:
                connected_score.append(f32(-1))
                continue
            score = f32(l1_score(bow, pKF.mBowVec))
            connected_score.append(score)
            if c == 0:      # isBad()
                continue
            if score < minScore:
                minScore = score
        return minScore, np.array(connected_score, f32)

    @staticmethod
    def _result(**kw):
        r = dict(n_sharing=0, max_common_words=0, min_common_words=0, min_score=f32(0), connected_score=np.zeros(0, f32), scored_id=[], scored_words=[],
                 scored_score=[], kept=[], acc_score=[], best_id=[], best_acc_score=f32(0), candidates=[], early=None, sharing_id=[], sharing_words=[])
        r.update(kw)
        return r

    # ---- :104-239
    def DetectLoopCandidates(self, words, values, connected=(), counts=None, min_score_in=1.0):
        bow = as_bow(words, values)
        counts = [1] * len(connected) if counts is None else counts
        minScore, connected_score = self.min_score(bow, connected, counts, min_score_in)
        mnId = self.next_query
        self.next_query += 1
        spConnectedKeyFrames = set(int(i) for i in connected)
        lKFsSharingWords = []
        for w, _ in bow:
            lKFs = self.mvInvertedFile.get(w, [])
            for pKFi in lKFs:
                if pKFi.mnLoopQuery != mnId:
                    pKFi.mnLoopWords = 0
                    if pKFi.mnId not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        res = self._result(min_score=minScore, connected_score=connected_score, best_acc_score=minScore, n_sharing=len(lKFsSharingWords))
        if not lKFsSharingWords:
            res["early"] = "sharing"
            return res
        lScoreAndMatch = []
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > maxCommonWords:
                maxCommonWords = pKFi.mnLoopWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        scored = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = f32(l1_score(bow, pKFi.mBowVec))
                pKFi.mLoopScore = si
                scored.append(pKFi)
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi, len(scored) - 1))
        res.update(max_common_words=maxCommonWords, min_common_words=minCommonWords, scored_id=[k.mnId for k in scored], scored_words=[k.mnLoopWords for k in scored],
                   scored_score=[k.mLoopScore for k in scored], sharing_id=[k.mnId for k in lKFsSharingWords], sharing_words=[k.mnLoopWords for k in lKFsSharingWords])
        if not lScoreAndMatch:
            res["early"] = "score"
            return res
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi, _ in lScoreAndMatch:
            vpNeighs = self._neighs(pKFi)
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in vpNeighs:
                if pKF2.mnLoopQuery == mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = f32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpLoopCandidates = []
        for accScore, pKFi in lAccScoreAndMatch:
            if accScore > minScoreToRetain:
                if pKFi.mnId not in spAlreadyAddedKF:
                    vpLoopCandidates.append(pKFi.mnId)
                    spAlreadyAddedKF.add(pKFi.mnId)
        res.update(kept=[k for _, _, k in lScoreAndMatch], acc_score=[a for a, _ in lAccScoreAndMatch], best_id=[k.mnId for _, k in lAccScoreAndMatch],
                   best_acc_score=bestAccScore, candidates=vpLoopCandidates)
        return res

    # ---- :252-374
    def DetectRelocalizationCandidates(self, words, values):
        bow = as_bow(words, values)
        mnId = self.next_query
        self.next_query += 1
        lKFsSharingWords = []
        for w, _ in bow:
            lKFs = self.mvInvertedFile.get(w, [])
            for pKFi in lKFs:
                if pKFi.mnRelocQuery != mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        res = self._result(n_sharing=len(lKFsSharingWords))
        if not lKFsSharingWords:
            res["early"] = "sharing"
            return res
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > maxCommonWords:
                maxCommonWords = pKFi.mnRelocWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = f32(l1_score(bow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        res.update(max_common_words=maxCommonWords, min_common_words=minCommonWords, scored_id=[k.mnId for _, k in lScoreAndMatch],
                   scored_words=[k.mnRelocWords for _, k in lScoreAndMatch], scored_score=[s for s, _ in lScoreAndMatch],
                   sharing_id=[k.mnId for k in lKFsSharingWords], sharing_words=[k.mnRelocWords for k in lKFsSharingWords])
        if not lScoreAndMatch:      # (unreachable: the keyframe with maxCommonWords always passes)
            res["early"] = "score"
            return res
        lAccScoreAndMatch = []
        bestAccScore = f32(0)
        for si, pKFi in lScoreAndMatch:
            vpNeighs = self._neighs(pKFi)
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in vpNeighs:
                if pKF2.mnRelocQuery != mnId:
                    continue
                if pKF2.mnRelocWords <= minCommonWords and pKF2.mRelocScore != 0:
                    self.stale_reads += 1
                accScore = f32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpRelocCandidates = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if pKFi.mnId not in spAlreadyAddedKF:
                    vpRelocCandidates.append(pKFi.mnId)
                    spAlreadyAddedKF.add(pKFi.mnId)
        res.update(kept=list(range(len(lScoreAndMatch))), acc_score=[a for a, _ in lAccScoreAndMatch], best_id=[k.mnId for _, k in lAccScoreAndMatch],
                   best_acc_score=bestAccScore, candidates=vpRelocCandidates)
        return res

    # ---- one call of several queries: dict(mode, words, values, connected, counts, min_score_in)
    def query(self, q):
        if q["mode"] == LOOP:
            return self.DetectLoopCandidates(q["words"], q["values"], q.get("connected", ()), q.get("counts"), q.get("min_score_in", 1.0))
        return self.DetectRelocalizationCandidates(q["words"], q["values"])

    def query_batch(self, queries):
        before = {i: k.mRelocScore for i, k in self.kfs.items()}
        after = dict(before)
        out = []
        for q in queries:
            for i, k in self.kfs.items():
                k.mRelocScore = before[i]
            r = self.query(q)
            out.append(r)
            if q["mode"] == RELOC:
                for i, s in zip(r["scored_id"], r["scored_score"]):
                    after[i] = s
        for i, k in self.kfs.items():
            k.mRelocScore = after[i]
        return out

    def reloc_score(self, mnId):
        return self.kfs[mnId].mRelocScore


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
class Scene:
    """P places, each a set of `place_words` words drawn over n_words; keyframe t belongs to place place_of[t] (visits of `visit` keyframes, places
    revisited), takes about 60 % of its `length` words from the place and the rest uniformly, with positive L1-normalised values."""

    def __init__(self, seed, n_words, n_kf, lengths, places=6, visit=6, edge_words=False):
        self.rng = np.random.default_rng(seed)
        rng = self.rng
        self.n_words, self.n_kf = n_words, n_kf
        lengths = list(lengths)
        maxlen = max(lengths)
        pw = int(min(n_words, max(4, 2.5 * maxlen)))
        self.place_words = [np.sort(rng.choice(n_words, pw, replace=False)) for _ in range(places)]
        self.place_of, self.bows = [], []
        p = 0
        for t in range(n_kf):
            if t % visit == 0:
                p = int(rng.integers(places))
            self.place_of.append(p)
            self.bows.append(self.draw(p, lengths[int(rng.integers(len(lengths)))], edge_words and t % 5 == 0))

    def draw(self, place, length, edges=False):
        rng = self.rng
        n_place = min(int(round(0.6 * length)), len(self.place_words[place]))
        w = set(int(x) for x in rng.choice(self.place_words[place], n_place, replace=False))
        if edges and length >= 2:
            w.update((0, self.n_words - 1))
        while len(w) < min(length, self.n_words):
            w.update(int(x) for x in rng.integers(0, self.n_words, length - len(w)))
        w = np.array(sorted(w)[:length] if not edges else sorted(w), np.int32)
        v = rng.random(len(w)) + 0.05
        v = v / v.sum()
        return w, v.astype(np.float64)

    def covisibles(self, t, present):
        """the temporally nearest keyframes of t's place among `present` (ids = indices), up to ten; some lists are shorter, some name absent ids"""
        rng = self.rng
        same = [u for u in range(max(0, t - 40), min(self.n_kf, t + 40)) if u != t and self.place_of[u] == self.place_of[t] and (u in present or rng.random() < 0.15)]
        same.sort(key=lambda u: (abs(u - t), u))
        n = 10 if rng.random() < 0.6 else int(rng.integers(0, 10))
        ids = same[:n]
        if rng.random() < 0.2 and len(ids) < 10:
            ids.append(self.n_kf + 1000 + t)      # never added
        return ids

    def loop_query(self, t, present):
        """a new keyframe behind t, of t's place, asks: connected = t and the keyframes just before it (some with count 0, one possibly absent)"""
        rng = self.rng
        con = [u for u in range(max(0, t - int(rng.integers(2, 8))), t + 1)]
        if rng.random() < 0.3:
            con.append(self.n_kf + 5000 + t)
        counts = [0 if rng.random() < 0.15 else int(rng.integers(15, 200)) for _ in con]
        lens = sorted(set(len(b[0]) for b in self.bows))
        w, v = self.draw(self.place_of[t], lens[int(rng.integers(len(lens)))])
        return dict(mode=LOOP, words=w, values=v, connected=con, counts=counts, min_score_in=1.0 if rng.random() < 0.7 else float(f32(rng.random() * 0.2)))

    def reloc_query(self, place=None):
        rng = self.rng
        place = int(rng.integers(len(self.place_words))) if place is None else place
        lens = sorted(set(len(b[0]) for b in self.bows))
        w, v = self.draw(place, lens[int(rng.integers(len(lens)))])
        return dict(mode=RELOC, words=w, values=v)
