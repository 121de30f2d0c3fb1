// tools/kfdb_host_baseline.cc -- the host baseline of tools/latency_kfdb.py: this project's own plain C++ statement of place recognition by an inverted
// file (one std::list of keyframes per word, std::map BowVectors, one thread): for every query word walk its list, count the shared words per
// keyframe, score the keyframes with more than 0.8 of the best count by the L1 score, add up the scores over each keyframe's ten covisibles and return
// the best keyframe of every group within 0.75 of the best group.  It reads the scene that the tool wrote and prints one line per query:
//   Q <index> <mode> <median microseconds of --reps runs> <candidates...>
// No GPU.   g++ -O2 -std=c++11 -o kfdb_host_baseline kfdb_host_baseline.cc ;  kfdb_host_baseline scene.bin [reps]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <list>
#include <map>
#include <set>
#include <vector>

typedef std::map<int, double> Bow;
struct KF {
    long id;
    Bow bow;
    long loopQuery, relocQuery;
    int loopWords, relocWords;
    float loopScore, relocScore;
    std::vector<KF *> cov;
    KF() : id(0), loopQuery(-1), relocQuery(-1), loopWords(0), relocWords(0), loopScore(0), relocScore(0) {}
};
struct Query { int mode; Bow bow; std::vector<long> connected; std::vector<int> counts; };

static double l1(const Bow &a, const Bow &b)
{
    Bow::const_iterator i = a.begin(), j = b.begin();
    double s = 0;
    while (i != a.end() && j != b.end()) {
        if (i->first == j->first) { s += fabs(i->second - j->second) - fabs(i->second) - fabs(j->second); ++i; ++j; }
        else if (i->first < j->first) i = a.lower_bound(j->first);
        else j = b.lower_bound(i->first);
    }
    return -s / 2.0;
}

static std::vector<long> run(std::vector<std::list<KF *> > &inv, std::vector<KF> &kfs, const Query &q, long qid)
{
    const bool loop = q.mode == 0;
    std::set<long> connected(q.connected.begin(), q.connected.end());
    float minScore = loop ? 1.f : 0.f;
    if (loop)
        for (size_t i = 0; i < q.connected.size(); i++) {
            if (q.connected[i] < 0 || q.connected[i] >= (long)kfs.size() || q.counts[i] == 0) continue;
            const float s = (float)l1(q.bow, kfs[(size_t)q.connected[i]].bow);
            if (s < minScore) minScore = s;
        }
    std::list<KF *> sharing;
    for (Bow::const_iterator it = q.bow.begin(); it != q.bow.end(); ++it) {
        std::list<KF *> &l = inv[(size_t)it->first];
        for (std::list<KF *>::iterator k = l.begin(); k != l.end(); ++k) {
            KF *kf = *k;
            if (loop) {
                if (kf->loopQuery != qid) { kf->loopWords = 0; if (!connected.count(kf->id)) { kf->loopQuery = qid; sharing.push_back(kf); } }
                kf->loopWords++;
            } else {
                if (kf->relocQuery != qid) { kf->relocWords = 0; kf->relocQuery = qid; sharing.push_back(kf); }
                kf->relocWords++;
            }
        }
    }
    std::vector<long> out;
    if (sharing.empty()) return out;
    int maxCommon = 0;
    for (std::list<KF *>::iterator k = sharing.begin(); k != sharing.end(); ++k) maxCommon = std::max(maxCommon, loop ? (*k)->loopWords : (*k)->relocWords);
    const int minCommon = (int)(maxCommon * 0.8f);
    std::list<std::pair<float, KF *> > scored;
    for (std::list<KF *>::iterator k = sharing.begin(); k != sharing.end(); ++k) {
        KF *kf = *k;
        if ((loop ? kf->loopWords : kf->relocWords) <= minCommon) continue;
        const float s = (float)l1(q.bow, kf->bow);
        if (loop) { kf->loopScore = s; if (s >= minScore) scored.push_back(std::make_pair(s, kf)); }
        else { kf->relocScore = s; scored.push_back(std::make_pair(s, kf)); }
    }
    if (scored.empty()) return out;
    std::list<std::pair<float, KF *> > groups;
    float bestAcc = minScore;
    for (std::list<std::pair<float, KF *> >::iterator it = scored.begin(); it != scored.end(); ++it) {
        float best = it->first, acc = it->first;
        KF *bestKF = it->second;
        const std::vector<KF *> &nb = it->second->cov;
        for (size_t i = 0; i < nb.size(); i++) {
            KF *k2 = nb[i];
            float s;
            if (loop) { if (k2->loopQuery != qid || k2->loopWords <= minCommon) continue; s = k2->loopScore; }
            else { if (k2->relocQuery != qid) continue; s = k2->relocScore; }
            acc += s;
            if (s > best) { best = s; bestKF = k2; }
        }
        groups.push_back(std::make_pair(acc, bestKF));
        if (acc > bestAcc) bestAcc = acc;
    }
    const float retain = 0.75f * bestAcc;
    std::set<KF *> seen;
    for (std::list<std::pair<float, KF *> >::iterator it = groups.begin(); it != groups.end(); ++it)
        if (it->first > retain && !seen.count(it->second)) { out.push_back(it->second->id); seen.insert(it->second); }
    return out;
}

template <typename T> static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s scene.bin [reps]\n", argv[0]); return 2; }
    const int reps = argc > 2 ? atoi(argv[2]) : 5;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[4];
    if (!rd(f, head, 4) || head[0] != 0x4b464442) { fprintf(stderr, "not a scene file\n"); return 2; }
    const int nWords = head[1], nKf = head[2], nQ = head[3];
    std::vector<int64_t> off((size_t)nKf + 1);
    if (!rd(f, off.data(), off.size())) return 2;
    std::vector<int32_t> words((size_t)off[(size_t)nKf]), cov((size_t)nKf * 10);
    std::vector<double> values(words.size());
    if (!rd(f, words.data(), words.size()) || !rd(f, values.data(), values.size()) || !rd(f, cov.data(), cov.size())) return 2;
    std::vector<KF> kfs((size_t)nKf);
    std::vector<std::list<KF *> > inv((size_t)nWords);
    for (int k = 0; k < nKf; k++) {      // add, in id order
        KF &kf = kfs[(size_t)k];
        kf.id = k;
        for (int64_t i = off[(size_t)k]; i < off[(size_t)k + 1]; i++) kf.bow[words[(size_t)i]] = values[(size_t)i];
        for (Bow::const_iterator it = kf.bow.begin(); it != kf.bow.end(); ++it) inv[(size_t)it->first].push_back(&kf);
        for (int i = 0; i < 10; i++) if (cov[(size_t)k * 10 + i] >= 0) kf.cov.push_back(&kfs[(size_t)cov[(size_t)k * 10 + i]]);
    }
    long qid = 1L << 40;
    for (int qi = 0; qi < nQ; qi++) {
        int32_t h[3];
        if (!rd(f, h, 3)) return 2;
        Query q;
        q.mode = h[0];
        std::vector<int32_t> w((size_t)h[1]), cnt((size_t)h[2]);
        std::vector<double> v((size_t)h[1]);
        std::vector<int64_t> con((size_t)h[2]);
        if (!rd(f, w.data(), w.size()) || !rd(f, v.data(), v.size()) || !rd(f, con.data(), con.size()) || !rd(f, cnt.data(), cnt.size())) return 2;
        for (size_t i = 0; i < w.size(); i++) q.bow[w[i]] = v[i];
        q.connected.assign(con.begin(), con.end());
        q.counts.assign(cnt.begin(), cnt.end());
        std::vector<double> us;
        std::vector<long> cand;
        for (int r = 0; r < reps; r++) {
            const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
            cand = run(inv, kfs, q, qid++);
            us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(us.begin(), us.end());
        printf("Q %d %d %.1f", qi, q.mode, us[us.size() / 2]);
        for (size_t i = 0; i < cand.size(); i++) printf(" %ld", cand[i]);
        printf("\n");
    }
    fclose(f);
    return 0;
}
