// tools/covis_host_baseline.cc -- one-thread host baseline of tools/latency_covis.py: this project's own statement of the two loops of
// KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling on std::map containers (a map point holds std::map<KeyFrame*, size_t>, the vote
// goes into a std::map<KeyFrame*, int>, the connections are sorted as pair<int, KeyFrame*>), on the scene file the tool writes.  The observations
// are walked in place (no copy of the map per point, no mutex): the baseline is at least as fast as a body that copies and locks.
//
//   covis_host_baseline scene.bin mode reps      mode 0: every list through the UpdateConnections loop, 1: the culling loop over the lists
//   -> "R <median us per call> <checksum>"        checksum 0: sum of counter weights + 1000003 * connections; 1: culled + 1000003 * sum of n_redundant
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

struct KeyFrame;
struct MapPoint {
    bool bad;
    int nObs;
    std::map<KeyFrame *, size_t> obs;
    std::vector<uint8_t> octave, stereo;      // by the index stored in obs
};
struct KeyFrame {
    int slot;
    uint8_t flags;
    bool erased;
    std::vector<MapPoint *> points;
    std::vector<uint8_t> octave, close;
};

template <typename T> static std::vector<T> readv(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short scene file\n"); exit(2); }
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: covis_host_baseline scene.bin mode reps\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int mode = atoi(argv[2]), reps = atoi(argv[3]);
    const std::vector<int32_t> hd = readv<int32_t>(f, 6);
    if (hd[0] != 0x434f5649) { fprintf(stderr, "not a covisibility scene\n"); return 2; }
    const size_t NK = (size_t)hd[1], M = (size_t)hd[2], T = (size_t)hd[3], Q = (size_t)hd[4], S = (size_t)hd[5];
    const std::vector<int32_t> rank = readv<int32_t>(f, NK);
    const std::vector<uint8_t> flags = readv<uint8_t>(f, NK);
    const std::vector<int32_t> obsOff = readv<int32_t>(f, M + 1), obsKf = readv<int32_t>(f, T);
    const std::vector<uint8_t> obsOct = readv<uint8_t>(f, T), obsSt = readv<uint8_t>(f, T), ptBad = readv<uint8_t>(f, M);
    const std::vector<int32_t> listOff = readv<int32_t>(f, Q + 1), listKf = readv<int32_t>(f, Q), listPt = readv<int32_t>(f, S);
    const std::vector<uint8_t> listOct = readv<uint8_t>(f, S), listClose = readv<uint8_t>(f, S);
    fclose(f);

    // keyframes live in one array in rank order, so that the order of their addresses is the order of the ranks
    std::vector<int> order(NK), at(NK);
    for (size_t i = 0; i < NK; i++) order[i] = (int)i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return rank[(size_t)a] < rank[(size_t)b]; });
    for (size_t i = 0; i < NK; i++) at[(size_t)order[i]] = (int)i;
    std::vector<double> us;
    long long checksum = 0;
    for (int rep = 0; rep < reps; rep++) {
        std::vector<KeyFrame> kfs(NK);
        std::vector<MapPoint> mps(M);
        for (size_t k = 0; k < NK; k++) { KeyFrame &K = kfs[(size_t)at[k]]; K.slot = (int)k; K.flags = flags[k]; K.erased = false; }
        for (size_t p = 0; p < M; p++) {
            MapPoint &P = mps[p];
            P.bad = ptBad[p] != 0; P.nObs = 0;
            for (int32_t o = obsOff[p]; o < obsOff[p + 1]; o++) {
                P.obs[&kfs[(size_t)at[(size_t)obsKf[(size_t)o]]]] = P.octave.size();
                P.octave.push_back(obsOct[(size_t)o]); P.stereo.push_back(obsSt[(size_t)o]);
                P.nObs += obsSt[(size_t)o] ? 2 : 1;
            }
        }
        std::vector<KeyFrame> frames(Q);      // the lists; an owned list's points are the owner's
        std::vector<KeyFrame *> owner(Q);
        for (size_t q = 0; q < Q; q++) {
            KeyFrame &L = frames[q];
            owner[q] = listKf[q] >= 0 ? &kfs[(size_t)at[(size_t)listKf[q]]] : (KeyFrame *)0;
            for (int32_t e = listOff[q]; e < listOff[q + 1]; e++) { L.points.push_back(&mps[(size_t)listPt[(size_t)e]]); L.octave.push_back(listOct[(size_t)e]); L.close.push_back(listClose[(size_t)e]); }
        }
        long long sum = 0;
        const auto t0 = std::chrono::steady_clock::now();
        if (mode == 0) {
            for (size_t q = 0; q < Q; q++) {
                std::map<KeyFrame *, int> KFcounter;
                for (MapPoint *pMP : frames[q].points) {
                    if (pMP->bad) continue;
                    for (std::map<KeyFrame *, size_t>::const_iterator mit = pMP->obs.begin(); mit != pMP->obs.end(); ++mit) {
                        if (mit->first == owner[q]) continue;
                        KFcounter[mit->first]++;
                    }
                }
                if (KFcounter.empty()) continue;
                int nmax = 0;
                KeyFrame *pKFmax = 0;
                std::vector<std::pair<int, KeyFrame *> > vPairs;
                vPairs.reserve(KFcounter.size());
                for (std::map<KeyFrame *, int>::iterator mit = KFcounter.begin(); mit != KFcounter.end(); ++mit) {
                    if (mit->second > nmax && (owner[q] || !(mit->first->flags & 4))) { nmax = mit->second; pKFmax = mit->first; }
                    if (mit->second >= 15) vPairs.push_back(std::make_pair(mit->second, mit->first));
                    sum += mit->second;
                }
                if (vPairs.empty() && pKFmax) vPairs.push_back(std::make_pair(nmax, pKFmax));
                std::sort(vPairs.begin(), vPairs.end());
                std::vector<KeyFrame *> ordered;
                std::vector<int> weights;
                for (size_t i = vPairs.size(); i-- > 0;) { ordered.push_back(vPairs[i].second); weights.push_back(vPairs[i].first); }
                sum += 1000003ll * (long long)ordered.size();
            }
        } else {
            for (size_t q = 0; q < Q; q++) {
                KeyFrame *pKF = owner[q];
                if (pKF->flags & 1) continue;
                const int thObs = 3;
                int nRedundant = 0, nMPs = 0;
                const KeyFrame &L = frames[q];
                for (size_t i = 0; i < L.points.size(); i++) {
                    MapPoint *pMP = L.points[i];
                    if (pMP->bad || !L.close[i]) continue;
                    nMPs++;
                    if (pMP->nObs > thObs) {
                        const int scaleLevel = L.octave[i];
                        int nObs = 0;
                        for (std::map<KeyFrame *, size_t>::const_iterator mit = pMP->obs.begin(); mit != pMP->obs.end(); ++mit) {
                            if (mit->first == pKF) continue;
                            if ((int)pMP->octave[mit->second] <= scaleLevel + 1 && ++nObs >= thObs) break;
                        }
                        if (nObs >= thObs) nRedundant++;
                    }
                }
                sum += 1000003ll * nRedundant;
                if (nRedundant > 0.9 * nMPs) {
                    sum++;
                    if (pKF->flags & 2) continue;
                    for (MapPoint *pP : frames[q].points) {      // SetBadFlag: every point of the keyframe loses its observation (:640-642)
                        MapPoint &P = *pP;
                        std::map<KeyFrame *, size_t>::iterator it = P.obs.find(pKF);
                        if (it == P.obs.end()) continue;
                        P.nObs -= P.stereo[it->second] ? 2 : 1;
                        P.obs.erase(it);
                        if (P.nObs <= 2) { P.bad = true; P.obs.clear(); }
                    }
                }
            }
        }
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        checksum = sum;
    }
    std::sort(us.begin(), us.end());
    printf("R %.3f %lld\n", us[us.size() / 2], checksum);
    return 0;
}
