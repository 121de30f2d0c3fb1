// tools/sin_host_baseline.cc -- the baseline of tools/latency_search_in_neighbors.py: steps 2 and 3 of LocalMapping::SearchInNeighbors the way the shim ran
// them before orbx_search_in_neighbors existed (shim/ORBmatcher_hip.cc, ORBmatcher::Fuse): per Fuse call the projection gates point by point on the
// host, ONE synchronous orbx_fuse_search with its own staging and wait, and the pointer surgery on the host.  The surgery is this project's plain
// one-thread statement on arrays (a point's observations are a rank-ordered vector, no mutex, no cv::Mat, no std::map): at least as fast as the
// reference's objects.  Linked against liborbx.so; reads the scene file the tool writes.
//
//   sin_host_baseline scene.bin reps  ->  "R <median us per SearchInNeighbors> <decisions> <checksum of the log> <nFused of every call ...>"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/orbx.h"

struct Obs { int kf, idx, st; const uint8_t *d; };
struct Kf {
    int n;
    std::vector<orbx_keypoint> kp;
    std::vector<uint8_t> desc;
    std::vector<float> ur;
    std::vector<int32_t> kfp;
    float tcw[12], ow[3];
};
struct Scene {
    int NK, S, P, T0, T, nlevels;
    float cam[5], bounds[4], logsf;
    std::vector<float> sf, invs2;
    std::vector<int32_t> rank, targets;
    std::vector<uint8_t> kfBad;
    std::vector<Kf> kfs;
    std::vector<float> pos, nrm, minD, maxD, rawMax;
    std::vector<uint8_t> desc, bad, obsSt, obsDesc;
    std::vector<int32_t> visible, found, obsOff, obsKf, obsIdx;
};
struct State {
    std::vector<std::vector<int32_t> > kfp;
    std::vector<std::vector<Obs> > obs;
    std::vector<int> nobs, visible, found;
    std::vector<uint8_t> bad, desc;
};

template <typename T> static void readv(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short scene file\n"); exit(2); }
}

static int hamming(const uint8_t *a, const uint8_t *b)
{
    int d = 0;
    for (int i = 0; i < 4; i++) { uint64_t x, y; memcpy(&x, a + 8 * i, 8); memcpy(&y, b + 8 * i, 8); d += __builtin_popcountll(x ^ y); }
    return d;
}

static bool in_kf(const State &st, int p, int kf)
{
    for (const Obs &o : st.obs[(size_t)p]) if (o.kf == kf) return true;
    return false;
}

static void insert_obs(const Scene &sc, std::vector<Obs> &ob, const Obs &o)
{
    size_t at = 0;
    while (at < ob.size() && sc.rank[(size_t)ob[at].kf] < sc.rank[(size_t)o.kf]) at++;
    ob.insert(ob.begin() + (long)at, o);
}

static void distinctive(const Scene &sc, State &st, int p)
{
    std::vector<const uint8_t *> d;
    for (const Obs &o : st.obs[(size_t)p]) if (!sc.kfBad[(size_t)o.kf]) d.push_back(o.d);
    const size_t N = d.size();
    if (!N) return;
    int bestMedian = INT32_MAX;
    size_t best = 0;
    std::vector<int> row(N);
    for (size_t i = 0; i < N; i++) {
        for (size_t j = 0; j < N; j++) row[j] = hamming(d[i], d[j]);
        std::sort(row.begin(), row.end());
        const int median = row[(size_t)(0.5 * (double)(N - 1))];
        if (median < bestMedian) { bestMedian = median; best = i; }
    }
    memcpy(&st.desc[32 * (size_t)p], d[best], 32);
}

static void replace(const Scene &sc, State &st, int a, int b)
{
    std::vector<Obs> obs;
    obs.swap(st.obs[(size_t)a]);
    st.bad[(size_t)a] = 1;
    for (const Obs &o : obs) {
        if (!in_kf(st, b, o.kf)) {
            if (o.kf < sc.S) st.kfp[(size_t)o.kf][(size_t)o.idx] = b;
            insert_obs(sc, st.obs[(size_t)b], o);
            st.nobs[(size_t)b] += o.st ? 2 : 1;
        } else if (o.kf < sc.S) st.kfp[(size_t)o.kf][(size_t)o.idx] = -1;
    }
    st.found[(size_t)b] += st.found[(size_t)a]; st.visible[(size_t)b] += st.visible[(size_t)a];
    distinctive(sc, st, b);
}

struct Buf { std::vector<float> u, v, ur, radius; std::vector<int32_t> level, bi, bd; std::vector<uint8_t> act, desc; };

// one ORBmatcher::Fuse as the shim ran it; -> nFused
static int fuse(orbx_matcher *m, const Scene &sc, State &st, int k, const std::vector<int32_t> &lst, int call, Buf &B, uint64_t &sum, long &decisions)
{
    const Kf &K = sc.kfs[(size_t)k];
    const int n = (int)lst.size();
    B.u.assign((size_t)n, 0.f); B.v.assign((size_t)n, 0.f); B.ur.assign((size_t)n, 0.f); B.radius.assign((size_t)n, 0.f);
    B.level.assign((size_t)n, 0); B.bi.assign((size_t)n, -1); B.bd.assign((size_t)n, 256); B.act.assign((size_t)n, 0); B.desc.assign((size_t)n * 32, 0);
    const float minX = (float)(int)sc.bounds[0], minY = (float)(int)sc.bounds[1], maxX = (float)(int)sc.bounds[2], maxY = (float)(int)sc.bounds[3];
    for (int i = 0; i < n; i++) {      // step 1, src/ORBmatcher.cc:1040-1086
        const int p = lst[(size_t)i];
        if (p < 0 || st.bad[(size_t)p] || in_kf(st, p, k)) continue;
        const float *Pw = &sc.pos[3 * (size_t)p], *Pn = &sc.nrm[3 * (size_t)p];
        float Pc[3];
        for (int r = 0; r < 3; r++) {
            float t = K.tcw[4 * r] * Pw[0];
            t = t + K.tcw[4 * r + 1] * Pw[1];
            t = t + K.tcw[4 * r + 2] * Pw[2];
            Pc[r] = t + K.tcw[4 * r + 3];
        }
        if (Pc[2] < 0.0f) continue;
        const float invz = 1.0f / Pc[2];
        const float x = Pc[0] * invz, y = Pc[1] * invz;
        const float u = sc.cam[0] * x + sc.cam[2], v = sc.cam[1] * y + sc.cam[3];
        if (!(u >= minX && u < maxX && v >= minY && v < maxY)) continue;
        const float ur = u - sc.cam[4] * invz;
        const float PO[3] = {Pw[0] - K.ow[0], Pw[1] - K.ow[1], Pw[2] - K.ow[2]};
        const float dist3D = (float)std::sqrt((double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2]);
        if (dist3D < sc.minD[(size_t)p] || dist3D > sc.maxD[(size_t)p]) continue;
        if ((double)PO[0] * Pn[0] + (double)PO[1] * Pn[1] + (double)PO[2] * Pn[2] < 0.5 * dist3D) continue;
        const float ratio = sc.rawMax[(size_t)p] / dist3D;
        int lvl = (int)std::ceil(std::log(ratio) / sc.logsf);
        lvl = lvl < 0 ? 0 : (lvl >= sc.nlevels ? sc.nlevels - 1 : lvl);
        B.u[(size_t)i] = u; B.v[(size_t)i] = v; B.ur[(size_t)i] = ur; B.level[(size_t)i] = lvl; B.radius[(size_t)i] = 3.0f * sc.sf[(size_t)lvl];
        B.act[(size_t)i] = 1;
        memcpy(&B.desc[32 * (size_t)i], &st.desc[32 * (size_t)p], 32);
    }
    for (int first = 0; first < n && K.n > 0; first += 60000) {      // steps 2-3: one synchronous device call (a matcher takes at most 65535 points: longer lists in pieces)
        const int32_t N = K.n, M = std::min(n - first, 60000);
        orbx_projection_frame kf = {K.kp.data(), K.desc.data(), K.ur.data(), 0, &N, N, 1, sc.bounds[0], sc.bounds[1], 64.0f / (sc.bounds[2] - sc.bounds[0]),
                                    48.0f / (sc.bounds[3] - sc.bounds[1])};
        orbx_fuse_points pt = {B.u.data() + first, B.v.data() + first, B.ur.data() + first, B.level.data() + first, B.radius.data() + first, B.act.data() + first,
                               B.desc.data() + 32 * (size_t)first, &M, M, minX, minY};
        if (orbx_fuse_search(m, &kf, &pt, sc.invs2.data(), sc.nlevels, 1, B.bi.data() + first, B.bd.data() + first) != ORBX_OK) { fprintf(stderr, "%s\n", orbx_last_error()); exit(3); }
    }
    int nFused = 0;
    for (int i = 0; i < n; i++) {      // :1150-1171 in list order
        const int p = lst[(size_t)i];
        if (p < 0 || st.bad[(size_t)p] || in_kf(st, p, k) || !B.act[(size_t)i] || B.bd[(size_t)i] > 50) continue;
        const int bi = B.bi[(size_t)i], q = st.kfp[(size_t)k][(size_t)bi];
        int kind;
        if (q >= 0) {
            if (!st.bad[(size_t)q]) {
                if (st.nobs[(size_t)q] > st.nobs[(size_t)p]) { kind = ORBX_FUSE_REPLACED_BY_HOLDER; replace(sc, st, p, q); }
                else { kind = ORBX_FUSE_REPLACED_HOLDER; replace(sc, st, q, p); }
            } else kind = ORBX_FUSE_HOLDER_BAD;
        } else {
            kind = ORBX_FUSE_ADDED;
            const Obs o = {k, bi, K.ur[(size_t)bi] >= 0 ? 1 : 0, &K.desc[32 * (size_t)bi]};
            insert_obs(sc, st.obs[(size_t)p], o);
            st.nobs[(size_t)p] += o.st ? 2 : 1;
            st.kfp[(size_t)k][(size_t)bi] = p;
        }
        sum = sum * 1000003ull + (uint64_t)(((call * 31 + i) * 31 + p) * 31 + bi) * 7ull + (uint64_t)kind;
        decisions++;
        nFused++;
    }
    return nFused;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: sin_host_baseline scene.bin reps\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int reps = atoi(argv[2]);
    Scene sc;
    std::vector<int32_t> hd;
    readv(f, hd, 8);
    if (hd[0] != 0x53494e42) { fprintf(stderr, "not a SearchInNeighbors scene\n"); return 2; }
    sc.NK = hd[1]; sc.S = hd[2]; sc.P = hd[3]; sc.T0 = hd[4]; sc.T = hd[5]; sc.nlevels = hd[6];
    std::vector<float> g;
    readv(f, g, 10);
    memcpy(sc.cam, g.data(), 20); memcpy(sc.bounds, g.data() + 5, 16); sc.logsf = g[9];
    readv(f, sc.sf, (size_t)sc.nlevels); readv(f, sc.invs2, (size_t)sc.nlevels);
    readv(f, sc.rank, (size_t)sc.NK); readv(f, sc.kfBad, (size_t)sc.NK); readv(f, sc.targets, (size_t)sc.T);
    sc.kfs.resize((size_t)sc.S);
    int maxN = 1;
    for (Kf &K : sc.kfs) {
        std::vector<int32_t> n1;
        readv(f, n1, 1);
        K.n = n1[0];
        maxN = std::max(maxN, K.n);
        readv(f, K.kp, (size_t)K.n); readv(f, K.desc, 32 * (size_t)K.n); readv(f, K.ur, (size_t)K.n); readv(f, K.kfp, (size_t)K.n);
        std::vector<float> t;
        readv(f, t, 15);
        memcpy(K.tcw, t.data(), 48); memcpy(K.ow, t.data() + 12, 12);
    }
    const size_t P = (size_t)sc.P, T0 = (size_t)sc.T0;
    readv(f, sc.pos, 3 * P); readv(f, sc.nrm, 3 * P); readv(f, sc.minD, P); readv(f, sc.maxD, P); readv(f, sc.rawMax, P);
    readv(f, sc.desc, 32 * P); readv(f, sc.bad, P); readv(f, sc.visible, P); readv(f, sc.found, P);
    readv(f, sc.obsOff, P + 1); readv(f, sc.obsKf, T0); readv(f, sc.obsIdx, T0); readv(f, sc.obsSt, T0); readv(f, sc.obsDesc, 32 * T0);
    fclose(f);

    orbx_matcher *m = 0;
    if (orbx_matcher_create(0, std::min(65535, std::max(maxN, sc.P)), 1, &m) != ORBX_OK) { fprintf(stderr, "%s\n", orbx_last_error()); return 3; }
    std::vector<double> us;
    std::vector<int> nFused;
    uint64_t sum = 0;
    long decisions = 0;
    Buf B;
    for (int rep = 0; rep < reps + 1; rep++) {      // (the first one warms the handle up)
        State st;      // the map as gathered: not timed
        st.kfp.resize((size_t)sc.S);
        for (int s = 0; s < sc.S; s++) st.kfp[(size_t)s] = sc.kfs[(size_t)s].kfp;
        st.obs.resize(P); st.nobs.assign(P, 0);
        for (size_t p = 0; p < P; p++)
            for (int o = sc.obsOff[p]; o < sc.obsOff[p + 1]; o++) {
                const Obs ob = {sc.obsKf[(size_t)o], sc.obsIdx[(size_t)o], sc.obsSt[(size_t)o] ? 1 : 0, &sc.obsDesc[32 * (size_t)o]};
                st.obs[p].push_back(ob);
                st.nobs[p] += ob.st ? 2 : 1;
            }
        st.visible.assign(sc.visible.begin(), sc.visible.end()); st.found.assign(sc.found.begin(), sc.found.end());
        st.bad = sc.bad; st.desc = sc.desc;
        nFused.clear(); sum = 0; decisions = 0;
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<int32_t> lst = st.kfp[0];      // vpMapPointMatches, captured once
        for (int t = 0; t < sc.T; t++) nFused.push_back(fuse(m, sc, st, sc.targets[(size_t)t], lst, t, B, sum, decisions));
        std::vector<int32_t> cand;
        std::vector<uint8_t> listed(P, 0);
        for (int t = 0; t < sc.T; t++)
            for (int32_t p : st.kfp[(size_t)sc.targets[(size_t)t]])
                if (p >= 0 && !st.bad[(size_t)p] && !listed[(size_t)p]) { listed[(size_t)p] = 1; cand.push_back(p); }
        nFused.push_back(fuse(m, sc, st, 0, cand, sc.T, B, sum, decisions));
        const auto t1 = std::chrono::steady_clock::now();
        if (rep) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
    }
    std::sort(us.begin(), us.end());
    printf("R %.1f %ld %llu", us.empty() ? 0.0 : us[us.size() / 2], decisions, (unsigned long long)sum);
    for (int v : nFused) printf(" %d", v);
    printf("\n");
    orbx_matcher_destroy(m);
    return 0;
}
