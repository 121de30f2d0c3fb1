// tools/voc_train_host_baseline.cc -- the host baseline of tools/latency_voc_train.py: this project's own one-thread statement of the vocabulary
// training on plain arrays (descriptors as four 64-bit words, a node = a range of one index array that is partitioned in place level after level
// of the recursion), with the draws, the empty-cluster rule and the cap of include/orbx.h, so that its tree is the device's bit for bit.
// It reads the scene the tool wrote and writes the tree:
//   scene:  int32 magic, N, images, k, L, weighting, max_iterations, pad; uint64 seed; int32 counts[images]; uint8 descriptors[N][32]
//   result: int32 nodes, words, unconverged, passes[10]; int32 parent[nodes]; uint8 leaf[nodes]; uint8 descriptors[nodes][32]; int32 ni[nodes];
//           double weight[nodes]
// and prints "T <total ms> <tree ms> <weights ms>".  No GPU.
//   g++ -O2 -std=c++11 -march=native -o voc_train_host_baseline voc_train_host_baseline.cc ;  voc_train_host_baseline scene.bin result.bin
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

typedef unsigned long long u64;
struct D256 { u64 w[4]; };

static inline int ham(const D256 &a, const D256 &b)
{
    return __builtin_popcountll(a.w[0] ^ b.w[0]) + __builtin_popcountll(a.w[1] ^ b.w[1]) + __builtin_popcountll(a.w[2] ^ b.w[2]) + __builtin_popcountll(a.w[3] ^ b.w[3]);
}
static inline u64 mix(u64 z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline u64 draw(u64 seed, u64 slot, u64 j) { return mix(mix(mix(seed) + slot) + j) >> 11; }
static const double TWO_M53 = 1.0 / 9007199254740992.0;      // 2^-53

struct Tree {
    int k, L, maxIt, unconverged;
    u64 seed;
    const D256 *desc;
    std::vector<int32_t> parent, firstChild, numChild;
    std::vector<D256> ndesc;
    int passes[10];
};

// majority of each of the 256 bits over idx[lo .. hi) with assoc == c; false when the group is empty
static bool mean_of(const Tree &t, const int32_t *idx, const int *assoc, int n, int c, D256 &out)
{
    int cnt[256] = {0}, size = 0;
    for (int i = 0; i < n; i++) {
        if (assoc[i] != c) continue;
        size++;
        const D256 &d = t.desc[idx[i]];
        for (int w = 0; w < 4; w++)
            for (u64 v = d.w[w]; v; v &= v - 1) cnt[64 * w + __builtin_ctzll(v)]++;
    }
    if (!size) return false;
    const int need = size / 2 + size % 2;
    for (int w = 0; w < 4; w++) {
        u64 v = 0;
        for (int b = 0; b < 64; b++)
            if (cnt[64 * w + b] >= need) v |= 1ull << b;
        out.w[w] = v;
    }
    return true;
}

static void split(Tree &t, int node, int32_t *idx, int n, int level, u64 slot)
{
    const int k = t.k;
    std::vector<D256> centres;
    std::vector<int> assoc((size_t)n);
    if (n <= k) {
        for (int i = 0; i < n; i++) { centres.push_back(t.desc[idx[i]]); assoc[(size_t)i] = i; }
    } else {
        // k-means++ with D(x), not D(x)^2
        long long first = (long long)(((double)draw(t.seed, slot, 0) * TWO_M53) * (double)n);
        if (first > n - 1) first = n - 1;
        centres.push_back(t.desc[idx[first]]);
        std::vector<int> md((size_t)n);
        for (int j = 1; j < k; j++) {
            u64 sum = 0;
            for (int i = 0; i < n; i++) {
                const int d = ham(t.desc[idx[i]], centres.back());
                if (j == 1 || d < md[(size_t)i]) md[(size_t)i] = d;
                sum += (u64)md[(size_t)i];
            }
            if (!sum) break;
            const double cut = ((double)(draw(t.seed, slot, (u64)j) + 1) * TWO_M53) * (double)sum;
            u64 up = 0;
            int pick = n - 1;
            for (int i = 0; i < n; i++) {
                up += (u64)md[(size_t)i];
                if ((double)up >= cut) { pick = i; break; }
            }
            centres.push_back(t.desc[idx[pick]]);
        }
        const int nc = (int)centres.size();
        int pass = 0;
        for (;;) {
            ++pass;
            if (pass > 1)
                for (int c = 0; c < nc; c++) mean_of(t, idx, assoc.data(), n, c, centres[(size_t)c]);      // (an empty group leaves the centre alone)
            bool changed = false;
            for (int i = 0; i < n; i++) {
                int best = 1 << 30, bi = 0;
                for (int c = 0; c < nc; c++) {
                    const int d = ham(t.desc[idx[i]], centres[(size_t)c]);
                    if (d < best) { best = d; bi = c; }
                }
                if (pass > 1 && assoc[(size_t)i] != bi) changed = true;
                assoc[(size_t)i] = bi;
            }
            if (pass >= 2 && !changed) break;
            if (pass >= t.maxIt) { t.unconverged++; break; }
        }
        t.passes[level - 1] = std::max(t.passes[level - 1], pass);
    }
    const int nc = (int)centres.size(), base = (int)t.parent.size();
    t.firstChild[(size_t)node] = base;
    t.numChild[(size_t)node] = nc;
    for (int c = 0; c < nc; c++) { t.parent.push_back(node); t.firstChild.push_back(0); t.numChild.push_back(0); t.ndesc.push_back(centres[(size_t)c]); }
    if (level >= t.L) return;
    // stable partition of the node's range by cluster, then the children in order
    std::vector<int32_t> tmp(idx, idx + n);
    std::vector<int> start((size_t)nc + 1, 0);
    for (int i = 0; i < n; i++) start[(size_t)assoc[(size_t)i] + 1]++;
    for (int c = 0; c < nc; c++) start[(size_t)c + 1] += start[(size_t)c];
    std::vector<int> at(start.begin(), start.end() - 1);
    for (int i = 0; i < n; i++) idx[at[(size_t)assoc[(size_t)i]]++] = tmp[(size_t)i];
    for (int c = 0; c < nc; c++)
        if (start[(size_t)c + 1] - start[(size_t)c] > 1) split(t, base + c, idx + start[(size_t)c], start[(size_t)c + 1] - start[(size_t)c], level + 1, slot * (u64)k + (u64)c + 1);
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s scene.bin result.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    int32_t head[8];
    u64 seed = 0;
    if (!f || fread(head, 4, 8, f) != 8 || head[0] != 0x564f4354 || fread(&seed, 8, 1, f) != 1) { fprintf(stderr, "bad scene\n"); return 2; }
    const int N = head[1], images = head[2], weighting = head[5];
    std::vector<int32_t> counts((size_t)images);
    std::vector<D256> desc((size_t)N);
    if ((images && fread(counts.data(), 4, (size_t)images, f) != (size_t)images) || fread(desc.data(), 32, (size_t)N, f) != (size_t)N) { fprintf(stderr, "short scene\n"); return 2; }
    fclose(f);
    Tree t;
    t.k = head[3]; t.L = head[4]; t.maxIt = head[6]; t.unconverged = 0; t.seed = seed; t.desc = desc.data();
    memset(t.passes, 0, sizeof(t.passes));
    const auto t0 = std::chrono::steady_clock::now();
    t.parent.assign(1, 0); t.firstChild.assign(1, 0); t.numChild.assign(1, 0); t.ndesc.assign(1, D256{{0, 0, 0, 0}});
    std::vector<int32_t> idx((size_t)N);
    for (int i = 0; i < N; i++) idx[(size_t)i] = i;
    if (N) split(t, 0, idx.data(), N, 1, 0);
    // node ids as the recursion hands them out: a node's children together, then the children's subtrees in order
    const int built = (int)t.parent.size();
    std::vector<int32_t> order, newId((size_t)built, -1), stack(1, 0);
    order.push_back(0); newId[0] = 0;
    while (!stack.empty()) {
        const int nd = stack.back();
        stack.pop_back();
        for (int c = 0; c < t.numChild[(size_t)nd]; c++) { newId[(size_t)(t.firstChild[(size_t)nd] + c)] = (int32_t)order.size(); order.push_back(t.firstChild[(size_t)nd] + c); }
        for (int c = t.numChild[(size_t)nd] - 1; c >= 0; c--)
            if (t.numChild[(size_t)(t.firstChild[(size_t)nd] + c)]) stack.push_back(t.firstChild[(size_t)nd] + c);
    }
    const int nodes = (int)order.size();
    std::vector<int32_t> parent((size_t)nodes, 0), word((size_t)nodes, -1), ni((size_t)nodes, 0), cs((size_t)nodes, 0), cn((size_t)nodes, 0);
    std::vector<uint8_t> leaf((size_t)nodes, 0);
    std::vector<D256> nd((size_t)nodes);
    std::vector<double> weight((size_t)nodes, 0.0);
    int words = 0;
    for (int id = 0; id < nodes; id++) {
        const int old = order[(size_t)id];
        parent[(size_t)id] = id ? newId[(size_t)t.parent[(size_t)old]] : 0;
        nd[(size_t)id] = t.ndesc[(size_t)old];
        cn[(size_t)id] = t.numChild[(size_t)old];
        cs[(size_t)id] = cn[(size_t)id] ? newId[(size_t)t.firstChild[(size_t)old]] : 0;
        leaf[(size_t)id] = id > 0 && !cn[(size_t)id];
        if (leaf[(size_t)id]) word[(size_t)id] = words++;
    }
    const auto t1 = std::chrono::steady_clock::now();
    // weights: every image's features descend the tree; a word counts an image once
    std::vector<int32_t> lastImage((size_t)nodes, -1);
    int at = 0;
    for (int m = 0; m < images; m++)
        for (int i = 0; i < counts[(size_t)m]; i++, at++) {
            int cur = 0;
            while (cn[(size_t)cur]) {
                int best = 1 << 30, bi = cs[(size_t)cur];
                for (int c = 0; c < cn[(size_t)cur]; c++) {
                    const int d = ham(desc[(size_t)at], nd[(size_t)(cs[(size_t)cur] + c)]);
                    if (d < best) { best = d; bi = cs[(size_t)cur] + c; }
                }
                cur = bi;
            }
            if (lastImage[(size_t)cur] != m) { lastImage[(size_t)cur] = m; ni[(size_t)cur]++; }
        }
    for (int id = 1; id < nodes; id++)
        if (leaf[(size_t)id]) weight[(size_t)id] = (weighting == 1 || weighting == 3) ? 1.0 : (ni[(size_t)id] > 0 ? log((double)images / (double)ni[(size_t)id]) : 0.0);
    const auto t2 = std::chrono::steady_clock::now();
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const int32_t out[3] = {nodes, words, t.unconverged};
    fwrite(out, 4, 3, o); fwrite(t.passes, 4, 10, o); fwrite(parent.data(), 4, (size_t)nodes, o); fwrite(leaf.data(), 1, (size_t)nodes, o);
    fwrite(nd.data(), 32, (size_t)nodes, o); fwrite(ni.data(), 4, (size_t)nodes, o); fwrite(weight.data(), 8, (size_t)nodes, o);
    fclose(o);
    typedef std::chrono::duration<double, std::milli> ms;
    printf("T %.3f %.3f %.3f\n", ms(t2 - t0).count(), ms(t1 - t0).count(), ms(t2 - t1).count());
    return 0;
}
