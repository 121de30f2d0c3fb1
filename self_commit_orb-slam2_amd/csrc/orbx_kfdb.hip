// orbx_kfdb.hip -- KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates (reference src/KeyFrameDatabase.cc:104-374) with
// L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) and the minimum-score loop of LoopClosing::DetectLoop (:160-176), for all
// queries of a call in one chain.  gfx950 only.
//
// The database lives on the device: an append-only pool of (word, value) entries (two arrays: 4 + 8 bytes per entry), one KfSlot per added
// keyframe (id, seq, offset, len, alive, the up-to-ten best covisibles resolved to slots by the host), and the persistent reloc_score.  No
// inverted file: the reference's list order is the order by (smallest word shared with the query, `add` sequence number), so every keyframe
// intersects its own sorted BowVector with the query.
//
//   k_kfdb_intersect  a wave per slot, the slot's words 64 at a time (four such loads in flight) against the query's sorted words in LDS by binary
//                     search: shared-word count, first shared word, connected or not; integer atomics for n_sharing and maxCommonWords.  A 2^18-bit
//                     LDS bitmap in front of the search was measured and is slower: the walk waits for its loads, not for LDS
//   k_kfdb_score      the walk by binary search (the index found is the one the score needs for the query's value) for the slots with words > minCommonWords (and, loop mode, the connected ones): the matched lanes' terms
//                     fabs(v - w) - fabs(v) - fabs(w) are added by ONE running sum in ascending word order (ballot, then lane by lane), so the
//                     double is the sequential one bit for bit; score = float(-sum / 2.0)
//   k_kfdb_commit     reloc_score of the next call: per slot the score of the highest-numbered relocalisation query that scored it, else the
//                     old value (written to the other of two buffers: the queries of this call read the old one)
//   k_kfdb_select     one workgroup per query: the scored slots ranked by (first word, seq), minScore from the connected keyframes,
//                     lScoreAndMatch, the covisibility groups (float accumulation in list order, strictly-greater best), bestAccScore as the
//                     first maximum, the candidates once each at their first occurrence; results into mapped pinned memory, sequence word behind
//
// Everything downstream of the scores compares bit-equal floats, so tests/kfdb_ref.py (a literal restatement of the inverted-file walk) equals
// this chain in every field without a tolerance.  PARITY UNPINNED against the reference: mRelocScore of a keyframe no query has scored (0 here,
// uninitialised there) and the covisibles (as last pushed here, as of the query there).
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "orbx_handle.h"

#define KF_THREADS 256
#define KF_SLOTS_PER_BLOCK 16        /* four slots per wave behind one load of the query into LDS */
#define KF_SEL_THREADS 1024
#define KF_MAX_QUERY_WORDS 8192      /* 32 KiB of LDS */
#define KF_UNROLL 4                  /* k_kfdb_intersect: chunks of 64 words whose loads are in flight together */
#define KF_COV 10
#define KF_FLAG_NONE 0               /* alive, not connected, not scored */
#define KF_FLAG_SCORED 1             /* alive, not connected, words > minCommonWords: scored by this query */
#define KF_FLAG_CONNECTED 2          /* alive and in the query's connected set */
#define KF_FLAG_DEAD 3

struct KfSlot { long long id; int32_t seq, offset, len, alive, ncov, pad; int32_t cov[KF_COV]; };
static_assert(sizeof(KfSlot) == 72, "slot layout");

struct KfQuery { int32_t mode, n, qoff, nconn, coff, nsorted, soff; float minScoreIn; unsigned long long outOff; };

struct KfOutOff { size_t conn, sid, bid, cand, swords, sscore, kept, acc, total; };
static __host__ __device__ inline size_t kf_pad(size_t b) { return (b + 255) & ~(size_t)255; }
static __host__ __device__ inline KfOutOff kf_out_layout(int Ns, int nconn)
{
    KfOutOff o;
    size_t at = 64;      // header: six int32, two floats
    o.conn = at; at += kf_pad(4 * (size_t)nconn);
    o.sid = at; at += kf_pad(8 * (size_t)Ns);
    o.bid = at; at += kf_pad(8 * (size_t)Ns);
    o.cand = at; at += kf_pad(8 * (size_t)Ns);
    o.swords = at; at += kf_pad(4 * (size_t)Ns);
    o.sscore = at; at += kf_pad(4 * (size_t)Ns);
    o.kept = at; at += kf_pad(4 * (size_t)Ns);
    o.acc = at; at += kf_pad(4 * (size_t)Ns);
    o.total = at;
    return o;
}

struct KfDev {
    int Ns, nq;
    const KfSlot *slots;
    const int32_t *poolW;
    const double *poolV;
    const float *relocOld;
    float *relocNew;
    const KfQuery *qs;
    const int32_t *qwords;
    const double *qvalues;
    const int32_t *connSorted, *connSlot, *connCount;
    int32_t *words, *first, *flag, *firstocc;      // [nq][Ns]
    float *score;                                   // [nq][Ns]
    int32_t *list, *order, *lsm, *best;             // [nq][Ns]
    float *acc;                                     // [nq][Ns]
    unsigned long long *key;                        // [nq][Ns]
    int32_t *counters;                              // [nq][2] n_sharing, maxCommonWords
    uint8_t *out;                                   // mapped pinned
};

// index of w in the ascending qw[0..n), -1 = absent
static __device__ __forceinline__ int kf_find(const int32_t *qw, int n, int w)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (qw[m] < w) lo = m + 1; else hi = m;
    }
    return (lo < n && qw[lo] == w) ? lo : -1;
}

static __device__ __forceinline__ void kf_load_query(int32_t *qw, const int32_t *src, int n)
{
    for (int i = threadIdx.x; i < n; i += KF_THREADS) qw[i] = src[i];
    __syncthreads();
}

static __global__ __launch_bounds__(KF_THREADS) void k_kfdb_intersect(KfDev D)
{
    extern __shared__ int32_t qw[];
    __shared__ int blockSharing, blockMax;      // the workgroup's part of n_sharing / maxCommonWords: 50,000 waves on two words of L2 cost more than the walk
    const int q = blockIdx.y, Ns = D.Ns;
    const KfQuery Q = D.qs[q];
    if (threadIdx.x == 0) { blockSharing = 0; blockMax = 0; }
    kf_load_query(qw, D.qwords + Q.qoff, Q.n);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int sEnd = min(Ns, ((int)blockIdx.x + 1) * KF_SLOTS_PER_BLOCK);
    for (int s = blockIdx.x * KF_SLOTS_PER_BLOCK + wave; s < sEnd; s += KF_THREADS / 64) {
        const KfSlot *S = D.slots + s;
        const int alive = S->alive, off = S->offset, len = S->len;
        int count = 0, first = -1;
        if (alive && Q.n > 0) {
            for (int base = 0; base < len; base += 64 * KF_UNROLL) {      // KF_UNROLL loads in flight per lane: the walk is bound by their latency
                int w[KF_UNROLL];
#pragma unroll
                for (int u = 0; u < KF_UNROLL; u++) {
                    const int i = base + 64 * u + lane;
                    w[u] = i < len ? D.poolW[(size_t)off + i] : -1;
                }
#pragma unroll
                for (int u = 0; u < KF_UNROLL; u++) {
                    const bool hit = base + 64 * u + lane < len && kf_find(qw, Q.n, w[u]) >= 0;
                    const unsigned long long mask = __ballot(hit);
                    if (mask) {
                        if (first < 0) first = __shfl(w[u], __ffsll((long long)mask) - 1);      // a slot's words ascend: the lowest hit of the first chunk with one
                        count += __popcll(mask);
                    }
                }
            }
        }
        if (lane == 0) {
            int flag = KF_FLAG_DEAD;
            if (alive) {
                int lo = 0, hi = Q.nsorted;      // is the slot in the query's connected set?
                const int32_t *cs = D.connSorted + Q.soff;
                while (lo < hi) {
                    const int m = (lo + hi) >> 1;
                    if (cs[m] < s) lo = m + 1; else hi = m;
                }
                flag = (lo < Q.nsorted && cs[lo] == s) ? KF_FLAG_CONNECTED : KF_FLAG_NONE;
                if (flag == KF_FLAG_NONE && count > 0) {
                    atomicAdd(&blockSharing, 1);
                    atomicMax(&blockMax, count);
                }
            }
            const size_t at = (size_t)q * Ns + s;
            D.words[at] = count;
            D.first[at] = first;
            D.flag[at] = flag;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && blockSharing > 0) {
        atomicAdd(&D.counters[2 * q], blockSharing);
        atomicMax(&D.counters[2 * q + 1], blockMax);
    }
}

static __global__ __launch_bounds__(KF_THREADS) void k_kfdb_score(KfDev D)
{
    extern __shared__ int32_t qw[];
    const int q = blockIdx.y, Ns = D.Ns;
    const KfQuery Q = D.qs[q];
    kf_load_query(qw, D.qwords + Q.qoff, Q.n);
    const int minCommon = (int)((float)D.counters[2 * q + 1] * 0.8f);
    const double *qv = D.qvalues + Q.qoff;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int sEnd = min(Ns, ((int)blockIdx.x + 1) * KF_SLOTS_PER_BLOCK);
    for (int s = blockIdx.x * KF_SLOTS_PER_BLOCK + wave; s < sEnd; s += KF_THREADS / 64) {
        const size_t at = (size_t)q * Ns + s;
        int flag = D.flag[at];
        const bool scored = flag == KF_FLAG_NONE && D.words[at] > minCommon;
        float sc = 0.f;
        if (scored || flag == KF_FLAG_CONNECTED) {
            const KfSlot *S = D.slots + s;
            const int off = S->offset, len = S->len;
            double sum = 0.0;
            for (int base = 0; base < len; base += 64) {
                const int i = base + lane;
                const int w = i < len ? D.poolW[(size_t)off + i] : -1;
                const int idx = i < len ? kf_find(qw, Q.n, w) : -1;
                double term = 0.0;
                if (idx >= 0) {
                    const double vi = qv[idx], wi = D.poolV[(size_t)off + i];
                    term = fabs(vi - wi) - fabs(vi) - fabs(wi);
                }
                unsigned long long mask = __ballot(idx >= 0);
                while (mask) {      // ONE running sum, the matched lanes in ascending word order
                    const int l = __ffsll((long long)mask) - 1;
                    sum += __shfl(term, l);
                    mask &= mask - 1;
                }
            }
            sc = (float)(-sum / 2.0);
            if (scored) flag = KF_FLAG_SCORED;
        }
        if (lane == 0) {
            D.score[at] = sc;
            D.flag[at] = flag;
            D.firstocc[at] = INT_MAX;
        }
    }
}

static __global__ __launch_bounds__(KF_THREADS) void k_kfdb_commit(KfDev D)
{
    const int s = blockIdx.x * KF_THREADS + threadIdx.x;
    if (s >= D.Ns) return;
    float v = D.relocOld[s];
    for (int q = D.nq - 1; q >= 0; q--) {
        if (D.qs[q].mode == ORBX_KFDB_RELOC && D.flag[(size_t)q * D.Ns + s] == KF_FLAG_SCORED) { v = D.score[(size_t)q * D.Ns + s]; break; }
    }
    D.relocNew[s] = v;
}

static __global__ __launch_bounds__(KF_SEL_THREADS) void k_kfdb_select(KfDev D, unsigned *counter, unsigned long long *flagWord, unsigned long long seq)
{
    __shared__ int sh[KF_SEL_THREADS / 64];
    __shared__ float shf[2];
    __shared__ float rv[KF_SEL_THREADS / 64];
    __shared__ int ri[KF_SEL_THREADS / 64];
    const int q = blockIdx.x, Ns = D.Ns, tid = threadIdx.x;
    const KfQuery Q = D.qs[q];
    const bool loop = Q.mode == ORBX_KFDB_LOOP;
    const size_t qb = (size_t)q * Ns;
    const int32_t *words = D.words + qb, *first = D.first + qb, *flg = D.flag + qb;
    const float *score = D.score + qb;
    int32_t *focc = D.firstocc + qb, *list = D.list + qb, *order = D.order + qb, *lsm = D.lsm + qb, *best = D.best + qb;
    float *acc = D.acc + qb;
    unsigned long long *key = D.key + qb;
    const KfOutOff O = kf_out_layout(Ns, Q.nconn);
    uint8_t *out = D.out + Q.outOff;
    long long *oSid = (long long *)(out + O.sid), *oBid = (long long *)(out + O.bid), *oCand = (long long *)(out + O.cand);
    int32_t *oWords = (int32_t *)(out + O.swords), *oKept = (int32_t *)(out + O.kept);
    float *oScore = (float *)(out + O.sscore), *oAcc = (float *)(out + O.acc), *oConn = (float *)(out + O.conn);

    // the scored slots in slot order (= `add` order), with their keys
    int M = 0;
    for (int s0 = 0; s0 < Ns; s0 += KF_SEL_THREADS) {
        const int s = s0 + tid;
        const bool pred = s < Ns && flg[s] == KF_FLAG_SCORED;
        const int k = block_ballot_rank<KF_SEL_THREADS>(pred, &M, sh);
        if (pred) { list[k] = s; key[k] = ((unsigned long long)(uint32_t)first[s] << 32) | (uint32_t)D.slots[s].seq; }
    }
    __syncthreads();
    // rank by (first shared word, seq): the keys are distinct
    for (int k = tid; k < M; k += KF_SEL_THREADS) {
        const unsigned long long me = key[k];
        int r = 0;
        for (int j = 0; j < M; j++) r += key[j] < me ? 1 : 0;
        const int s = list[k];
        order[r] = s;
        oSid[r] = D.slots[s].id;
        oWords[r] = words[s];
        oScore[r] = score[s];
    }
    // minScore (LoopClosing.cc:160-176 over the connected keyframes the database holds)
    if (tid == 0) {
        float ms = loop ? Q.minScoreIn : 0.f;
        if (loop) {
            for (int j = 0; j < Q.nconn; j++) {
                const int cs = D.connSlot[Q.coff + j];
                const float sc = cs < 0 ? -1.f : score[cs];
                oConn[j] = sc;
                if (cs >= 0 && D.connCount[Q.coff + j] != 0 && sc < ms) ms = sc;
            }
        }
        shf[0] = ms;
    }
    __syncthreads();
    const float minScore = shf[0];
    // lScoreAndMatch
    int E = 0;
    for (int r0 = 0; r0 < M; r0 += KF_SEL_THREADS) {
        const int r = r0 + tid;
        const bool pred = r < M && (!loop || score[order[r]] >= minScore);
        const int e = block_ballot_rank<KF_SEL_THREADS>(pred, &E, sh);
        if (pred) lsm[e] = r;
    }
    __syncthreads();
    // the covisibility groups (:190-215, :325-350)
    float bv = 0.f;
    int bi = INT_MAX;
    for (int e = tid; e < E; e += KF_SEL_THREADS) {
        const int r = lsm[e], s = order[r];
        const KfSlot *S = D.slots + s;
        float bs = score[s], ac = bs;
        int bk = s;
        const int ncov = S->ncov;
        for (int i = 0; i < ncov; i++) {
            const int nb = S->cov[i];
            if (nb < 0 || nb >= Ns) continue;
            const int f = flg[nb];
            bool ok;
            float val;
            if (loop) { ok = f == KF_FLAG_SCORED; val = ok ? score[nb] : 0.f; }
            else { ok = f != KF_FLAG_DEAD && words[nb] > 0; val = f == KF_FLAG_SCORED ? score[nb] : D.relocOld[nb]; }
            if (ok) {
                ac += val;
                if (val > bs) { bk = nb; bs = val; }
            }
        }
        acc[e] = ac;
        best[e] = bk;
        oKept[e] = r;
        oAcc[e] = ac;
        oBid[e] = D.slots[bk].id;
        if (bi == INT_MAX || ac > bv) { bv = ac; bi = e; }
    }
    // bestAccScore: the sequential `if (acc > best) best = acc` keeps the FIRST of equal maxima
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(bv, d);
        const int oi = __shfl_xor(bi, d);
        if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { rv[tid >> 6] = bv; ri[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < KF_SEL_THREADS / 64; w++) {
            const float ov = rv[w];
            const int oi = ri[w];
            if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        float bestAcc = minScore;
        if (bi != INT_MAX && bv > bestAcc) bestAcc = bv;
        shf[0] = bestAcc;
        shf[1] = 0.75f * bestAcc;
    }
    __syncthreads();
    const float bestAcc = shf[0], minRetain = shf[1];
    for (int e = tid; e < E; e += KF_SEL_THREADS)
        if (acc[e] > minRetain) atomicMin(&focc[best[e]], e);
    __syncthreads();
    int C = 0;
    for (int e0 = 0; e0 < E; e0 += KF_SEL_THREADS) {
        const int e = e0 + tid;
        const bool pred = e < E && acc[e] > minRetain && focc[best[e]] == e;
        const int c = block_ballot_rank<KF_SEL_THREADS>(pred, &C, sh);
        if (pred) oCand[c] = D.slots[best[e]].id;
    }
    if (tid == 0) {
        int32_t *hi = (int32_t *)out;
        float *hf = (float *)out;
        const int maxc = D.counters[2 * q + 1];
        hi[0] = D.counters[2 * q]; hi[1] = maxc; hi[2] = (int)((float)maxc * 0.8f); hi[3] = M; hi[4] = E; hi[5] = C;
        hf[6] = minScore; hf[7] = bestAcc;
    }
    orbx_publish(counter, flagWord, seq, gridDim.x);
}

// compaction: slot s of the new numbering takes its entries and its reloc_score from where they were
static __global__ __launch_bounds__(KF_THREADS) void k_kfdb_compact(const int4 *__restrict__ plan, const int32_t *__restrict__ srcW, const double *__restrict__ srcV,
                                                                    const float *__restrict__ srcR, int32_t *__restrict__ dstW, double *__restrict__ dstV, float *__restrict__ dstR)
{
    const int4 p = plan[blockIdx.x];      // old offset, new offset, len, old slot
    for (int i = threadIdx.x; i < p.z; i += KF_THREADS) { dstW[(size_t)p.y + i] = srcW[(size_t)p.x + i]; dstV[(size_t)p.y + i] = srcV[(size_t)p.x + i]; }
    if (threadIdx.x == 0) dstR[blockIdx.x] = srcR[p.w];
}

struct orbx_kf_database : OrbxHandle {
    int nWords = 0, maxKf = 0, maxEntries = 0, maxQueries = 0, maxQueryWords = 0;
    OrbxCallTimer timer;
    hipEvent_t pev[4] = {nullptr, nullptr, nullptr, nullptr};      // behind the staging, k_kfdb_intersect, k_kfdb_score, k_kfdb_commit (profiling only)
    bool profile = false, profiled = false;
    OrbxCallBox box;
    OrbxOwnedBuf<uint8_t> arena;
    OrbxOwnedBuf<int32_t> poolW, work;
    OrbxOwnedBuf<double> poolV;
    OrbxOwnedBuf<unsigned long long> key;
    OrbxOwnedBuf<KfSlot> dslots;
    OrbxOwnedBuf<float> reloc[2];
    ~orbx_kf_database() { for (hipEvent_t e : pev) if (e) (void)hipEventDestroy(e); }
    int cur = 0;                          // which reloc buffer holds the state
    std::vector<KfSlot> slots;            // host mirror, nslots entries in use
    std::vector<long long> covId;         // [slot][KF_COV] the ids as pushed
    std::unordered_map<long long, int> slotOf;               // alive ids
    std::unordered_multimap<long long, int> namedBy;         // id -> slots whose covisibles name it (stale entries are harmless)
    int nslots = 0, nalive = 0, cursor = 0, dead = 0;
    int32_t nextSeq = 0;
};

namespace {
int kf_upload_slot(orbx_kf_database *h, int s)
{
    ORBX_HIP_CHECK(hipMemcpyAsync(h->dslots.p + s, &h->slots[s], sizeof(KfSlot), hipMemcpyHostToDevice, h->stream));
    return ORBX_OK;
}

int kf_check_words(const orbx_kf_database *h, const int32_t *words, const double *values, int n, const char *what)
{
    if (n < 0 || (n > 0 && (!words || !values))) { orbx_set_error("%s: n < 0 or NULL words / values", what); return ORBX_ERR_ARG; }
    for (int i = 0; i < n; i++) {
        if (words[i] < 0 || words[i] >= h->nWords) { orbx_set_error("%s: word %d outside 0..%d", what, words[i], h->nWords - 1); return ORBX_ERR_ARG; }
        if (i && words[i] <= words[i - 1]) { orbx_set_error("%s: words must ascend without repeats", what); return ORBX_ERR_ARG; }
    }
    return ORBX_OK;
}

// every named covisible of slot s resolved against the alive ids
void kf_resolve(orbx_kf_database *h, int s)
{
    KfSlot &S = h->slots[s];
    for (int i = 0; i < S.ncov; i++) {
        auto it = h->slotOf.find(h->covId[(size_t)s * KF_COV + i]);
        S.cov[i] = it == h->slotOf.end() ? -1 : it->second;
    }
}

// the slots naming `id` point at `slot` (-1: nowhere) from now on
int kf_retarget(orbx_kf_database *h, long long id, int slot)
{
    auto range = h->namedBy.equal_range(id);
    for (auto it = range.first; it != range.second; ++it) {
        const int s = it->second;
        if (s >= h->nslots || !h->slots[s].alive) continue;
        KfSlot &S = h->slots[s];
        bool changed = false;
        for (int i = 0; i < S.ncov; i++)
            if (h->covId[(size_t)s * KF_COV + i] == id && S.cov[i] != slot) { S.cov[i] = slot; changed = true; }
        if (changed) { int rc = kf_upload_slot(h, s); if (rc != ORBX_OK) return rc; }
    }
    return ORBX_OK;
}

int kf_compact(orbx_kf_database *h)
{
    std::vector<int4> plan;
    plan.reserve((size_t)h->nalive);
    std::vector<KfSlot> ns;
    std::vector<long long> nc;
    ns.reserve(h->slots.capacity());
    int at = 0;
    for (int s = 0; s < h->nslots; s++) {
        if (!h->slots[s].alive) continue;
        KfSlot S = h->slots[s];
        plan.push_back(make_int4(S.offset, at, S.len, s));
        S.offset = at;
        at += S.len;
        ns.push_back(S);
        nc.insert(nc.end(), h->covId.begin() + (size_t)s * KF_COV, h->covId.begin() + (size_t)(s + 1) * KF_COV);
    }
    const int n = (int)ns.size();
    if (n) {
        int4 *dplan = nullptr;
        int32_t *tw = nullptr;
        double *tv = nullptr;
        float *tr = nullptr;
        hipError_t e = hipMalloc((void **)&dplan, sizeof(int4) * (size_t)n);
        if (e == hipSuccess) e = hipMalloc((void **)&tw, 4 * (size_t)std::max(at, 1));
        if (e == hipSuccess) e = hipMalloc((void **)&tv, 8 * (size_t)std::max(at, 1));
        if (e == hipSuccess) e = hipMalloc((void **)&tr, 4 * (size_t)n);
        if (e == hipSuccess) e = hipMemcpyAsync(dplan, plan.data(), sizeof(int4) * (size_t)n, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_kfdb_compact, dim3((unsigned)n), dim3(KF_THREADS), 0, h->stream, dplan, h->poolW.p, h->poolV.p, h->reloc[h->cur].p, tw, tv, tr);
            e = hipGetLastError();
        }
        if (e == hipSuccess && at) e = hipMemcpyAsync(h->poolW.p, tw, 4 * (size_t)at, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess && at) e = hipMemcpyAsync(h->poolV.p, tv, 8 * (size_t)at, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h->reloc[h->cur].p, tr, 4 * (size_t)n, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (dplan) (void)hipFree(dplan);
        if (tw) (void)hipFree(tw);
        if (tv) (void)hipFree(tv);
        if (tr) (void)hipFree(tr);
        if (e != hipSuccess) { orbx_set_error("compaction failed: %s", hipGetErrorString(e)); return ORBX_ERR_HIP; }
    }
    h->slots.swap(ns);
    h->slots.resize((size_t)h->maxKf);
    nc.resize((size_t)h->maxKf * KF_COV);
    h->covId.swap(nc);
    h->nslots = h->nalive = n;
    h->cursor = at;
    h->dead = 0;
    h->slotOf.clear();
    h->namedBy.clear();
    for (int s = 0; s < n; s++) h->slotOf[h->slots[s].id] = s;
    for (int s = 0; s < n; s++) {
        kf_resolve(h, s);
        for (int i = 0; i < h->slots[s].ncov; i++) h->namedBy.emplace(h->covId[(size_t)s * KF_COV + i], s);
    }
    if (n) {
        ORBX_HIP_CHECK(hipMemcpyAsync(h->dslots.p, h->slots.data(), sizeof(KfSlot) * (size_t)n, hipMemcpyHostToDevice, h->stream));
        ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    return ORBX_OK;
}

void kf_reset(orbx_kf_database *h)
{
    h->slotOf.clear();
    h->namedBy.clear();
    h->nslots = h->nalive = h->cursor = h->dead = 0;
}
}  // namespace

extern "C" int orbx_kfdb_create(int device, int n_words, int max_keyframes, int max_entries, int max_queries, int max_query_words, orbx_kf_database **out)
{
    if (!out || n_words < 1 || max_keyframes < 1 || max_entries < 1 || max_queries < 1 || max_query_words < 1 || max_query_words > KF_MAX_QUERY_WORDS ||
        (long long)max_queries * max_keyframes > (1ll << 28)) {
        orbx_set_error("bad keyframe database arguments (n_words, max_keyframes, max_entries, max_queries >= 1, 1 <= max_query_words <= %d, max_queries * max_keyframes <= 2^28)",
                       KF_MAX_QUERY_WORDS);
        return ORBX_ERR_ARG;
    }
    *out = nullptr;
    orbx_kf_database *h = new orbx_kf_database();
    h->nWords = n_words; h->maxKf = max_keyframes; h->maxEntries = max_entries; h->maxQueries = max_queries; h->maxQueryWords = max_query_words;
    h->slots.resize((size_t)max_keyframes);
    h->covId.resize((size_t)max_keyframes * KF_COV);
    const size_t per = (size_t)max_queries * (size_t)max_keyframes;
    int rc = h->open(device);
    if (rc == ORBX_OK) rc = h->timer.create();
    for (int i = 0; i < 4 && rc == ORBX_OK; i++) rc = orbx_event_create(&h->pev[i]);
    if (rc == ORBX_OK) rc = h->poolW.ensure((size_t)max_entries);
    if (rc == ORBX_OK) rc = h->poolV.ensure((size_t)max_entries);
    if (rc == ORBX_OK) rc = h->dslots.ensure((size_t)max_keyframes);
    if (rc == ORBX_OK) rc = h->reloc[0].ensure((size_t)max_keyframes);
    if (rc == ORBX_OK) rc = h->reloc[1].ensure((size_t)max_keyframes);
    if (rc == ORBX_OK) rc = h->work.ensure(10 * per + 2 * (size_t)max_queries + 64);
    if (rc == ORBX_OK) rc = h->key.ensure(per);
    if (rc != ORBX_OK) { orbx_kfdb_destroy(h); return rc; }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_kfdb_destroy(orbx_kf_database *h) { orbx_destroy_handle(h); }

extern "C" int orbx_kfdb_add(orbx_kf_database *h, int64_t id, const int32_t *words, const double *values, int n)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = kf_check_words(h, words, values, n, "orbx_kfdb_add")) != ORBX_OK) return rc;
    if (h->slotOf.count((long long)id)) { orbx_set_error("orbx_kfdb_add: keyframe %lld is in the database", (long long)id); return ORBX_ERR_STATE; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const bool noRoom = h->nslots >= h->maxKf || (long long)h->cursor + n > h->maxEntries;
    if (h->nslots > h->nalive && ((long long)h->dead * 2 > h->cursor || noRoom || h->nalive == 0)) {      // dead entries exceed half of those in use, or the room is needed
        if ((rc = kf_compact(h)) != ORBX_OK) return rc;
    }
    if (h->nslots >= h->maxKf || (long long)h->cursor + n > h->maxEntries) {
        orbx_set_error("orbx_kfdb_add: database full (%d / %d keyframes, %d + %d / %d entries)", h->nslots, h->maxKf, h->cursor, n, h->maxEntries);
        return ORBX_ERR_CAPACITY;
    }
    const int s = h->nslots;
    KfSlot &S = h->slots[s];
    memset(&S, 0, sizeof(S));
    S.id = (long long)id; S.seq = h->nextSeq++; S.offset = h->cursor; S.len = n; S.alive = 1; S.ncov = 0;
    for (int i = 0; i < KF_COV; i++) S.cov[i] = -1;
    static const float zero = 0.f;      // mRelocScore of a keyframe that no query has scored (uninitialised in the reference)
    if (n) {
        ORBX_HIP_CHECK(hipMemcpyAsync(h->poolW.p + h->cursor, words, 4 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        ORBX_HIP_CHECK(hipMemcpyAsync(h->poolV.p + h->cursor, values, 8 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    }
    ORBX_HIP_CHECK(hipMemcpyAsync(h->reloc[h->cur].p + s, &zero, 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = kf_upload_slot(h, s)) != ORBX_OK) return rc;
    h->nslots++; h->nalive++; h->cursor += n;
    h->slotOf[(long long)id] = s;
    if ((rc = kf_retarget(h, (long long)id, s)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    return ORBX_OK;
}

extern "C" int orbx_kfdb_erase(orbx_kf_database *h, int64_t id)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    auto it = h->slotOf.find((long long)id);
    if (it == h->slotOf.end()) return ORBX_OK;
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const int s = it->second;
    h->slotOf.erase(it);
    h->slots[s].alive = 0;
    h->nalive--;
    h->dead += h->slots[s].len;
    int rc;
    if ((rc = kf_upload_slot(h, s)) != ORBX_OK) return rc;
    if ((rc = kf_retarget(h, (long long)id, -1)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    return ORBX_OK;
}

extern "C" int orbx_kfdb_clear(orbx_kf_database *h)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    kf_reset(h);
    return ORBX_OK;
}

extern "C" int orbx_kfdb_set_covisibles(orbx_kf_database *h, int64_t id, const int64_t *ids, int n)
{
    if (!h || n < 0 || n > KF_COV || (n > 0 && !ids)) { orbx_set_error("orbx_kfdb_set_covisibles: NULL argument or n outside 0..%d", KF_COV); return ORBX_ERR_ARG; }
    auto it = h->slotOf.find((long long)id);
    if (it == h->slotOf.end()) { orbx_set_error("orbx_kfdb_set_covisibles: keyframe %lld is not in the database", (long long)id); return ORBX_ERR_STATE; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const int s = it->second;
    KfSlot &S = h->slots[s];
    S.ncov = n;
    for (int i = 0; i < KF_COV; i++) S.cov[i] = -1;
    for (int i = 0; i < n; i++) {
        h->covId[(size_t)s * KF_COV + i] = (long long)ids[i];
        bool known = false;      // a keyframe whose covisibles are pushed again and again names the same ids: one entry per (id, slot)
        auto range = h->namedBy.equal_range((long long)ids[i]);
        for (auto nb = range.first; nb != range.second && !known; ++nb) known = nb->second == s;
        if (!known) h->namedBy.emplace((long long)ids[i], s);
    }
    kf_resolve(h, s);
    int rc;
    if ((rc = kf_upload_slot(h, s)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    return ORBX_OK;
}

extern "C" int orbx_kfdb_size(orbx_kf_database *h, int *keyframes, int *entries, int *dead_entries)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (keyframes) *keyframes = h->nalive;
    if (entries) *entries = h->cursor;
    if (dead_entries) *dead_entries = h->dead;
    return ORBX_OK;
}

extern "C" int orbx_kfdb_reloc_score(orbx_kf_database *h, int64_t id, float *score)
{
    if (!h || !score) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    auto it = h->slotOf.find((long long)id);
    if (it == h->slotOf.end()) { orbx_set_error("orbx_kfdb_reloc_score: keyframe %lld is not in the database", (long long)id); return ORBX_ERR_STATE; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    ORBX_HIP_CHECK(hipMemcpyAsync(score, h->reloc[h->cur].p + it->second, 4, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    return ORBX_OK;
}

extern "C" int orbx_kfdb_query(orbx_kf_database *h, const orbx_kfdb_query_t *queries, int nq, const orbx_kfdb_result *results)
{
    if (!h || !queries || !results || nq < 1) { orbx_set_error("orbx_kfdb_query: NULL argument or nq < 1"); return ORBX_ERR_ARG; }
    if (nq > h->maxQueries) { orbx_set_error("orbx_kfdb_query: %d queries, the handle takes %d", nq, h->maxQueries); return ORBX_ERR_CAPACITY; }
    int rc;
    size_t nw = 0, nc = 0, nsorted = 0;
    int maxn = 0;
    for (int q = 0; q < nq; q++) {
        const orbx_kfdb_query_t &Q = queries[q];
        if (Q.mode != ORBX_KFDB_LOOP && Q.mode != ORBX_KFDB_RELOC) { orbx_set_error("orbx_kfdb_query: query %d: unknown mode %d", q, Q.mode); return ORBX_ERR_ARG; }
        if ((rc = kf_check_words(h, Q.words, Q.values, Q.n, "orbx_kfdb_query")) != ORBX_OK) return rc;
        if (Q.capacity < 0) { orbx_set_error("orbx_kfdb_query: query %d: capacity < 0", q); return ORBX_ERR_ARG; }
        if (Q.mode == ORBX_KFDB_LOOP && (Q.n_connected < 0 || (Q.n_connected > 0 && (!Q.connected || !Q.connected_counts)))) {
            orbx_set_error("orbx_kfdb_query: query %d: n_connected < 0 or NULL connected / connected_counts", q);
            return ORBX_ERR_ARG;
        }
    }
    for (int q = 0; q < nq; q++) {
        if (queries[q].n > h->maxQueryWords) { orbx_set_error("orbx_kfdb_query: query %d has %d words, the handle takes %d", q, queries[q].n, h->maxQueryWords); return ORBX_ERR_CAPACITY; }
        nw += (size_t)queries[q].n;
        maxn = std::max(maxn, queries[q].n);
        if (queries[q].mode == ORBX_KFDB_LOOP) nc += (size_t)queries[q].n_connected;
    }
    const int Ns = h->nslots;
    h->timer.timed = false;
    if (Ns == 0) {      // an empty database: nothing is launched
        for (int q = 0; q < nq; q++) {
            const orbx_kfdb_query_t &Q = queries[q];
            const orbx_kfdb_result &R = results[q];
            const float ms = Q.mode == ORBX_KFDB_LOOP ? Q.min_score_in : 0.f;
            if (R.n_sharing) *R.n_sharing = 0;
            if (R.max_common_words) *R.max_common_words = 0;
            if (R.min_common_words) *R.min_common_words = 0;
            if (R.min_score) *R.min_score = ms;
            if (R.connected_score && Q.mode == ORBX_KFDB_LOOP) for (int j = 0; j < Q.n_connected; j++) R.connected_score[j] = -1.f;
            if (R.n_scored) *R.n_scored = 0;
            if (R.n_kept) *R.n_kept = 0;
            if (R.best_acc_score) *R.best_acc_score = ms;
            if (R.n_candidates) *R.n_candidates = 0;
        }
        return ORBX_OK;
    }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    // the call's inputs: query table, words, values, connected slots (caller order and sorted), counts
    std::vector<KfQuery> qs((size_t)nq);
    std::vector<int32_t> connSlot(nc ? nc : 1), connCount(nc ? nc : 1), connSorted(nc ? nc : 1);
    size_t outTotal = 0;
    {
        size_t wo = 0, co = 0;
        for (int q = 0; q < nq; q++) {
            const orbx_kfdb_query_t &Q = queries[q];
            KfQuery &K = qs[(size_t)q];
            const bool loop = Q.mode == ORBX_KFDB_LOOP;
            K.mode = Q.mode; K.n = Q.n; K.qoff = (int32_t)wo; K.nconn = loop ? Q.n_connected : 0; K.coff = (int32_t)co; K.soff = (int32_t)nsorted;
            K.minScoreIn = Q.min_score_in;
            int ns = 0;
            for (int j = 0; j < K.nconn; j++) {
                auto it = h->slotOf.find((long long)Q.connected[j]);
                const int s = it == h->slotOf.end() ? -1 : it->second;
                connSlot[co + j] = s;
                connCount[co + j] = Q.connected_counts[j];
                if (s >= 0) connSorted[nsorted + ns++] = s;
            }
            std::sort(connSorted.begin() + nsorted, connSorted.begin() + nsorted + ns);
            K.nsorted = ns;
            nsorted += (size_t)ns;
            K.outOff = outTotal;
            outTotal += kf_out_layout(Ns, K.nconn).total;
            wo += (size_t)Q.n; co += (size_t)K.nconn;
        }
    }
    OrbxCallBox &bx = h->box;
    auto [pin, pout] = bx.plan();
    const auto sQs = pin.add(qs.data(), (size_t)nq);
    const auto sW = pin.hole<int32_t>(nw);      // the queries' words and values, concatenated: filled below
    const auto sV = pin.hole<double>(nw);
    const auto sCs = pin.add(connSlot.data(), nc), sCc = pin.add(connCount.data(), nc), sSo = pin.add(connSorted.data(), nsorted);
    const auto rOut = pout.hole<uint8_t>(outTotal);      // the queries' kf_out_layout blocks
    const OrbxStaged sg = bx.begin(h->stream, &rc);
    if (rc != ORBX_OK) return rc;
    {
        size_t wo = 0;
        for (int q = 0; q < nq; q++) {
            orbx_put_at(sg, sW, wo, queries[q].words, (size_t)queries[q].n);
            orbx_put_at(sg, sV, wo, queries[q].values, (size_t)queries[q].n);
            wo += (size_t)queries[q].n;
        }
    }
    if ((rc = h->timer.begin(h->stream)) != ORBX_OK) return rc;
    uint8_t *A;
    if ((rc = orbx_stage_to_arena(bx, h->arena, h->stream, 256, &A)) != ORBX_OK) return rc;
    ORBX_LAUNCH_CHECK();

    KfDev D;
    const size_t per = (size_t)nq * (size_t)Ns;
    D.Ns = Ns; D.nq = nq;
    D.slots = h->dslots.p; D.poolW = h->poolW.p; D.poolV = h->poolV.p;
    D.relocOld = h->reloc[h->cur].p; D.relocNew = h->reloc[h->cur ^ 1].p;
    D.qs = sQs.in(A); D.qwords = sW.in(A); D.qvalues = sV.in(A);
    D.connSlot = sCs.in(A); D.connCount = sCc.in(A); D.connSorted = sSo.in(A);
    int32_t *W = h->work.p;
    D.words = W; D.first = W + per; D.flag = W + 2 * per; D.firstocc = W + 3 * per; D.score = (float *)(W + 4 * per);
    D.list = W + 5 * per; D.order = W + 6 * per; D.lsm = W + 7 * per; D.best = W + 8 * per; D.acc = (float *)(W + 9 * per);
    D.counters = W + 10 * (size_t)h->maxQueries * (size_t)h->maxKf;
    D.key = h->key.p;
    D.out = sg.dev(rOut);

    ORBX_HIP_CHECK(hipMemsetAsync(D.counters, 0, 8 * (size_t)nq, h->stream));
    h->profiled = false;
    if (h->profile) ORBX_HIP_CHECK(hipEventRecord(h->pev[0], h->stream));
    const dim3 grid((unsigned)((Ns + KF_SLOTS_PER_BLOCK - 1) / KF_SLOTS_PER_BLOCK), (unsigned)nq);
    const size_t lds = 4 * (size_t)std::max(maxn, 1);
    hipLaunchKernelGGL(k_kfdb_intersect, grid, dim3(KF_THREADS), lds, h->stream, D);
    ORBX_LAUNCH_CHECK();
    if (h->profile) ORBX_HIP_CHECK(hipEventRecord(h->pev[1], h->stream));
    hipLaunchKernelGGL(k_kfdb_score, grid, dim3(KF_THREADS), lds, h->stream, D);
    ORBX_LAUNCH_CHECK();
    if (h->profile) ORBX_HIP_CHECK(hipEventRecord(h->pev[2], h->stream));
    hipLaunchKernelGGL(k_kfdb_commit, dim3((unsigned)((Ns + KF_THREADS - 1) / KF_THREADS)), dim3(KF_THREADS), 0, h->stream, D);
    ORBX_LAUNCH_CHECK();
    if (h->profile) ORBX_HIP_CHECK(hipEventRecord(h->pev[3], h->stream));
    const unsigned long long seq = bx.arm();
    hipLaunchKernelGGL(k_kfdb_select, dim3((unsigned)nq), dim3(KF_SEL_THREADS), 0, h->stream, D, bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_CHECK();
    h->timer.launches = 5;
    if ((rc = h->timer.end(h->stream)) != ORBX_OK) return rc;
    h->profiled = h->profile;
    if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;
    h->cur ^= 1;      // the scores of this call's relocalisation queries are the state now

    for (int q = 0; q < nq; q++) {      // nothing is written when one list does not fit
        const int32_t *hi = (const int32_t *)(sg.host(rOut) + qs[(size_t)q].outOff);
        const orbx_kfdb_result &R = results[q];
        const int cap = queries[q].capacity;
        if (((R.scored_id || R.scored_words || R.scored_score) && hi[3] > cap) || ((R.kept || R.acc_score || R.best_id) && hi[4] > cap) || (R.candidates && hi[5] > cap)) {
            orbx_set_error("orbx_kfdb_query: query %d: %d scored, %d kept, %d candidates for a capacity of %d (the query has run: reloc scores are updated)", q, hi[3], hi[4],
                           hi[5], cap);
            return ORBX_ERR_CAPACITY;
        }
    }
    for (int q = 0; q < nq; q++) {
        const KfQuery &K = qs[(size_t)q];
        const uint8_t *o = sg.host(rOut) + K.outOff;
        const int32_t *hi = (const int32_t *)o;
        const float *hf = (const float *)o;
        const KfOutOff O = kf_out_layout(Ns, K.nconn);
        const orbx_kfdb_result &R = results[q];
        const size_t M = (size_t)hi[3], E = (size_t)hi[4], C = (size_t)hi[5];
        if (R.n_sharing) *R.n_sharing = hi[0];
        if (R.max_common_words) *R.max_common_words = hi[1];
        if (R.min_common_words) *R.min_common_words = hi[2];
        if (R.min_score) *R.min_score = hf[6];
        if (R.connected_score && K.nconn) memcpy(R.connected_score, o + O.conn, 4 * (size_t)K.nconn);
        if (R.scored_id && M) memcpy(R.scored_id, o + O.sid, 8 * M);
        if (R.scored_words && M) memcpy(R.scored_words, o + O.swords, 4 * M);
        if (R.scored_score && M) memcpy(R.scored_score, o + O.sscore, 4 * M);
        if (R.n_scored) *R.n_scored = hi[3];
        if (R.kept && E) memcpy(R.kept, o + O.kept, 4 * E);
        if (R.acc_score && E) memcpy(R.acc_score, o + O.acc, 4 * E);
        if (R.best_id && E) memcpy(R.best_id, o + O.bid, 8 * E);
        if (R.n_kept) *R.n_kept = hi[4];
        if (R.best_acc_score) *R.best_acc_score = hf[7];
        if (R.candidates && C) memcpy(R.candidates, o + O.cand, 8 * C);
        if (R.n_candidates) *R.n_candidates = hi[5];
    }
    return ORBX_OK;
}

extern "C" int orbx_kfdb_last_timing(orbx_kf_database *h, float *device_ms, int *launches)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    return h->timer.read(h->device, device_ms, launches, nullptr);      // zeros when no chain ran (no call yet, or an empty database)
}

extern "C" int orbx_kfdb_stage_timing(orbx_kf_database *h, int enable, float *stage_ms)
{
    if (!h) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (stage_ms) {
        if (!h->timer.timed || !h->profiled) { orbx_set_error("orbx_kfdb_stage_timing: the last query was not profiled"); return ORBX_ERR_STATE; }
        ORBX_HIP_CHECK(hipSetDevice(h->device));
        ORBX_HIP_CHECK(hipEventSynchronize(h->timer.ev[1]));
        hipEvent_t e[6] = {h->timer.ev[0], h->pev[0], h->pev[1], h->pev[2], h->pev[3], h->timer.ev[1]};
        for (int i = 0; i < 5; i++) ORBX_HIP_CHECK(hipEventElapsedTime(&stage_ms[i], e[i], e[i + 1]));
    }
    h->profile = enable != 0;
    return ORBX_OK;
}
