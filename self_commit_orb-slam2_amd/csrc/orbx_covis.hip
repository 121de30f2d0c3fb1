// orbx_covis.hip -- the counting inside KeyFrame::UpdateConnections, Tracking::UpdateLocalKeyFrames and LocalMapping::KeyFrameCulling (gfx950 only).
//
// Reference: src/KeyFrame.cc:386-507, src/Tracking.cc:1895-1955, src/LocalMapping.cc:873-956.  All three count integers over ragged observation
// lists; the pointer-graph bookkeeping around them (AddConnection, the spanning tree, SetBadFlag) stays with the host.  A call is stateless: the map
// slice comes in host arrays (include/orbx.h), goes through mapped pinned memory (OrbxCallBox: no copy engine, no stream synchronisation) and is copied
// once into device memory by k_stage_copy, because a point observed from several lists is read several times.
//
// The order of std::map<KeyFrame*, ...> is the caller's kf_rank.  The host sorts the ranks once per call (that also finds duplicates) and the kernels
// work on POSITIONS in that order: a histogram indexed by position comes out in the map's iteration order without a sort.
//
//   k_covis_connect<true>   one workgroup per list, NK <= COVIS_LDS_NK: the histogram (one int per keyframe slot) and the counter's keys live in LDS
//   k_covis_connect<false>  NK beyond: the same code on one global-memory row of NK ints per workgroup (at most COVIS_GLOBAL_BLOCKS workgroups stride
//                           over the lists)
//       vote (a thread per list entry walks the point's observers) -> order-keeping compaction of the non-zero bins 256 at a time (the counter, as
//       (slot, weight) in ascending rank) with the arg-max key (weight, lowest position) on the way -> the connections with weight >= th placed by
//       counting the greater keys (weight << 32 | position: distinct, so the place is exact; a keyframe has tens of connections, the quadratic
//       count is shorter than a sort's barriers).  Every list owns a worst-case region of the outputs (min(NK, observations under its entries)
//       pairs, known to the host from the offsets alone), so the lists need no prefix sum across workgroups; the host packs the regions into
//       the caller's CSR arrays and checks the capacities before it writes anything.
//
//   culling: the loop of :884-955 is sequential only through its culls.  k_covis_cull_init derives Observations() from the lists; a round is
//   k_covis_cull_eval over every undecided list against the current masks - its last workgroup to finish (an arrival counter, nobody waits for
//   anybody) hands the first list that is culled AND erasable to the host through the mapped record - and, if there is one, k_covis_cull_apply
//   with that keyframe's erase; everything up to that list is final, the lists behind it are evaluated again.  A culled keyframe with
//   mbNotErase changes nothing, so it ends no round.  c erasing culls: 1 staging + 1 init + (c + 1) eval + c apply launches and c + 1 waits (the
//   last eval is not needed when the last cull is the last list: then the apply publishes).
#include <algorithm>
#include <climits>
#include <numeric>
#include <vector>

#include "orbx_handle.h"

#define COVIS_THREADS 256
#define COVIS_LDS_NK ORBX_COVIS_LDS_KEYFRAMES      /* 12 bytes of LDS per slot: 48 KB per workgroup at the limit */
#define COVIS_GLOBAL_BLOCKS 64
#define COVIS_MAX_BLOCKS 4096

namespace {

struct CvDev {
    int NK, M, Q, th;
    const int32_t *pos, *slotAt;      // [NK] slot -> position in ascending rank, and back
    const uint8_t *flags;             // [NK]
    const int32_t *obsOff, *obsKf;    // [M + 1], [T]
    const uint8_t *obsOct, *obsSt, *ptBad;
    const int32_t *listOff, *listKf, *listPt;
    const uint8_t *listOct, *listClose;
    const int32_t *outOff;            // [Q + 1] first pair of each list's worst-case output region
    int32_t *hist;                    // k_covis_connect<false>: gridDim.x rows of NK
    unsigned long long *keys;         // k_covis_connect<false>: [outOff[Q]] weight << 32 | position of the counter's entries
    int32_t *head;                    // mapped [Q][4]: n_counter, n_max, kf_max, n_conn
    int32_t *cnt, *conn;              // mapped [outOff[Q]][2]: (slot, weight)
    uint8_t *state;                   // [M] bit 0 bad, bit 1 observations cleared (the point went bad through an erase)
    int32_t *nobs;                    // [M] Observations()
    uint8_t *erased;                  // [NK]
    int32_t *firstCull;               // device word
    int32_t *record;                  // mapped: [0] the round's first erasing cull or INT_MAX
    int32_t *res;                     // mapped [Q][3]: n_mps, n_redundant, culled
    int32_t *outObs;                  // mapped [M]
    uint8_t *outBad;                  // mapped [M]
};

template <bool LDS> __global__ __launch_bounds__(COVIS_THREADS) void k_covis_connect(CvDev D, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    extern __shared__ __attribute__((aligned(16))) int32_t cvLds[];
    __shared__ int sW[4];
    __shared__ unsigned long long sBest[4];
    __shared__ int sSel;
    int32_t *hist = LDS ? cvLds : D.hist + (size_t)blockIdx.x * (size_t)D.NK;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, NK = D.NK;
    unsigned long long *ldsKeys = (unsigned long long *)(cvLds + ((NK + 1) & ~1));      // LDS path: the counter's keys behind the histogram, [NK]
    for (int q = blockIdx.x; q < D.Q; q += gridDim.x) {
        for (int i = t; i < NK; i += COVIS_THREADS) hist[i] = 0;
        if (t == 0) sSel = 0;
        __syncthreads();
        const int owner = D.listKf[q], e1 = D.listOff[q + 1];
        for (int e = D.listOff[q] + t; e < e1; e += COVIS_THREADS) {
            const int p = D.listPt[e];
            if (D.ptBad[p]) continue;
            const int o1 = D.obsOff[p + 1];
            for (int o = D.obsOff[p]; o < o1; o++) {
                const int k = D.obsKf[o];
                if (k != owner) atomicAdd(&hist[D.pos[k]], 1);
            }
        }
        __syncthreads();
        // the counter in ascending rank; the arg-max key prefers the lowest position among equal weights (`>` is strict, :445-453)
        const size_t base = (size_t)D.outOff[q];
        unsigned long long *keys = LDS ? ldsKeys : D.keys + base;      // read n times by the placement below: LDS broadcasts where they fit
        int n = 0;
        unsigned long long best = 0;
        for (int c0 = 0; c0 < NK; c0 += COVIS_THREADS) {
            const int i = c0 + t;
            // (the global row was written by atomics, which live in L2: read it there too)
            const int wgt = i >= NK ? 0 : LDS ? hist[i] : __hip_atomic_load(&hist[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool v = wgt != 0;
            const unsigned long long m = __ballot(v);
            int rank = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) sW[w] = __popcll(m);
            __syncthreads();
            int tot = 0;
            for (int j = 0; j < 4; j++) { if (j < w) rank += sW[j]; tot += sW[j]; }
            if (v) {
                const size_t at = base + (size_t)(n + rank);
                const int slot = D.slotAt[i];
                keys[n + rank] = (unsigned long long)(unsigned)wgt << 32 | (unsigned)i;
                D.cnt[2 * at] = slot; D.cnt[2 * at + 1] = wgt;
                if (owner >= 0 || !(D.flags[slot] & 4)) {      // Tracking.cc:1941: a bad keyframe is no candidate of a Frame's vote
                    const unsigned long long key = (unsigned long long)(unsigned)wgt << 32 | (0xffffffffu - (unsigned)i);
                    best = key > best ? key : best;
                }
            }
            n += tot;
            __syncthreads();
        }
        best = wave_max(best);
        if (lane == 0) sBest[w] = best;
        int sel = 0;
        for (int i = t; i < n; i += COVIS_THREADS) sel += (int)(keys[i] >> 32) >= D.th ? 1 : 0;      // (own workgroup's stores, behind a barrier)
        if (sel) atomicAdd(&sSel, sel);
        __syncthreads();
        for (int j = 0; j < 4; j++) best = sBest[j] > best ? sBest[j] : best;
        const int nMax = (int)(best >> 32), kfMax = best ? D.slotAt[0xffffffffu - (unsigned)(best & 0xffffffffu)] : -1;
        const int nSel = sSel;
        if (nSel == 0) {
            if (t == 0 && kfMax >= 0) { D.conn[2 * base] = kfMax; D.conn[2 * base + 1] = nMax; }
        } else {
            for (int i = t; i < n; i += COVIS_THREADS) {
                const unsigned long long key = keys[i];
                if ((int)(key >> 32) < D.th) continue;
                int place = 0;      // descending weight, descending rank within a weight: sort + push_front of pair<int, KeyFrame*>
                for (int j = 0; j < n; j++) place += keys[j] > key ? 1 : 0;
                const size_t at = base + (size_t)place;
                D.conn[2 * at] = D.slotAt[(unsigned)(key & 0xffffffffu)]; D.conn[2 * at + 1] = (int)(key >> 32);
            }
        }
        if (t == 0) {
            int32_t *h = D.head + (size_t)q * 4;
            h[0] = n; h[1] = nMax; h[2] = kfMax; h[3] = nSel ? nSel : (kfMax >= 0 ? 1 : 0);
        }
        __syncthreads();      // sSel, sBest and the histogram are reused by the next list
    }
    orbx_publish(counter, flag, seq, gridDim.x);
}

// Observations() of every point (MapPoint.cc:154-200: 2 for a stereo observation), the mutable masks, and the outputs as they stand without a cull
__global__ __launch_bounds__(COVIS_THREADS) void k_covis_cull_init(CvDev D)
{
    const int g = blockIdx.x * COVIS_THREADS + threadIdx.x;
    if (g < D.M) {
        int s = 0;
        const int o1 = D.obsOff[g + 1];
        for (int o = D.obsOff[g]; o < o1; o++) s += D.obsSt[o] ? 2 : 1;
        const uint8_t b = D.ptBad[g] ? 1 : 0;
        D.nobs[g] = s; D.state[g] = b;
        D.outObs[g] = s; D.outBad[g] = b;
    }
    if (g < D.NK) D.erased[g] = 0;
    if (g == 0) *D.firstCull = INT_MAX;
    __threadfence_system();
}

// lists first .. Q-1 against the current masks, one workgroup each
__global__ __launch_bounds__(COVIS_THREADS) void k_covis_cull_eval(CvDev D, int first, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    __shared__ int sN, sR;
    const int t = threadIdx.x, q = first + (int)blockIdx.x;
    const int owner = D.listKf[q];
    const uint8_t fl = D.flags[owner];
    if (t == 0) { sN = 0; sR = 0; }
    __syncthreads();
    if (!(fl & 1)) {      // mnId == 0 is never culled (:889)
        int n = 0, r = 0;
        const int e1 = D.listOff[q + 1];
        for (int e = D.listOff[q] + t; e < e1; e += COVIS_THREADS) {
            const int p = D.listPt[e];
            if ((D.state[p] & 1) || !D.listClose[e]) continue;
            n++;
            if (D.nobs[p] <= 3) continue;
            const int lim = (int)D.listOct[e] + 1, o1 = D.obsOff[p + 1];
            int c = 0;
            for (int o = D.obsOff[p]; o < o1; o++) {
                const int k = D.obsKf[o];
                c += (k != owner && !D.erased[k] && (int)D.obsOct[o] <= lim) ? 1 : 0;
            }
            r += c >= 3 ? 1 : 0;
        }
        for (int s = 32; s >= 1; s >>= 1) { n += __shfl_xor(n, s); r += __shfl_xor(r, s); }
        if ((t & 63) == 0) { atomicAdd(&sN, n); atomicAdd(&sR, r); }
    }
    __syncthreads();
    if (t == 0) {
        const int n = sN, r = sR;
        const bool culled = !(fl & 1) && (double)r > 0.9 * (double)n;      // the double product of :951
        int32_t *o = D.res + (size_t)q * 3;
        o[0] = n; o[1] = r; o[2] = culled ? 1 : 0;
        if (culled && !(fl & 2)) atomicMin(D.firstCull, q);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {      // the last workgroup to arrive: nobody waits
            __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            D.record[0] = __hip_atomic_load(D.firstCull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(D.firstCull, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// the erase of list `f`'s keyframe (KeyFrame::SetBadFlag -> MapPoint::EraseObservation, KeyFrame.cc:640-642, MapPoint.cc:171-200): a thread per point
__global__ __launch_bounds__(COVIS_THREADS) void k_covis_cull_apply(CvDev D, int f, unsigned *counter, unsigned long long *flag, unsigned long long seq)
{
    const int g = blockIdx.x * COVIS_THREADS + threadIdx.x;
    const int k = D.listKf[f];
    if (g < D.M && !(D.state[g] & 2)) {
        const int o1 = D.obsOff[g + 1];
        for (int o = D.obsOff[g]; o < o1; o++) {
            if (D.obsKf[o] != k) continue;
            const int v = D.nobs[g] - (D.obsSt[o] ? 2 : 1);
            D.nobs[g] = v; D.outObs[g] = v;
            if (v <= 2) { D.state[g] = 3; D.outBad[g] = 1; }      // SetBadFlag of the point: bad, and its observations are gone
            break;
        }
    }
    if (g == 0) D.erased[k] = 1;
    __threadfence_system();
    if (seq) orbx_publish(counter, flag, seq, gridDim.x);
}

}  // namespace

struct orbx_covis : OrbxHandle {
    OrbxCallTimer timer;
    OrbxCallBox box;
    OrbxOwnedBuf<uint8_t> arena;              // the call's inputs in device memory
    OrbxOwnedBuf<unsigned long long> work;    // keys | global histogram rows | culling state
    OrbxWorkPlan workPlan;                    // layout of the culling state inside `work`
    std::vector<int32_t> order, pos, outOff;
    std::vector<uint8_t> seen;
};

extern "C" int orbx_covis_create(int device, orbx_covis **out)
{
    if (!out) { orbx_set_error("orbx_covis_create: NULL argument"); return ORBX_ERR_ARG; }
    *out = nullptr;
    orbx_covis *h = new orbx_covis();
    int rc;
    if ((rc = h->open(device)) || (rc = h->timer.create())) { orbx_destroy_handle(h); return rc; }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_covis_destroy(orbx_covis *h) { orbx_destroy_handle(h); }

namespace {

// everything a kernel indexes with is checked here, before anything is launched
// (the slice is checked before the handle is looked at: a bad slice is reported as such on a machine without a device too)
int cv_validate(orbx_covis *h, const orbx_covis_slice *s, bool culling, const char *who)
{
    if (!s) { orbx_set_error("%s: NULL slice", who); return ORBX_ERR_ARG; }
    std::vector<int32_t> ownOrder, ownPos;
    std::vector<uint8_t> ownSeen;
    std::vector<int32_t> &order = h ? h->order : ownOrder, &pos = h ? h->pos : ownPos;
    std::vector<uint8_t> &seen = h ? h->seen : ownSeen;
    const int NK = s->num_keyframes, M = s->num_points, T = s->num_obs, Q = s->num_lists, S = s->num_entries;
    if (NK < 1 || M < 0 || T < 0 || Q < 1 || S < 0) { orbx_set_error("%s: num_keyframes < 1, num_lists < 1 or a negative size", who); return ORBX_ERR_ARG; }
    if (!s->kf_rank || !s->kf_flags || !s->obs_offset || !s->list_offset || !s->list_kf || (M > 0 && !s->point_bad) ||
        (T > 0 && (!s->obs_kf || (culling && (!s->obs_octave || !s->obs_stereo)))) || (S > 0 && (!s->list_point || (culling && (!s->list_octave || !s->list_close))))) {
        orbx_set_error("%s: NULL slice array", who);
        return ORBX_ERR_ARG;
    }
    if (s->obs_offset[0] != 0 || s->list_offset[0] != 0) { orbx_set_error("%s: an offset array does not start at 0", who); return ORBX_ERR_ARG; }
    for (int p = 0; p < M; p++)
        if (s->obs_offset[p + 1] < s->obs_offset[p]) { orbx_set_error("%s: obs_offset decreases at point %d", who, p); return ORBX_ERR_ARG; }
    if (s->obs_offset[M] != T) { orbx_set_error("%s: obs_offset[num_points] = %d, num_obs = %d", who, s->obs_offset[M], T); return ORBX_ERR_ARG; }
    for (int q = 0; q < Q; q++)
        if (s->list_offset[q + 1] < s->list_offset[q]) { orbx_set_error("%s: list_offset decreases at list %d", who, q); return ORBX_ERR_ARG; }
    if (s->list_offset[Q] != S) { orbx_set_error("%s: list_offset[num_lists] = %d, num_entries = %d", who, s->list_offset[Q], S); return ORBX_ERR_ARG; }
    for (int o = 0; o < T; o++)
        if (s->obs_kf[o] < 0 || s->obs_kf[o] >= NK) { orbx_set_error("%s: obs_kf[%d] = %d is no keyframe slot (0..%d)", who, o, s->obs_kf[o], NK - 1); return ORBX_ERR_ARG; }
    for (int e = 0; e < S; e++)
        if (s->list_point[e] < 0 || s->list_point[e] >= M) { orbx_set_error("%s: list_point[%d] = %d is no point (0..%d)", who, e, s->list_point[e], M - 1); return ORBX_ERR_ARG; }
    seen.assign((size_t)NK, 0);
    for (int q = 0; q < Q; q++) {
        const int k = s->list_kf[q];
        if (k < (culling ? 0 : -1) || k >= NK) { orbx_set_error("%s: list_kf[%d] = %d is no keyframe slot", who, q, k); return ORBX_ERR_ARG; }
        if (culling) {
            if (seen[(size_t)k]) { orbx_set_error("%s: keyframe slot %d owns two lists", who, k); return ORBX_ERR_ARG; }
            seen[(size_t)k] = 1;
        }
    }
    // the order of std::map<KeyFrame*, ...>
    order.resize((size_t)NK);
    std::iota(order.begin(), order.end(), 0);
    const int32_t *rk = s->kf_rank;
    std::sort(order.begin(), order.end(), [rk](int32_t a, int32_t b) { return rk[a] < rk[b]; });
    for (int i = 1; i < NK; i++)
        if (rk[order[(size_t)i]] == rk[order[(size_t)i - 1]]) {
            orbx_set_error("%s: keyframe slots %d and %d have the same rank %d", who, order[(size_t)i - 1], order[(size_t)i], rk[order[(size_t)i]]);
            return ORBX_ERR_ARG;
        }
    pos.resize((size_t)NK);
    for (int i = 0; i < NK; i++) pos[(size_t)order[(size_t)i]] = i;
    if (!h) { orbx_set_error("%s: NULL handle", who); return ORBX_ERR_ARG; }
    return ORBX_OK;
}

// the slice's place in the call box: planned before the box's begin() ...
struct CvSlots {
    OrbxSlot<int32_t, ORBX_STAGE_IN> pos, slotAt, obsOff, obsKf, listOff, outOff, listKf, listPt;
    OrbxSlot<uint8_t, ORBX_STAGE_IN> flags, ptBad, obsOct, obsSt, listOct, listClose;
    CvSlots(OrbxInPlan &pin, const orbx_covis *h, const orbx_covis_slice *s, bool culling)
    {
        const size_t NK = (size_t)s->num_keyframes, M = (size_t)s->num_points, T = (size_t)s->num_obs, Q = (size_t)s->num_lists, S = (size_t)s->num_entries;
        pos = pin.add(h->pos.data(), NK);
        slotAt = pin.add(h->order.data(), NK);
        flags = pin.add(s->kf_flags, NK);
        obsOff = pin.add(s->obs_offset, M + 1);
        obsKf = pin.add(s->obs_kf, T);
        ptBad = pin.add(s->point_bad, M);
        listOff = pin.add(s->list_offset, Q + 1);
        outOff = pin.add(h->outOff.data(), Q + 1);
        listKf = pin.add(s->list_kf, Q);
        listPt = pin.add(s->list_point, S);
        obsOct = pin.add(s->obs_octave, culling ? T : 0);
        obsSt = pin.add(s->obs_stereo, culling ? T : 0);
        listOct = pin.add(s->list_octave, culling ? S : 0);
        listClose = pin.add(s->list_close, culling ? S : 0);
    }
};

// ... and behind it copied into the arena by k_stage_copy; D's input pointers address the arena
int cv_stage(orbx_covis *h, const orbx_covis_slice *s, bool culling, const CvSlots &I, CvDev &D)
{
    int rc;
    uint8_t *A;
    if ((rc = orbx_stage_to_arena(h->box, h->arena, h->stream, 256, &A)) != ORBX_OK) return rc;
    ORBX_LAUNCH_COUNT(h->timer);
    D.NK = s->num_keyframes; D.M = s->num_points; D.Q = s->num_lists;
    D.pos = I.pos.in(A); D.slotAt = I.slotAt.in(A); D.flags = I.flags.in(A); D.obsOff = I.obsOff.in(A); D.obsKf = I.obsKf.in(A); D.ptBad = I.ptBad.in(A);
    D.listOff = I.listOff.in(A); D.outOff = I.outOff.in(A); D.listKf = I.listKf.in(A); D.listPt = I.listPt.in(A);
    D.obsOct = D.obsSt = D.listOct = D.listClose = nullptr;
    if (culling) { D.obsOct = I.obsOct.in(A); D.obsSt = I.obsSt.in(A); D.listOct = I.listOct.in(A); D.listClose = I.listClose.in(A); }
    return ORBX_OK;
}

}  // namespace

extern "C" int orbx_covis_update_connections(orbx_covis *h, const orbx_covis_slice *s, int th, const orbx_covis_connections *out)
{
    int rc;
    if (!out) { orbx_set_error("orbx_covis_update_connections: NULL argument"); return ORBX_ERR_ARG; }
    if ((rc = cv_validate(h, s, false, "orbx_covis_update_connections")) != ORBX_OK) return rc;
    if (out->counter_capacity < 0 || out->conn_capacity < 0) { orbx_set_error("orbx_covis_update_connections: negative capacity"); return ORBX_ERR_ARG; }
    const int NK = s->num_keyframes, Q = s->num_lists;
    h->timer.timed = false;
    // a list's counter has at most min(NK, observations under its entries) keyframes (at least 1 pair: the below-threshold fallback writes one)
    h->outOff.resize((size_t)Q + 1);
    long long tot = 0;
    for (int q = 0; q < Q; q++) {
        h->outOff[(size_t)q] = (int32_t)tot;
        long long n = 0;
        for (int e = s->list_offset[q]; e < s->list_offset[q + 1] && n < NK; e++) n += s->obs_offset[s->list_point[e] + 1] - s->obs_offset[s->list_point[e]];
        tot += std::max<long long>(1, std::min<long long>(n, NK));
        if (tot > (1ll << 24)) { orbx_set_error("orbx_covis_update_connections: more than 2^24 possible connections in one call"); return ORBX_ERR_CAPACITY; }
    }
    h->outOff[(size_t)Q] = (int32_t)tot;
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const size_t P = (size_t)tot;
    const bool lds = NK <= COVIS_LDS_NK;
    const unsigned grid = (unsigned)std::min(Q, lds ? COVIS_MAX_BLOCKS : COVIS_GLOBAL_BLOCKS);
    const size_t histWords = lds ? 0 : ((size_t)grid * (size_t)NK + 1) / 2;      // int32 rows inside the u64 work buffer
    if ((rc = h->work.ensure((lds ? 1 : P) + histWords)) != ORBX_OK) return rc;
    CvDev D = {};
    OrbxCallBox &bx = h->box;
    auto [pin, pout] = bx.plan();
    const CvSlots I(pin, h, s, false);
    const auto rHead = pout.hole<int32_t>(4 * (size_t)Q), rCnt = pout.hole<int32_t>(2 * P), rConn = pout.hole<int32_t>(2 * P);
    if ((rc = h->timer.begin(h->stream)) != ORBX_OK) return rc;
    const OrbxStaged sg = bx.begin(h->stream, &rc);
    if (rc != ORBX_OK || (rc = cv_stage(h, s, false, I, D)) != ORBX_OK) return rc;
    D.th = th;
    D.keys = h->work.p; D.hist = (int32_t *)(h->work.p + (lds ? 1 : P));
    D.head = sg.dev(rHead); D.cnt = sg.dev(rCnt); D.conn = sg.dev(rConn);
    const unsigned long long seq = bx.arm();
    if (lds) hipLaunchKernelGGL(k_covis_connect<true>, dim3(grid), dim3(COVIS_THREADS), 4 * (size_t)((NK + 1) & ~1) + 8 * (size_t)NK, h->stream, D, bx.counter, bx.flagDev, seq);
    else hipLaunchKernelGGL(k_covis_connect<false>, dim3(grid), dim3(COVIS_THREADS), 0, h->stream, D, bx.counter, bx.flagDev, seq);
    ORBX_LAUNCH_COUNT(h->timer);
    if ((rc = h->timer.end(h->stream)) != ORBX_OK) return rc;
    if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;

    const int32_t *head = sg.host(rHead), *cnt = sg.host(rCnt), *conn = sg.host(rConn);
    long long nc = 0, nn = 0;
    for (int q = 0; q < Q; q++) { nc += head[4 * q]; nn += head[4 * q + 3]; }
    if (((out->counter_kf || out->counter_weight) && nc > out->counter_capacity) || ((out->conn_kf || out->conn_weight) && nn > out->conn_capacity)) {      // nothing is written
        orbx_set_error("orbx_covis_update_connections: %lld counter entries and %lld connections for capacities of %d and %d", nc, nn, out->counter_capacity, out->conn_capacity);
        return ORBX_ERR_CAPACITY;
    }
    int32_t co = 0, no = 0;
    for (int q = 0; q < Q; q++) {
        const int32_t *hq = head + 4 * q;
        const size_t base = (size_t)h->outOff[(size_t)q];
        if (out->n_max) out->n_max[q] = hq[1];
        if (out->kf_max) out->kf_max[q] = hq[2];
        if (out->counter_offset) out->counter_offset[q] = co;
        if (out->conn_offset) out->conn_offset[q] = no;
        for (int i = 0; i < hq[0]; i++) {
            if (out->counter_kf) out->counter_kf[co + i] = cnt[2 * (base + (size_t)i)];
            if (out->counter_weight) out->counter_weight[co + i] = cnt[2 * (base + (size_t)i) + 1];
        }
        for (int i = 0; i < hq[3]; i++) {
            if (out->conn_kf) out->conn_kf[no + i] = conn[2 * (base + (size_t)i)];
            if (out->conn_weight) out->conn_weight[no + i] = conn[2 * (base + (size_t)i) + 1];
        }
        co += hq[0]; no += hq[3];
    }
    if (out->counter_offset) out->counter_offset[Q] = co;
    if (out->conn_offset) out->conn_offset[Q] = no;
    return ORBX_OK;
}

extern "C" int orbx_covis_keyframe_culling(orbx_covis *h, const orbx_covis_slice *s, const orbx_covis_culling *out)
{
    int rc;
    if (!out) { orbx_set_error("orbx_covis_keyframe_culling: NULL argument"); return ORBX_ERR_ARG; }
    if ((rc = cv_validate(h, s, true, "orbx_covis_keyframe_culling")) != ORBX_OK) return rc;
    const int NK = s->num_keyframes, M = s->num_points, Q = s->num_lists;
    h->timer.timed = false;
    h->outOff.assign((size_t)Q + 1, 0);
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const size_t m = (size_t)M;
    // device state: nobs [M] int32 | firstCull (16 bytes) | state [M] | erased [NK]
    OrbxWorkPlan &work = h->workPlan;
    work.reset();
    const auto wObs = work.hole<int32_t>(m), wFirst = work.hole<int32_t>(4);
    const auto wState = work.hole<uint8_t>(m), wErased = work.hole<uint8_t>((size_t)NK);
    const size_t wBytes = work.total();
    if ((rc = h->work.ensure(wBytes / 8)) != ORBX_OK) return rc;
    CvDev D = {};
    OrbxCallBox &bx = h->box;
    auto [pin, pout] = bx.plan();
    const CvSlots I(pin, h, s, true);
    const auto rRec = pout.hole<int32_t>(1), rRes = pout.hole<int32_t>(3 * (size_t)Q), rObs = pout.hole<int32_t>(m);
    const auto rBad = pout.hole<uint8_t>(m);
    if ((rc = h->timer.begin(h->stream)) != ORBX_OK) return rc;
    const OrbxStaged sg = bx.begin(h->stream, &rc);
    if (rc != ORBX_OK || (rc = cv_stage(h, s, true, I, D)) != ORBX_OK) return rc;
    void *W = h->work.p;
    D.nobs = wObs.in(W); D.firstCull = wFirst.in(W); D.state = wState.in(W); D.erased = wErased.in(W);
    D.record = sg.dev(rRec); D.res = sg.dev(rRes); D.outObs = sg.dev(rObs); D.outBad = sg.dev(rBad);
    const unsigned pointBlocks = (unsigned)((std::max(std::max(M, NK), 1) + COVIS_THREADS - 1) / COVIS_THREADS);
    hipLaunchKernelGGL(k_covis_cull_init, dim3(pointBlocks), dim3(COVIS_THREADS), 0, h->stream, D);
    ORBX_LAUNCH_COUNT(h->timer);
    for (int first = 0; first < Q;) {
        unsigned long long seq = bx.arm();
        hipLaunchKernelGGL(k_covis_cull_eval, dim3((unsigned)(Q - first)), dim3(COVIS_THREADS), 0, h->stream, D, first, bx.counter, bx.flagDev, seq);
        ORBX_LAUNCH_COUNT(h->timer);
        if ((rc = h->timer.end(h->stream)) != ORBX_OK) return rc;
        if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;
        const int f = *sg.host(rRec);
        if (f < first || f >= Q) break;      // (INT_MAX: nothing behind `first` is culled and erasable)
        first = f + 1;
        seq = first < Q ? 0 : bx.arm();      // the last list: no round follows, the erase itself publishes
        hipLaunchKernelGGL(k_covis_cull_apply, dim3((unsigned)((std::max(M, 1) + COVIS_THREADS - 1) / COVIS_THREADS)), dim3(COVIS_THREADS), 0, h->stream, D, f, bx.counter, bx.flagDev, seq);
        ORBX_LAUNCH_COUNT(h->timer);
        if (seq) {
            if ((rc = h->timer.end(h->stream)) != ORBX_OK) return rc;
            if ((rc = bx.wait(h->stream)) != ORBX_OK) return rc;
        }
    }
    const int32_t *res = sg.host(rRes);
    for (int q = 0; q < Q; q++) {
        if (out->n_mps) out->n_mps[q] = res[3 * q];
        if (out->n_redundant) out->n_redundant[q] = res[3 * q + 1];
        if (out->culled) out->culled[q] = (uint8_t)res[3 * q + 2];
    }
    if (out->point_obs && M) memcpy(out->point_obs, sg.host(rObs), 4 * m);
    if (out->point_bad && M) memcpy(out->point_bad, sg.host(rBad), m);
    return ORBX_OK;
}

extern "C" int orbx_covis_last_timing(orbx_covis *h, float *kernel_ms, int *launches)
{
    if (!h) { orbx_set_error("NULL covisibility handle"); return ORBX_ERR_ARG; }
    return h->timer.read(h->device, kernel_ms, launches, nullptr);
}
