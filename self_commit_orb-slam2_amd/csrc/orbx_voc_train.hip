// orbx_voc_train.hip -- training a DBoW2 ORB vocabulary on gfx950: hierarchical k-means++ and IDF weights.
//
//   orbx_voc_train  ==  DBoW2::TemplatedVocabulary<FORB::TDescriptor,FORB>::create(training_features, k, L, weighting, scoring)
//                       (reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:557-587): HKmeansStep (:641-819),
//                       initiateClustersKMpp (:832-913), FORB::meanValue / FORB::distance (FORB.cpp:28-101), createWords (:917-938),
//                       setNodeWeights (:942-996), for 256-bit descriptors.
//
// Three stated differences (include/orbx.h, README): the random draws are a counter hash of (seed, heap slot of the node, draw number) instead
// of rand() consumed in depth-first order; a cluster that receives no feature keeps its previous centre (the reference reads a released
// cv::Mat there); the assignment passes of a node are capped.  Everything else is literal.
//
// One LEVEL of the tree is processed for all its nodes at once.  A node is a contiguous SEGMENT [start, end) of `perm`, a permutation of the
// descriptors; inside a segment the features stand in training order (the partition is stable), which initiateClustersKMpp depends on.
// Every per-feature kernel runs one thread per POSITION of the permutation and looks its segment up in segOf[] (-1: the position belongs to a
// finished leaf), so a segment may start and end anywhere inside a wave or a workgroup and may span many workgroups.
//
//   seeding      k_seed_first, then k - 1 rounds of: k_seed_min (min against the last centre), an inclusive 64-bit sum over ALL positions
//                (k_scan_reduce / k_scan_blocks / k_scan_apply: three launches, the carry across workgroups is the scanned block sums), and
//                k_seed_pick (one thread per segment: the running sum inside a segment is G[p] - G[start - 1], exact integers; the first
//                position that reaches the cut is found by bisection, the sums being monotone).
//   Lloyd pass   k_mean (+ k_mean_final) and k_assign; k_assign's last workgroup writes the number of segments whose association changed into
//                mapped host memory and raises the sequence word the host polls (OrbxCallBox): no stream synchronisation, no copy engine.
//   partition    per pair of clusters one scan of the flags (assoc == c), both counts packed into one 64-bit sum, then k_part_scatter /
//                k_part_advance: the stable rank of a feature is its flag sum inside the segment.
//   weights      k_descend (the real descent, first minimum wins) and k_ni (distinct (image, word) pairs through an open-addressing table of
//                64-bit keys filled with compare-and-swap; the count of distinct pairs does not depend on the order of arrival).
//
// The mean (256 counters per segment and cluster): a workgroup stages a tile of 512 positions in LDS; thread t owns bit t and walks the tile's
// features in order, adding into ITS column of an LDS table [cluster][256] - no atomics, no conflicts between threads.  Positions are ordered
// by segment, so the table belongs to one segment at a time: when the segment changes it is flushed.  A segment that lies wholly inside the
// tile is thresholded there and its centres are written directly (the many small segments of the deep levels); a segment that crosses a
// tile border adds its partial columns to counters in device memory with integer atomics and k_mean_final thresholds them (the few long
// segments of the first levels: at most one per tile border).  LDS: 16 KB of descriptors + 32 KB of counters + 4 KB of keys = 52 KB.
//
// No floating point on the device except the draws' two products and the compare against cut_d (doubles; the build has -ffp-contract=off).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "orbx_handle.h"

namespace {

typedef unsigned long long u64;

constexpr int VT_MEAN_TILE = 512;      // positions per workgroup of k_mean
constexpr int VT_SCAN_TILE = 1024;     // positions per workgroup of the scans (256 threads x 4)
constexpr int VT_ASSIGN_BLOCKS = 2048;  // workgroups of k_assign at most (8 per CU)

struct VtSeg {
    int32_t start, end;   // positions [start, end) of perm
    int32_t cOff;         // first centre slot of the segment (min(n, k) slots; the stage entry points use k per segment)
    int32_t x;            // index among the segments that cross a tile border of k_mean, -1 = none
    u64 slot;             // heap index of the node in the complete k-ary tree: what the draws are keyed by
    int32_t big;          // 1: clustered by k-means (n > k); 0: one cluster per feature
    int32_t pad;
};

// splitmix64's output function over a counter (Steele, Lea, Flood: "Fast splittable pseudorandom number generators", OOPSLA 2014), chained
// over the three words of a draw; tests/voc_train_ref.py and tools/voc_train_host_baseline.cc state the same lines.
__host__ __device__ inline u64 vt_mix(u64 z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline u64 vt_draw(u64 seed, u64 slot, u64 j) { return vt_mix(vt_mix(vt_mix(seed) + slot) + j) >> 11; }   // top 53 bits

__device__ __forceinline__ int vt_ham(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1)
{
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
           __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// segOf[p] = the segment that holds position p, -1 = none (segments sorted by start, disjoint)
__global__ __launch_bounds__(256) void k_seg_of(const VtSeg *__restrict__ segs, int S, int N, int32_t *__restrict__ segOf)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    int lo = 0, hi = S - 1;      // the last segment with start <= p
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].start <= p) lo = mid; else hi = mid - 1;
    }
    const VtSeg sg = segs[lo];
    segOf[p] = (p >= sg.start && p < sg.end) ? lo : -1;
}

__global__ __launch_bounds__(256) void k_iota(int N, int32_t *__restrict__ perm)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < N) perm[p] = p;
}

// One thread per segment.  n <= k: one cluster per feature, no de-duplication (:660-670).  Otherwise the first centre: RandomInt(0, n - 1)
// (DUtils Random.cpp:47-50) with the draw in place of rand() / RAND_MAX.
__global__ __launch_bounds__(256) void k_seed_first(const VtSeg *__restrict__ segs, int S, int k, u64 seed, const int32_t *__restrict__ perm,
                                                    const uint4 *__restrict__ desc, uint4 *__restrict__ centres, int32_t *__restrict__ nc,
                                                    int32_t *__restrict__ chosen, int32_t *__restrict__ assoc, int32_t *__restrict__ changedPass,
                                                    int32_t *__restrict__ cursor)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const VtSeg sg = segs[s];
    const int n = sg.end - sg.start;
    changedPass[s] = 0;
    cursor[s] = sg.start;
    if (!sg.big) {
        for (int i = 0; i < n; i++) {
            const size_t f = (size_t)perm[sg.start + i];
            centres[2 * (size_t)(sg.cOff + i)] = desc[2 * f];
            centres[2 * (size_t)(sg.cOff + i) + 1] = desc[2 * f + 1];
            chosen[sg.cOff + i] = i;
            assoc[sg.start + i] = i;
        }
        nc[s] = n;
        return;
    }
    const double u = (double)vt_draw(seed, sg.slot, 0) * 0x1p-53;      // [0, 1)
    long long idx = (long long)(u * (double)n);                        // floor: the product is not negative
    if (idx > n - 1) idx = n - 1;
    const size_t f = (size_t)perm[sg.start + (int)idx];
    centres[2 * (size_t)sg.cOff] = desc[2 * f];
    centres[2 * (size_t)sg.cOff + 1] = desc[2 * f + 1];
    chosen[sg.cOff] = (int)idx;
    for (int c = 1; c < k; c++) chosen[sg.cOff + c] = -1;
    nc[s] = 1;
}

// Round j of the seeding: min_dists against the LAST centre only (:872-880; the first round initialises them, :861-867).  Segments whose
// seeding ended early (nc < j) and segments with n <= k take no part.
__global__ __launch_bounds__(256) void k_seed_min(const VtSeg *__restrict__ segs, const int32_t *__restrict__ segOf, int N, int j,
                                                  const int32_t *__restrict__ perm, const uint4 *__restrict__ desc, const uint4 *__restrict__ centres,
                                                  const int32_t *__restrict__ nc, int32_t *__restrict__ md)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const int s = segOf[p];
    if (s < 0) return;
    const VtSeg sg = segs[s];
    if (!sg.big || nc[s] != j) return;
    const size_t f = (size_t)perm[p], c = (size_t)(sg.cOff + j - 1);
    const int d = vt_ham(desc[2 * f], desc[2 * f + 1], centres[2 * c], centres[2 * c + 1]);
    md[p] = j == 1 ? d : min(md[p], d);
}

// ---- inclusive 64-bit sum over all positions.  MODE 0: min_dists; MODE 1: the flags (assoc == c0) and (assoc == c0 + 1) in the two halves.
// Values of positions outside the segments of interest do not matter: every reader subtracts the sum in front of its segment.
template <int MODE> __device__ __forceinline__ u64 vt_val(int p, const int32_t *__restrict__ src, int c0)
{
    const int v = src[p];
    if (MODE == 0) return (u64)(uint32_t)v;
    return (u64)(v == c0) | ((u64)(v == c0 + 1) << 32);
}

template <int MODE> __global__ __launch_bounds__(256) void k_scan_reduce(int N, const int32_t *__restrict__ src, int c0, u64 *__restrict__ blockSum)
{
    __shared__ u64 sh[4];
    const int base = blockIdx.x * VT_SCAN_TILE + threadIdx.x * 4;
    u64 v = 0;
    for (int i = 0; i < 4; i++)
        if (base + i < N) v += vt_val<MODE>(base + i, src, c0);
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);      // (not wave_sum_xor: as a call the scheduler orders this kernel's address arithmetic differently)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) blockSum[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// (an LDS tree with two barriers per step, not a wave scan: kept here so that k_scan_blocks / k_scan_apply keep their instructions; orbx_wave.h has the wave forms)
__device__ __forceinline__ u64 vt_block_exclusive(u64 mine, u64 *sh)      // exclusive sum of `mine` over the 256 threads of the workgroup
{
    const int t = threadIdx.x;
    sh[t] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const u64 x = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    return sh[t] - mine;
}

// one workgroup: block sums -> the sum in front of each block (65536 blocks at 2^26 positions: 256 per thread)
__global__ __launch_bounds__(256) void k_scan_blocks(int nb, u64 *__restrict__ blockSum)
{
    __shared__ u64 sh[256];
    const int per = (nb + 255) / 256, lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
    u64 mine = 0;
    for (int i = lo; i < hi; i++) mine += blockSum[i];
    u64 run = vt_block_exclusive(mine, sh);
    for (int i = lo; i < hi; i++) { const u64 v = blockSum[i]; blockSum[i] = run; run += v; }
}

template <int MODE> __global__ __launch_bounds__(256) void k_scan_apply(int N, const int32_t *__restrict__ src, int c0, const u64 *__restrict__ blockSum,
                                                                        u64 *__restrict__ G)
{
    __shared__ u64 sh[256];
    const int base = blockIdx.x * VT_SCAN_TILE + threadIdx.x * 4;
    u64 v[4], mine = 0;
    for (int i = 0; i < 4; i++) { v[i] = base + i < N ? vt_val<MODE>(base + i, src, c0) : 0; mine += v[i]; }
    u64 run = vt_block_exclusive(mine, sh) + blockSum[blockIdx.x];
    for (int i = 0; i < 4; i++) { run += v[i]; if (base + i < N) G[base + i] = run; }
}

// Round j, one thread per segment: dist_sum = 0 ends the seeding with fewer than k clusters (:885, :908); otherwise cut_d = u * dist_sum with
// u in (0, 1] and the chosen feature is the first whose running sum is >= cut_d, the last one if none (:893-903).  The sums are exact
// integers, compared as doubles; they do not fall along the segment, so the first position is found by bisection.  D(x), not D(x)^2.
__global__ __launch_bounds__(256) void k_seed_pick(const VtSeg *__restrict__ segs, int S, int j, u64 seed, const u64 *__restrict__ G,
                                                   const int32_t *__restrict__ perm, const uint4 *__restrict__ desc, uint4 *__restrict__ centres,
                                                   int32_t *__restrict__ nc, int32_t *__restrict__ chosen)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const VtSeg sg = segs[s];
    if (!sg.big || nc[s] != j) return;
    const u64 before = sg.start ? G[sg.start - 1] : 0, total = G[sg.end - 1] - before;
    if (total == 0) return;
    const double cut = ((double)(vt_draw(seed, sg.slot, (u64)j) + 1) * 0x1p-53) * (double)total;
    int lo = sg.start, hi = sg.end - 1;      // the answer lies in [lo, hi]; hi = the last feature covers "none"
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)(G[mid] - before) >= cut) hi = mid; else lo = mid + 1;
    }
    const size_t f = (size_t)perm[lo], c = (size_t)(sg.cOff + j);
    centres[2 * c] = desc[2 * f];
    centres[2 * c + 1] = desc[2 * f + 1];
    chosen[sg.cOff + j] = lo - sg.start;
    nc[s] = j + 1;
}

// Assignment pass (:730-751): the descriptor in 8 VGPRs, <= k distances, strict '<' (the lowest cluster index wins ties).  A feature whose
// cluster differs from the previous pass stamps its segment with the pass number; the first to stamp a segment counts it.  The last workgroup
// to arrive writes the count into mapped host memory and raises the sequence word behind it.
__global__ __launch_bounds__(256) void k_assign(const VtSeg *__restrict__ segs, const int32_t *__restrict__ segOf, int N, int pass,
                                                const int32_t *__restrict__ perm, const uint4 *__restrict__ desc, const uint4 *__restrict__ centres,
                                                const int32_t *__restrict__ nc, int32_t *__restrict__ assoc, int32_t *__restrict__ changedPass,
                                                unsigned *__restrict__ devCount, unsigned *pubCounter, int32_t *recOut, u64 *pubFlag, u64 pubSeq)
{
    // a bounded grid walks the positions: every workgroup ends with one add to the arrival counter, and tens of thousands of adds to one address
    // cost more than the pass itself (3 ms against 0.4 ms per pass at 10^7 positions)
    for (int base = blockIdx.x * 256; base < N; base += gridDim.x * 256) {      // (uniform per workgroup: the ballot below sees whole waves)
        const int p = base + threadIdx.x;
        int s = -1;
        bool changed = false;
        if (p < N) {
            s = segOf[p];
            if (s >= 0) {
                const VtSeg sg = segs[s];
                if (sg.big) {
                    const size_t f = (size_t)perm[p];
                    const uint4 a0 = desc[2 * f], a1 = desc[2 * f + 1];
                    const int n = nc[s];
                    int best = 0x7fffffff, bi = 0;
                    for (int c = 0; c < n; c++) {
                        const int d = vt_ham(a0, a1, centres[2 * (size_t)(sg.cOff + c)], centres[2 * (size_t)(sg.cOff + c) + 1]);
                        if (d < best) { best = d; bi = c; }
                    }
                    changed = pass > 1 && assoc[p] != bi;
                    assoc[p] = bi;
                }
            }
        }
        // one atomic per wave and segment in the common case: the first changed lane speaks for every lane of its segment
        const u64 mask = __ballot(changed);
        const int lead = mask ? __ffsll((long long)mask) - 1 : 0, leadSeg = __shfl(s, lead);
        if (changed && ((int)(threadIdx.x & 63) == lead || s != leadSeg)) {
            if (__hip_atomic_load(&changedPass[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != pass &&
                atomicMax(&changedPass[s], pass) < pass)
                atomicAdd(devCount, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (__hip_atomic_fetch_add(pubCounter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
            __hip_atomic_store(pubCounter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned cnt = __hip_atomic_exchange(devCount, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *recOut = (int32_t)cnt;
            __hip_atomic_store(pubFlag, pubSeq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// FORB::meanValue (FORB.cpp:28-77): bit i of the mean is set when count_i >= n / 2 + n % 2.  Thread t owns the bit of byte t >> 3 whose mask is
// 1 << (t & 7): the threshold is the same for every bit, and a wave's ballot of its 64 bits is then the 8 bytes 8w .. 8w + 7 of the centre as
// they lie in memory.  A cluster without features keeps its previous centre.
__device__ __forceinline__ void vt_store_mean_bits(uint4 *__restrict__ centres, int slot, bool bit)
{
    const u64 b = __ballot(bit);
    if ((threadIdx.x & 63) == 0) ((u64 *)centres)[4 * (size_t)slot + (threadIdx.x >> 6)] = b;
}

__global__ __launch_bounds__(256) void k_mean(const VtSeg *__restrict__ segs, const int32_t *__restrict__ segOf, int N, int k, const int32_t *__restrict__ perm,
                                              const uint4 *__restrict__ desc, const int32_t *__restrict__ assoc, const int32_t *__restrict__ nc,
                                              uint4 *__restrict__ centres, unsigned *__restrict__ cntG, unsigned *__restrict__ sizeG)
{
    __shared__ uint4 sDesc[VT_MEAN_TILE * 2];
    __shared__ __attribute__((aligned(16))) int32_t sSeg[VT_MEAN_TILE];
    __shared__ __attribute__((aligned(16))) int32_t sA[VT_MEAN_TILE];
    __shared__ unsigned sCnt[32 * 256];
    __shared__ unsigned sSize[32];
    const int t = threadIdx.x, tile0 = blockIdx.x * VT_MEAN_TILE;
    for (int i = t; i < VT_MEAN_TILE; i += 256) {
        const int p = tile0 + i;
        int s = p < N ? segOf[p] : -1;
        if (s >= 0 && !segs[s].big) s = -1;
        sSeg[i] = s;
        if (s >= 0) {
            const size_t f = (size_t)perm[p];
            sDesc[2 * i] = desc[2 * f];
            sDesc[2 * i + 1] = desc[2 * f + 1];
            sA[i] = assoc[p];
        }
    }
    for (int c = 0; c < 32; c++) sCnt[c * 256 + t] = 0;
    if (t < 32) sSize[t] = 0;
    __syncthreads();
    const uint32_t *words = (const uint32_t *)sDesc + (t >> 5);
    const int sh = t & 31;
    int cur = -1;
    for (int i = 0; i <= VT_MEAN_TILE; i++) {      // (one step past the end flushes the last segment)
        // four features of the current segment at a time: their keys and words are independent loads, only the counters are a chain
        // (a step of the one-by-one walk below is three dependent LDS accesses)
        if ((i & 3) == 0 && i + 4 <= VT_MEAN_TILE) {
            const int4 s4 = *(const int4 *)&sSeg[i];
            if (s4.x == cur && s4.y == cur && s4.z == cur && s4.w == cur) {
                if (cur >= 0) {
                    const int4 c4 = *(const int4 *)&sA[i];
                    const unsigned b0 = (words[8 * i] >> sh) & 1u, b1 = (words[8 * i + 8] >> sh) & 1u, b2 = (words[8 * i + 16] >> sh) & 1u,
                                   b3 = (words[8 * i + 24] >> sh) & 1u;
                    sCnt[c4.x * 256 + t] += b0;
                    sCnt[c4.y * 256 + t] += b1;
                    sCnt[c4.z * 256 + t] += b2;
                    sCnt[c4.w * 256 + t] += b3;
                    if (t < 32) sSize[t] += (unsigned)(c4.x == t) + (unsigned)(c4.y == t) + (unsigned)(c4.z == t) + (unsigned)(c4.w == t);
                }
                i += 3;
                continue;
            }
        }
        const int s = i < VT_MEAN_TILE ? sSeg[i] : -1;
        if (s != cur) {      // uniform: every thread reads the same key
            if (cur >= 0) {
                const VtSeg sg = segs[cur];
                const int n = nc[cur];
                const bool inside = sg.start >= tile0 && sg.end <= tile0 + VT_MEAN_TILE;
                __syncthreads();      // sSize is complete
                for (int c = 0; c < n; c++) {
                    const unsigned sz = sSize[c], v = sCnt[c * 256 + t];
                    if (inside) {
                        if (sz) vt_store_mean_bits(centres, sg.cOff + c, v >= sz / 2 + sz % 2);
                    } else {
                        if (v) atomicAdd(&cntG[((size_t)sg.x * k + c) * 256 + t], v);
                        if (t == 0 && sz) atomicAdd(&sizeG[(size_t)sg.x * k + c], sz);
                    }
                    sCnt[c * 256 + t] = 0;
                }
                __syncthreads();
                if (t < 32) sSize[t] = 0;
                __syncthreads();
            }
            cur = s;
        }
        if (s >= 0) {
            const int c = sA[i];
            if ((words[8 * i] >> sh) & 1u) sCnt[c * 256 + t]++;
            if (t == c) sSize[c]++;
        }
    }
}

// the segments that cross a tile border of k_mean: one workgroup each; leaves the counters zero for the next pass
__global__ __launch_bounds__(256) void k_mean_final(const VtSeg *__restrict__ segs, const int32_t *__restrict__ xSeg, int k, const int32_t *__restrict__ nc,
                                                    uint4 *__restrict__ centres, unsigned *__restrict__ cntG, unsigned *__restrict__ sizeG)
{
    const int x = blockIdx.x, s = xSeg[x], t = threadIdx.x, n = nc[s];
    const int cOff = segs[s].cOff;
    for (int c = 0; c < n; c++) {
        const unsigned sz = sizeG[(size_t)x * k + c], v = cntG[((size_t)x * k + c) * 256 + t];
        if (sz) vt_store_mean_bits(centres, cOff + c, v >= sz / 2 + sz % 2);
        cntG[((size_t)x * k + c) * 256 + t] = 0;
    }
    __syncthreads();
    if (t < n) sizeG[(size_t)x * k + t] = 0;
}

// Stable partition by (segment, cluster), clusters c0 and c0 + 1: G holds the inclusive flag sums of both.  cursor[s] = where cluster c0 of
// segment s begins.
__global__ __launch_bounds__(256) void k_part_scatter(const VtSeg *__restrict__ segs, const int32_t *__restrict__ segOf, int N, int c0, const u64 *__restrict__ G,
                                                      const int32_t *__restrict__ assoc, const int32_t *__restrict__ perm, int32_t *__restrict__ permNew,
                                                      const int32_t *__restrict__ cursor)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const int s = segOf[p];
    if (s < 0) return;
    const VtSeg sg = segs[s];
    if (!sg.big) return;
    const int a = assoc[p];
    if (a != c0 && a != c0 + 1) return;
    const u64 before = sg.start ? G[sg.start - 1] : 0, g = G[p] - before;      // (neither half borrows: both sums are monotone)
    int dest;
    if (a == c0) dest = cursor[s] + (int)(uint32_t)g - 1;
    else dest = cursor[s] + (int)(uint32_t)(G[sg.end - 1] - before) + (int)(g >> 32) - 1;
    permNew[dest] = perm[p];
}

__global__ __launch_bounds__(256) void k_part_advance(const VtSeg *__restrict__ segs, int S, int k, int c0, const u64 *__restrict__ G, int32_t *__restrict__ cursor,
                                                      int32_t *__restrict__ counts)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const VtSeg sg = segs[s];
    if (!sg.big) return;
    const u64 tot = G[sg.end - 1] - (sg.start ? G[sg.start - 1] : 0);
    counts[sg.cOff + c0] = (int)(uint32_t)tot;
    if (c0 + 1 < k) counts[sg.cOff + c0 + 1] = (int)(tot >> 32);
    cursor[s] += (int)(uint32_t)tot + (int)(tot >> 32);
}

__global__ __launch_bounds__(256) void k_changed_flags(int S, int pass, const int32_t *__restrict__ changedPass, uint8_t *__restrict__ out)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < S) out[s] = changedPass[s] == pass;
}

// transform() of every training feature through the finished tree (TemplatedVocabulary.h:1201-1262): the children of a node have consecutive
// ids from childStart; first minimum wins.
__global__ __launch_bounds__(256) void k_descend(int N, const uint4 *__restrict__ desc, const int32_t *__restrict__ childStart, const int32_t *__restrict__ childCount,
                                                 const uint4 *__restrict__ nodeDesc, const int32_t *__restrict__ nodeWord, int32_t *__restrict__ word)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint4 a0 = desc[2 * (size_t)i], a1 = desc[2 * (size_t)i + 1];
    int cur = 0, n = childCount[0];
    while (n > 0) {
        const int first = childStart[cur];
        int best = 0x7fffffff, bi = first;
        for (int c = 0; c < n; c++) {
            const int d = vt_ham(a0, a1, nodeDesc[2 * (size_t)(first + c)], nodeDesc[2 * (size_t)(first + c) + 1]);
            if (d < best) { best = d; bi = first + c; }
        }
        cur = bi;
        n = childCount[cur];
    }
    word[i] = nodeWord[cur];
}

// Ni[w] = the number of images with a feature on word w (:962-983): every feature files the key (image, word) in an open-addressing table;
// whoever files a key first counts it.  imgStart[m] = first feature of image m (nImg + 1 entries).
__global__ __launch_bounds__(256) void k_ni(int N, const int32_t *__restrict__ word, const int32_t *__restrict__ imgStart, int nImg, u64 *__restrict__ table, u64 mask,
                                            int32_t *__restrict__ ni)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int lo = 0, hi = nImg - 1;      // the last image that starts at or before feature i (empty images share a start with their successor)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (imgStart[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const int w = word[i];
    const u64 key = ((u64)(uint32_t)lo << 32) | (uint32_t)w;
    u64 h = vt_mix(key) & mask;
    for (u64 probe = 0; probe <= mask; probe++) {      // (the table has at least twice as many slots as there are features)
        const u64 old = atomicCAS(&table[h], ~0ull, key);
        if (old == ~0ull) { atomicAdd(&ni[w], 1); return; }
        if (old == key) return;
        h = (h + 1) & mask;
    }
}

// add_extracted: the frames of an extractor's last batch, compacted behind the descriptors the trainer holds.  state = {descriptors, images,
// overflow}; every workgroup (one per frame) reads it, k_append_commit (the next launch) advances it.
__global__ __launch_bounds__(256) void k_append_extracted(const uint8_t *__restrict__ src, const int32_t *__restrict__ counts, int batch, int cap,
                                                          const int32_t *__restrict__ state, int maxDesc, int maxImg, uint4 *__restrict__ desc,
                                                          int32_t *__restrict__ imgCount)
{
    const int f = blockIdx.x;
    long long before = 0, total = 0;
    for (int g = 0; g < batch; g++) {
        const int n = min(max(counts[g], 0), cap);
        if (g < f) before += n;
        total += n;
    }
    if (state[0] + total > maxDesc || state[1] + batch > maxImg) return;      // (k_append_commit raises the overflow word)
    const int n = min(max(counts[f], 0), cap);
    const uint4 *from = (const uint4 *)(src + (size_t)f * cap * 32);
    uint4 *to = desc + 2 * ((size_t)state[0] + (size_t)before);
    for (int i = threadIdx.x; i < 2 * n; i += 256) to[i] = from[i];
    if (threadIdx.x == 0) imgCount[state[1] + f] = n;
}

__global__ void k_append_commit(const int32_t *__restrict__ counts, int batch, int cap, int32_t *__restrict__ state, int maxDesc, int maxImg)
{
    long long total = 0;
    for (int g = 0; g < batch; g++) total += min(max(counts[g], 0), cap);
    if (state[0] + total > maxDesc || state[1] + batch > maxImg) { state[2] = 1; return; }
    state[0] += (int)total;
    state[1] += batch;
}

}  // namespace

struct orbx_voc_trainer : OrbxHandle {
    int k = 0, L = 0, maxDesc = 0, maxImg = 0;
    hipEvent_t extEvent = nullptr;
    // the training set: descriptors in training order, features per image, {descriptors, images, overflow} (authoritative on the device while
    // `dirty`: add_extracted appends without a download)
    OrbxOwnedBuf<uint4> desc;
    OrbxOwnedBuf<int32_t> imgCount, state;
    int nDesc = 0, nImg = 0;
    bool dirty = false;
    // work arrays (grow-only, sized by the call)
    OrbxOwnedBuf<uint4> stageDesc, centres, nodeDesc;
    OrbxOwnedBuf<int32_t> perm[2], segOf, assoc, md, nc, changedPass, cursor, chosen, counts, xSeg, imgStart, word, ni, childStart, childCount, nodeWord;
    OrbxOwnedBuf<u64> G, blockSum, table;
    OrbxOwnedBuf<VtSeg> segs;
    OrbxOwnedBuf<unsigned> cntG, sizeG, devCount;
    OrbxOwnedBuf<uint8_t> flags;
    OrbxCallBox box;
    int32_t *changedDev = nullptr;            // the box's one result, planned once at creation: a pass's changed-assignment count
    const int32_t *changedHost = nullptr;
    // the last result, flat arrays in orbx_vocabulary_create's layout
    bool trained = false;
    std::vector<int32_t> parent, ni_;
    std::vector<uint8_t> isLeaf, nodeDescHost;
    std::vector<double> weights;
    int numNodes = 0, numWords = 0;
    // timing
    bool profiling = false;
    std::vector<hipEvent_t> ev;
    std::vector<int> evTag;
    size_t evUsed = 0;
    float totalMs = 0, levelMs[ORBX_VOC_MAX_L] = {0}, stageMs[5] = {0};
    int launches = 0;
    ~orbx_voc_trainer()      // (add_extracted's work on the extractor's stream ends before the members free what it writes)
    {
        if (extEvent) { (void)hipEventSynchronize(extEvent); (void)hipEventDestroy(extEvent); }
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};

namespace {

enum { VT_SEED = 0, VT_ASSIGN = 1, VT_MEAN = 2, VT_PART = 3, VT_OTHER = 4 };

void vt_mark(orbx_voc_trainer *h, int tag)      // (profiling only) what is launched from here on belongs to stage `tag`
{
    if (!h->profiling) return;
    if (h->evUsed == h->ev.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        h->ev.push_back(e); h->evTag.push_back(0);
    }
    (void)hipEventRecord(h->ev[h->evUsed], h->stream);
    h->evTag[h->evUsed++] = tag;
}

void vt_collect(orbx_voc_trainer *h)      // after a stream synchronisation
{
    for (size_t i = 1; i < h->evUsed; i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, h->ev[i - 1], h->ev[i]) == hipSuccess) h->stageMs[h->evTag[i - 1]] += ms;
    }
    h->evUsed = 0;
}

inline unsigned vt_blocks(size_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

int vt_launch_check(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { orbx_set_error("%s: kernel launch failed: %s", what, hipGetErrorString(e)); return ORBX_ERR_HIP; }
    return ORBX_OK;
}

// everything one level needs that the host prepares: the segments (sorted by start) and the list of those that cross a tile border of k_mean
struct VtLevel {
    std::vector<VtSeg> segs;
    std::vector<int32_t> xSeg;
    int slots = 0;      // centre slots of all segments
    bool anyBig = false;
    void finish(int k, bool dense)
    {
        slots = 0; anyBig = false; xSeg.clear();
        for (size_t s = 0; s < segs.size(); s++) {
            VtSeg &sg = segs[s];
            const int n = sg.end - sg.start;
            sg.cOff = slots;
            slots += dense ? k : (n < k ? n : k);
            sg.x = -1; sg.pad = 0;
            if (sg.big) {
                anyBig = true;
                if (sg.start / VT_MEAN_TILE != (sg.end - 1) / VT_MEAN_TILE) { sg.x = (int32_t)xSeg.size(); xSeg.push_back((int32_t)s); }
            }
        }
    }
};

int vt_ensure_work(orbx_voc_trainer *h, size_t N, const VtLevel &lv)
{
    int rc;
    const size_t S = lv.segs.size(), slots = (size_t)lv.slots, X = lv.xSeg.size();
    if ((rc = h->perm[0].ensure(N)) || (rc = h->perm[1].ensure(N)) || (rc = h->segOf.ensure(N)) || (rc = h->assoc.ensure(N)) || (rc = h->md.ensure(N)) ||
        (rc = h->G.ensure(N)) || (rc = h->blockSum.ensure(vt_blocks(N, VT_SCAN_TILE))) || (rc = h->segs.ensure(S)) || (rc = h->nc.ensure(S)) ||
        (rc = h->changedPass.ensure(S)) || (rc = h->cursor.ensure(S)) || (rc = h->centres.ensure(2 * slots)) || (rc = h->chosen.ensure(slots)) ||
        (rc = h->counts.ensure(slots)) || (rc = h->xSeg.ensure(X ? X : 1)))
        return rc;
    const size_t oldCnt = h->cntG.n, oldSize = h->sizeG.n;
    if ((rc = h->cntG.ensure((X ? X : 1) * (size_t)h->k * 256)) || (rc = h->sizeG.ensure((X ? X : 1) * (size_t)h->k))) return rc;
    // the counters are zero between passes (k_mean_final leaves them so); a buffer that grew starts from zero
    if (h->cntG.n != oldCnt) ORBX_HIP_CHECK(hipMemsetAsync(h->cntG.p, 0, h->cntG.n * sizeof(unsigned), h->stream));
    if (h->sizeG.n != oldSize) ORBX_HIP_CHECK(hipMemsetAsync(h->sizeG.p, 0, h->sizeG.n * sizeof(unsigned), h->stream));
    if (!h->devCount.p) {
        if ((rc = h->devCount.ensure(16))) return rc;
        ORBX_HIP_CHECK(hipMemsetAsync(h->devCount.p, 0, 16 * sizeof(unsigned), h->stream));
    }
    return ORBX_OK;
}

int vt_upload_level(orbx_voc_trainer *h, int N, const VtLevel &lv)
{
    const int S = (int)lv.segs.size();
    ORBX_HIP_CHECK(hipMemcpyAsync(h->segs.p, lv.segs.data(), (size_t)S * sizeof(VtSeg), hipMemcpyHostToDevice, h->stream));
    if (!lv.xSeg.empty()) ORBX_HIP_CHECK(hipMemcpyAsync(h->xSeg.p, lv.xSeg.data(), lv.xSeg.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));      // (the vectors are pageable memory and may change once this returns)
    hipLaunchKernelGGL(k_seg_of, dim3(vt_blocks((size_t)N)), dim3(256), 0, h->stream, (const VtSeg *)h->segs.p, S, N, h->segOf.p);
    h->launches++;
    return vt_launch_check("k_seg_of");
}

template <int MODE> int vt_scan(orbx_voc_trainer *h, int N, const int32_t *src, int c0)
{
    const unsigned nb = vt_blocks((size_t)N, VT_SCAN_TILE);
    hipLaunchKernelGGL((k_scan_reduce<MODE>), dim3(nb), dim3(256), 0, h->stream, N, src, c0, h->blockSum.p);
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(256), 0, h->stream, (int)nb, h->blockSum.p);
    hipLaunchKernelGGL((k_scan_apply<MODE>), dim3(nb), dim3(256), 0, h->stream, N, src, c0, (const u64 *)h->blockSum.p, h->G.p);
    h->launches += 3;
    return vt_launch_check("scan");
}

// k-means++ seeding of every segment of the level (initiateClustersKMpp)
int vt_seed(orbx_voc_trainer *h, const uint4 *desc, int N, const VtLevel &lv, u64 seed, int cur)
{
    const int S = (int)lv.segs.size(), k = h->k;
    int rc;
    vt_mark(h, VT_SEED);
    hipLaunchKernelGGL(k_seed_first, dim3(vt_blocks((size_t)S)), dim3(256), 0, h->stream, (const VtSeg *)h->segs.p, S, k, seed, (const int32_t *)h->perm[cur].p, desc,
                       h->centres.p, h->nc.p, h->chosen.p, h->assoc.p, h->changedPass.p, h->cursor.p);
    h->launches++;
    if ((rc = vt_launch_check("k_seed_first"))) return rc;
    if (!lv.anyBig) return ORBX_OK;
    for (int j = 1; j < k; j++) {
        hipLaunchKernelGGL(k_seed_min, dim3(vt_blocks((size_t)N)), dim3(256), 0, h->stream, (const VtSeg *)h->segs.p, (const int32_t *)h->segOf.p, N, j,
                           (const int32_t *)h->perm[cur].p, desc, (const uint4 *)h->centres.p, (const int32_t *)h->nc.p, h->md.p);
        if ((rc = vt_scan<0>(h, N, h->md.p, 0))) return rc;
        hipLaunchKernelGGL(k_seed_pick, dim3(vt_blocks((size_t)S)), dim3(256), 0, h->stream, (const VtSeg *)h->segs.p, S, j, seed, (const u64 *)h->G.p,
                           (const int32_t *)h->perm[cur].p, desc, h->centres.p, h->nc.p, h->chosen.p);
        h->launches += 2;
        if ((rc = vt_launch_check("seeding round"))) return rc;
    }
    return ORBX_OK;
}

int vt_mean(orbx_voc_trainer *h, const uint4 *desc, int N, const VtLevel &lv, int cur)
{
    vt_mark(h, VT_MEAN);
    hipLaunchKernelGGL(k_mean, dim3(vt_blocks((size_t)N, VT_MEAN_TILE)), dim3(256), 0, h->stream, (const VtSeg *)h->segs.p, (const int32_t *)h->segOf.p, N, h->k,
                       (const int32_t *)h->perm[cur].p, desc, (const int32_t *)h->assoc.p, (const int32_t *)h->nc.p, h->centres.p, h->cntG.p, h->sizeG.p);
    h->launches++;
    if (!lv.xSeg.empty()) {
        hipLaunchKernelGGL(k_mean_final, dim3((unsigned)lv.xSeg.size()), dim3(256), 0, h->stream, (const VtSeg *)h->segs.p, (const int32_t *)h->xSeg.p, h->k,
                           (const int32_t *)h->nc.p, h->centres.p, h->cntG.p, h->sizeG.p);
        h->launches++;
    }
    return vt_launch_check("k_mean");
}

// one assignment pass; *changed = the segments whose association differs from the previous pass (0 in pass 1, which has none)
int vt_assign(orbx_voc_trainer *h, const uint4 *desc, int N, int pass, int cur, int *changed)
{
    OrbxCallBox &bx = h->box;
    vt_mark(h, VT_ASSIGN);
    const u64 seq = bx.arm();
    hipLaunchKernelGGL(k_assign, dim3(std::min(vt_blocks((size_t)N), (unsigned)VT_ASSIGN_BLOCKS)), dim3(256), 0, h->stream, (const VtSeg *)h->segs.p, (const int32_t *)h->segOf.p, N, pass,
                       (const int32_t *)h->perm[cur].p, desc, (const uint4 *)h->centres.p, (const int32_t *)h->nc.p, h->assoc.p, h->changedPass.p, h->devCount.p, bx.counter,
                       h->changedDev, bx.flagDev, seq);
    h->launches++;
    int rc = vt_launch_check("k_assign");
    if (rc) return rc;
    if ((rc = bx.wait(h->stream))) return rc;
    *changed = *h->changedHost;
    return ORBX_OK;
}

int vt_sync_state(orbx_voc_trainer *h)
{
    if (!h->dirty) return ORBX_OK;
    int32_t st[3];
    if (h->extEvent) ORBX_HIP_CHECK(hipEventSynchronize(h->extEvent));
    ORBX_HIP_CHECK(hipMemcpy(st, h->state.p, sizeof(st), hipMemcpyDeviceToHost));
    h->nDesc = st[0]; h->nImg = st[1];
    h->dirty = false;
    if (st[2]) {
        st[2] = 0;
        ORBX_HIP_CHECK(hipMemcpy(h->state.p, st, sizeof(st), hipMemcpyHostToDevice));
        orbx_set_error("an add_extracted batch did not fit (%d of %d descriptors, %d of %d images held) and was dropped", h->nDesc, h->maxDesc, h->nImg, h->maxImg);
        return ORBX_ERR_CAPACITY;
    }
    return ORBX_OK;
}

int vt_push_state(orbx_voc_trainer *h)
{
    const int32_t st[3] = {h->nDesc, h->nImg, 0};
    ORBX_HIP_CHECK(hipMemcpy(h->state.p, st, sizeof(st), hipMemcpyHostToDevice));
    return ORBX_OK;
}

bool vt_tree_fits(int k, int L)
{
    u64 nodes = 1, pw = 1;
    for (int i = 1; i <= L; i++) { pw *= (u64)k; nodes += pw; if (nodes >= (1ull << 31)) return false; }
    return true;
}

// segments from offsets (the stage entry points): segment s = [off[s], off[s + 1])
int vt_check_offsets(const int32_t *off, int S, int n)
{
    if (off[0] != 0 || off[S] != n) { orbx_set_error("segment offsets must run from 0 to n"); return ORBX_ERR_ARG; }
    for (int s = 0; s < S; s++)
        if (off[s + 1] <= off[s]) { orbx_set_error("segment %d is empty or the offsets fall", s); return ORBX_ERR_ARG; }
    return ORBX_OK;
}

}  // namespace

extern "C" int orbx_voc_trainer_create(int device, int k, int L, int max_descriptors, int max_images, orbx_voc_trainer **out)
{
    if (!out) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    *out = nullptr;
    if (k < 2 || k > ORBX_VOC_MAX_K) { orbx_set_error("k = %d outside 2..%d", k, ORBX_VOC_MAX_K); return ORBX_ERR_ARG; }
    if (L < 1 || L > ORBX_VOC_MAX_L) { orbx_set_error("L = %d outside 1..%d", L, ORBX_VOC_MAX_L); return ORBX_ERR_ARG; }
    if (!vt_tree_fits(k, L)) { orbx_set_error("a complete tree with k = %d, L = %d has 2^31 nodes or more", k, L); return ORBX_ERR_ARG; }
    if (max_descriptors < 1 || max_descriptors > (1 << 26)) { orbx_set_error("max_descriptors = %d outside 1..2^26", max_descriptors); return ORBX_ERR_ARG; }
    if (max_images < 1) { orbx_set_error("max_images = %d < 1", max_images); return ORBX_ERR_ARG; }
    orbx_voc_trainer *h = new orbx_voc_trainer();
    h->k = k; h->L = L; h->maxDesc = max_descriptors; h->maxImg = max_images;
    int rc = h->open(device);
    if (!rc) rc = orbx_event_create(&h->extEvent, hipEventDisableTiming);
    if (!rc) rc = h->desc.ensure(2 * (size_t)max_descriptors);
    if (!rc) rc = h->imgCount.ensure((size_t)max_images);
    if (!rc) rc = h->state.ensure(4);
    if (!rc) rc = vt_push_state(h);
    if (!rc) {
        auto [pin, pout] = h->box.plan();
        (void)pin;
        const auto rChanged = pout.hole<int32_t>(1);
        const OrbxStaged sg = h->box.begin(h->stream, &rc);
        if (!rc) { h->changedDev = sg.dev(rChanged); h->changedHost = sg.host(rChanged); }
    }
    if (rc) { orbx_voc_trainer_destroy(h); return rc; }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_voc_trainer_destroy(orbx_voc_trainer *h) { orbx_destroy_handle(h); }

extern "C" int orbx_voc_trainer_add(orbx_voc_trainer *h, const uint8_t *descriptors, const int32_t *counts, int num_images)
{
    if (!h || !counts || num_images < 0) { orbx_set_error("NULL handle or bad argument"); return ORBX_ERR_ARG; }
    long long total = 0;
    for (int i = 0; i < num_images; i++) {
        if (counts[i] < 0) { orbx_set_error("image %d has a negative feature count", i); return ORBX_ERR_ARG; }
        total += counts[i];
    }
    if (total > 0 && !descriptors) { orbx_set_error("NULL descriptors"); return ORBX_ERR_ARG; }
    if (num_images == 0) return ORBX_OK;
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    int rc = vt_sync_state(h);
    if (rc) return rc;
    if (h->nDesc + total > h->maxDesc || (long long)h->nImg + num_images > h->maxImg) {
        orbx_set_error("%lld descriptors in %d images do not fit behind %d / %d (capacity %d / %d)", total, num_images, h->nDesc, h->nImg, h->maxDesc, h->maxImg);
        return ORBX_ERR_CAPACITY;
    }
    if (total) ORBX_HIP_CHECK(hipMemcpy(h->desc.p + 2 * (size_t)h->nDesc, descriptors, (size_t)total * 32, hipMemcpyHostToDevice));
    ORBX_HIP_CHECK(hipMemcpy(h->imgCount.p + h->nImg, counts, (size_t)num_images * sizeof(int32_t), hipMemcpyHostToDevice));
    h->nDesc += (int)total; h->nImg += num_images;
    return vt_push_state(h);
}

extern "C" int orbx_voc_trainer_add_extracted(orbx_voc_trainer *h, orbx_extractor *ext)
{
    if (!h || !ext) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    OrbxLastBatchView view;
    int rc = orbx_extractor_last_batch_view_internal(ext, &view);      // ORBX_ERR_STATE e.g. after a chunked host batch
    if (rc != ORBX_OK) return rc;
    if (view.batch < 1) { orbx_set_error("the extractor's last batch is empty"); return ORBX_ERR_STATE; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    // on the extractor's stream: ordered behind the extraction and ahead of the batch that overwrites these results; the trainer's own stream
    // (and the host, before it reads the state) waits for the event behind it
    hipStream_t es = orbx_extractor_stream_internal(ext);
    hipLaunchKernelGGL(k_append_extracted, dim3((unsigned)view.batch), dim3(256), 0, es, view.desc, view.counts, view.batch, view.cap, (const int32_t *)h->state.p,
                       h->maxDesc, h->maxImg, h->desc.p, h->imgCount.p);
    hipLaunchKernelGGL(k_append_commit, dim3(1), dim3(1), 0, es, view.counts, view.batch, view.cap, h->state.p, h->maxDesc, h->maxImg);
    if ((rc = vt_launch_check("k_append_extracted"))) return rc;
    ORBX_HIP_CHECK(hipEventRecord(h->extEvent, es));
    ORBX_HIP_CHECK(hipStreamWaitEvent(h->stream, h->extEvent, 0));
    h->dirty = true;
    return ORBX_OK;
}

extern "C" int orbx_voc_trainer_clear(orbx_voc_trainer *h)
{
    if (!h) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    if (h->dirty) { if (h->extEvent) ORBX_HIP_CHECK(hipEventSynchronize(h->extEvent)); h->dirty = false; }
    h->nDesc = 0; h->nImg = 0;
    return vt_push_state(h);
}

extern "C" int orbx_voc_trainer_size(orbx_voc_trainer *h, int *descriptors, int *images)
{
    if (!h) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    int rc = vt_sync_state(h);
    if (descriptors) *descriptors = h->nDesc;
    if (images) *images = h->nImg;
    return rc;
}

extern "C" int orbx_voc_trainer_set_profiling(orbx_voc_trainer *h, int enable)
{
    if (!h) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    h->profiling = enable != 0;
    return ORBX_OK;
}

extern "C" int orbx_voc_train(orbx_voc_trainer *h, const orbx_voc_train_params *params, orbx_voc_train_summary *summary)
{
    if (!h || !params) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (params->weighting < 0 || params->weighting > 3) { orbx_set_error("weighting %d: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY", params->weighting); return ORBX_ERR_ARG; }
    if (params->max_iterations < 2) { orbx_set_error("max_iterations = %d < 2", params->max_iterations); return ORBX_ERR_ARG; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    int rc = vt_sync_state(h);
    if (rc) return rc;
    const int N = h->nDesc, k = h->k, L = h->L, nImg = h->nImg;
    if (N < 1) { orbx_set_error("no descriptors to train on"); return ORBX_ERR_STATE; }
    h->trained = false;
    const auto t0 = std::chrono::steady_clock::now();
    h->totalMs = 0; h->launches = 0; h->evUsed = 0;
    for (float &v : h->levelMs) v = 0;
    for (float &v : h->stageMs) v = 0;
    const u64 seed = params->seed;
    const uint4 *desc = h->desc.p;

    // the tree as it grows, level by level: the children of a node are appended together, so a node names them by first + count
    struct TNode { int32_t parent, firstChild, numChild; };
    std::vector<TNode> tree(1, TNode{-1, -1, 0});
    std::vector<uint8_t> tdesc(32, 0);
    std::vector<int32_t> nodeOfSeg(1, 0), hostNc, hostCounts;
    VtLevel lv;
    lv.segs.assign(1, VtSeg{0, N, 0, -1, 0, N > k ? 1 : 0, 0});
    int cur = 0, unconverged = 0, passes[ORBX_VOC_MAX_L] = {0};
    bool first = true;
    for (int level = 1; level <= L && !lv.segs.empty(); level++) {
        const auto tl = std::chrono::steady_clock::now();
        lv.finish(k, false);
        const int S = (int)lv.segs.size();
        if ((rc = vt_ensure_work(h, (size_t)N, lv))) return rc;
        if (first) {
            hipLaunchKernelGGL(k_iota, dim3(vt_blocks((size_t)N)), dim3(256), 0, h->stream, N, h->perm[0].p);
            ORBX_HIP_CHECK(hipMemsetAsync(h->md.p, 0, (size_t)N * sizeof(int32_t), h->stream));
            ORBX_HIP_CHECK(hipMemsetAsync(h->assoc.p, 0, (size_t)N * sizeof(int32_t), h->stream));
            first = false;
        }
        vt_mark(h, VT_OTHER);
        if ((rc = vt_upload_level(h, N, lv))) return rc;
        if ((rc = vt_seed(h, desc, N, lv, seed, cur))) return rc;
        if (lv.anyBig) {
            // Lloyd passes for all segments of the level together, until no segment changes or the cap.  A segment that has converged keeps
            // running with the others: on a fixed point a pass changes nothing - the means of an unchanged association are the centres that
            // produced it (an empty cluster keeps its centre in both passes alike), so the next association is the same again - and its
            // stamp stays behind the pass number.  The host reads one mapped record per pass: no stream synchronisation, no copy.
            int pass = 0, changed = 0;
            for (;;) {
                ++pass;
                if (pass > 1 && (rc = vt_mean(h, desc, N, lv, cur))) return rc;
                if ((rc = vt_assign(h, desc, N, pass, cur, &changed))) return rc;
                if (pass >= 2 && changed == 0) break;
                if (pass >= params->max_iterations) { unconverged += changed; break; }
            }
            passes[level - 1] = pass;
        }
        if (lv.anyBig && level < L) {
            vt_mark(h, VT_PART);
            for (int c0 = 0; c0 < k; c0 += 2) {
                if ((rc = vt_scan<1>(h, N, h->assoc.p, c0))) return rc;
                hipLaunchKernelGGL(k_part_scatter, dim3(vt_blocks((size_t)N)), dim3(256), 0, h->stream, (const VtSeg *)h->segs.p, (const int32_t *)h->segOf.p, N, c0,
                                   (const u64 *)h->G.p, (const int32_t *)h->assoc.p, (const int32_t *)h->perm[cur].p, h->perm[cur ^ 1].p, (const int32_t *)h->cursor.p);
                hipLaunchKernelGGL(k_part_advance, dim3(vt_blocks((size_t)S)), dim3(256), 0, h->stream, (const VtSeg *)h->segs.p, S, k, c0, (const u64 *)h->G.p, h->cursor.p,
                                   h->counts.p);
                h->launches += 2;
                if ((rc = vt_launch_check("partition"))) return rc;
            }
        }
        vt_mark(h, VT_OTHER);
        // the level's result: clusters per segment, their centres, and (where the tree goes on) their sizes
        hostNc.resize((size_t)S);
        const size_t base = tdesc.size() / 32;      // the first node of this level's children
        tdesc.resize((base + (size_t)lv.slots) * 32);
        ORBX_HIP_CHECK(hipMemcpyAsync(hostNc.data(), h->nc.p, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        ORBX_HIP_CHECK(hipMemcpyAsync(tdesc.data() + base * 32, h->centres.p, (size_t)lv.slots * 32, hipMemcpyDeviceToHost, h->stream));
        const bool deeper = lv.anyBig && level < L;
        if (deeper) {
            hostCounts.resize((size_t)lv.slots);
            ORBX_HIP_CHECK(hipMemcpyAsync(hostCounts.data(), h->counts.p, (size_t)lv.slots * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        }
        ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
        vt_collect(h);
        // children: node base + cOff + c for cluster c (slots beyond a segment's clusters stay unused and are dropped by the renumbering);
        // recursion only below level L and only into a child with more than one feature (:796-817)
        tree.resize(base + (size_t)lv.slots, TNode{-1, -1, 0});
        VtLevel next;
        std::vector<int32_t> nextNode;
        for (int s = 0; s < S; s++) {
            const VtSeg &sg = lv.segs[(size_t)s];
            const int node = nodeOfSeg[(size_t)s], n = hostNc[(size_t)s];
            tree[(size_t)node].firstChild = (int32_t)base + sg.cOff;
            tree[(size_t)node].numChild = n;
            int at = sg.start;
            for (int c = 0; c < n; c++) {
                const size_t child = base + (size_t)sg.cOff + (size_t)c;
                tree[child].parent = node;
                if (!sg.big || !deeper) continue;
                const int cnt = hostCounts[(size_t)sg.cOff + (size_t)c];
                if (cnt > 1) {
                    next.segs.push_back(VtSeg{at, at + cnt, 0, -1, sg.slot * (u64)k + (u64)c + 1, cnt > k ? 1 : 0, 0});
                    nextNode.push_back((int32_t)child);
                }
                at += cnt;
            }
        }
        if (deeper) cur ^= 1;
        lv.segs.swap(next.segs);
        nodeOfSeg.swap(nextNode);
        h->levelMs[level - 1] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - tl).count();
    }

    // node ids in the reference's order: a node's children take the next consecutive ids when the node is clustered, then the children are
    // recursed in order (:786-817); word ids count the leaves in node-id order (createWords)
    std::vector<int32_t> newId(tree.size(), -1), order;
    order.reserve(tree.size());
    {
        std::vector<int32_t> stack(1, 0);
        newId[0] = 0; order.push_back(0);
        while (!stack.empty()) {
            const int32_t nd = stack.back();
            stack.pop_back();
            const TNode &t = tree[(size_t)nd];
            for (int c = 0; c < t.numChild; c++) { newId[(size_t)(t.firstChild + c)] = (int32_t)order.size(); order.push_back(t.firstChild + c); }
            for (int c = t.numChild - 1; c >= 0; c--)
                if (tree[(size_t)(t.firstChild + c)].numChild > 0) stack.push_back(t.firstChild + c);
        }
    }
    const int numNodes = (int)order.size();
    h->parent.assign((size_t)numNodes, 0); h->isLeaf.assign((size_t)numNodes, 0); h->nodeDescHost.assign((size_t)numNodes * 32, 0);
    h->weights.assign((size_t)numNodes, 0.0); h->ni_.assign((size_t)numNodes, 0);
    std::vector<int32_t> cStart((size_t)numNodes, 0), cCount((size_t)numNodes, 0), nWord((size_t)numNodes, -1);
    int words = 0;
    for (int id = 0; id < numNodes; id++) {
        const int32_t old = order[(size_t)id];
        const TNode &t = tree[(size_t)old];
        h->parent[(size_t)id] = id ? newId[(size_t)t.parent] : 0;
        memcpy(&h->nodeDescHost[(size_t)id * 32], &tdesc[(size_t)old * 32], 32);
        cCount[(size_t)id] = t.numChild;
        cStart[(size_t)id] = t.numChild ? newId[(size_t)t.firstChild] : 0;
        const bool leaf = id > 0 && t.numChild == 0;
        h->isLeaf[(size_t)id] = leaf;
        if (leaf) nWord[(size_t)id] = words++;
    }

    // setNodeWeights: Ni counted on the device from the real descent; the logarithm is libm's, taken here
    std::vector<int32_t> wordNi((size_t)(words ? words : 1), 0);
    if (words > 0) {
        std::vector<int32_t> imgCount((size_t)(nImg ? nImg : 1), 0), imgStart((size_t)nImg + 1, 0);
        if (nImg) ORBX_HIP_CHECK(hipMemcpy(imgCount.data(), h->imgCount.p, (size_t)nImg * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int m = 0; m < nImg; m++) imgStart[(size_t)m + 1] = imgStart[(size_t)m] + imgCount[(size_t)m];
        u64 slots = 1024;
        while (slots < 2 * (u64)N) slots <<= 1;
        if ((rc = h->nodeDesc.ensure(2 * (size_t)numNodes)) || (rc = h->childStart.ensure((size_t)numNodes)) || (rc = h->childCount.ensure((size_t)numNodes)) ||
            (rc = h->nodeWord.ensure((size_t)numNodes)) || (rc = h->word.ensure((size_t)N)) || (rc = h->ni.ensure((size_t)words)) ||
            (rc = h->imgStart.ensure((size_t)nImg + 1)) || (rc = h->table.ensure((size_t)slots)))
            return rc;
        vt_mark(h, VT_OTHER);
        ORBX_HIP_CHECK(hipMemcpyAsync(h->nodeDesc.p, h->nodeDescHost.data(), (size_t)numNodes * 32, hipMemcpyHostToDevice, h->stream));
        ORBX_HIP_CHECK(hipMemcpyAsync(h->childStart.p, cStart.data(), (size_t)numNodes * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        ORBX_HIP_CHECK(hipMemcpyAsync(h->childCount.p, cCount.data(), (size_t)numNodes * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        ORBX_HIP_CHECK(hipMemcpyAsync(h->nodeWord.p, nWord.data(), (size_t)numNodes * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        ORBX_HIP_CHECK(hipMemcpyAsync(h->imgStart.p, imgStart.data(), ((size_t)nImg + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        ORBX_HIP_CHECK(hipMemsetAsync(h->ni.p, 0, (size_t)words * sizeof(int32_t), h->stream));
        ORBX_HIP_CHECK(hipMemsetAsync(h->table.p, 0xff, (size_t)slots * sizeof(u64), h->stream));
        hipLaunchKernelGGL(k_descend, dim3(vt_blocks((size_t)N)), dim3(256), 0, h->stream, N, desc, (const int32_t *)h->childStart.p, (const int32_t *)h->childCount.p,
                           (const uint4 *)h->nodeDesc.p, (const int32_t *)h->nodeWord.p, h->word.p);
        if (nImg > 0)
            hipLaunchKernelGGL(k_ni, dim3(vt_blocks((size_t)N)), dim3(256), 0, h->stream, N, (const int32_t *)h->word.p, (const int32_t *)h->imgStart.p, nImg, h->table.p,
                               slots - 1, h->ni.p);
        h->launches += 2;
        if ((rc = vt_launch_check("k_descend / k_ni"))) return rc;
        vt_mark(h, VT_OTHER);
        ORBX_HIP_CHECK(hipMemcpyAsync(wordNi.data(), h->ni.p, (size_t)words * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
        vt_collect(h);
    }
    const bool idf = params->weighting == 0 || params->weighting == 2;
    for (int id = 1; id < numNodes; id++) {
        if (!h->isLeaf[(size_t)id]) continue;
        const int n = wordNi[(size_t)nWord[(size_t)id]];
        h->ni_[(size_t)id] = n;
        h->weights[(size_t)id] = idf ? (n > 0 ? log((double)nImg / (double)n) : 0.0) : 1.0;
    }
    h->numNodes = numNodes; h->numWords = words;
    h->trained = true;
    h->totalMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (summary) {
        summary->num_nodes = numNodes; summary->num_words = words; summary->unconverged_nodes = unconverged;
        for (int l = 0; l < ORBX_VOC_MAX_L; l++) summary->passes_per_level[l] = passes[l];
    }
    return ORBX_OK;
}

extern "C" int orbx_voc_trainer_result(orbx_voc_trainer *h, int32_t *parent, uint8_t *is_leaf, uint8_t *descriptors, double *weights, int32_t *ni, int capacity_nodes)
{
    if (!h) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    if (!h->trained) { orbx_set_error("no vocabulary has been trained yet"); return ORBX_ERR_STATE; }
    if (capacity_nodes < h->numNodes) { orbx_set_error("%d nodes, room for %d", h->numNodes, capacity_nodes); return ORBX_ERR_CAPACITY; }
    const size_t n = (size_t)h->numNodes;
    if (parent) memcpy(parent, h->parent.data(), n * sizeof(int32_t));
    if (is_leaf) memcpy(is_leaf, h->isLeaf.data(), n);
    if (descriptors) memcpy(descriptors, h->nodeDescHost.data(), n * 32);
    if (weights) memcpy(weights, h->weights.data(), n * sizeof(double));
    if (ni) memcpy(ni, h->ni_.data(), n * sizeof(int32_t));
    return ORBX_OK;
}

extern "C" int orbx_voc_trainer_vocabulary(orbx_voc_trainer *h, orbx_vocabulary **voc)
{
    if (!h || !voc) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    *voc = nullptr;
    if (!h->trained) { orbx_set_error("no vocabulary has been trained yet"); return ORBX_ERR_STATE; }
    return orbx_vocabulary_create(h->device, h->k, h->L, h->numNodes, h->parent.data(), h->isLeaf.data(), h->nodeDescHost.data(), h->weights.data(), voc);
}

extern "C" int orbx_voc_trainer_last_timing(orbx_voc_trainer *h, float *total_ms, float *level_ms, float *stage_ms, int *launches)
{
    if (!h) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    if (!h->trained) { orbx_set_error("no vocabulary has been trained yet"); return ORBX_ERR_STATE; }
    if (total_ms) *total_ms = h->totalMs;
    if (level_ms) for (int l = 0; l < ORBX_VOC_MAX_L; l++) level_ms[l] = h->levelMs[l];
    if (stage_ms) for (int i = 0; i < 5; i++) stage_ms[i] = h->stageMs[i];
    if (launches) *launches = h->launches;
    return ORBX_OK;
}

// ---- the two stages on explicit inputs ----
static int vt_stage_begin(orbx_voc_trainer *h, const uint8_t *descriptors, int n, const int32_t *seg_offsets, int num_segments, VtLevel &lv, bool allBig, const int32_t *numCentres,
                          const u64 *slots)
{
    if (!h || !descriptors || !seg_offsets || n < 1 || num_segments < 1) { orbx_set_error("NULL handle or bad argument"); return ORBX_ERR_ARG; }
    if (n > h->maxDesc) { orbx_set_error("%d descriptors, the handle holds %d", n, h->maxDesc); return ORBX_ERR_CAPACITY; }
    int rc = vt_check_offsets(seg_offsets, num_segments, n);
    if (rc) return rc;
    if ((long long)num_segments * h->k >= (1ll << 31)) { orbx_set_error("too many segments"); return ORBX_ERR_ARG; }
    lv.segs.resize((size_t)num_segments);
    for (int s = 0; s < num_segments; s++) {
        if (numCentres && (numCentres[s] < 1 || numCentres[s] > h->k)) { orbx_set_error("segment %d: %d centres outside 1..%d", s, numCentres[s], h->k); return ORBX_ERR_ARG; }
        lv.segs[(size_t)s] = VtSeg{seg_offsets[s], seg_offsets[s + 1], 0, -1, slots ? slots[s] : 0, (allBig || seg_offsets[s + 1] - seg_offsets[s] > h->k) ? 1 : 0, 0};
    }
    lv.finish(h->k, true);
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    if ((rc = vt_ensure_work(h, (size_t)n, lv)) || (rc = h->stageDesc.ensure(2 * (size_t)n))) return rc;
    ORBX_HIP_CHECK(hipMemcpyAsync(h->stageDesc.p, descriptors, (size_t)n * 32, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_iota, dim3(vt_blocks((size_t)n)), dim3(256), 0, h->stream, n, h->perm[0].p);
    ORBX_HIP_CHECK(hipMemsetAsync(h->md.p, 0, (size_t)n * sizeof(int32_t), h->stream));
    return vt_upload_level(h, n, lv);
}

extern "C" int orbx_voc_seed_segments(orbx_voc_trainer *h, const uint8_t *descriptors, int n, const int32_t *seg_offsets, const uint64_t *slots, int num_segments,
                                      uint64_t seed, int32_t *chosen)
{
    if (!slots || !chosen) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    VtLevel lv;
    int rc = vt_stage_begin(h, descriptors, n, seg_offsets, num_segments, lv, false, nullptr, (const u64 *)slots);
    if (rc) return rc;
    // (a segment with n <= k reports 0 .. n - 1; the slots it does not use are filled here)
    ORBX_HIP_CHECK(hipMemsetAsync(h->chosen.p, 0xff, (size_t)lv.slots * sizeof(int32_t), h->stream));
    if ((rc = vt_seed(h, h->stageDesc.p, n, lv, (u64)seed, 0))) return rc;
    ORBX_HIP_CHECK(hipMemcpyAsync(chosen, h->chosen.p, (size_t)lv.slots * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->evUsed = 0;
    return ORBX_OK;
}

extern "C" int orbx_voc_lloyd_pass(orbx_voc_trainer *h, const uint8_t *descriptors, int n, const int32_t *seg_offsets, int num_segments, const uint8_t *centres,
                                   const int32_t *num_centres, const int32_t *prev_assoc, uint8_t *centres_out, int32_t *assoc_out, uint8_t *changed_out)
{
    if (!centres || !num_centres) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (h && prev_assoc && seg_offsets && num_segments >= 1 && n >= 1)
        for (int s = 0; s < num_segments; s++)
            for (int p = seg_offsets[s]; p >= 0 && p < seg_offsets[s + 1] && p < n; p++)
                if (prev_assoc[p] < 0 || prev_assoc[p] >= num_centres[s]) { orbx_set_error("previous association of feature %d outside its segment's centres", p); return ORBX_ERR_ARG; }
    VtLevel lv;
    int rc = vt_stage_begin(h, descriptors, n, seg_offsets, num_segments, lv, true, num_centres, nullptr);
    if (rc) return rc;
    const int S = num_segments;
    ORBX_HIP_CHECK(hipMemcpyAsync(h->centres.p, centres, (size_t)lv.slots * 32, hipMemcpyHostToDevice, h->stream));
    ORBX_HIP_CHECK(hipMemcpyAsync(h->nc.p, num_centres, (size_t)S * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(h->changedPass.p, 0, (size_t)S * sizeof(int32_t), h->stream));
    if (prev_assoc) ORBX_HIP_CHECK(hipMemcpyAsync(h->assoc.p, prev_assoc, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    int changed = 0;
    const int pass = prev_assoc ? 2 : 1;
    if (prev_assoc && (rc = vt_mean(h, h->stageDesc.p, n, lv, 0))) return rc;
    if ((rc = vt_assign(h, h->stageDesc.p, n, pass, 0, &changed))) return rc;
    if ((rc = h->flags.ensure((size_t)S))) return rc;
    hipLaunchKernelGGL(k_changed_flags, dim3(vt_blocks((size_t)S)), dim3(256), 0, h->stream, S, pass, (const int32_t *)h->changedPass.p, h->flags.p);
    if ((rc = vt_launch_check("k_changed_flags"))) return rc;
    if (centres_out) ORBX_HIP_CHECK(hipMemcpyAsync(centres_out, h->centres.p, (size_t)lv.slots * 32, hipMemcpyDeviceToHost, h->stream));
    if (assoc_out) ORBX_HIP_CHECK(hipMemcpyAsync(assoc_out, h->assoc.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (changed_out) ORBX_HIP_CHECK(hipMemcpyAsync(changed_out, h->flags.p, (size_t)S, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->evUsed = 0;
    return ORBX_OK;
}
