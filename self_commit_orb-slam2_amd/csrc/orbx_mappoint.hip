// orbx_mappoint.hip -- MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth for a batch of points (gfx950 only).
//
// Reference: src/MapPoint.cc:359-439 and :477-521, run by the local mapper, the tracker, the bundle adjustments and the loop corrector over
// hundreds to tens of thousands of points, one point at a time.  Here: M points with ragged observation lists (CSR, the CALLER's order = the
// order of std::map<KeyFrame*, size_t>; never reordered) in one launch chain.
//
// Descriptor choice.  N = the point's valid descriptors in list order; row i = Hamming distances of descriptor i to all N (self-distance 0
// included); median = the element at sorted position (N - 1) / 2 (the reference's vDists[0.5*(N-1)] truncates the same way); the winner is the
// LOWEST i with the smallest median (`median < BestMedian` is strict).  Nothing is sorted: distances live in 0..256, so
//   n <= 64 / 128 / 256 (k_mp_block<64 / 128 / 256>, one workgroup of that many threads per point): thread i owns row i, the descriptors sit in
//       LDS and are read as wave-uniform broadcasts (2 x ds_read_b128 per column), a column costs 8 v_xor + 8 v_bcnt (accumulating); the row is
//       kept ONCE as u16 in LDS ([column][thread]: conflict free) and the k-th smallest is a 9-step bisection on the value with a count of d <= v;
//   larger n (k_mp_strided, 256 threads stride over the rows): a row does not fit, so it is histogrammed instead - 257 u16 bins per thread in
//       LDS ([bin][thread]), one pass over the columns (staged through LDS 256 at a time), then a walk over the bins.  n <= 65535 here.
// The arg-min over the rows with the lowest-index tie is a butterfly minimum of (median << 16 | i).  (DESIGN.md section 5 prices the variants.)
//
// Normal and depth, bit for bit what the compiled reference computes on the project's OpenCV stand-in (oracle/cvshim/cvshim.hpp:411-418,
// 480-492): per observer, in list order, v = pos - Ow in float, s = sqrt(v0^2 + v1^2 + v2^2) accumulated in double from 0, u = (float)((double)v / s);
// normal += u in float, SEQUENTIALLY in observation order (a float sum of three or more terms depends on the order: one lane per component
// walks the list, nothing is tree-reduced); normal = (float)((double)normal / (double)n); dist = (float)sqrt(double sum of (pos - refOw)^2);
// max = dist * refScale, min = max / topScale.  The unit vectors are independent and computed one observation per thread.
// Stock OpenCV's Mat / double multiplies by a float reciprocal instead of dividing in double: parity unpinned for the quotient.
// Observers whose keyframe isBad() (desc_valid == 0) are skipped for the descriptor (:384) and still count for the normal, as in the reference.
//
// Results leave through a plain stream synchronisation (one pinned upload, the kernels, one pinned download, hipStreamSynchronize): a call moves
// megabytes and runs for tens of microseconds to milliseconds, the 40 us the mapped-memory convention of orbx_internal.h saves do not matter here.
#include <algorithm>
#include <climits>
#include <vector>

#include "orbx_handle.h"
#include "orbx_normal_depth.h"

namespace {

struct MpDev {
    const int32_t *off;          // [M + 1]
    const uint32_t *desc;        // [T][8]
    const uint8_t *valid;        // [T] or nullptr = all valid
    const float *cam;            // [T][3]
    const float *pos, *refc;     // [M][3]
    const float *rsc, *tsc;      // [M]
    const int32_t *list;         // points of this launch
    int32_t *bestObs, *bestMed;  // [M]
    float *normal, *maxD, *minD; // [M][3], [M], [M]
    float *unit;                 // scratch [T][3]: unit vectors of the strided class
    int32_t *comp;               // scratch [T]: valid observations of a point of the strided class, compacted (local indices)
};

__device__ __forceinline__ int mp_dist(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1)
{
    int d = __popc(a0.x ^ b0.x);
    d += __popc(a0.y ^ b0.y); d += __popc(a0.z ^ b0.z); d += __popc(a0.w ^ b0.w);
    d += __popc(a1.x ^ b1.x); d += __popc(a1.y ^ b1.y); d += __popc(a1.z ^ b1.z); d += __popc(a1.w ^ b1.w);
    return d;
}

// (mp_unit, mp_normal_component and mp_depth, the arithmetic the header spells, live in orbx_normal_depth.h: the loop corrector shares them)

// the ordered part, after the unit vectors are visible to the workgroup: threads 0..2 sum one component each over the list, thread 3 the distances
__device__ __forceinline__ void mp_normal_depth(const MpDev &D, int p, int n, const float *unit, int t)
{
    if (t < 3) D.normal[(size_t)p * 3 + t] = mp_normal_component(unit, n, t);
    else if (t == 3) mp_depth(D.pos + (size_t)p * 3, D.refc + (size_t)p * 3, D.rsc[p], D.tsc[p], &D.maxD[p], &D.minD[p]);
}

constexpr size_t mp_block_lds(int tpp) { return (size_t)tpp * 32 + (size_t)tpp * tpp * 2 + (size_t)tpp * 12 + (size_t)tpp * 2 + 64; }

// One workgroup of TPP threads per point with n <= TPP observations.
template <int TPP> __global__ __launch_bounds__(TPP) void k_mp_block(MpDev D)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t mpLds[];
    uint32_t *sDesc = (uint32_t *)mpLds;                    // [TPP][8]   valid descriptors, compacted in list order
    uint16_t *sRow = (uint16_t *)(sDesc + TPP * 8);         // [TPP][TPP] distance of row `thread` to column j at [j][thread]
    float *sUnit = (float *)(sRow + TPP * TPP);             // [TPP][3]
    uint16_t *sIdx = (uint16_t *)(sUnit + TPP * 3);         // [TPP]      compacted -> position in the observation list
    int *sW = (int *)(sIdx + TPP);                          // [0..3] valid count per wave, [4..7] minimum key per wave
    constexpr int NW = TPP / 64;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int p = D.list[blockIdx.x];
    const int o0 = D.off[p], n = D.off[p + 1] - o0;

    bool v = false;
    uint4 d0 = {}, d1 = {};
    if (t < n) {
        v = !D.valid || D.valid[o0 + t] != 0;
        const uint4 *g = (const uint4 *)(D.desc + (size_t)(o0 + t) * 8);
        d0 = g[0]; d1 = g[1];
        mp_unit(D.pos + (size_t)p * 3, D.cam + (size_t)(o0 + t) * 3, sUnit + t * 3);
    }
    const unsigned long long m = __ballot(v);
    int rank = __popcll(m & ((1ull << lane) - 1ull)), N = __popcll(m);
    if (NW > 1) {
        if (lane == 0) sW[w] = N;
        __syncthreads();
        N = 0;
        for (int i = 0; i < NW; i++) { if (i < w) rank += sW[i]; N += sW[i]; }
    }
    if (v) {
        uint4 *s = (uint4 *)(sDesc + rank * 8);
        s[0] = d0; s[1] = d1;
        sIdx[rank] = (uint16_t)t;
    }
    __syncthreads();

    unsigned key = 0xffffffffu;
    if (t < N) {
        const uint4 a0 = ((const uint4 *)(sDesc + t * 8))[0], a1 = ((const uint4 *)(sDesc + t * 8))[1];
        for (int j = 0; j < N; j++) {
            const uint4 *c = (const uint4 *)(sDesc + j * 8);      // wave-uniform address: an LDS broadcast
            sRow[j * TPP + t] = (uint16_t)mp_dist(a0, a1, c[0], c[1]);
        }
        // k-th smallest of the row, k = (N - 1) / 2: the smallest value v with count(d <= v) >= k + 1.  257 candidates = 9 halvings; a lane whose
        // interval closed early keeps lo == hi (count(d <= lo) >= k + 1 holds there), so the loops stay uniform.
        const int need = ((N - 1) >> 1) + 1;
        int lo = 0, hi = 256;
        for (int s = 0; s < 9; s++) {
            const int mid = (lo + hi) >> 1;
            int cnt = 0;
            for (int j = 0; j < N; j++) cnt += (int)sRow[j * TPP + t] <= mid ? 1 : 0;
            if (cnt >= need) hi = mid; else lo = mid + 1;
        }
        key = (unsigned)lo << 16 | (unsigned)t;
    }
    key = wave_min(key);
    if (NW > 1) {
        if (lane == 0) sW[4 + w] = (int)key;
        __syncthreads();
        for (int i = 0; i < NW; i++) key = min(key, (unsigned)sW[4 + i]);
    }
    if (t == 0) {
        D.bestObs[p] = N ? (int32_t)sIdx[key & 0xffffu] : -1;
        D.bestMed[p] = N ? (int32_t)(key >> 16) : INT_MAX;
    }
    mp_normal_depth(D, p, n, sUnit, t);
}

#define MP_HIST_BINS 257
constexpr size_t mp_strided_lds() { return (size_t)MP_HIST_BINS * 256 * 2 + 256 * 32 + 64; }

// One workgroup of 256 threads per point with more than 256 (and at most 65535) observations.
__global__ __launch_bounds__(256) void k_mp_strided(MpDev D)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t mpLds[];
    uint32_t *sDesc = (uint32_t *)mpLds;                    // [256][8]  one chunk of columns
    uint16_t *sHist = (uint16_t *)(sDesc + 256 * 8);        // [257][256] bins of row `thread` at [bin][thread]
    int *sW = (int *)(sHist + MP_HIST_BINS * 256);          // [0..3] valid count per wave, [4..7] minimum key per wave
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int p = D.list[blockIdx.x];
    const int o0 = D.off[p], n = D.off[p + 1] - o0;
    int32_t *comp = D.comp + o0;
    float *unit = D.unit + (size_t)o0 * 3;

    // unit vectors and the compacted list of valid observations, 256 observations at a time
    int N = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int o = c0 + t;
        bool v = false;
        if (o < n) {
            v = !D.valid || D.valid[o0 + o] != 0;
            mp_unit(D.pos + (size_t)p * 3, D.cam + (size_t)(o0 + o) * 3, unit + (size_t)o * 3);
        }
        const unsigned long long m = __ballot(v);
        int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) sW[w] = __popcll(m);
        __syncthreads();
        int tot = 0;
        for (int i = 0; i < 4; i++) { if (i < w) rank += sW[i]; tot += sW[i]; }
        if (v) comp[N + rank] = o;
        N += tot;
        __syncthreads();
    }
    // (the second barrier of the last round also orders the comp / unit stores before the loads below: same workgroup, global memory)

    const int need = ((N - 1) >> 1) + 1;
    unsigned key = 0xffffffffu;
    for (int i0 = 0; i0 < N; i0 += 256) {
        const int i = i0 + t;
        const bool act = i < N;
        uint4 a0 = {}, a1 = {};
        if (act) {
            const uint4 *g = (const uint4 *)(D.desc + (size_t)(o0 + comp[i]) * 8);
            a0 = g[0]; a1 = g[1];
        }
        for (int b = 0; b < MP_HIST_BINS; b++) sHist[b * 256 + t] = 0;      // own column only: no barrier
        for (int j0 = 0; j0 < N; j0 += 256) {
            __syncthreads();      // the previous chunk has been consumed
            if (j0 + t < N) {
                const uint4 *g = (const uint4 *)(D.desc + (size_t)(o0 + comp[j0 + t]) * 8);
                uint4 *s = (uint4 *)(sDesc + t * 8);
                s[0] = g[0]; s[1] = g[1];
            }
            __syncthreads();
            if (act) {
                const int nj = min(256, N - j0);
                for (int j = 0; j < nj; j++) {
                    const uint4 *c = (const uint4 *)(sDesc + j * 8);
                    const int d = mp_dist(a0, a1, c[0], c[1]);
                    sHist[d * 256 + t] = (uint16_t)(sHist[d * 256 + t] + 1);
                }
            }
        }
        if (act) {
            int acc = 0, med = 0;
            for (int b = 0; b < MP_HIST_BINS; b++) {
                acc += sHist[b * 256 + t];
                if (acc >= need) { med = b; break; }
            }
            key = min(key, (unsigned)med << 16 | (unsigned)i);
        }
    }
    key = wave_min(key);
    if (lane == 0) sW[4 + w] = (int)key;
    __syncthreads();
    for (int i = 0; i < 4; i++) key = min(key, (unsigned)sW[4 + i]);
    if (t == 0) {
        D.bestObs[p] = N ? comp[key & 0xffffu] : -1;
        D.bestMed[p] = N ? (int32_t)(key >> 16) : INT_MAX;
    }
    mp_normal_depth(D, p, n, unit, t);
}

}  // namespace

#define MP_MAX_OBS 65535      /* per point: u16 bins and the 16-bit row index of the arg-min key */

struct orbx_mappoint_ops : OrbxHandle {
    int maxPoints = 0, maxObs = 0;
    OrbxCallTimer timer;
    OrbxHostStage stage;                 // inputs of a call: one pinned buffer, one copy
    OrbxOwnedBuf<uint8_t> out;             // bestObs | bestMed | normal | maxD | minD
    OrbxOwnedBuf<float> unit;
    OrbxOwnedBuf<int32_t> comp;
    uint8_t *hostOut = nullptr;          // pinned, sized for maxPoints
    std::vector<int32_t> lists[4];
    float kernelMs = 0.0f;               // read inside the call, behind its synchronisation: what orbx_mappoint_last_timing returns
    bool ldsSet = false;
    ~orbx_mappoint_ops() { if (hostOut) (void)hipHostFree(hostOut); }
};

extern "C" int orbx_mappoint_ops_create(int device, int max_points, int max_obs_total, orbx_mappoint_ops **out)
{
    if (!out || max_points < 1 || max_obs_total < 1) { orbx_set_error("bad map point ops arguments"); return ORBX_ERR_ARG; }
    *out = nullptr;
    orbx_mappoint_ops *h = new orbx_mappoint_ops();
    h->maxPoints = max_points; h->maxObs = max_obs_total;
    int rc;
    if ((rc = h->open(device)) || (rc = h->timer.create())) { orbx_destroy_handle(h); return rc; }
    if (hipHostMalloc((void **)&h->hostOut, (size_t)max_points * 28, hipHostMallocDefault) != hipSuccess) {
        orbx_set_error("map point ops: pinned memory allocation failed");
        orbx_destroy_handle(h);
        return ORBX_ERR_HIP;
    }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_mappoint_ops_destroy(orbx_mappoint_ops *h) { orbx_destroy_handle(h); }

extern "C" int orbx_mappoint_refresh(orbx_mappoint_ops *h, const orbx_mappoint_batch *b, const orbx_mappoint_result *r)
{
    if (!h || !b) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    const int M = b->num_points, T = b->num_obs;
    if (M < 0 || T < 0) { orbx_set_error("negative batch size"); return ORBX_ERR_ARG; }
    if (M > h->maxPoints || T > h->maxObs) { orbx_set_error("batch (%d points, %d observations) exceeds the handle (%d, %d)", M, T, h->maxPoints, h->maxObs); return ORBX_ERR_ARG; }
    h->kernelMs = 0.0f; h->timer.launches = 0;
    if (M == 0) return ORBX_OK;
    if (!b->obs_offset || !b->pos || !b->ref_center || !b->ref_scale || !b->top_scale || (T > 0 && (!b->desc || !b->cam_center))) { orbx_set_error("NULL batch array"); return ORBX_ERR_ARG; }
    if (b->obs_offset[0] != 0) { orbx_set_error("obs_offset[0] must be 0"); return ORBX_ERR_ARG; }
    for (int p = 0; p < M; p++)
        if (b->obs_offset[p + 1] < b->obs_offset[p]) { orbx_set_error("obs_offset decreases at point %d", p); return ORBX_ERR_ARG; }
    if (b->obs_offset[M] != T) { orbx_set_error("obs_offset[num_points] = %d, num_obs = %d", b->obs_offset[M], T); return ORBX_ERR_ARG; }

    // classes by observation count; the order inside a point is never touched
    for (auto &l : h->lists) l.clear();
    for (int p = 0; p < M; p++) {
        const int n = b->obs_offset[p + 1] - b->obs_offset[p];
        if (n == 0) continue;
        if (n > MP_MAX_OBS) { orbx_set_error("point %d has %d observations, the limit is %d", p, n, MP_MAX_OBS); return ORBX_ERR_CAPACITY; }
        h->lists[n <= 64 ? 0 : n <= 128 ? 1 : n <= 256 ? 2 : 3].push_back(p);
    }

    ORBX_HIP_CHECK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    if (!h->ldsSet) {
        ORBX_HIP_CHECK(hipFuncSetAttribute((const void *)k_mp_block<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mp_block_lds(256)));
        ORBX_HIP_CHECK(hipFuncSetAttribute((const void *)k_mp_strided, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mp_strided_lds()));
        h->ldsSet = true;
    }
    OrbxHostStage &S = h->stage;
    const size_t m = (size_t)M, t = (size_t)T;
    OrbxInPlan &pl = S.plan();
    const auto sOff = pl.add(b->obs_offset, m + 1);
    const auto sDesc = pl.add(b->desc, t * 32);
    const auto sValid = pl.add(b->desc_valid, b->desc_valid ? t : 0);
    const auto sCam = pl.add(b->cam_center, t * 3);
    const auto sPos = pl.add(b->pos, m * 3), sRefc = pl.add(b->ref_center, m * 3);
    const auto sRsc = pl.add(b->ref_scale, m), sTsc = pl.add(b->top_scale, m);
    OrbxSlot<int32_t, ORBX_STAGE_IN> sList[4];
    for (int c = 0; c < 4; c++) sList[c] = pl.add((const int32_t *)h->lists[c].data(), h->lists[c].size());
    int rc;
    const OrbxStaged sg = S.begin(&rc);
    if (rc != ORBX_OK) return rc;
    const size_t outBytes = m * 28;
    if ((rc = h->out.ensure(outBytes)) != ORBX_OK) return rc;
    if (!h->lists[3].empty() && ((rc = h->unit.ensure(t * 3)) != ORBX_OK || (rc = h->comp.ensure(t)) != ORBX_OK)) return rc;

    MpDev D;
    D.off = sg.dev(sOff);
    D.desc = (const uint32_t *)sg.dev(sDesc);
    D.valid = b->desc_valid ? sg.dev(sValid) : nullptr;
    D.cam = sg.dev(sCam);
    D.pos = sg.dev(sPos); D.refc = sg.dev(sRefc);
    D.rsc = sg.dev(sRsc); D.tsc = sg.dev(sTsc);
    const int32_t *lists[4];
    for (int c = 0; c < 4; c++) lists[c] = sg.dev(sList[c]);
    D.bestObs = (int32_t *)h->out.p; D.bestMed = D.bestObs + m;
    D.normal = (float *)(D.bestMed + m); D.maxD = D.normal + 3 * m; D.minD = D.maxD + m;
    D.unit = h->unit.p; D.comp = h->comp.p;
    D.list = nullptr;

    if ((rc = S.flush(st)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipMemsetAsync(h->out.p, 0, outBytes, st));      // points without observations read 0: the same bits on every call
    if ((rc = h->timer.begin(st)) != ORBX_OK) return rc;
    for (int c = 0; c < 4; c++) {
        const unsigned cnt = (unsigned)h->lists[c].size();
        if (!cnt) continue;
        D.list = lists[c];
        if (c == 0) hipLaunchKernelGGL((k_mp_block<64>), dim3(cnt), dim3(64), mp_block_lds(64), st, D);
        else if (c == 1) hipLaunchKernelGGL((k_mp_block<128>), dim3(cnt), dim3(128), mp_block_lds(128), st, D);
        else if (c == 2) hipLaunchKernelGGL((k_mp_block<256>), dim3(cnt), dim3(256), mp_block_lds(256), st, D);
        else hipLaunchKernelGGL(k_mp_strided, dim3(cnt), dim3(256), mp_strided_lds(), st, D);
        ORBX_LAUNCH_COUNT(h->timer);
    }
    if ((rc = h->timer.end(st)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipMemcpyAsync(h->hostOut, h->out.p, outBytes, hipMemcpyDeviceToHost, st));
    ORBX_HIP_CHECK(hipStreamSynchronize(st));
    ORBX_HIP_CHECK(hipEventElapsedTime(&h->kernelMs, h->timer.ev[0], h->timer.ev[1]));
    if (r) {
        const uint8_t *o = h->hostOut;
        if (r->best_obs) memcpy(r->best_obs, o, m * 4);
        if (r->best_median) memcpy(r->best_median, o + m * 4, m * 4);
        if (r->normal) memcpy(r->normal, o + m * 8, m * 12);
        if (r->max_dist) memcpy(r->max_dist, o + m * 20, m * 4);
        if (r->min_dist) memcpy(r->min_dist, o + m * 24, m * 4);
        if (r->updated)
            for (int p = 0; p < M; p++) r->updated[p] = b->obs_offset[p + 1] > b->obs_offset[p] ? 1 : 0;
    }
    return ORBX_OK;
}

extern "C" int orbx_mappoint_last_timing(orbx_mappoint_ops *h, float *kernel_ms, int *launches)
{
    if (!h) { orbx_set_error("NULL map point ops handle"); return ORBX_ERR_ARG; }
    if (kernel_ms) *kernel_ms = h->kernelMs;
    if (launches) *launches = h->timer.launches;
    return ORBX_OK;
}
