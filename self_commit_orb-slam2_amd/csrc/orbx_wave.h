// orbx_wave.h -- cross-lane (wave64) and workgroup primitives of liborbx's kernels (gfx950).  Included by orbx_internal.h; a new module takes its
// sums, minima, scans and ranks from here instead of writing the butterfly out again.
//
// Floating-point sums come in TWO orders of additions, and the two round differently - they are never merged, and a call site never changes family:
//   wave_sum_f64 / block_sum_f64   DPP order: pairs, quads, half rows, rows, then (r0 + r1) + (r2 + r3) over the four rows (and over the four waves).
//                                  Pinned bit for bit by tests/test_pose_optimization.py (k_pose_opt) and tests/optsim3_ref.py (k_optsim3).
//   wave_sum_xor on a double       xor-butterfly order: lane ^ 32, 16, ..., 1 (from WIDTH / 2 down inside groups of WIDTH lanes).
//                                  The local bundle adjustment's sums; pinned by the batched-equals-single check of tests/test_lba_batch.py.
// Integer sums, minima, maxima and scans have one value whatever the order; their forms differ in cost only.
//
// A helper is optimised on its own before it is inlined, so replacing a written-out loop by a call can reorder a kernel's instructions.  The few call
// sites where it did keep their loop, with a comment naming the kernel.  The arg-max over (score, index) pairs has no home here: the initializer's
// (wave_first_argmax, sentinel score -1) and the keyframe database's (any score, empty lanes marked by INT_MAX) follow different tie rules.
#ifndef ORBX_WAVE_H
#define ORBX_WAVE_H

#ifdef __HIPCC__

// ---- lane moves of a double ---------------------------------------------------------------------------------------------------------------
// a lane's value moved by a DPP control (two full-rate v_mov_b32_dpp, ~8 cycles of latency; __shfl_xor of a double is two ds_bpermute_b32 through the LDS
// crossbar, ~130 cycles per step of a dependent chain)
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u & 0xffffffffu), CTRL, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// value of lane `src` (compile-time constant after unrolling) as a scalar broadcast: two v_readlane_b32 instead of two ds_bpermute_b32
__device__ __forceinline__ double readlane_f64(double v, int src)
{
    const unsigned long long u = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(u & 0xffffffffu), src), hi = (unsigned)__builtin_amdgcn_readlane((int)(u >> 32), src);
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

// ---- sums ---------------------------------------------------------------------------------------------------------------------------------
// DPP order.  The wave's sum in every lane: pairs, quads, half rows, rows (DPP butterflies), then the four rows' sums as scalar broadcasts
__device__ __forceinline__ double wave_sum_f64(double v)
{
    v += dpp_f64<0xb1>(v);      // quad_perm [1,0,3,2]
    v += dpp_f64<0x4e>(v);      // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);     // row_half_mirror
    v += dpp_f64<0x140>(v);     // row_mirror: every lane holds its row's sum
    const double r0 = readlane_f64(v, 0), r1 = readlane_f64(v, 16), r2 = readlane_f64(v, 32), r3 = readlane_f64(v, 48);
    return (r0 + r1) + (r2 + r3);
}
// DPP order, 256 threads.  v[0..N) per thread -> v[0..N) of EVERY thread = the sums over the workgroup (N is a template argument: v stays in registers).
// One barrier: the four waves' sums meet in red[wave][k] (rows of NRED) and every thread adds them itself, in the same order.  The caller keeps a barrier
// between two calls (red is reused).
template <int N, int NRED> __device__ inline void block_sum_f64(double (&v)[N], double (*red)[NRED], int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const double x = wave_sum_f64(v[k]);
        if (lane == 0) red[wave][k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}
// xor-butterfly order: the sum over each group of WIDTH lanes in every lane of the group (doubles: see the two orders above)
template <int WIDTH = 64, typename T> __device__ __forceinline__ T wave_sum_xor(T v)
{
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) {
        if constexpr (WIDTH == 64) v += __shfl_xor(v, o);
        else v += __shfl_xor(v, o, WIDTH);
    }
    return v;
}
// integer sum over the 64 lanes with data-parallel-primitive adds (one VALU instruction per step, no LDS crossbar): quad, half row, row, then the
// two row broadcasts of gfx9; the total lands in lane 63 and is returned as a scalar
__device__ __forceinline__ int wave_sum_dpp(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xb1, 0xf, 0xf, true);      // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4e, 0xf, 0xf, true);      // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);     // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);     // row_mirror: every lane holds its row's sum
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);     // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, true);     // row_bcast:31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}

// integer sums over the two halves of the wave (lanes 0 - 31, lanes 32 - 63) at once: the reduction above stopped before its last step; the totals
// land in lanes 31 and 63 (every other lane holds a partial sum)
__device__ __forceinline__ int halfwave_sum_dpp(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xb1, 0xf, 0xf, true);      // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4e, 0xf, 0xf, true);      // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);     // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);     // row_mirror: every lane holds its row's sum
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);     // row_bcast:15 into rows 1 and 3
    return v;
}

// ---- minimum / maximum of 32- and 64-bit keys, in every lane ------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o); v = u < v ? u : v; }
    return v;
}
template <typename T> __device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}

// ---- inclusive scans over the 64 lanes ----------------------------------------------------------------------------------------------------
// shuffle-up form (six dependent LDS-crossbar round trips): the one a later performance change may retire in favour of wave_incl_scan_dpp
template <typename T> __device__ __forceinline__ T wave_incl_scan_shfl(T v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        T u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}
// inclusive prefix sum over the 64 lanes with data-parallel-primitive adds: four shifts inside the rows of 16, then the two row broadcasts of gfx9
// (six VALU instructions; __shfl_up is six dependent LDS-crossbar round trips)
__device__ __forceinline__ int wave_incl_scan_dpp(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);     // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);     // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);     // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);     // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);     // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);     // row_bcast:31 into rows 2 and 3
    return v;
}

// ---- workgroup helpers --------------------------------------------------------------------------------------------------------------------
// position of a thread with `pred` among the workgroup's NT threads, behind *base; *base advances by the workgroup's count (uniform)
template <int NT> __device__ __forceinline__ int block_ballot_rank(bool pred, int *base, int *sh /* NT / 64 */)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long mask = __ballot(pred);
    const int pre = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) sh[wave] = __popcll(mask);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < NT / 64; w++) {
        const int c = sh[w];
        if (w < wave) off += c;
        tot += c;
    }
    __syncthreads();
    const int r = *base + off + pre;
    *base += tot;
    return r;
}

// exclusive scan of arr[0..n) in place (LDS); returns the total.  All BT threads of the workgroup call.
template <int BT = 256, typename T> __device__ T block_exscan(T *arr, int n, T *wsum /* >= BT / 64 entries */)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (n + BT - 1) / BT;
    const int b = tid * per;
    T s = 0;
    for (int k = 0; k < per; k++) if (b + k < n) s += arr[b + k];
    T inc = wave_incl_scan_shfl(s, lane);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    T off = 0, total = 0;
#pragma unroll
    for (int i = 0; i < BT / 64; i++) { const T v = wsum[i]; off += i < w ? v : (T)0; total += v; }
    T run = off + inc - s;
    for (int k = 0; k < per; k++)
        if (b + k < n) { T v = arr[b + k]; arr[b + k] = run; run += v; }
    __syncthreads();
    return total;
}

// Two exclusive scans at once over entries that the calling thread FILLS itself: thread t owns the contiguous entries
// [t*per, (t+1)*per), fill(i, a, b) produces entry i of both arrays, so no barrier is needed between filling and scanning.
template <int BT = 256, typename F> __device__ __forceinline__ void block_fill_exscan2(int *A, int *B, int n, int *wsA, int *wsB, int &totA, int &totB, F fill)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (n + BT - 1) / BT;
    const int b = tid * per;
    int sa = 0, sb = 0;
    for (int k = 0; k < per; k++)
        if (b + k < n) { int a, c; fill(b + k, a, c); A[b + k] = a; B[b + k] = c; sa += a; sb += c; }
    const int incA = wave_incl_scan_shfl(sa, lane), incB = wave_incl_scan_shfl(sb, lane);
    if (lane == 63) { wsA[w] = incA; wsB[w] = incB; }
    __syncthreads();
    int offA = 0, offB = 0;
    totA = 0; totB = 0;
#pragma unroll
    for (int i = 0; i < BT / 64; i++) { const int va = wsA[i], vb = wsB[i]; offA += i < w ? va : 0; offB += i < w ? vb : 0; totA += va; totB += vb; }
    int runA = offA + incA - sa, runB = offB + incB - sb;
    for (int k = 0; k < per; k++)
        if (b + k < n) { const int a = A[b + k], c = B[b + k]; A[b + k] = runA; B[b + k] = runB; runA += a; runB += c; }
    __syncthreads();
}

#endif      // __HIPCC__
#endif
