// orbx_frame.hip -- the rest of the Frame constructor on gfx950.
//
//   orbx_frame_undistort     ==  Frame::UndistortKeyPoints    (reference src/Frame.cc:899-947)
//   orbx_frame_image_bounds  ==  Frame::ComputeImageBounds    (src/Frame.cc:950-1004)
//   orbx_frame_assign_grid   ==  Frame::AssignFeaturesToGrid  (src/Frame.cc:460-491, PosInGrid :868-878)
//   orbx_frame_finish_device ==  the first and the last fused, on an extractor's device-resident batch
//   orbx_frame_rgbd_device   ==  ... plus Frame::ComputeStereoFromRGBD (src/Frame.cc:1423-1461) and what the tracker derives from mvDepth
//                                (depth order, Frame::UnprojectStereo :1478-1491 in camera coordinates, close-point count), same launch
//
// cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) is OpenCV's fixed five-iteration
// inverse of the radial/tangential model, evaluated in double from float inputs and stored as
// float (cvUndistortPoints; un-vendored, see DESIGN.md section 3 "parity unpinned").  The
// operation order below is that function's; the library is built with -ffp-contract=off and
// double division is IEEE, so the device result equals the host result bit for bit.
//
// One workgroup per frame: undistort + cell id per keypoint, then the 64x48 grid as CSR
// (cell = x*48 + y as in mGrid[x][y]; indices of a cell ascending = push_back order):
// LDS histogram, scan, unordered scatter, per-cell insertion sort (cells hold < 1 feature on
// average).  A few hundred bytes per keypoint and ~200 FP64 flops: negligible next to the
// extraction it follows on the same stream.
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>

#include "orbx_handle.h"

namespace {

const int GC = ORBX_FRAME_GRID_COLS, GR = ORBX_FRAME_GRID_ROWS, NCELL = GC * GR;

struct CamDev {
    double fx, fy, cx, cy, k[8];
    int distorted;
};

__device__ __forceinline__ void undistort_point(const CamDev &c, float u, float v, float *ou, float *ov)
{
    const double ifx = 1. / c.fx, ify = 1. / c.fy;
    double x = u, y = v, x0, y0;
    x0 = x = (x - c.cx) * ifx;
    y0 = y = (y - c.cy) * ify;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((c.k[7] * r2 + c.k[6]) * r2 + c.k[5]) * r2) / (1 + ((c.k[4] * r2 + c.k[1]) * r2 + c.k[0]) * r2);
        const double deltaX = 2 * c.k[2] * x * y + c.k[3] * (r2 + 2 * x * x);
        const double deltaY = c.k[2] * (r2 + 2 * y * y) + 2 * c.k[3] * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    // P = K, R = I: RR = K
    const double xx = c.fx * x + 0.0 * y + c.cx;
    const double yy = 0.0 * x + c.fy * y + c.cy;
    const double ww = 1. / (0.0 * x + 0.0 * y + 1.0);
    *ou = (float)(xx * ww);
    *ov = (float)(yy * ww);
}

__global__ void k_undistort_corners(CamDev c, float cols, float rows, float *out)
{
    const int t = threadIdx.x;
    if (t >= 4) return;
    const float u = (t & 1) ? cols : 0.0f, v = (t & 2) ? rows : 0.0f;   // (0,0) (cols,0) (0,rows) (cols,rows), src/Frame.cc:961-968
    undistort_point(c, u, v, out + 2 * t, out + 2 * t + 1);
}

// The RGB-D step of k_frame_finish<true> (include/orbx.h: "The RGB-D Frame constructor").
struct RgbdDev {
    const uint8_t *depth;      // frame f at depth + f * framePitch, rows `stride` bytes apart; NULL: `values`
    const float *values;       // one frame: d of feature i, looked up by the host (latency form)
    size_t framePitch;
    int format, cols, rows, stride;
    float factor, bf, thDepth, cx, cy, invfx, invfy;
    float *outDepth, *outURight, *outXyz;      // [f*cap + i], xyz [(f*cap + i)*3]
    int32_t *outOrder, *outNValid, *outNClose; // [f*cap + r], [f], [f]
};

// mvDepth / mvuRight (src/Frame.cc:1451-1458) and UnprojectStereo's camera-frame point (:1488-1489) of one feature: z = the looked-up depth, NaN = none
__device__ __forceinline__ void rgbd_point(const RgbdDev &r, float z, float uUn, float vUn, float *depth, float *uRight, float *xyz)
{
    if (z > 0.0f) {
        *depth = z;
        *uRight = __fsub_rn(uUn, __fdiv_rn(r.bf, z));
        xyz[0] = __fmul_rn(__fmul_rn(__fsub_rn(uUn, r.cx), z), r.invfx);
        xyz[1] = __fmul_rn(__fmul_rn(__fsub_rn(vUn, r.cy), z), r.invfy);
        xyz[2] = z;
    } else {
        *depth = -1.0f; *uRight = -1.0f;
        xyz[0] = xyz[1] = xyz[2] = 0.0f;
    }
}

// imDepth.at<float>(v, u) with float -> int truncation (:1440-1444); NaN where the feature has no depth (d > 0 is false, also for a NaN pixel)
__device__ __forceinline__ float rgbd_lookup(const RgbdDev &r, int f, int i, float u, float v)
{
    float d = 0.0f;
    if (r.values) d = r.values[i];
    else {
        const int iu = (int)u, iv = (int)v;
        if (iu >= 0 && iu < r.cols && iv >= 0 && iv < r.rows) {
            const uint8_t *row = r.depth + (size_t)f * r.framePitch + (size_t)iv * (size_t)r.stride;
            d = r.format == ORBX_DEPTH_U16 ? __fmul_rn((float)((const uint16_t *)row)[iu], r.factor) : ((const float *)row)[iu];
        }
    }
    return d > 0.0f ? d : __builtin_nanf("");
}

#define FT 1024
// After the undistortion loop has left z / mvKeysUn.pt of the frame's n features in LDS: results out, then the depth order by a bitonic network
// over keys (z bits << 32 | i): positive floats order like their bit patterns, so ascending keys = ascending (z, i); features without depth
// carry the all-ones key and end up behind.  wide: 16-byte stores into buffers padded to multiples of four entries (pinned host memory).
__device__ __forceinline__ void rgbd_tail(const RgbdDev &r, int f, int n, int cap, int wide, const float *zk, const float *ux, const float *uy,
                                          unsigned long long *keys, int *sCnt)
{
    const int tid = threadIdx.x, lane = tid & 63;
    int N2 = 2;
    while (N2 < n) N2 <<= 1;
    if (tid < 2) sCnt[tid] = 0;
    for (int i = tid; i < N2; i += FT) {
        const float z = i < n ? zk[i] : -1.0f;
        keys[i] = z > 0.0f ? ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)i : ~0ull;
    }
    __syncthreads();
    float *od = r.outDepth + (size_t)f * cap, *ou = r.outURight + (size_t)f * cap, *ox = r.outXyz + (size_t)f * cap * 3;
    if (wide) {
        for (int i4 = tid * 4; i4 < n; i4 += FT * 4) {
            float dz[4], ur[4], p[12];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = i4 + j;
                rgbd_point(r, i < n ? zk[i] : -1.0f, i < n ? ux[i] : 0.0f, i < n ? uy[i] : 0.0f, &dz[j], &ur[j], &p[3 * j]);
            }
            *(float4 *)(od + i4) = make_float4(dz[0], dz[1], dz[2], dz[3]);
            *(float4 *)(ou + i4) = make_float4(ur[0], ur[1], ur[2], ur[3]);
            float4 *o4 = (float4 *)(ox + 3 * (size_t)i4);
            o4[0] = make_float4(p[0], p[1], p[2], p[3]);
            o4[1] = make_float4(p[4], p[5], p[6], p[7]);
            o4[2] = make_float4(p[8], p[9], p[10], p[11]);
        }
    } else {
        for (int i = tid; i < n; i += FT) {
            float dz, ur, p[3];
            rgbd_point(r, zk[i], ux[i], uy[i], &dz, &ur, p);
            od[i] = dz; ou[i] = ur;
            ox[3 * (size_t)i] = p[0]; ox[3 * (size_t)i + 1] = p[1]; ox[3 * (size_t)i + 2] = p[2];
        }
    }
    for (int k = 2; k <= N2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < N2 / 2; t += FT) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a > b) == ((lo & k) == 0)) { keys[lo] = b; keys[hi] = a; }
            }
            // a step with j <= 64 stays inside the 128 keys of one wave (pairs t = 64w .. 64w + 63): between two such steps the wave only has to
            // order its own LDS accesses; the workgroup meets when this step or the next one crosses waves
            const int jn = j > 1 ? j >> 1 : k;
            if (j > 64 || jn > 64) __syncthreads();
            else {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
    // n_valid, n_close (0 < z < thDepth): one ballot per wave
    for (int base = 0; base < N2; base += FT) {
        const int q = base + tid;
        const unsigned long long key = q < N2 ? keys[q] : ~0ull;
        const bool valid = key != ~0ull, close = valid && __uint_as_float((unsigned)(key >> 32)) < r.thDepth;
        const unsigned long long mv = __ballot(valid), mc = __ballot(close);
        if (lane == 0 && mv) { atomicAdd(&sCnt[0], __popcll(mv)); if (mc) atomicAdd(&sCnt[1], __popcll(mc)); }
    }
    int32_t *oo = r.outOrder + (size_t)f * cap;
    if (wide) {
        for (int q4 = tid * 4; q4 < n; q4 += FT * 4) {
            int v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) { const unsigned long long key = q4 + j < N2 ? keys[q4 + j] : ~0ull; v[j] = key != ~0ull ? (int)(unsigned)key : -1; }
            *(int4 *)(oo + q4) = make_int4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (int q = tid; q < n; q += FT) { const unsigned long long key = keys[q]; oo[q] = key != ~0ull ? (int)(unsigned)key : -1; }
    }
    __syncthreads();
    if (tid == 0) { r.outNValid[f] = sCnt[0]; r.outNClose[f] = sCnt[1]; }
}

// undistort: kp -> kpUn (else kp is already mvKeysUn and kpUn may be NULL); grid: build the CSR
// FT threads per frame (1024: the kernel is one workgroup's chain of dependent steps - histogram, scan, scatter, sort, write-out -, sixteen
// waves shorten every one of them; 24 -> 11 us for 2000 keypoints).  doneFlag != NULL (latency form, one frame): doneSeq is written there
// - pinned host memory - after the last result, the host polls it instead of synchronising the stream.
// RGBD: the RGB-D step rides along (r; more LDS behind `sorted`: z, mvKeysUn.pt.x / .y [cap rounded up to 4] and the sort keys [power of two >= cap]).
static_assert(NCELL % FT == 0, "cells per thread");
template <bool RGBD>
__global__ __launch_bounds__(FT) void k_frame_finish(CamDev c, orbx_frame_grid g, int undistort, int grid, const orbx_keypoint *__restrict__ kp,
                                                     const int32_t *__restrict__ counts, int cap, orbx_keypoint *__restrict__ kpUn,
                                                     int32_t *__restrict__ gridOff, int32_t *__restrict__ gridIdx, int *__restrict__ doneFlag, int doneSeq, int wide, RgbdDev r)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int sWave[FT / 64];
    __shared__ int sRgbd[2];
    int *cnt = (int *)smem;                                   // [NCELL] counts, then cursors
    int *off = cnt + NCELL;                                   // [NCELL + 1]
    unsigned short *cell = (unsigned short *)(off + NCELL + 4);       // [cap]  (off padded to a multiple of four entries: 16-byte rows for the write-out)
    int *sorted = (int *)(cell + ((cap + 7) & ~7));           // [cap rounded up to 4]
    const int cap4 = (cap + 3) & ~3;
    float *zk = (float *)(sorted + cap4), *ux = zk + cap4, *uy = ux + cap4;      // (RGBD only)
    unsigned long long *keys = (unsigned long long *)(uy + cap4);
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = counts ? min(counts[f], cap) : cap;
    const orbx_keypoint *in = kp + (size_t)f * cap;
    for (int t = tid; t < NCELL; t += FT) cnt[t] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += FT) {
        orbx_keypoint k = in[i];
        if (RGBD) zk[i] = rgbd_lookup(r, f, i, k.x, k.y);      // from the keypoint as extracted, not the undistorted one (:1436-1444)
        if (undistort) {
            if (c.distorted) undistort_point(c, k.x, k.y, &k.x, &k.y);   // else mvKeysUn = mvKeys, src/Frame.cc:901-905
            kpUn[(size_t)f * cap + i] = k;
        }
        if (RGBD) { ux[i] = k.x; uy[i] = k.y; }
        if (grid) {
            // PosInGrid, src/Frame.cc:868-878 (round() of a float: half away from zero)
            const int px = (int)roundf((k.x - g.min_x) * g.width_inv), py = (int)roundf((k.y - g.min_y) * g.height_inv);
            int ce = 0xffff;
            if (!(px < 0 || px >= GC || py < 0 || py >= GR)) { ce = px * GR + py; atomicAdd(&cnt[ce], 1); }
            cell[i] = (unsigned short)ce;
        }
    }
    if (!grid) {
        if (RGBD) { __syncthreads(); rgbd_tail(r, f, n, cap, wide, zk, ux, uy, keys, sRgbd); }
        if (doneFlag) {
            __threadfence_system();
            __syncthreads();
            if (tid == 0) __hip_atomic_store(doneFlag, doneSeq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    __syncthreads();
    // exclusive scan of the NCELL counts: 12 consecutive cells per thread
    const int PER = NCELL / FT;
    int local = 0;
    for (int t = 0; t < PER; t++) local += cnt[tid * PER + t];
    const int incl = wave_incl_scan_shfl(local, lane);
    if (lane == 63) sWave[wv] = incl;
    __syncthreads();
    int base = incl - local;
    for (int w = 0; w < wv; w++) base += sWave[w];
    for (int t = 0; t < PER; t++) { const int cval = cnt[tid * PER + t]; off[tid * PER + t] = base; base += cval; }
    if (tid == FT - 1) off[NCELL] = base;
    __syncthreads();
    for (int t = tid; t < NCELL; t += FT) cnt[t] = off[t];   // cursors
    __syncthreads();
    for (int i = tid; i < n; i += FT) {
        const int ce = cell[i];
        if (ce != 0xffff) sorted[atomicAdd(&cnt[ce], 1)] = i;
    }
    __syncthreads();
    for (int ce = tid; ce < NCELL; ce += FT) {
        const int b = off[ce], e = off[ce + 1];
        for (int a = b + 1; a < e; a++) {
            const int v = sorted[a];
            int q = a - 1;
            while (q >= b && sorted[q] > v) { sorted[q + 1] = sorted[q]; q--; }
            sorted[q + 1] = v;
        }
    }
    __syncthreads();
    int32_t *go = gridOff + (size_t)f * (NCELL + 1), *gi = gridIdx + (size_t)f * cap;
    // 16 bytes per lane: in the latency form the destination is pinned host memory, and four-byte stores across PCIe made the release below
    // wait 6-8 us for their completion (s_memrealtime: 7 of the kernel's 16 us); the rows and the buffers are padded to multiples of four entries
    // (wide: one frame, 16-byte aligned destinations padded to multiples of four entries - the latency forms; the batched form packs the frames)
    const int total = off[NCELL];
    if (wide) {
        for (int t = tid; t < (NCELL + 4) / 4; t += FT) ((uint4 *)go)[t] = ((const uint4 *)off)[t];
        for (int t = tid; t < (total + 3) / 4; t += FT) ((uint4 *)gi)[t] = ((const uint4 *)sorted)[t];
    } else {
        for (int t = tid; t <= NCELL; t += FT) go[t] = off[t];
        for (int t = tid; t < total; t += FT) gi[t] = sorted[t];
    }
    if (RGBD) rgbd_tail(r, f, n, cap, wide, zk, ux, uy, keys, sRgbd);
    if (doneFlag) {
        __threadfence_system();
        __syncthreads();
        if (tid == 0) __hip_atomic_store(doneFlag, doneSeq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

struct orbx_frame_ops : OrbxHandle {      // (the stream: host-array forms and the corner pass; the device form runs on the extractor's stream)
    CamDev cam;
    // results, double buffered in lockstep with the extractor's result buffers
    OrbxOwnedBuf<orbx_keypoint> kpUn[2];
    OrbxOwnedBuf<int32_t> gridOff[2], gridIdx[2];
    int cur = 0, lastBatch = 0, lastCap = 0;
    // capacity word of the extractor batch behind result buffer b (device form only): COPIED into this handle's own memory on the
    // extractor's stream when the frame is finished - the extractor may grow, reuse or free its result buffers before the download
    OrbxOwnedBuf<int> producerCopy;
    bool producerValid[2] = {false, false};
    uint8_t *hostIO = nullptr, *hostIODev = nullptr;   // pinned: inputs and outputs of the host-array forms, read / written by the kernel itself
    size_t hostIOBytes = 0;
    // orbx_frame_finish_begin .. _end: offsets of mvKeysUn / grid offsets / grid indices inside hostIO, the frame's keypoint count
    int pending = 0, pendingN = 0;
    bool pendingUn = false, pendingGrid = false;
    size_t pendUn = 0, pendOff = 0, pendIdx = 0, pendFlag = 0;
    int pendSeq = 0;
    OrbxOwnedBuf<orbx_keypoint> hostKp;
    OrbxOwnedBuf<int32_t> hostCount;
    OrbxOwnedBuf<float> corners;
    // the RGB-D step: results of the batch form (double buffered with the rest), the depth images of orbx_upload_depth, the latency form's
    // offsets inside hostIO and its pinned copy of the depth image (ORBX_RGBD_STAGE_IMAGE=1 only)
    OrbxOwnedBuf<float> rDepth[2], rURight[2], rXyz[2];
    OrbxOwnedBuf<int32_t> rOrder[2], rCounts[2];
    bool rgbdValid[2] = {false, false};
    OrbxOwnedBuf<uint8_t> depthDev;
    int depthDevFrames = 0;
    bool pendingRgbd = false;
    size_t pendDepth = 0, pendURight = 0, pendXyz = 0, pendOrder = 0, pendCounts = 0;
    uint8_t *depthStage = nullptr, *depthStageDev = nullptr;
    size_t depthStageBytes = 0;
    ~orbx_frame_ops()
    {
        if (depthStage) (void)hipHostFree(depthStage);
        if (hostIO) (void)hipHostFree(hostIO);
    }
};

static size_t finish_lds_bytes(int cap, bool rgbd)
{
    size_t lds = (size_t)(2 * NCELL + 4) * 4 + (size_t)((cap + 7) & ~7) * 2 + (size_t)((cap + 3) & ~3) * 4;
    if (rgbd) {
        size_t n2 = 2;
        while (n2 < (size_t)cap) n2 <<= 1;
        lds += (size_t)((cap + 3) & ~3) * 12 + n2 * 8;
    }
    return lds;
}

static int pixel_bytes(int format) { return format == ORBX_DEPTH_F32 ? 4 : format == ORBX_DEPTH_U16 ? 2 : 0; }

// the checks every RGB-D entry point makes on its depth descriptor against the size of the frames the extractor ran on
static int check_depth(const orbx_depth_desc *d, const orbx_rgbd_params *p, const OrbxLastBatchView &view)
{
    if (!d || !p || !d->data) { orbx_set_error("NULL depth image or parameters"); return ORBX_ERR_ARG; }
    const int px = pixel_bytes(d->format);
    if (!px) { orbx_set_error("unknown depth format %d (ORBX_DEPTH_F32 = 0, ORBX_DEPTH_U16 = 1)", d->format); return ORBX_ERR_ARG; }
    if (d->cols != view.geom->W || d->rows != view.geom->H) {
        orbx_set_error("the depth image is %d x %d, the extractor's frames are %d x %d", d->cols, d->rows, view.geom->W, view.geom->H);
        return ORBX_ERR_ARG;
    }
    if (d->stride_bytes < d->cols * px || d->stride_bytes % px) { orbx_set_error("bad depth stride %d", d->stride_bytes); return ORBX_ERR_ARG; }
    return ORBX_OK;
}

static RgbdDev rgbd_args(const orbx_frame_ops *h, const orbx_depth_desc *d, const orbx_rgbd_params *p)
{
    RgbdDev r;
    memset(&r, 0, sizeof(r));
    r.format = d->format; r.cols = d->cols; r.rows = d->rows; r.stride = d->stride_bytes;
    r.framePitch = (size_t)d->stride_bytes * (size_t)d->rows;
    r.factor = d->factor; r.bf = p->bf; r.thDepth = p->th_depth;
    // Frame's statics: cx, cy, invfx = 1.0f / fx, invfy = 1.0f / fy (src/Frame.cc:327-334), from the float mK the handle was made with
    r.cx = (float)h->cam.cx; r.cy = (float)h->cam.cy;
    r.invfx = 1.0f / (float)h->cam.fx; r.invfy = 1.0f / (float)h->cam.fy;
    return r;
}

extern "C" int orbx_frame_ops_create(int device, const orbx_camera *cam, orbx_frame_ops **out)
{
    if (!out || !cam) { orbx_set_error("bad frame-ops arguments"); return ORBX_ERR_ARG; }
    *out = nullptr;
    if (cam->ndist != 4 && cam->ndist != 5) { orbx_set_error("ndist must be 4 or 5 (k1 k2 p1 p2 [k3]), got %d", cam->ndist); return ORBX_ERR_ARG; }
    if (!(cam->fx != 0.0f) || !(cam->fy != 0.0f)) { orbx_set_error("focal length must be non-zero"); return ORBX_ERR_ARG; }
    orbx_frame_ops *h = new orbx_frame_ops();
    // (a plain stream: on a high-priority one - tried for the latency forms - the kernel shared a hardware queue with the combiner's second engines,
    // which are the other high-priority streams of the process: the stereo constructor went from 265 to 390 us once a second image size had been used)
    int rc = h->open(device);
    CamDev &c = h->cam;
    c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy;
    for (int i = 0; i < 8; i++) c.k[i] = i < cam->ndist ? (double)cam->dist[i] : 0.0;
    c.distorted = cam->dist[0] != 0.0f;   // the reference's test, src/Frame.cc:901, 953
    if (rc == ORBX_OK) rc = h->corners.ensure(8);
    if (rc == ORBX_OK) rc = h->hostCount.ensure(1);
    if (rc != ORBX_OK) { orbx_frame_ops_destroy(h); return rc; }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_frame_ops_destroy(orbx_frame_ops *h) { orbx_destroy_handle(h); }

// Frame::ComputeImageBounds, src/Frame.cc:950-1004
extern "C" int orbx_frame_image_bounds(orbx_frame_ops *h, int cols, int rows, float *bounds)
{
    if (!h || !bounds || cols < 1 || rows < 1) { orbx_set_error("bad argument"); return ORBX_ERR_ARG; }
    if (!h->cam.distorted) {
        bounds[0] = 0.0f; bounds[1] = (float)cols; bounds[2] = 0.0f; bounds[3] = (float)rows;
        return ORBX_OK;
    }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    float hc[8];
    hipLaunchKernelGGL(k_undistort_corners, dim3(1), dim3(64), 0, h->stream, h->cam, (float)cols, (float)rows, h->corners.p);
    ORBX_HIP_CHECK(hipMemcpyAsync(hc, h->corners.p, sizeof(hc), hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    bounds[0] = hc[0] < hc[4] ? hc[0] : hc[4];   // mnMinX = min(top-left.x, bottom-left.x)
    bounds[1] = hc[2] > hc[6] ? hc[2] : hc[6];   // mnMaxX = max(top-right.x, bottom-right.x)
    bounds[2] = hc[1] < hc[3] ? hc[1] : hc[3];   // mnMinY = min(top-left.y, top-right.y)
    bounds[3] = hc[5] > hc[7] ? hc[5] : hc[7];   // mnMaxY = max(bottom-left.y, bottom-right.y)
    return ORBX_OK;
}

static int launch_finish(orbx_frame_ops *h, hipStream_t stream, const orbx_frame_grid *grid, bool undistort, const orbx_keypoint *kp, const int32_t *counts,
                         int batch, int cap, RgbdDev *rgbd = nullptr)
{
    int rc;
    if (cap < 1 || cap > 0xfff0) { orbx_set_error("feature capacity %d out of range", cap); return ORBX_ERR_CAPACITY; }
    h->cur ^= 1;
    const int b = h->cur;
    if (undistort && (rc = h->kpUn[b].ensure((size_t)batch * cap))) return rc;
    if (grid && ((rc = h->gridOff[b].ensure((size_t)batch * (NCELL + 1))) || (rc = h->gridIdx[b].ensure((size_t)batch * cap)))) return rc;
    h->rgbdValid[b] = false;
    if (rgbd) {
        const size_t bc = (size_t)batch * cap;
        if ((rc = h->rDepth[b].ensure(bc)) || (rc = h->rURight[b].ensure(bc)) || (rc = h->rXyz[b].ensure(bc * 3)) || (rc = h->rOrder[b].ensure(bc)) ||
            (rc = h->rCounts[b].ensure((size_t)batch * 2))) return rc;
        rgbd->outDepth = h->rDepth[b].p; rgbd->outURight = h->rURight[b].p; rgbd->outXyz = h->rXyz[b].p; rgbd->outOrder = h->rOrder[b].p;
        rgbd->outNValid = h->rCounts[b].p; rgbd->outNClose = h->rCounts[b].p + batch;
    }
    const size_t lds = finish_lds_bytes(cap, rgbd != nullptr);
    if (lds > 160 * 1024) { orbx_set_error("feature capacity %d too large for the LDS tile", cap); return ORBX_ERR_CAPACITY; }
    orbx_frame_grid g = {0.0f, 0.0f, 0.0f, 0.0f};
    if (grid) g = *grid;
    if (rgbd) {
        if (lds > 48 * 1024) ORBX_HIP_CHECK(hipFuncSetAttribute((const void *)k_frame_finish<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_frame_finish<true>, dim3((unsigned)batch), dim3(FT), lds, stream, h->cam, g, undistort ? 1 : 0, grid ? 1 : 0, kp, counts, cap,
                           undistort ? h->kpUn[b].p : nullptr, grid ? h->gridOff[b].p : nullptr, grid ? h->gridIdx[b].p : nullptr, (int *)nullptr, 0, 0, *rgbd);
    } else {
        if (lds > 48 * 1024) ORBX_HIP_CHECK(hipFuncSetAttribute((const void *)k_frame_finish<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_frame_finish<false>, dim3((unsigned)batch), dim3(FT), lds, stream, h->cam, g, undistort ? 1 : 0, grid ? 1 : 0, kp, counts, cap,
                           undistort ? h->kpUn[b].p : nullptr, grid ? h->gridOff[b].p : nullptr, grid ? h->gridIdx[b].p : nullptr, (int *)nullptr, 0, 0, RgbdDev());
    }
    ORBX_LAUNCH_CHECK();
    h->lastBatch = batch; h->lastCap = cap;
    h->rgbdValid[b] = rgbd != nullptr;
    return ORBX_OK;
}

static int finish_device(orbx_frame_ops *h, orbx_extractor *ext, const orbx_frame_grid *grid, const orbx_depth_desc *depth, const orbx_rgbd_params *params, bool rgbd)
{
    if (!h || !ext || !grid) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    OrbxLastBatchView view;
    int rc = orbx_extractor_last_batch_view_internal(ext, &view);
    if (rc != ORBX_OK) return rc;
    RgbdDev r;
    if (rgbd) {
        if ((rc = check_depth(depth, params, view)) != ORBX_OK) return rc;
        if (depth->data == h->depthDev.p && h->depthDevFrames < view.batch) {
            orbx_set_error("%d depth images were uploaded, the extractor's last batch has %d frames", h->depthDevFrames, view.batch);
            return ORBX_ERR_ARG;
        }
        r = rgbd_args(h, depth, params);
        r.depth = (const uint8_t *)depth->data;
    }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    rc = launch_finish(h, orbx_extractor_stream_internal(ext), grid, true, view.kp, view.counts, view.batch, view.cap, rgbd ? &r : nullptr);
    // the capacity word of the batch these results come from (it lives in the extractor's result buffer): orbx_frame_download reports it
    h->producerValid[h->cur] = false;
    const int *word = rc == ORBX_OK ? orbx_extractor_status_word_internal(ext) : nullptr;
    if (word) {
        if ((rc = h->producerCopy.ensure(2)) != ORBX_OK) return rc;
        ORBX_HIP_CHECK(hipMemcpyAsync(h->producerCopy.p + h->cur, word, sizeof(int), hipMemcpyDeviceToDevice, orbx_extractor_stream_internal(ext)));
        h->producerValid[h->cur] = true;
    }
    return rc;
}

extern "C" int orbx_frame_finish_device(orbx_frame_ops *h, orbx_extractor *ext, const orbx_frame_grid *grid)
{
    return finish_device(h, ext, grid, nullptr, nullptr, false);
}

extern "C" int orbx_frame_rgbd_device(orbx_frame_ops *h, orbx_extractor *ext, const orbx_frame_grid *grid, const orbx_depth_desc *depth_dev,
                                      const orbx_rgbd_params *params)
{
    if (!depth_dev || !params) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    return finish_device(h, ext, grid, depth_dev, params, true);
}

extern "C" int orbx_frame_rgbd_results_device(orbx_frame_ops *h, const float **depth_dev, const float **u_right_dev, const int32_t **order_dev,
                                              const int32_t **n_valid_dev, const int32_t **n_close_dev, const float **xyz_cam_dev, int *capacity)
{
    if (!h) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    const int b = h->cur;
    if (!h->lastBatch || !h->rgbdValid[b]) { orbx_set_error("no RGB-D frame has been finished yet"); return ORBX_ERR_STATE; }
    if (depth_dev) *depth_dev = h->rDepth[b].p;
    if (u_right_dev) *u_right_dev = h->rURight[b].p;
    if (order_dev) *order_dev = h->rOrder[b].p;
    if (n_valid_dev) *n_valid_dev = h->rCounts[b].p;
    if (n_close_dev) *n_close_dev = h->rCounts[b].p + h->lastBatch;
    if (xyz_cam_dev) *xyz_cam_dev = h->rXyz[b].p;
    if (capacity) *capacity = h->lastCap;
    return ORBX_OK;
}

extern "C" int orbx_frame_rgbd_download(orbx_frame_ops *h, orbx_extractor *ext, int batch, float *depth, float *u_right, int32_t *order, int32_t *n_valid,
                                        int32_t *n_close, float *xyz_cam)
{
    if (!h) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    const int b = h->cur;
    if (batch < 1 || batch > h->lastBatch || !h->rgbdValid[b]) { orbx_set_error("RGB-D batch not available"); return ORBX_ERR_STATE; }
    int rc = orbx_frame_download(h, ext, batch, nullptr, nullptr, nullptr);      // (the wait and the producer's capacity word)
    if (rc != ORBX_OK) return rc;
    const size_t bc = (size_t)batch * h->lastCap;
    if (depth) ORBX_HIP_CHECK(hipMemcpy(depth, h->rDepth[b].p, bc * sizeof(float), hipMemcpyDeviceToHost));
    if (u_right) ORBX_HIP_CHECK(hipMemcpy(u_right, h->rURight[b].p, bc * sizeof(float), hipMemcpyDeviceToHost));
    if (order) ORBX_HIP_CHECK(hipMemcpy(order, h->rOrder[b].p, bc * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (n_valid) ORBX_HIP_CHECK(hipMemcpy(n_valid, h->rCounts[b].p, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (n_close) ORBX_HIP_CHECK(hipMemcpy(n_close, h->rCounts[b].p + h->lastBatch, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (xyz_cam) ORBX_HIP_CHECK(hipMemcpy(xyz_cam, h->rXyz[b].p, bc * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return ORBX_OK;
}

// B host depth images -> one device block in the batch form's layout (rows packed: stride = cols * pixel size), through the handle's own stream
extern "C" int orbx_upload_depth(orbx_frame_ops *h, const void *const *images, int batch, int format, int cols, int rows, int stride_bytes, float factor,
                                 orbx_depth_desc *depth_dev)
{
    if (!h || !images || !depth_dev) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    const int px = pixel_bytes(format);
    if (!px) { orbx_set_error("unknown depth format %d (ORBX_DEPTH_F32 = 0, ORBX_DEPTH_U16 = 1)", format); return ORBX_ERR_ARG; }
    if (batch < 1 || cols < 1 || rows < 1 || stride_bytes < cols * px || stride_bytes % px) { orbx_set_error("bad depth batch / size / stride"); return ORBX_ERR_ARG; }
    for (int f = 0; f < batch; f++) if (!images[f]) { orbx_set_error("depth image %d is NULL", f); return ORBX_ERR_ARG; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const size_t row = (size_t)cols * px, frame = row * rows;
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    int rc = h->depthDev.ensure(frame * batch);
    if (rc != ORBX_OK) return rc;
    for (int f = 0; f < batch; f++)
        ORBX_HIP_CHECK(hipMemcpy2DAsync(h->depthDev.p + frame * f, row, images[f], (size_t)stride_bytes, row, (size_t)rows, hipMemcpyHostToDevice, h->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->depthDevFrames = batch;
    depth_dev->data = h->depthDev.p; depth_dev->format = format; depth_dev->cols = cols; depth_dev->rows = rows; depth_dev->stride_bytes = (int)row;
    depth_dev->factor = factor;
    return ORBX_OK;
}

extern "C" int orbx_frame_results_device(orbx_frame_ops *h, const orbx_keypoint **kp_un_dev, const int32_t **grid_offsets_dev, const int32_t **grid_indices_dev,
                                         int *capacity)
{
    if (!h) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    if (!h->lastBatch) { orbx_set_error("no frame has been finished yet"); return ORBX_ERR_STATE; }
    if (kp_un_dev) *kp_un_dev = h->kpUn[h->cur].p;
    if (grid_offsets_dev) *grid_offsets_dev = h->gridOff[h->cur].p;
    if (grid_indices_dev) *grid_indices_dev = h->gridIdx[h->cur].p;
    if (capacity) *capacity = h->lastCap;
    return ORBX_OK;
}

extern "C" int orbx_frame_download(orbx_frame_ops *h, orbx_extractor *ext, int batch, orbx_keypoint *kp_un, int32_t *grid_offsets, int32_t *grid_indices)
{
    if (!h) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    if (batch < 1 || batch > h->lastBatch) { orbx_set_error("batch not available"); return ORBX_ERR_STATE; }
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    ORBX_HIP_CHECK(hipStreamSynchronize(ext ? orbx_extractor_stream_internal(ext) : h->stream));
    const int b = h->cur;
    if (ext && h->producerValid[b]) {
        int v = 0;
        ORBX_HIP_CHECK(hipMemcpy(&v, h->producerCopy.p + b, sizeof(int), hipMemcpyDeviceToHost));
        if (v) {
            orbx_set_error("the extractor batch these results were computed from overflowed a device capacity (bits 0x%x): results are not the reference's", v);
            return ORBX_ERR_CAPACITY;
        }
    }
    if (kp_un) ORBX_HIP_CHECK(hipMemcpy(kp_un, h->kpUn[b].p, (size_t)batch * h->lastCap * sizeof(orbx_keypoint), hipMemcpyDeviceToHost));
    if (grid_offsets) ORBX_HIP_CHECK(hipMemcpy(grid_offsets, h->gridOff[b].p, (size_t)batch * (NCELL + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (grid_indices) ORBX_HIP_CHECK(hipMemcpy(grid_indices, h->gridIdx[b].p, (size_t)batch * h->lastCap * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ORBX_OK;
}

// Host-array forms (UndistortKeyPoints / AssignFeaturesToGrid of ONE frame, called from the tracking thread: latency is what counts).
// Inputs and outputs live in ONE pinned buffer that the kernel reads and writes directly across PCIe (56 KB in, <= 80 KB out for 2000
// keypoints): memcpy in, one launch, one synchronisation, memcpy out - no copy engine, no device staging (the former form issued two uploads,
// a stream synchronisation and three blocking downloads: 0.07-0.10 ms per call).
static int host_form(orbx_frame_ops *h, const orbx_frame_grid *grid, bool undistort, const orbx_keypoint *keypoints, int n, orbx_keypoint *kp_un,
                     int32_t *grid_offsets, int32_t *grid_indices)
{
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    if (h->pending == 2) ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));      // a frame begun and never ended: its kernel may still be storing into the pinned buffer this call reuses
    h->pending = 0;      // (... and that frame is dropped)
    const int cap = n > 0 ? n : 1;
    if (cap > 0xfff0) { orbx_set_error("feature capacity %d out of range", cap); return ORBX_ERR_CAPACITY; }
    const size_t A = 256, szKp = ((size_t)cap * sizeof(orbx_keypoint) + A - 1) / A * A, szIdx = ((size_t)cap * 4 + A - 1) / A * A, szOff = ((size_t)(NCELL + 1) * 4 + A - 1) / A * A;
    const size_t oIn = 0, oCnt = oIn + szKp, oUn = oCnt + A, oOff = oUn + szKp, oIdx = oOff + szOff, total = oIdx + szIdx;
    if (total > h->hostIOBytes) {
        ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
        if (h->hostIO) (void)hipHostFree(h->hostIO);
        h->hostIO = nullptr; h->hostIOBytes = 0;
        ORBX_HIP_CHECK(hipHostMalloc((void **)&h->hostIO, total, hipHostMallocDefault));
        void *dp = nullptr;
        ORBX_HIP_CHECK(hipHostGetDevicePointer(&dp, h->hostIO, 0));
        h->hostIODev = (uint8_t *)dp;
        h->hostIOBytes = total;
    }
    if (n > 0) memcpy(h->hostIO + oIn, keypoints, (size_t)n * sizeof(orbx_keypoint));
    *(int32_t *)(h->hostIO + oCnt) = n;
    const size_t lds = finish_lds_bytes(cap, false);
    if (lds > 160 * 1024) { orbx_set_error("feature capacity %d too large for the LDS tile", cap); return ORBX_ERR_CAPACITY; }
    if (lds > 48 * 1024) ORBX_HIP_CHECK(hipFuncSetAttribute((const void *)k_frame_finish<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    orbx_frame_grid g = {0.0f, 0.0f, 0.0f, 0.0f};
    if (grid) g = *grid;
    uint8_t *d = h->hostIODev;
    hipLaunchKernelGGL(k_frame_finish<false>, dim3(1), dim3(FT), lds, h->stream, h->cam, g, undistort ? 1 : 0, grid ? 1 : 0, (const orbx_keypoint *)(d + oIn), (const int32_t *)(d + oCnt), cap,
                       undistort ? (orbx_keypoint *)(d + oUn) : nullptr, grid ? (int32_t *)(d + oOff) : nullptr, grid ? (int32_t *)(d + oIdx) : nullptr, (int *)nullptr, 0, 1, RgbdDev());
    ORBX_LAUNCH_CHECK();
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    if (undistort && n > 0 && kp_un) memcpy(kp_un, h->hostIO + oUn, (size_t)n * sizeof(orbx_keypoint));
    if (grid && grid_offsets) memcpy(grid_offsets, h->hostIO + oOff, (size_t)(NCELL + 1) * 4);
    if (grid && n > 0 && grid_indices) memcpy(grid_indices, h->hostIO + oIdx, (size_t)n * 4);
    return ORBX_OK;
}

// The latency form behind the Frame constructors (include/orbx.h): input = the extractor's device-resident keypoints of its last single-frame
// call, output = this handle's pinned memory, written by the kernel itself; nothing is waited for here.
// depth != NULL: the RGB-D constructor (orbx_frame_rgbd_begin) - the same launch with the RGB-D step behind the grid.
static int finish_begin(orbx_frame_ops *h, orbx_extractor *ext, const orbx_frame_grid *grid, const orbx_depth_desc *depth, const orbx_rgbd_params *params)
{
    if (!h || !ext) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (h->pending == 2) {      // a frame begun and never ended: its kernel may still be storing into the pinned buffer (and its completion word) this call reuses
        ORBX_HIP_CHECK(hipSetDevice(h->device));
        ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    h->pending = 0;
    int st = 0;
    if (!orbx_extractor_host_complete_internal(ext, &st)) { orbx_set_error("the extractor's last call was not a completed single-frame call"); return ORBX_ERR_STATE; }
    if (st) { orbx_set_error("the extractor call these features come from overflowed a device capacity (bits 0x%x): results are not the reference's", st); return ORBX_ERR_CAPACITY; }
    OrbxLastBatchView view;
    int rc = orbx_extractor_last_batch_view_internal(ext, &view);
    if (rc != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipSetDevice(h->device));
    const int cap = view.cap, n = orbx_extractor_host_count_internal(ext);
    if (cap < 1 || cap > 0xfff0 || n > cap) { orbx_set_error("feature capacity %d out of range", cap); return ORBX_ERR_CAPACITY; }
    const bool undist = h->cam.distorted != 0;
    if (depth && (rc = check_depth(depth, params, view)) != ORBX_OK) return rc;
    h->pendingRgbd = false;
    if (!undist && !grid && !depth) { h->pending = 1; h->pendingN = n; h->pendingUn = h->pendingGrid = false; return ORBX_OK; }      // (nothing to compute)
    const size_t A = 256, szKp = ((size_t)cap * sizeof(orbx_keypoint) + A - 1) / A * A, szIdx = ((size_t)cap * 4 + A - 1) / A * A, szOff = ((size_t)(NCELL + 1) * 4 + A - 1) / A * A;
    // (+ the host-array forms' input area: one buffer serves both; + the RGB-D results and the looked-up depth values, cap rounded up to 4 entries each)
    const size_t oUn = 0, oOff = oUn + szKp, oIdx = oOff + szOff, oFlag = oIdx + szIdx, oDepth = oFlag + A + szKp + A, oUR = oDepth + szIdx, oXyz = oUR + szIdx,
                 oOrder = oXyz + 3 * szIdx, oCnt = oOrder + szIdx, oVal = oCnt + A, total = depth ? oVal + szIdx : oDepth;
    if (total > h->hostIOBytes) {
        ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
        if (h->hostIO) (void)hipHostFree(h->hostIO);
        h->hostIO = nullptr; h->hostIOBytes = 0;
        ORBX_HIP_CHECK(hipHostMalloc((void **)&h->hostIO, total, hipHostMallocDefault));
        void *dp = nullptr;
        ORBX_HIP_CHECK(hipHostGetDevicePointer(&dp, h->hostIO, 0));
        h->hostIODev = (uint8_t *)dp;
        h->hostIOBytes = total;
    }
    const size_t lds = finish_lds_bytes(cap, depth != nullptr);
    if (lds > 160 * 1024) { orbx_set_error("feature capacity %d too large for the LDS tile", cap); return ORBX_ERR_CAPACITY; }
    orbx_frame_grid g = {0.0f, 0.0f, 0.0f, 0.0f};
    if (grid) g = *grid;
    uint8_t *d = h->hostIODev;
    RgbdDev r;
    if (depth) {
        r = rgbd_args(h, depth, params);
        r.outDepth = (float *)(d + oDepth); r.outURight = (float *)(d + oUR); r.outXyz = (float *)(d + oXyz); r.outOrder = (int32_t *)(d + oOrder);
        r.outNValid = (int32_t *)(d + oCnt); r.outNClose = r.outNValid + 1;
        const char *env = getenv("ORBX_RGBD_STAGE_IMAGE");
        if (env && env[0] == '1') {
            // the whole image into pinned memory, gathered by the kernel across PCIe (the measured alternative, profiles/rgbd_latency.txt)
            const size_t bytes = (size_t)depth->stride_bytes * (depth->rows - 1) + (size_t)depth->cols * pixel_bytes(depth->format);      // (the last row ends with its last pixel)
            if (bytes > h->depthStageBytes) {
                ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
                if (h->depthStage) (void)hipHostFree(h->depthStage);
                h->depthStage = nullptr; h->depthStageBytes = 0;
                ORBX_HIP_CHECK(hipHostMalloc((void **)&h->depthStage, bytes, hipHostMallocDefault));
                void *dp = nullptr;
                ORBX_HIP_CHECK(hipHostGetDevicePointer(&dp, h->depthStage, 0));
                h->depthStageDev = (uint8_t *)dp;
                h->depthStageBytes = bytes;
            }
            memcpy(h->depthStage, depth->data, bytes);
            r.depth = h->depthStageDev;
        } else {
            // imDepth.at<float>(v, u) for the n keypoints (src/Frame.cc:1440-1444), read where the extractor's call left them in pinned memory
            const orbx_keypoint *kps = orbx_extractor_host_keypoints_internal(ext);
            float *val = (float *)(h->hostIO + oVal);
            const uint8_t *img = (const uint8_t *)depth->data;
            for (int i = 0; i < n; i++) {
                const int iu = (int)kps[i].x, iv = (int)kps[i].y;
                float dv = 0.0f;
                if (iu >= 0 && iu < depth->cols && iv >= 0 && iv < depth->rows) {
                    const uint8_t *row = img + (size_t)iv * (size_t)depth->stride_bytes;
                    if (depth->format == ORBX_DEPTH_U16) dv = (float)((const uint16_t *)row)[iu] * depth->factor;
                    else memcpy(&dv, row + (size_t)iu * 4, 4);
                }
                val[i] = dv;
            }
            r.values = (const float *)(d + oVal);
        }
    }
    const int seq = ++h->pendSeq;
    *(volatile int *)(h->hostIO + oFlag) = 0;
    if (depth) {
        if (lds > 48 * 1024) ORBX_HIP_CHECK(hipFuncSetAttribute((const void *)k_frame_finish<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_frame_finish<true>, dim3(1), dim3(FT), lds, h->stream, h->cam, g, undist ? 1 : 0, grid ? 1 : 0, view.kp, view.counts, cap,
                           undist ? (orbx_keypoint *)(d + oUn) : nullptr, grid ? (int32_t *)(d + oOff) : nullptr, grid ? (int32_t *)(d + oIdx) : nullptr, (int *)(d + oFlag), seq, 1, r);
    } else {
        if (lds > 48 * 1024) ORBX_HIP_CHECK(hipFuncSetAttribute((const void *)k_frame_finish<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_frame_finish<false>, dim3(1), dim3(FT), lds, h->stream, h->cam, g, undist ? 1 : 0, grid ? 1 : 0, view.kp, view.counts, cap,
                           undist ? (orbx_keypoint *)(d + oUn) : nullptr, grid ? (int32_t *)(d + oOff) : nullptr, grid ? (int32_t *)(d + oIdx) : nullptr, (int *)(d + oFlag), seq, 1, RgbdDev());
    }
    ORBX_LAUNCH_CHECK();
    h->pending = 2; h->pendingN = n; h->pendingUn = undist; h->pendingGrid = grid != nullptr;
    h->pendUn = oUn; h->pendOff = oOff; h->pendIdx = oIdx; h->pendFlag = oFlag;
    h->pendingRgbd = depth != nullptr;
    h->pendDepth = oDepth; h->pendURight = oUR; h->pendXyz = oXyz; h->pendOrder = oOrder; h->pendCounts = oCnt;
    return ORBX_OK;
}

extern "C" int orbx_frame_finish_begin(orbx_frame_ops *h, orbx_extractor *ext, const orbx_frame_grid *grid)
{
    return finish_begin(h, ext, grid, nullptr, nullptr);
}

extern "C" int orbx_frame_rgbd_begin(orbx_frame_ops *h, orbx_extractor *ext, const orbx_frame_grid *grid, const orbx_depth_desc *depth_host,
                                     const orbx_rgbd_params *params)
{
    if (!depth_host || !params) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    return finish_begin(h, ext, grid, depth_host, params);
}

extern "C" int orbx_frame_finish_end(orbx_frame_ops *h, const orbx_keypoint **kp_un, const int32_t **grid_offsets, const int32_t **grid_indices, int *n)
{
    if (!h) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    const int pending = h->pending;
    h->pending = 0;
    if (!pending) { orbx_set_error("no frame has been begun"); return ORBX_ERR_STATE; }
    if (pending == 2) {      // the kernel's completion word in pinned memory (written behind its last result); the stream only if that takes implausibly long
        const volatile int *flag = (const volatile int *)(h->hostIO + h->pendFlag);
        const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        bool arrived = false;
        for (int spin = 0; !(arrived = *flag == h->pendSeq); spin++) {
            __builtin_ia32_pause();
            if ((spin & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (!arrived) {
            ORBX_HIP_CHECK(hipSetDevice(h->device));
            ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
    }
    if (kp_un) *kp_un = h->pendingUn ? (const orbx_keypoint *)(h->hostIO + h->pendUn) : nullptr;
    if (grid_offsets) *grid_offsets = h->pendingGrid ? (const int32_t *)(h->hostIO + h->pendOff) : nullptr;
    if (grid_indices) *grid_indices = h->pendingGrid ? (const int32_t *)(h->hostIO + h->pendIdx) : nullptr;
    if (n) *n = h->pendingN;
    return ORBX_OK;
}

extern "C" int orbx_frame_rgbd_end(orbx_frame_ops *h, const orbx_keypoint **kp_un, const int32_t **grid_offsets, const int32_t **grid_indices, int *n,
                                   orbx_rgbd_frame *rgbd)
{
    if (!h || !rgbd) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    if (h->pending && !h->pendingRgbd) { orbx_set_error("the frame that was begun is not an RGB-D frame (orbx_frame_finish_begin): end it with orbx_frame_finish_end"); return ORBX_ERR_STATE; }
    const int rc = orbx_frame_finish_end(h, kp_un, grid_offsets, grid_indices, n);
    if (rc != ORBX_OK) return rc;
    h->pendingRgbd = false;
    rgbd->depth = (const float *)(h->hostIO + h->pendDepth); rgbd->u_right = (const float *)(h->hostIO + h->pendURight);
    rgbd->order = (const int32_t *)(h->hostIO + h->pendOrder); rgbd->xyz_cam = (const float *)(h->hostIO + h->pendXyz);
    const int32_t *cnt = (const int32_t *)(h->hostIO + h->pendCounts);
    rgbd->n_valid = cnt[0]; rgbd->n_close = cnt[1];
    return ORBX_OK;
}

extern "C" int orbx_frame_undistort(orbx_frame_ops *h, const orbx_keypoint *keypoints, int n, orbx_keypoint *kp_un)
{
    if (!h || n < 0 || (n > 0 && (!keypoints || !kp_un))) { orbx_set_error("bad argument"); return ORBX_ERR_ARG; }
    if (n == 0) return ORBX_OK;
    return host_form(h, nullptr, true, keypoints, n, kp_un, nullptr, nullptr);
}

extern "C" int orbx_frame_assign_grid(orbx_frame_ops *h, const orbx_frame_grid *grid, const orbx_keypoint *kp_un, int n, int32_t *grid_offsets,
                                      int32_t *grid_indices)
{
    if (!h || !grid || !grid_offsets || n < 0 || (n > 0 && (!kp_un || !grid_indices))) { orbx_set_error("bad argument"); return ORBX_ERR_ARG; }
    return host_form(h, grid, false, kp_un, n, nullptr, grid_offsets, grid_indices);
}
