// orbx_image.hip -- the image front end (gfx950 only): colour to grey and stereo rectification, in front of the extractor.
//
// Reference: Tracking::GrabImageMonocular / GrabImageStereo / GrabImageRGBD (src/Tracking.cc:250-278, 311-326, 369-384: cvtColor to grey by mbRGB) and
// Examples/Stereo/stereo_euroc.cc:124-134, 181-188 (cv::initUndistortRectifyMap once, cv::remap(INTER_LINEAR) on both images of every pair).
//
// PARITY WITH OpenCV IS UNPINNED (as oracle/prims.h says of resize): cvtColor's weights and SIMD path differ between OpenCV versions, initUndistortRectifyMap
// inverts Pnew * R by LU, and remap corrects the sum of its four 16-bit weights on one of them.  What is pinned is the arithmetic stated in include/orbx.h and
// restated in tests/imgprep_ref.py; the device equals it byte for byte, and the restatement shows that the weight fix-up changes no output.
//
// Output: frame f at out + f * pitch, stride = round_up(round_up(w, 4) + 12, 16), pitch = stride * h, every pad byte 0: the layout k_pyr_band reads with
// aligned windows everywhere.  The kernels store whole rows, one dword per lane.
//   k_maps_fixed   once per map pair: float maps -> ix | iy << 16 (one dword) and fx | fy << 5 (16 bits): 6 bytes per pixel, shared by all frames of a batch
//   k_gray         a lane = 4 output pixels.  Sources whose pointer, stride and pitch are multiples of 4: three dwords (3 channels) or one dwordx4 (4 channels)
//                  per lane, bytes cut out with v_bfe_u32, weighted with v_mad_u32_u24; every other source, and the last group of a row whose width is no
//                  multiple of 4, takes byte loads.  One channel: the copy into the padded layout.
//   k_remap        a lane = 4 consecutive output pixels: one dwordx4 + one dwordx2 of map words.  Rectification maps are smooth: when the lane's four pixels
//                  read two or three consecutive source rows within 8 columns, as many wide loads at the byte address fetch all 16 taps; otherwise 4 x 4 byte loads
//                  (neighbouring lanes hit the same lines, no LDS).  The border test is made once per lane for its 4 pixels; only a lane that fails it
//                  tests every tap.  Colour sources: the grey value is computed per source pixel in the same kernel, so grey + remap is ONE launch and
//                  no grey frame is staged.
// Block mapping: the same XCD-aware bijection as the pyramid kernels (orbx_kernels.hip: XCD_REMAP_XY), so a frame's rows are written by the XCD whose L2
// the extractor's level-0 reads then find them in (a speed assumption only).
#include <algorithm>
#include <cmath>
#include <vector>

#include "orbx_internal.h"

#define IP_MAX_DIM 16384
#define IP_ROWS 4          // rows per wave of a block: a block is 4 waves = 64 dword columns x 16 rows

namespace {

// (orbx_kernels.hip: xcd_remap)  linear block b runs on XCD b % 8; XCD x gets the contiguous range [x q + min(x, r), ...) of the (frame, item) space
__device__ __forceinline__ void ip_xcd_remap(int gx, int total, int linear, int &bx, int &by)
{
    const int xcd = linear & 7, slot = linear >> 3, q = total >> 3, r = total & 7;
    const int t = xcd * q + min(xcd, r) + slot;
    by = t / gx;
    bx = t - by * gx;
}
#define IP_XCD_REMAP_XY(BX, BY) int BX, BY; ip_xcd_remap((int)gridDim.x, (int)(gridDim.x * gridDim.y), (int)(blockIdx.y * gridDim.x + blockIdx.x), BX, BY)

struct __attribute__((packed, aligned(4))) IpU3 { uint32_t a, b, c; };
struct __attribute__((packed, aligned(4))) IpU4 { uint32_t a, b, c, d; };

struct IpGray { uint32_t c0, c1, c2, round, shift; };      // weights of byte 0, 1, 2 of a pixel (the host swaps them for BGR), 1 << (shift - 1), shift

struct IpFrames {
    const uint8_t *src; int srcStride; size_t srcPitch;
    uint8_t *dst; int dstStride; size_t dstPitch;           // dstStride is a multiple of 16
    int w, h, colBlocks;                                    // colBlocks = ceil(dstStride / 4 / 64)
};

__device__ __forceinline__ uint32_t ip_gray(uint32_t b0, uint32_t b1, uint32_t b2, const IpGray &g)
{
    return (__umul24(b0, g.c0) + __umul24(b1, g.c1) + __umul24(b2, g.c2) + g.round) >> g.shift;      // v_mad_u32_u24 x 3: at most 255 * 65536 + 32768
}
#define IP_BYTE(W, J) __builtin_amdgcn_ubfe((W), 8 * (J), 8)

// the grey value of one source pixel by byte loads
template <int C> __device__ __forceinline__ uint32_t ip_tap(const uint8_t *__restrict__ p, const IpGray &g)
{
    if (C == 1) return p[0];
    return ip_gray(p[0], p[1], p[2], g);
}

// pixels x .. x + 3 of one row as a dword; pixels at and behind w are 0
template <int C, bool ALIGNED> __device__ __forceinline__ uint32_t ip_gray4(const uint8_t *__restrict__ row, int x, int w, const IpGray &g)
{
    if (x >= w) return 0u;
    if (ALIGNED && x + 4 <= w) {
        if (C == 1) return *(const uint32_t *)(row + x);
        if (C == 3) {
            const IpU3 v = *(const IpU3 *)(row + 3 * x);
            return ip_gray(IP_BYTE(v.a, 0), IP_BYTE(v.a, 1), IP_BYTE(v.a, 2), g) | ip_gray(IP_BYTE(v.a, 3), IP_BYTE(v.b, 0), IP_BYTE(v.b, 1), g) << 8 |
                   ip_gray(IP_BYTE(v.b, 2), IP_BYTE(v.b, 3), IP_BYTE(v.c, 0), g) << 16 | ip_gray(IP_BYTE(v.c, 1), IP_BYTE(v.c, 2), IP_BYTE(v.c, 3), g) << 24;
        }
        const IpU4 v = *(const IpU4 *)(row + 4 * x);
        return ip_gray(IP_BYTE(v.a, 0), IP_BYTE(v.a, 1), IP_BYTE(v.a, 2), g) | ip_gray(IP_BYTE(v.b, 0), IP_BYTE(v.b, 1), IP_BYTE(v.b, 2), g) << 8 |
               ip_gray(IP_BYTE(v.c, 0), IP_BYTE(v.c, 1), IP_BYTE(v.c, 2), g) << 16 | ip_gray(IP_BYTE(v.d, 0), IP_BYTE(v.d, 1), IP_BYTE(v.d, 2), g) << 24;
    }
    uint32_t out = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (x + k < w) out |= ip_tap<C>(row + (size_t)(x + k) * C, g) << (8 * k);
    return out;
}

template <int C, bool ALIGNED> __global__ __launch_bounds__(256) void k_gray(IpFrames F, IpGray g)
{
    IP_XCD_REMAP_XY(bx, f);
    const int by = bx / F.colBlocks, cx = bx - by * F.colBlocks;
    const int x4 = cx * 64 + (int)(threadIdx.x & 63);
    if (4 * x4 >= F.dstStride) return;
    const uint8_t *__restrict__ src = F.src + (size_t)f * F.srcPitch;
    uint32_t *__restrict__ dst = (uint32_t *)(F.dst + (size_t)f * F.dstPitch) + x4;
    const int y0 = by * (4 * IP_ROWS) + (int)(threadIdx.x >> 6);
#pragma unroll
    for (int r = 0; r < IP_ROWS; r++) {
        const int y = y0 + 4 * r;
        if (y < F.h) dst[(size_t)y * (size_t)(F.dstStride >> 2)] = ip_gray4<C, ALIGNED>(src + (size_t)y * (size_t)F.srcStride, 4 * x4, F.w, g);
    }
}

// the grey values of 8 consecutive source pixels at p (any alignment, all 8 inside the row), pixel j in byte j: C words by dword loads that the
// hardware takes at any byte address, instead of 8 C byte loads
template <int N> struct __attribute__((packed, aligned(1))) IpWords { uint32_t w[N]; };
template <int C> __device__ __forceinline__ uint64_t ip_row8(const uint8_t *__restrict__ p, const IpGray &g)
{
    const IpWords<2 * C> v = *(const IpWords<2 * C> *)p;
    if (C == 1) return (uint64_t)v.w[0] | (uint64_t)v.w[1] << 32;
    uint32_t o[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int b = C * j;      // first byte of pixel j
        o[j >> 2] |= ip_gray(IP_BYTE(v.w[b >> 2], b & 3), IP_BYTE(v.w[(b + 1) >> 2], (b + 1) & 3), IP_BYTE(v.w[(b + 2) >> 2], (b + 2) & 3), g) << (8 * (j & 3));
    }
    return (uint64_t)o[0] | (uint64_t)o[1] << 32;
}

// one remapped pixel from its four taps (each already grey)
__device__ __forceinline__ uint32_t ip_blend(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t fx, uint32_t fy)
{
    const uint32_t gx = 32u - fx, gy = 32u - fy;
    return (__umul24(__umul24(gx, gy), p00) + __umul24(__umul24(fx, gy), p01) + __umul24(__umul24(gx, fy), p10) + __umul24(__umul24(fx, fy), p11) + 512u) >> 10;
}

template <int C> __global__ __launch_bounds__(256) void k_remap(IpFrames F, IpGray g, const uint32_t *__restrict__ mapXY, const uint16_t *__restrict__ mapF, int mapStride)
{
    IP_XCD_REMAP_XY(bx, f);
    const int by = bx / F.colBlocks, cx = bx - by * F.colBlocks;
    const int x4 = cx * 64 + (int)(threadIdx.x & 63);
    if (4 * x4 >= F.dstStride) return;
    const uint8_t *__restrict__ src = F.src + (size_t)f * F.srcPitch;
    uint32_t *__restrict__ dst = (uint32_t *)(F.dst + (size_t)f * F.dstPitch) + x4;
    const int y0 = by * (4 * IP_ROWS) + (int)(threadIdx.x >> 6), x = 4 * x4;
    const int W = F.w, H = F.h, S = F.srcStride;
#pragma unroll 1
    for (int r = 0; r < IP_ROWS; r++) {
        const int y = y0 + 4 * r;
        if (y >= H) break;
        uint32_t out = 0u;
        if (x < W) {      // (the map rows are padded to a multiple of 4 entries, the padding holds 0)
            const uint4 xy4 = *(const uint4 *)(mapXY + (size_t)y * (size_t)mapStride + x);
            const uint2 f4 = *(const uint2 *)(mapF + (size_t)y * (size_t)mapStride + x);
            const uint32_t xy[4] = {xy4.x, xy4.y, xy4.z, xy4.w};
            const uint32_t fr[4] = {f4.x & 0xffffu, f4.x >> 16, f4.y & 0xffffu, f4.y >> 16};
            int ix[4], iy[4];
            bool inside = true;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                ix[k] = (int)(short)(xy[k] & 0xffffu);
                iy[k] = (int)xy[k] >> 16;
                inside = inside && (unsigned)ix[k] < (unsigned)(W - 1) && (unsigned)iy[k] < (unsigned)(H - 1);      // taps ix, ix + 1, iy, iy + 1 all inside
            }
            // rectification maps are smooth: a lane's four pixels read two or three consecutive source rows within 8 columns.  Then two or three
            // wide loads fetch all 16 taps (grey computed once per source pixel), and a pixel picks its taps with a select and a 64-bit shift.
            // (Lanes whose four pixels cross a source row are one in ~35 with EuRoC's maps - nearly every wave has one, so they must not leave this path.)
            const int base = min(min(ix[0], ix[1]), min(ix[2], ix[3])), last = max(max(ix[0], ix[1]), max(ix[2], ix[3]));
            const int r0 = min(min(iy[0], iy[1]), min(iy[2], iy[3])), r1 = max(max(iy[0], iy[1]), max(iy[2], iy[3]));
            const bool segment = inside && r1 - r0 <= 1 && last - base <= 6 && base + 8 <= W;
            if (segment) {
                const uint8_t *p = src + (r0 * S + base * C);
                const uint64_t row0 = ip_row8<C>(p, g), row1 = ip_row8<C>(p + S, g);
                const uint64_t row2 = r1 != r0 ? ip_row8<C>(p + 2 * S, g) : 0;      // r1 + 1 = r0 + 2 is inside, as every iy + 1 is
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const bool lower = iy[k] != r0;
                    const uint32_t t = (uint32_t)((lower ? row1 : row0) >> (8 * (ix[k] - base))), b = (uint32_t)((lower ? row2 : row1) >> (8 * (ix[k] - base)));
                    out |= ip_blend(t & 255u, (t >> 8) & 255u, b & 255u, (b >> 8) & 255u, fr[k] & 31u, fr[k] >> 5) << (8 * k);
                }
            } else if (inside) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint8_t *p = src + (iy[k] * S + ix[k] * C);
                    out |= ip_blend(ip_tap<C>(p, g), ip_tap<C>(p + C, g), ip_tap<C>(p + S, g), ip_tap<C>(p + S + C, g), fr[k] & 31u, fr[k] >> 5) << (8 * k);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const bool x0 = (unsigned)ix[k] < (unsigned)W, x1 = (unsigned)(ix[k] + 1) < (unsigned)W;
                    const bool r0 = (unsigned)iy[k] < (unsigned)H, r1 = (unsigned)(iy[k] + 1) < (unsigned)H;
                    const uint8_t *p = src + ((ptrdiff_t)iy[k] * S + ix[k] * C);      // formed, not read, when a tap is outside
                    const uint32_t p00 = r0 && x0 ? ip_tap<C>(p, g) : 0u, p01 = r0 && x1 ? ip_tap<C>(p + C, g) : 0u;
                    const uint32_t p10 = r1 && x0 ? ip_tap<C>(p + S, g) : 0u, p11 = r1 && x1 ? ip_tap<C>(p + S + C, g) : 0u;
                    out |= ip_blend(p00, p01, p10, p11, fr[k] & 31u, fr[k] >> 5) << (8 * k);
                }
            }
            if (x + 4 > W) out &= 0xffffffffu >> (8 * (x + 4 - W));
        }
        dst[(size_t)y * (size_t)(F.dstStride >> 2)] = out;
    }
}

// float maps (rows w apart) -> fixed point (rows mapStride apart, the padding 0)
__global__ __launch_bounds__(256) void k_maps_fixed(const float *__restrict__ mx, const float *__restrict__ my, int w, int h, int mapStride, uint32_t *__restrict__ mapXY,
                                                     uint16_t *__restrict__ mapF)
{
    const int x = (int)(blockIdx.x * 256 + threadIdx.x), y = (int)blockIdx.y;
    if (x >= mapStride || y >= h) return;
    uint32_t xy = 0u, fr = 0u;
    if (x < w) {
        const size_t i = (size_t)y * (size_t)w + x;
        // the product by 32 is exact (or infinite, which the clamp takes); rintf = v_rndne_f32, half to even
        const int sx = (int)fminf(fmaxf(rintf(mx[i] * 32.0f), -1073741824.0f), 1073741824.0f);
        const int sy = (int)fminf(fmaxf(rintf(my[i] * 32.0f), -1073741824.0f), 1073741824.0f);
        const int ix = min(max(sx >> 5, -32768), 32767), iy = min(max(sy >> 5, -32768), 32767);
        xy = ((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16);
        fr = (uint32_t)(sx & 31) | (uint32_t)(sy & 31) << 5;
    }
    mapXY[(size_t)y * (size_t)mapStride + x] = xy;
    mapF[(size_t)y * (size_t)mapStride + x] = (uint16_t)fr;
}

int ip_out_stride(int w) { return (((w + 3) & ~3) + 12 + 15) & ~15; }

}  // namespace

struct orbx_image_prep {
    orbx_image_prep_config cfg = {};
    IpGray grayRGB = {};                 // c0 = R
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t lastStream = nullptr;    // the stream of the last call (ev1 is its end): a call on ANOTHER stream waits for it before it overwrites the output
    OrbxDevBuf<uint8_t> out, srcBuf;
    uint8_t *pinned = nullptr;           // staging of orbx_image_prep_upload and of the synchronous form's results
    size_t pinnedBytes = 0;
    struct Maps { OrbxDevBuf<uint32_t> xy; OrbxDevBuf<uint16_t> fr; int w = 0, h = 0, stride = 0; bool set = false; } maps[2];
    OrbxDevBuf<float> mapTmp;
    int lastStride = 0, lastBatch = 0;
    size_t lastPitch = 0;
    bool timed = false;
    int launches = 0;

    int ensure_pinned(size_t bytes)
    {
        if (bytes <= pinnedBytes) return ORBX_OK;
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr; pinnedBytes = 0;
        ORBX_HIP_CHECK(hipHostMalloc((void **)&pinned, bytes, hipHostMallocDefault));
        pinnedBytes = bytes;
        return ORBX_OK;
    }
};

extern "C" int orbx_image_prep_create(const orbx_image_prep_config *cfg, orbx_image_prep **out)
{
    if (!cfg || !out) { orbx_set_error("orbx_image_prep_create: NULL argument"); return ORBX_ERR_ARG; }
    *out = nullptr;
    if (cfg->max_width < 1 || cfg->max_width > IP_MAX_DIM || cfg->max_height < 1 || cfg->max_height > IP_MAX_DIM || cfg->max_batch < 1 || cfg->max_batch > 65535) {
        orbx_set_error("orbx_image_prep_create: max_width / max_height must lie in 1..%d and max_batch in 1..65535", IP_MAX_DIM);
        return ORBX_ERR_ARG;
    }
    uint32_t c[3] = {cfg->gray_coef[0], cfg->gray_coef[1], cfg->gray_coef[2]}, shift = cfg->gray_shift;
    if (c[0] == 0 && c[1] == 0 && c[2] == 0 && shift == 0) { c[0] = 9798; c[1] = 19235; c[2] = 3735; shift = 15; }      // OpenCV 4.x, 8-bit path
    if (shift < 8 || shift > 16 || c[0] + c[1] + c[2] != (1u << shift)) {
        orbx_set_error("orbx_image_prep_create: the grey weights must sum to 1 << gray_shift with gray_shift in 8..16 (got %u + %u + %u, shift %u)", c[0], c[1], c[2], shift);
        return ORBX_ERR_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { orbx_set_error("no HIP device available: liborbx has no CPU fallback"); return ORBX_ERR_NODEVICE; }
    if (cfg->device < 0 || cfg->device >= ndev) { orbx_set_error("device %d out of range", cfg->device); return ORBX_ERR_ARG; }
    ORBX_HIP_CHECK(hipSetDevice(cfg->device));
    orbx_image_prep *h = new orbx_image_prep();
    h->cfg = *cfg;
    h->grayRGB = IpGray{c[0], c[1], c[2], 1u << (shift - 1), shift};
    const size_t outBytes = (size_t)cfg->max_batch * (size_t)ip_out_stride(cfg->max_width) * (size_t)cfg->max_height;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
        h->out.ensure(outBytes) != ORBX_OK) {
        orbx_set_error("image front end: stream / event / buffer creation failed");
        orbx_image_prep_destroy(h);
        return ORBX_ERR_HIP;
    }
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_image_prep_destroy(orbx_image_prep *h)
{
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    if (h->timed) (void)hipEventSynchronize(h->ev1);      // the last call may have run on a consumer's stream
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    h->out.release(); h->srcBuf.release(); h->mapTmp.release();
    for (auto &m : h->maps) { m.xy.release(); m.fr.release(); }
    if (h->pinned) (void)hipHostFree(h->pinned);
    delete h;
}

extern "C" int orbx_rectify_maps(const double K[9], const double *D, int num_d, const double R[9], const double Pnew[9], int width, int height, float *map_x, float *map_y)
{
    if (!K || !D || !R || !Pnew || !map_x || !map_y) { orbx_set_error("orbx_rectify_maps: NULL argument"); return ORBX_ERR_ARG; }
    if (num_d != 4 && num_d != 5) { orbx_set_error("orbx_rectify_maps: num_d must be 4 or 5 (k1 k2 p1 p2 [k3]), got %d", num_d); return ORBX_ERR_ARG; }
    if (width < 1 || height < 1) { orbx_set_error("orbx_rectify_maps: empty size %d x %d", width, height); return ORBX_ERR_ARG; }
    double A[9], iR[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) A[3 * i + j] = (Pnew[3 * i] * R[j] + Pnew[3 * i + 1] * R[3 + j]) + Pnew[3 * i + 2] * R[6 + j];
    // the inverse by cofactors: C[i][j] = A[i+1][j+1] A[i+2][j+2] - A[i+1][j+2] A[i+2][j+1] (indices mod 3), det along row 0, inverse = C^T * (1 / det)
    double Cf[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            Cf[3 * i + j] = A[3 * i1 + j1] * A[3 * i2 + j2] - A[3 * i1 + j2] * A[3 * i2 + j1];
        }
    const double det = (A[0] * Cf[0] + A[1] * Cf[1]) + A[2] * Cf[2];
    if (!(std::isfinite(det)) || det == 0.0) { orbx_set_error("orbx_rectify_maps: Pnew * R is singular or not finite"); return ORBX_ERR_ARG; }
    const double idet = 1.0 / det;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) iR[3 * i + j] = Cf[3 * j + i] * idet;
    const double fx = K[0], fy = K[4], u0 = K[2], v0 = K[5];
    const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = num_d == 5 ? D[4] : 0.0;
    for (int i = 0; i < height; i++) {
        double _x = (double)i * iR[1] + iR[2], _y = (double)i * iR[4] + iR[5], _w = (double)i * iR[7] + iR[8];
        float *m1 = map_x + (size_t)i * (size_t)width, *m2 = map_y + (size_t)i * (size_t)width;
        for (int j = 0; j < width; j++) {
            const double w = 1.0 / _w, x = _x * w, y = _y * w;
            const double x2 = x * x, y2 = y * y;
            const double r2 = x2 + y2, _2xy = (2.0 * x) * y;
            const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
            const double u = fx * ((x * kr + p1 * _2xy) + p2 * (r2 + 2.0 * x2)) + u0;
            const double v = fy * ((y * kr + p1 * (r2 + 2.0 * y2)) + p2 * _2xy) + v0;
            m1[j] = (float)u;
            m2[j] = (float)v;
            _x += iR[0]; _y += iR[3]; _w += iR[6];
        }
    }
    return ORBX_OK;
}

#define IP_LAUNCH_CHECK()                                                                                                  \
    do {                                                                                                                   \
        const hipError_t le_ = hipGetLastError();                                                                          \
        if (le_ != hipSuccess) { orbx_set_error("image front end kernel launch failed: %s", hipGetErrorString(le_)); return ORBX_ERR_HIP; } \
        h->launches++;                                                                                                     \
    } while (0)

extern "C" int orbx_image_prep_set_maps(orbx_image_prep *h, int side, const float *map_x, const float *map_y, int map_stride_floats, int width, int height)
{
    // the maps themselves are checked before the handle is looked at, so a caller learns about them without a device
    if (!map_x || !map_y) { orbx_set_error("orbx_image_prep_set_maps: NULL map"); return ORBX_ERR_ARG; }
    if (side != 0 && side != 1) { orbx_set_error("orbx_image_prep_set_maps: side must be 0 (left) or 1 (right), got %d", side); return ORBX_ERR_ARG; }
    if (width < 1 || height < 1 || width > IP_MAX_DIM || height > IP_MAX_DIM || map_stride_floats < width) {
        orbx_set_error("orbx_image_prep_set_maps: bad size %d x %d (stride %d floats)", width, height, map_stride_floats);
        return ORBX_ERR_ARG;
    }
    const size_t n = (size_t)width * (size_t)height;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            if (!std::isfinite(map_x[(size_t)y * map_stride_floats + x]) || !std::isfinite(map_y[(size_t)y * map_stride_floats + x])) {
                orbx_set_error("orbx_image_prep_set_maps: the map value at (%d, %d) is not finite", x, y);
                return ORBX_ERR_ARG;
            }
    if (!h) { orbx_set_error("orbx_image_prep_set_maps: NULL handle"); return ORBX_ERR_ARG; }
    if (width > h->cfg.max_width || height > h->cfg.max_height) {
        orbx_set_error("orbx_image_prep_set_maps: maps of %d x %d for a handle of %d x %d", width, height, h->cfg.max_width, h->cfg.max_height);
        return ORBX_ERR_ARG;
    }
    ORBX_HIP_CHECK(hipSetDevice(h->cfg.device));
    if (h->timed && h->lastStream != h->stream) ORBX_HIP_CHECK(hipEventSynchronize(h->ev1));      // a batch on a consumer's stream may still read the old maps
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    orbx_image_prep::Maps &m = h->maps[side];
    m.set = false;
    const int ms = (width + 3) & ~3;
    int rc;
    if ((rc = h->mapTmp.ensure(2 * n)) != ORBX_OK || (rc = m.xy.ensure((size_t)ms * height)) != ORBX_OK || (rc = m.fr.ensure((size_t)ms * height)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipMemcpy2DAsync(h->mapTmp.p, (size_t)width * 4, map_x, (size_t)map_stride_floats * 4, (size_t)width * 4, (size_t)height, hipMemcpyHostToDevice, h->stream));
    ORBX_HIP_CHECK(hipMemcpy2DAsync(h->mapTmp.p + n, (size_t)width * 4, map_y, (size_t)map_stride_floats * 4, (size_t)width * 4, (size_t)height, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_maps_fixed, dim3((unsigned)((ms + 255) / 256), (unsigned)height), dim3(256), 0, h->stream, (const float *)h->mapTmp.p, (const float *)(h->mapTmp.p + n), width, height,
                       ms, m.xy.p, m.fr.p);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { orbx_set_error("k_maps_fixed launch failed: %s", hipGetErrorString(le)); return ORBX_ERR_HIP; }
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    m.w = width; m.h = height; m.stride = ms; m.set = true;
    return ORBX_OK;
}

namespace {

int ip_check_frames(const orbx_image_prep *h, int batch, int width, int height, int channels, const char *who)
{
    if (batch < 1 || batch > h->cfg.max_batch) { orbx_set_error("%s: batch %d outside 1..%d", who, batch, h->cfg.max_batch); return ORBX_ERR_ARG; }
    if (width < 1 || height < 1 || width > h->cfg.max_width || height > h->cfg.max_height) {
        orbx_set_error("%s: size %d x %d outside the handle's %d x %d", who, width, height, h->cfg.max_width, h->cfg.max_height);
        return ORBX_ERR_ARG;
    }
    if (channels != 1 && channels != 3 && channels != 4) { orbx_set_error("%s: channels must be 1, 3 or 4, got %d", who, channels); return ORBX_ERR_ARG; }
    return ORBX_OK;
}

template <int C> void ip_launch(orbx_image_prep *h, hipStream_t st, const IpFrames &F, const IpGray &g, dim3 grid, bool aligned, const orbx_image_prep::Maps *m)
{
    if (m) hipLaunchKernelGGL(k_remap<C>, grid, dim3(256), 0, st, F, g, (const uint32_t *)m->xy.p, (const uint16_t *)m->fr.p, m->stride);
    else if (aligned) hipLaunchKernelGGL((k_gray<C, true>), grid, dim3(256), 0, st, F, g);
    else hipLaunchKernelGGL((k_gray<C, false>), grid, dim3(256), 0, st, F, g);
}

}  // namespace

extern "C" int orbx_image_prep_batch_device(orbx_image_prep *h, orbx_extractor *consumer, const void *src_dev, int batch, int width, int height, int channels, int rgb_order,
                                            int src_stride, size_t src_pitch, int rectify_side)
{
    if (!h || !src_dev) { orbx_set_error("orbx_image_prep_batch_device: NULL argument"); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = ip_check_frames(h, batch, width, height, channels, "orbx_image_prep_batch_device")) != ORBX_OK) return rc;
    if (rgb_order != 0 && rgb_order != 1) { orbx_set_error("orbx_image_prep_batch_device: rgb_order must be 1 (R first) or 0 (B first), got %d", rgb_order); return ORBX_ERR_ARG; }
    const size_t rowBytes = (size_t)width * (size_t)channels;
    if (src_stride < 0 || (size_t)src_stride < rowBytes || src_pitch < (size_t)src_stride * (size_t)(height - 1) + rowBytes) {
        orbx_set_error("orbx_image_prep_batch_device: bad source stride / pitch");
        return ORBX_ERR_ARG;
    }
    if ((size_t)src_stride * (size_t)height > (size_t)INT32_MAX) { orbx_set_error("orbx_image_prep_batch_device: a source frame spans more than 2^31 bytes"); return ORBX_ERR_ARG; }
    if (rectify_side < -1 || rectify_side > 1) { orbx_set_error("orbx_image_prep_batch_device: rectify_side must be -1, 0 or 1, got %d", rectify_side); return ORBX_ERR_ARG; }
    const orbx_image_prep::Maps *m = rectify_side >= 0 ? &h->maps[rectify_side] : nullptr;
    if (m && !m->set) { orbx_set_error("orbx_image_prep_batch_device: no maps set for side %d", rectify_side); return ORBX_ERR_STATE; }
    if (m && (m->w != width || m->h != height)) {
        orbx_set_error("orbx_image_prep_batch_device: the maps of side %d are %d x %d, the frames %d x %d", rectify_side, m->w, m->h, width, height);
        return ORBX_ERR_ARG;
    }
    ORBX_HIP_CHECK(hipSetDevice(h->cfg.device));
    hipStream_t st = consumer ? orbx_extractor_stream_internal(consumer) : h->stream;
    if (h->timed && h->lastStream != st) ORBX_HIP_CHECK(hipStreamWaitEvent(st, h->ev1, 0));
    IpFrames F;
    F.src = (const uint8_t *)src_dev; F.srcStride = src_stride; F.srcPitch = src_pitch;
    F.dst = h->out.p; F.dstStride = ip_out_stride(width); F.dstPitch = (size_t)F.dstStride * (size_t)height;
    F.w = width; F.h = height; F.colBlocks = (F.dstStride / 4 + 63) / 64;
    IpGray g = h->grayRGB;
    if (!rgb_order) std::swap(g.c0, g.c2);
    const bool aligned = ((uintptr_t)src_dev & 3) == 0 && (src_stride & 3) == 0 && (src_pitch & 3) == 0;
    const dim3 grid((unsigned)(F.colBlocks * ((height + 4 * IP_ROWS - 1) / (4 * IP_ROWS))), (unsigned)batch);
    h->timed = false; h->launches = 0;
    ORBX_HIP_CHECK(hipEventRecord(h->ev0, st));
    if (channels == 1) ip_launch<1>(h, st, F, g, grid, aligned, m);
    else if (channels == 3) ip_launch<3>(h, st, F, g, grid, aligned, m);
    else ip_launch<4>(h, st, F, g, grid, aligned, m);
    IP_LAUNCH_CHECK();
    ORBX_HIP_CHECK(hipEventRecord(h->ev1, st));
    h->timed = true; h->lastStream = st;
    h->lastStride = F.dstStride; h->lastPitch = F.dstPitch; h->lastBatch = batch;
    return ORBX_OK;
}

extern "C" int orbx_image_prep_results_device(orbx_image_prep *h, const void **images_dev, int *stride, size_t *frame_pitch)
{
    if (!h) { orbx_set_error("orbx_image_prep_results_device: NULL handle"); return ORBX_ERR_ARG; }
    if (!h->lastBatch) { orbx_set_error("orbx_image_prep_results_device: no batch has run on this handle"); return ORBX_ERR_STATE; }
    if (images_dev) *images_dev = h->out.p;
    if (stride) *stride = h->lastStride;
    if (frame_pitch) *frame_pitch = h->lastPitch;
    return ORBX_OK;
}

extern "C" int orbx_image_prep_sync(orbx_image_prep *h)
{
    if (!h) { orbx_set_error("orbx_image_prep_sync: NULL handle"); return ORBX_ERR_ARG; }
    ORBX_HIP_CHECK(hipSetDevice(h->cfg.device));
    if (h->timed) ORBX_HIP_CHECK(hipEventSynchronize(h->ev1));
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    return ORBX_OK;
}

extern "C" int orbx_image_prep_upload(orbx_image_prep *h, const uint8_t *const *images, int batch, int width, int height, int channels, int stride, int dev_stride, int dev_offset,
                                      const void **src_dev, int *src_stride, size_t *src_pitch)
{
    if (!h || !images) { orbx_set_error("orbx_image_prep_upload: NULL argument"); return ORBX_ERR_ARG; }
    int rc;
    if ((rc = ip_check_frames(h, batch, width, height, channels, "orbx_image_prep_upload")) != ORBX_OK) return rc;
    const size_t rowBytes = (size_t)width * (size_t)channels;
    if (stride < 0 || (size_t)stride < rowBytes) { orbx_set_error("orbx_image_prep_upload: stride %d below the row's %zu bytes", stride, rowBytes); return ORBX_ERR_ARG; }
    if (dev_stride != 0 && (dev_stride < 0 || (size_t)dev_stride < rowBytes)) { orbx_set_error("orbx_image_prep_upload: dev_stride %d below the row's %zu bytes", dev_stride, rowBytes); return ORBX_ERR_ARG; }
    if (dev_offset < 0 || dev_offset > 15) { orbx_set_error("orbx_image_prep_upload: dev_offset must lie in 0..15, got %d", dev_offset); return ORBX_ERR_ARG; }
    for (int f = 0; f < batch; f++)
        if (!images[f]) { orbx_set_error("orbx_image_prep_upload: image %d is NULL", f); return ORBX_ERR_ARG; }
    const size_t ds = dev_stride ? (size_t)dev_stride : (rowBytes + 15) & ~(size_t)15;
    if (ds > (size_t)INT32_MAX) { orbx_set_error("orbx_image_prep_upload: dev_stride too large"); return ORBX_ERR_ARG; }
    const size_t pitch = ds * (size_t)height, total = pitch * (size_t)batch;
    ORBX_HIP_CHECK(hipSetDevice(h->cfg.device));
    if (h->timed) ORBX_HIP_CHECK(hipEventSynchronize(h->ev1));      // the last batch may still read the source buffer
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    if ((rc = h->srcBuf.ensure(total + 16)) != ORBX_OK || (rc = h->ensure_pinned(total)) != ORBX_OK) return rc;
    for (int f = 0; f < batch; f++)
        for (int y = 0; y < height; y++) {
            uint8_t *d = h->pinned + (size_t)f * pitch + (size_t)y * ds;
            memcpy(d, images[f] + (size_t)y * (size_t)stride, rowBytes);
            if (ds > rowBytes) memset(d + rowBytes, 0, ds - rowBytes);
        }
    ORBX_HIP_CHECK(hipMemcpyAsync(h->srcBuf.p + dev_offset, h->pinned, total, hipMemcpyHostToDevice, h->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    if (src_dev) *src_dev = h->srcBuf.p + dev_offset;
    if (src_stride) *src_stride = (int)ds;
    if (src_pitch) *src_pitch = pitch;
    return ORBX_OK;
}

extern "C" int orbx_image_prep_download(orbx_image_prep *h, int batch, int width, int height, uint8_t *out, int out_stride)
{
    if (!h || !out) { orbx_set_error("orbx_image_prep_download: NULL argument"); return ORBX_ERR_ARG; }
    if (!h->lastBatch) { orbx_set_error("orbx_image_prep_download: no batch has run on this handle"); return ORBX_ERR_STATE; }
    if (batch < 1 || batch > h->lastBatch || width < 1 || width > h->lastStride || height < 1 || (size_t)height * (size_t)h->lastStride > h->lastPitch || out_stride < width) {
        orbx_set_error("orbx_image_prep_download: %d frames of %d x %d (out_stride %d) do not fit the last batch", batch, width, height, out_stride);
        return ORBX_ERR_ARG;
    }
    ORBX_HIP_CHECK(hipSetDevice(h->cfg.device));
    ORBX_HIP_CHECK(hipEventSynchronize(h->ev1));      // (the batch may have run on a consumer's stream)
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    // the rows without their padding, through the pinned buffer (the upload's staging is free: its copy is complete)
    const size_t rows = (size_t)batch * (size_t)height;
    int rc;
    if ((rc = h->ensure_pinned(rows * (size_t)width)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipMemcpy2DAsync(h->pinned, (size_t)width, h->out.p, (size_t)h->lastStride, (size_t)width, rows, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(h->stream));
    for (size_t r = 0; r < rows; r++) memcpy(out + r * (size_t)out_stride, h->pinned + r * (size_t)width, (size_t)width);
    return ORBX_OK;
}

extern "C" int orbx_image_prep_run(orbx_image_prep *h, const uint8_t *const *images, int batch, int width, int height, int channels, int rgb_order, int stride, int rectify_side,
                                   uint8_t *out, int out_stride)
{
    if (!h || !images || !out) { orbx_set_error("orbx_image_prep_run: NULL argument"); return ORBX_ERR_ARG; }
    if (out_stride < width) { orbx_set_error("orbx_image_prep_run: out_stride %d below the width %d", out_stride, width); return ORBX_ERR_ARG; }
    const void *src = nullptr;
    int ss = 0, rc;
    size_t sp = 0;
    if ((rc = orbx_image_prep_upload(h, images, batch, width, height, channels, stride, 0, 0, &src, &ss, &sp)) != ORBX_OK) return rc;
    if ((rc = orbx_image_prep_batch_device(h, nullptr, src, batch, width, height, channels, rgb_order, ss, sp, rectify_side)) != ORBX_OK) return rc;
    return orbx_image_prep_download(h, batch, width, height, out, out_stride);
}

extern "C" int orbx_image_prep_last_timing(orbx_image_prep *h, float *device_ms, int *launches)
{
    if (!h) { orbx_set_error("NULL image front end handle"); return ORBX_ERR_ARG; }
    float ms = 0.f;
    if (h->timed) {
        ORBX_HIP_CHECK(hipSetDevice(h->cfg.device));
        ORBX_HIP_CHECK(hipEventSynchronize(h->ev1));
        ORBX_HIP_CHECK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    }
    if (device_ms) *device_ms = ms;
    if (launches) *launches = h->timed ? h->launches : 0;
    return ORBX_OK;
}
