// orbx_voc_text.hip -- a DBoW2 text vocabulary from the file to the device tree, on gfx950.
//
//   orbx_vocabulary_load_text*  ==  DBoW2::TemplatedVocabulary<FORB::TDescriptor,FORB>::loadFromTextFile
//                                   (reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1420), what System::System runs before its first frame,
//                                   followed by what orbx_vocabulary_create does with the flattened nodes.
//
// The file: "k L scoring weighting", then one line per node in id order: "parent isLeaf d0 .. d31 weight" (node id = line number, :1385).
//
// The chain (one enqueue, one host wait; a second wait only when the device flagged lines):
//   k_vt_count      '\n' per chunk of VT_CHUNK bytes, 16-byte loads
//   k_vt_scan       exclusive scan of the chunk counts: the id of a chunk's first line; the number of nodes
//   k_vt_parse      a chunk + VT_OVER bytes of overhang staged in LDS; the workgroup lists the newlines of its chunk (a line belongs to the chunk that
//                   holds the newline in FRONT of it, so it starts at most one byte behind the chunk and VT_OVER - 1 = 1023 bytes of it plus its own
//                   newline are always staged), one line per lane parsed from LDS: parent, isLeaf, 32 bytes, the weight.  The line index never
//                   leaves LDS; the start offsets that reach memory are those of the flagged lines, which is all the host needs.
//   k_vt_children   orbx_vocabulary_create's checks on the parents; children per node
//   k_vt_sum / k_vt_scan_sums / k_vt_nodes   exclusive scans of the child counts (childStart) and of is_leaf (word ids); the childless inner nodes
//   k_vt_place / k_vt_rank   the children of a node in arrival order, then each child's rank among its siblings by id: childList in ascending id for
//                   ANY line order with parent < id; childDesc gathered on the way
//   k_vt_publish    the record and the list of flagged lines into mapped host memory, the call's sequence word behind them (OrbxCallBox)
//
// The weight is converted with the Eisel-Lemire algorithm (D. Lemire, "Number parsing at a gigabyte per second", SPE 51 (8), 2021): up to 19
// significant digits in a 64-bit integer w and a decimal exponent q, w * 5^q from a table of 128-bit powers (orbx_pow5_128.inc), the rounding proven
// from the product's low bits.  Whatever it cannot prove is FLAGGED and parsed again by the host statement (strtol / strtod on the line): more
// than 19 significant digits, q outside the table, a subnormal or overflowing result, a product too close to a boundary, a tie.  The device never
// guesses.  vt_weight_token is __host__ __device__, so the rule is testable without a device (orbx_voc_text_weight_rule).
//
// Anything the chain cannot carry - more lines than a 70-byte minimum line allows (a format error somewhere), more than VT_MAXL lines in a chunk
// (likewise), more than VT_FLAGCAP flagged lines, a node with more than VT_MAXFAN children - takes the host statement over the whole text and
// orbx_vocabulary_create: slow and right.
#include <errno.h>
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "orbx_voc.h"

#define VT_CHUNK 16384      /* bytes of text per workgroup of k_vt_count / k_vt_parse (tests/test_voc_text.py names it) */
#define VT_OVER 1024        /* overhang staged behind a chunk: a line of up to 1023 bytes and its newline */
#define VT_MAXL 1024        /* lines per chunk that k_vt_parse lists (a valid line has 69 bytes or more: 238 per chunk) */
#define VT_MINLINE 70       /* "0 0" + 32 x " 0" + " 0" + '\n' */
#define VT_FLAGCAP 4096     /* flagged lines the record carries */
#define VT_MAXFAN 4096      /* children per node that k_vt_rank ranks */
#define VT_TILE 2048        /* nodes per workgroup of the node scans */
#define VT_SLICE ((size_t)8 << 20)      /* bytes per pinned upload slice */
#define VT_Q_MIN (-342)
#define VT_Q_MAX 308

namespace {

static const uint64_t kPow5Host[VT_Q_MAX - VT_Q_MIN + 1][2] = {
#include "orbx_pow5_128.inc"
};
__device__ const uint64_t kPow5Dev[VT_Q_MAX - VT_Q_MIN + 1][2] = {
#include "orbx_pow5_128.inc"
};

__host__ __device__ __forceinline__ uint64_t vt_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// w * 10^q (w != 0, VT_Q_MIN <= q <= VT_Q_MAX) as the correctly rounded double, or false: not proven here
__host__ __device__ __forceinline__ bool vt_eisel_lemire(uint64_t w, int q, const uint64_t (*tab)[2], uint64_t *bits)
{
    const int lz = __builtin_clzll(w);
    w <<= lz;
    const uint64_t p5hi = tab[q - VT_Q_MIN][0], p5lo = tab[q - VT_Q_MIN][1];
    uint64_t lo = w * p5hi, hi = vt_mulhi(w, p5hi);
    if ((hi & 0x1ffull) == 0x1ffull) {      // the 55 bits that decide are not settled by the high word of the power alone
        const uint64_t shi = vt_mulhi(w, p5lo);
        lo += shi;
        if (shi > lo) hi++;
    }
    if (lo == ~0ull && (q < -27 || q > 55)) return false;      // the truncated power could have carried into the bits that decide
    const int upperbit = (int)(hi >> 63), shift = upperbit + 9;
    uint64_t m = hi >> shift;
    int power2 = (((152170 + 65536) * q) >> 16) + 63 + upperbit - lz + 1023;
    if (power2 <= 0) return false;                               // subnormal or zero
    if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << shift) == hi) return false;      // exactly half way: a tie
    m += m & 1;
    m >>= 1;
    if (m >= (2ull << 52)) { m = 1ull << 52; power2++; }
    m &= ~(1ull << 52);
    if (power2 >= 0x7ff) return false;                           // overflow
    *bits = m | ((uint64_t)power2 << 52);
    return true;
}

__host__ __device__ __forceinline__ bool vt_is_sep(int c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// byte `pos` of the staged text; behind `lim` every byte reads as a newline
__host__ __device__ __forceinline__ int vt_ch(const uint8_t *s, int pos, int lim) { return pos < lim ? (int)s[pos] : '\n'; }

__host__ __device__ __forceinline__ bool vt_skip(const uint8_t *s, int &pos, int lim)      // false: the line ended
{
    int c = vt_ch(s, pos, lim);
    while (vt_is_sep(c)) c = vt_ch(s, ++pos, lim);
    return c != '\n';
}

// an unsigned token of 1 .. maxDigits digits, ended by a separator or the line's end
__host__ __device__ __forceinline__ bool vt_uint_token(const uint8_t *s, int &pos, int lim, int maxDigits, int &val)
{
    if (!vt_skip(s, pos, lim)) return false;
    unsigned v = 0;
    int n = 0, c = vt_ch(s, pos, lim);
    while (c >= '0' && c <= '9' && n <= maxDigits) { v = v * 10u + (unsigned)(c - '0'); n++; c = vt_ch(s, ++pos, lim); }
    val = (int)v;
    return n >= 1 && n <= maxDigits && (vt_is_sep(c) || c == '\n');
}

// The weight token: [+-]?(digits[.digits*]|.digits)([eE][+-]?digits)?  ->  true and the double's bits when this code can PROVE the correctly rounded
// value: at most 19 significant digits, the decimal exponent inside the table, and Eisel-Lemire decides.  false: flagged (or not a number at all).
__host__ __device__ __forceinline__ bool vt_weight_token(const uint8_t *s, int &pos, int lim, const uint64_t (*tab)[2], uint64_t *bits)
{
    if (!vt_skip(s, pos, lim)) return false;
    int c = vt_ch(s, pos, lim);
    bool neg = false;
    if (c == '+' || c == '-') { neg = c == '-'; c = vt_ch(s, ++pos, lim); }
    uint64_t w = 0;
    int nd = 0, q = 0;
    bool any = false, over = false;
    while (c >= '0' && c <= '9') {
        any = true;
        if (w != 0 || c != '0') { if (nd < 19) { w = w * 10 + (uint64_t)(c - '0'); nd++; } else over = true; }
        c = vt_ch(s, ++pos, lim);
    }
    if (c == '.') {
        c = vt_ch(s, ++pos, lim);
        while (c >= '0' && c <= '9') {
            any = true;
            if (w != 0 || c != '0') { if (nd < 19) { w = w * 10 + (uint64_t)(c - '0'); nd++; q--; } else over = true; }
            else q--;
            c = vt_ch(s, ++pos, lim);
        }
    }
    if (!any) return false;
    if (c == 'e' || c == 'E') {
        c = vt_ch(s, ++pos, lim);
        bool eneg = false;
        if (c == '+' || c == '-') { eneg = c == '-'; c = vt_ch(s, ++pos, lim); }
        int e = 0, en = 0;
        while (c >= '0' && c <= '9') { if (e < 100000) e = e * 10 + (c - '0'); en++; c = vt_ch(s, ++pos, lim); }
        if (!en) return false;
        q += eneg ? -e : e;
    }
    if (!(vt_is_sep(c) || c == '\n') || over) return false;
    if (w == 0) { *bits = neg ? 0x8000000000000000ull : 0ull; return true; }
    if (q < VT_Q_MIN || q > VT_Q_MAX) return false;
    uint64_t b;
    if (!vt_eisel_lemire(w, q, tab, &b)) return false;
    *bits = b | (neg ? 0x8000000000000000ull : 0ull);
    return true;
}

// what the kernels leave for the host (device memory; k_vt_publish copies it into the call's mapped record)
struct VtRec {
    int32_t newlines, numNodes, numWords, flagCount, overflow, bigFan, errParent, errLeaf, errChildless, pad[7];
};
struct VtFlag { uint32_t id, start; };
struct VtPatch { int32_t id, parent, leaf, pad; uint8_t desc[32]; double weight; };

// '\n' among the 4 bytes of x, exactly (no borrow between bytes)
__device__ __forceinline__ int vt_newlines4(uint32_t x)
{
    const uint32_t y = x ^ 0x0a0a0a0au;
    return __popc(~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu));
}
__device__ __forceinline__ int vt_newlines16(uint4 v) { return vt_newlines4(v.x) + vt_newlines4(v.y) + vt_newlines4(v.z) + vt_newlines4(v.w); }

// the text buffer is zero-filled from `size` to the end of the last chunk's overhang: no load below needs a bound of its own
__global__ __launch_bounds__(256) void k_vt_count(const uint4 *__restrict__ text, int32_t *__restrict__ counts)
{
    __shared__ int sh[4];
    const int tid = threadIdx.x;
    const uint4 *p = text + (size_t)blockIdx.x * (VT_CHUNK / 16);
    int n = 0;
#pragma unroll
    for (int i = 0; i < VT_CHUNK / 16 / 256; i++) n += vt_newlines16(p[i * 256 + tid]);
    n = wave_sum_dpp(n);
    if ((tid & 63) == 0) sh[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// exclusive scan of arr[0..n) in place by ONE workgroup of 256 threads; returns the total
__device__ int vt_scan_global(int32_t *arr, int n, int *sh /* 256 */, int *wsum /* 4 */)
{
    const int tid = threadIdx.x, per = (n + 255) / 256, b = tid * per;
    int s = 0;
    for (int k = 0; k < per; k++) if (b + k < n) s += arr[b + k];
    sh[tid] = s;
    __syncthreads();
    const int total = block_exscan<256>(sh, 256, wsum);
    int run = sh[tid];
    for (int k = 0; k < per; k++)
        if (b + k < n) { const int v = arr[b + k]; arr[b + k] = run; run += v; }
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(256) void k_vt_scan(int32_t *chunkBase, int nChunks, int finalNewline, int capNodes, VtRec *rec)
{
    __shared__ int sh[256], wsum[4];
    const int total = vt_scan_global(chunkBase, nChunks, sh, wsum);
    if (threadIdx.x == 0) {
        const int lines = total + 1 - finalNewline;      // the header line is the root's: node id = line number
        rec->newlines = total;
        rec->overflow = lines > capNodes ? 1 : 0;
        rec->numNodes = lines > capNodes ? 0 : lines;
        rec->flagCount = 0;
    }
}

__global__ __launch_bounds__(256) void k_vt_parse(const uint4 *__restrict__ text, unsigned size, const int32_t *__restrict__ chunkBase, int capNodes,
                                                  int32_t *__restrict__ parent, uint8_t *__restrict__ leaf, uint32_t *__restrict__ desc, unsigned long long *__restrict__ weight,
                                                  VtRec *rec, VtFlag *flags)
{
    __shared__ uint4 stage[(VT_CHUNK + VT_OVER) / 16];
    __shared__ int cnt[256], wsum[4];
    __shared__ uint16_t nlPos[VT_MAXL];
    const int tid = threadIdx.x;
    const unsigned base = blockIdx.x * (unsigned)VT_CHUNK;
    const uint4 *p = text + (size_t)blockIdx.x * (VT_CHUNK / 16);
    for (int i = tid; i < (VT_CHUNK + VT_OVER) / 16; i += 256) stage[i] = p[i];
    __syncthreads();
    const uint8_t *s = (const uint8_t *)stage;
    // the newlines of the chunk itself (64 bytes per thread), listed in order
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) n += vt_newlines16(stage[tid * 4 + i]);
    cnt[tid] = n;
    __syncthreads();
    const int total = block_exscan<256>(cnt, 256, wsum);
    if (total > VT_MAXL) {      // (uniform) lines of 16 bytes: a format error somewhere, the host statement names it
        if (tid == 0) rec->overflow = 1;
        return;
    }
    if (n) {
        int r = cnt[tid];
        for (int b = 0; b < 64; b++)
            if (s[tid * 64 + b] == '\n') nlPos[r++] = (uint16_t)(tid * 64 + b);
    }
    __syncthreads();
    const unsigned left = size - base;      // (base < size: the grid covers the text)
    const int lim = left < (unsigned)(VT_CHUNK + VT_OVER) ? (int)left : VT_CHUNK + VT_OVER;
    const bool cut = left > (unsigned)(VT_CHUNK + VT_OVER);
    const int first = chunkBase[blockIdx.x];
    for (int j = tid; j < total; j += 256) {
        int pos = (int)nlPos[j] + 1;
        const unsigned start = base + (unsigned)pos;
        const int id = first + j + 1;
        if (start >= size || id >= capNodes) continue;      // the empty piece behind a final newline; lines beyond the capacity (k_vt_scan has said so)
        int par = 0, lf = 0;
        bool ok = vt_uint_token(s, pos, lim, 9, par) && vt_uint_token(s, pos, lim, 9, lf);
        uint32_t *d = desc + (size_t)id * 8;
        for (int w = 0; w < 8; w++) {
            uint32_t word = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                int v = 0;
                ok = ok && vt_uint_token(s, pos, lim, 3, v) && v <= 255;
                word |= (uint32_t)v << (8 * b);
            }
            d[w] = word;
        }
        uint64_t wb = 0;
        ok = ok && vt_weight_token(s, pos, lim, kPow5Dev, &wb);
        if (ok && cut && pos >= lim) ok = false;      // the token ran into the end of the staged bytes: the line is longer than the overhang
        if (!ok) {
            par = 0; lf = 0; wb = 0;
            const int at = atomicAdd(&rec->flagCount, 1);
            if (at < VT_FLAGCAP) { flags[at].id = (uint32_t)id; flags[at].start = start; }
        }
        parent[id] = par;
        leaf[id] = lf > 0 ? 1 : 0;
        weight[id] = wb;
    }
}

// flagged lines as the host statement read them
__global__ __launch_bounds__(256) void k_vt_patch(const VtPatch *__restrict__ patches, int n, int32_t *__restrict__ parent, uint8_t *__restrict__ leaf, uint32_t *__restrict__ desc,
                                                  double *__restrict__ weight)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const VtPatch pt = patches[i];
    parent[pt.id] = pt.parent;
    leaf[pt.id] = (uint8_t)pt.leaf;
    weight[pt.id] = pt.weight;
    const uint32_t *src = (const uint32_t *)pt.desc;
    for (int w = 0; w < 8; w++) desc[(size_t)pt.id * 8 + w] = src[w];
}

__global__ void k_vt_struct_begin(VtRec *rec)
{
    rec->errParent = rec->errLeaf = rec->errChildless = INT_MAX;
    rec->bigFan = 0;
    rec->numWords = 0;
}

// orbx_vocabulary_create's first loop: a parent must be a smaller node id and no leaf; the smallest offending id of each kind
__device__ __forceinline__ bool vt_parent_ok(const int32_t *parent, const uint8_t *leaf, int id, int &p)
{
    p = parent[id];
    return p >= 0 && p < id && !leaf[p];
}
__global__ __launch_bounds__(256) void k_vt_children(const int32_t *__restrict__ parent, uint8_t *__restrict__ leaf, int32_t *__restrict__ childCount, VtRec *rec)
{
    const int n = rec->numNodes;
    if (blockIdx.x == 0 && threadIdx.x == 0) leaf[0] = 0;      // (the root has no line and is never a leaf)
    for (int id = 1 + blockIdx.x * 256 + threadIdx.x; id < n; id += gridDim.x * 256) {
        const int p = parent[id];
        if (p < 0 || p >= id) atomicMin(&rec->errParent, id);
        else if (p > 0 && leaf[p]) atomicMin(&rec->errLeaf, id);
        else atomicAdd(&childCount[p], 1);
    }
}

// per tile of VT_TILE nodes: children and leaves
__global__ __launch_bounds__(256) void k_vt_sum(const int32_t *__restrict__ childCount, const uint8_t *__restrict__ leaf, const VtRec *rec, int32_t *__restrict__ sumChild,
                                                int32_t *__restrict__ sumLeaf)
{
    __shared__ int sh[2][4];
    const int n = rec->numNodes, tid = threadIdx.x;
    int a = 0, b = 0;
    for (int k = 0; k < VT_TILE / 256; k++) {
        const int i = blockIdx.x * VT_TILE + k * 256 + tid;
        if (i < n) { a += childCount[i]; b += i > 0 && leaf[i]; }
    }
    a = wave_sum_dpp(a); b = wave_sum_dpp(b);
    if ((tid & 63) == 0) { sh[0][tid >> 6] = a; sh[1][tid >> 6] = b; }
    __syncthreads();
    if (tid == 0) { sumChild[blockIdx.x] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3]; sumLeaf[blockIdx.x] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]; }
}
__global__ __launch_bounds__(256) void k_vt_scan_sums(int32_t *sumChild, int32_t *sumLeaf, int nTiles, VtRec *rec)
{
    __shared__ int sh[256], wsum[4];
    vt_scan_global(sumChild, nTiles, sh, wsum);
    const int words = vt_scan_global(sumLeaf, nTiles, sh, wsum);
    if (threadIdx.x == 0) rec->numWords = words;
}
// childStart and the word ids: the scans inside a tile behind the tile's offsets; create's second loop: an inner node has children
__global__ __launch_bounds__(256) void k_vt_nodes(const int32_t *__restrict__ childCount, const uint8_t *__restrict__ leaf, const int32_t *__restrict__ sumChild,
                                                  const int32_t *__restrict__ sumLeaf, VtRec *rec, VocNode *__restrict__ nodes)
{
    __shared__ int A[VT_TILE], B[VT_TILE], wsA[4], wsB[4];
    const int n = rec->numNodes, t0 = blockIdx.x * VT_TILE;
    if (t0 >= n) return;
    const int m = min(VT_TILE, n - t0);
    int totA, totB;
    block_fill_exscan2<256>(A, B, m, wsA, wsB, totA, totB, [&](int i, int &a, int &b) { a = childCount[t0 + i]; b = (t0 + i > 0 && leaf[t0 + i]) ? 1 : 0; });
    const int offA = sumChild[blockIdx.x], offB = sumLeaf[blockIdx.x];
    for (int i = threadIdx.x; i < m; i += 256) {
        const int id = t0 + i, cc = childCount[id];
        const bool lf = id > 0 && leaf[id];
        if (!lf && cc == 0) atomicMin(&rec->errChildless, id);
        VocNode nd;
        nd.childStart = offA + A[i]; nd.childCount = cc; nd.word = lf ? offB + B[i] : -1; nd.pad = 0;
        nodes[id] = nd;
    }
}

__global__ __launch_bounds__(256) void k_vt_place(const int32_t *__restrict__ parent, const uint8_t *__restrict__ leaf, const VocNode *__restrict__ nodes, int32_t *__restrict__ cursor,
                                                  int32_t *__restrict__ arrival, const VtRec *rec)
{
    const int n = rec->numNodes;
    for (int id = 1 + blockIdx.x * 256 + threadIdx.x; id < n; id += gridDim.x * 256) {
        int p;
        if (!vt_parent_ok(parent, leaf, id, p)) continue;
        arrival[nodes[p].childStart + atomicAdd(&cursor[p], 1)] = id;
    }
}
// a child's place among its siblings = the siblings with a smaller id (the arrival order is whatever the atomics gave; the result is not)
__global__ __launch_bounds__(256) void k_vt_rank(const int32_t *__restrict__ parent, const uint8_t *__restrict__ leaf, const VocNode *__restrict__ nodes,
                                                 const int32_t *__restrict__ arrival, const uint4 *__restrict__ desc, int32_t *__restrict__ childList, uint4 *__restrict__ childDesc,
                                                 VtRec *rec)
{
    const int n = rec->numNodes;
    for (int id = 1 + blockIdx.x * 256 + threadIdx.x; id < n; id += gridDim.x * 256) {
        int p;
        if (!vt_parent_ok(parent, leaf, id, p)) continue;
        const VocNode nd = nodes[p];
        if (nd.childCount > VT_MAXFAN) { rec->bigFan = 1; continue; }
        int r = 0;
        for (int c = 0; c < nd.childCount; c++) r += arrival[nd.childStart + c] < id;
        const size_t at = (size_t)nd.childStart + r;
        childList[at] = id;
        childDesc[2 * at] = desc[2 * (size_t)id];
        childDesc[2 * at + 1] = desc[2 * (size_t)id + 1];
    }
}

__global__ __launch_bounds__(256) void k_vt_publish(const VtRec *rec, const VtFlag *flags, VtRec *recOut, VtFlag *flagsOut, unsigned *pubCounter, unsigned long long *pubFlag,
                                                    unsigned long long pubSeq)
{
    const int nf = min(rec->flagCount, VT_FLAGCAP);
    for (int i = threadIdx.x; i < nf; i += 256) flagsOut[i] = flags[i];
    if (threadIdx.x == 0) *recOut = *rec;
    orbx_publish(pubCounter, pubFlag, pubSeq, 1);
}

// ---- the host statement -------------------------------------------------------------------------------------------------------------------
struct VtTok { const char *b, *e; };
static bool next_token(const char *&p, const char *e, VtTok &t)
{
    while (p < e && vt_is_sep((unsigned char)*p)) p++;
    if (p >= e) return false;
    t.b = p;
    while (p < e && !vt_is_sep((unsigned char)*p)) p++;
    t.e = p;
    return true;
}
static bool tok_int(const VtTok &t, long &v)      // [+-]?digits inside int
{
    const char *p = t.b;
    if (p < t.e && (*p == '+' || *p == '-')) p++;
    if (p >= t.e) return false;
    for (const char *c = p; c < t.e; c++) if (*c < '0' || *c > '9') return false;
    const std::string s(t.b, t.e);
    errno = 0;
    v = strtol(s.c_str(), nullptr, 10);
    return errno == 0 && v >= INT_MIN && v <= INT_MAX;
}
static bool tok_weight(const VtTok &t, double &w)      // [+-]?(digits[.digits*]|.digits)([eE][+-]?digits)?  - no inf, nan or hex floats - then strtod
{
    const char *p = t.b;
    if (p < t.e && (*p == '+' || *p == '-')) p++;
    int nd = 0;
    while (p < t.e && *p >= '0' && *p <= '9') { p++; nd++; }
    if (p < t.e && *p == '.') { p++; while (p < t.e && *p >= '0' && *p <= '9') { p++; nd++; } }
    if (!nd) return false;
    if (p < t.e && (*p == 'e' || *p == 'E')) {
        p++;
        if (p < t.e && (*p == '+' || *p == '-')) p++;
        int ne = 0;
        while (p < t.e && *p >= '0' && *p <= '9') { p++; ne++; }
        if (!ne) return false;
    }
    if (p != t.e) return false;
    const std::string s(t.b, t.e);
    w = strtod(s.c_str(), nullptr);
    return true;
}
// one node line [p, e): false and `why` on a format error
static bool host_line(const char *p, const char *e, int32_t *parent, int32_t *leaf, uint8_t *desc, double *weight, const char **why)
{
    VtTok t;
    long v;
    if (!next_token(p, e, t)) { *why = "the line is empty"; return false; }
    if (!tok_int(t, v)) { *why = "the parent is not an integer"; return false; }
    *parent = (int32_t)v;
    if (!next_token(p, e, t)) { *why = "too few tokens (35 wanted: parent, isLeaf, 32 bytes, weight)"; return false; }
    if (!tok_int(t, v)) { *why = "isLeaf is not an integer"; return false; }
    *leaf = v > 0 ? 1 : 0;
    for (int i = 0; i < 32; i++) {
        if (!next_token(p, e, t)) { *why = "too few tokens (35 wanted: parent, isLeaf, 32 bytes, weight)"; return false; }
        if (!tok_int(t, v)) { *why = "a descriptor byte is not an integer"; return false; }
        if (v < 0 || v > 255) { *why = "a descriptor byte is outside 0..255"; return false; }
        desc[i] = (uint8_t)v;
    }
    if (!next_token(p, e, t)) { *why = "too few tokens (35 wanted: parent, isLeaf, 32 bytes, weight)"; return false; }
    if (!tok_weight(t, *weight)) { *why = "the weight is not a decimal number"; return false; }
    return true;
}
static int fail_line(orbx_voc_text_info *info, int line, const char *fmt, ...)
{
    char msg[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    if (info) info->error_line = line;
    orbx_set_error("vocabulary text, line %d: %s", line, msg);
    return ORBX_ERR_ARG;
}
// the header [p, e): k L scoring weighting, the reference's range check (:1359) and orbx_vocabulary_create's k >= 1
static int host_header(const char *p, const char *e, orbx_voc_text_info *info)
{
    long v[4];
    for (int i = 0; i < 4; i++) {
        VtTok t;
        if (!next_token(p, e, t) || !tok_int(t, v[i])) return fail_line(info, 1, "the header is not \"k L scoring weighting\"");
    }
    if (v[0] < 1 || v[0] > 20 || v[1] < 1 || v[1] > 10 || v[2] < 0 || v[2] > 5 || v[3] < 0 || v[3] > 3)
        return fail_line(info, 1, "header %ld %ld %ld %ld out of range (k 1..20, L 1..10, scoring 0..5, weighting 0..3)", v[0], v[1], v[2], v[3]);
    info->k = (int32_t)v[0]; info->L = (int32_t)v[1]; info->scoring = (int32_t)v[2]; info->weighting = (int32_t)v[3];
    return ORBX_OK;
}
// orbx_vocabulary_create's three checks, with its messages, as errors of the line the node stands on
static int fail_parent(orbx_voc_text_info *info, int id, int p) { return fail_line(info, id + 1, "node %d: parent %d must be a smaller node id", id, p); }
static int fail_leaf(orbx_voc_text_info *info, int id, int p) { return fail_line(info, id + 1, "node %d hangs under leaf %d", id, p); }
static int fail_childless(orbx_voc_text_info *info, int id) { return fail_line(info, id + 1, "inner node %d has no children", id); }

static int parse_host(const char *text, size_t size, orbx_voc_text_info *info, std::vector<int32_t> &parent, std::vector<uint8_t> &leaf, uint8_t *desc, double *weights,
                      int32_t capacity)
{
    memset(info, 0, sizeof(*info));
    info->bytes = (int64_t)size;
    if (!size) return fail_line(info, 1, "the text is empty");
    const char *end = text + size;
    const char *nl = (const char *)memchr(text, '\n', size);
    int rc = host_header(text, nl ? nl : end, info);
    if (rc != ORBX_OK) return rc;
    info->final_newline = text[size - 1] == '\n';
    parent.assign(1, 0);
    leaf.assign(1, 0);
    if (desc && capacity > 0) memset(desc, 0, 32);
    if (weights && capacity > 0) weights[0] = 0.0;
    const char *p = nl ? nl + 1 : end;
    int id = 1;
    while (p < end) {
        const char *e = (const char *)memchr(p, '\n', (size_t)(end - p));
        if (!e) e = end;
        int32_t par = 0, lf = 0;
        uint8_t d[32];
        double w = 0;
        const char *why = "";
        if (!host_line(p, e, &par, &lf, d, &w, &why)) return fail_line(info, id + 1, "%s", why);
        parent.push_back(par);
        leaf.push_back((uint8_t)lf);
        if (id < capacity) {
            if (desc) memcpy(desc + 32 * (size_t)id, d, 32);
            if (weights) weights[id] = w;
        }
        id++;
        p = e + 1;
        if (id == INT_MAX) return fail_line(info, id, "too many lines");
    }
    info->num_nodes = id;
    info->host_lines = id - 1;
    if (id < 2) return fail_line(info, 1, "the file has no node lines");
    std::vector<int32_t> nchild((size_t)id, 0);
    for (int i = 1; i < id; i++) {
        if (parent[(size_t)i] < 0 || parent[(size_t)i] >= i) return fail_parent(info, i, parent[(size_t)i]);
        if (leaf[(size_t)parent[(size_t)i]]) return fail_leaf(info, i, parent[(size_t)i]);
        nchild[(size_t)parent[(size_t)i]]++;
    }
    int words = 0;
    for (int i = 0; i < id; i++) {
        const bool lf = i > 0 && leaf[(size_t)i];
        if (!lf && !nchild[(size_t)i]) return fail_childless(info, i);
        words += lf;
    }
    info->num_words = words;
    return ORBX_OK;
}

typedef std::chrono::steady_clock VtClock;
static float ms_since(VtClock::time_point t0) { return std::chrono::duration<float, std::milli>(VtClock::now() - t0).count(); }

// where the text comes from: a caller's buffer, or a file read with pread-style seeks
struct VtSource {
    const uint8_t *mem = nullptr;
    FILE *f = nullptr;
    size_t size = 0;
    bool read(size_t off, size_t n, void *dst) const
    {
        if (mem) { memcpy(dst, mem + off, n); return true; }
        return fseeko(f, (off_t)off, SEEK_SET) == 0 && fread(dst, 1, n, f) == n;
    }
};
struct VtPinned {
    uint8_t *p = nullptr;
    ~VtPinned() { if (p) (void)hipHostFree(p); }
};
struct VtEvents {
    hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~VtEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
// the chain's working arrays: sized for the most lines the text can hold, freed when the call returns (the handle keeps exact-size copies)
struct VtWork {
    OrbxOwnedBuf<uint4> text;
    OrbxOwnedBuf<int32_t> chunkBase, parent, childCount, cursor, arrival, childList, sumChild, sumLeaf;
    OrbxOwnedBuf<uint8_t> leaf;
    OrbxOwnedBuf<uint4> desc, childDesc;
    OrbxOwnedBuf<double> weight;
    OrbxOwnedBuf<VocNode> nodes;
    OrbxOwnedBuf<VtRec> rec;
    OrbxOwnedBuf<VtFlag> flags;
};

static int launch_structure(orbx_vocabulary *v, VtWork &wk, int capNodes, const OrbxStaged &sg, OrbxSlot<VtRec, ORBX_STAGE_OUT> sRec, OrbxSlot<VtFlag, ORBX_STAGE_OUT> sFlags,
                            unsigned long long seq, int *launches)
{
    hipStream_t st = v->stream;
    const unsigned grid = (unsigned)((capNodes + 255) / 256), tiles = (unsigned)((capNodes + VT_TILE - 1) / VT_TILE);
    ORBX_HIP_CHECK(hipMemsetAsync(wk.childCount.p, 0, (size_t)capNodes * 4, st));
    ORBX_HIP_CHECK(hipMemsetAsync(wk.cursor.p, 0, (size_t)capNodes * 4, st));
    hipLaunchKernelGGL(k_vt_struct_begin, dim3(1), dim3(1), 0, st, wk.rec.p);
    hipLaunchKernelGGL(k_vt_children, dim3(grid), dim3(256), 0, st, (const int32_t *)wk.parent.p, wk.leaf.p, wk.childCount.p, wk.rec.p);
    hipLaunchKernelGGL(k_vt_sum, dim3(tiles), dim3(256), 0, st, (const int32_t *)wk.childCount.p, (const uint8_t *)wk.leaf.p, (const VtRec *)wk.rec.p, wk.sumChild.p, wk.sumLeaf.p);
    hipLaunchKernelGGL(k_vt_scan_sums, dim3(1), dim3(256), 0, st, wk.sumChild.p, wk.sumLeaf.p, (int)tiles, wk.rec.p);
    hipLaunchKernelGGL(k_vt_nodes, dim3(tiles), dim3(256), 0, st, (const int32_t *)wk.childCount.p, (const uint8_t *)wk.leaf.p, (const int32_t *)wk.sumChild.p,
                       (const int32_t *)wk.sumLeaf.p, wk.rec.p, wk.nodes.p);
    hipLaunchKernelGGL(k_vt_place, dim3(grid), dim3(256), 0, st, (const int32_t *)wk.parent.p, (const uint8_t *)wk.leaf.p, (const VocNode *)wk.nodes.p, wk.cursor.p, wk.arrival.p,
                       (const VtRec *)wk.rec.p);
    hipLaunchKernelGGL(k_vt_rank, dim3(grid), dim3(256), 0, st, (const int32_t *)wk.parent.p, (const uint8_t *)wk.leaf.p, (const VocNode *)wk.nodes.p, (const int32_t *)wk.arrival.p,
                       (const uint4 *)wk.desc.p, wk.childList.p, wk.childDesc.p, wk.rec.p);
    hipLaunchKernelGGL(k_vt_publish, dim3(1), dim3(256), 0, st, (const VtRec *)wk.rec.p, (const VtFlag *)wk.flags.p, sg.dev(sRec), sg.dev(sFlags), v->box.counter, v->box.flagDev, seq);
    ORBX_LAUNCH_CHECK();
    *launches += 8;
    return ORBX_OK;
}

// everything the chain cannot carry: the host statement over the whole text, then orbx_vocabulary_create
static int load_on_host(int device, const VtSource &src, orbx_vocabulary **out, orbx_voc_text_info *info)
{
    std::vector<uint8_t> all;
    const uint8_t *text = src.mem;
    if (!text) {
        all.resize(src.size);
        if (!src.read(0, src.size, all.data())) { orbx_set_error("reading the vocabulary file failed"); return ORBX_ERR_ARG; }
        text = all.data();
    }
    std::vector<int32_t> parent;
    std::vector<uint8_t> leaf;
    orbx_voc_text_info sized;
    int rc = parse_host((const char *)text, src.size, &sized, parent, leaf, nullptr, nullptr, 0);
    if (rc != ORBX_OK) { info->error_line = sized.error_line; return rc; }
    std::vector<uint8_t> desc((size_t)sized.num_nodes * 32);
    std::vector<double> weights((size_t)sized.num_nodes);
    orbx_voc_text_info full;
    if ((rc = parse_host((const char *)text, src.size, &full, parent, leaf, desc.data(), weights.data(), sized.num_nodes)) != ORBX_OK) return rc;
    const orbx_voc_text_info keep = *info;
    *info = full;
    info->launches = keep.launches; info->waits = keep.waits; info->read_ms = keep.read_ms; info->upload_ms = keep.upload_ms; info->kernel_ms = keep.kernel_ms;
    info->host_ms += keep.host_ms;
    return orbx_vocabulary_create(device, full.k, full.L, full.num_nodes, parent.data(), leaf.data(), desc.data(), weights.data(), out);
}

static int load_text(int device, const VtSource &src, orbx_vocabulary **out, orbx_voc_text_info *info)
{
    const VtClock::time_point t0 = VtClock::now();
    const size_t size = src.size;
    if (size >= ((size_t)1 << 31)) { orbx_set_error("vocabulary text of %zu bytes: 2^31 bytes or more", size); return ORBX_ERR_CAPACITY; }
    if (!size) return fail_line(info, 1, "the text is empty");
    info->bytes = (int64_t)size;
    if (const int rcDev = orbx_select_device(device)) return rcDev;

    // the header: the host has the bytes
    VtPinned pin[2];
    const size_t n0 = size < VT_SLICE ? size : VT_SLICE;
    ORBX_HIP_CHECK(hipHostMalloc((void **)&pin[0].p, n0, hipHostMallocDefault));
    if (size > n0) ORBX_HIP_CHECK(hipHostMalloc((void **)&pin[1].p, VT_SLICE, hipHostMallocDefault));
    VtClock::time_point tr = VtClock::now();
    if (!src.read(0, n0, pin[0].p)) { orbx_set_error("reading the vocabulary file failed"); return ORBX_ERR_ARG; }
    uint8_t last = 0;
    if (!src.read(size - 1, 1, &last)) { orbx_set_error("reading the vocabulary file failed"); return ORBX_ERR_ARG; }
    info->read_ms += ms_since(tr);
    const VtClock::time_point th = VtClock::now();
    const char *nl = (const char *)memchr(pin[0].p, '\n', n0);
    if (!nl && size > n0) return load_on_host(device, src, out, info);      // (a header of 8 MB)
    int rc = host_header((const char *)pin[0].p, nl ? nl : (const char *)pin[0].p + n0, info);
    if (rc != ORBX_OK) return rc;
    info->final_newline = last == '\n';
    if (!nl || (size_t)(nl + 1 - (const char *)pin[0].p) >= size) return fail_line(info, 1, "the file has no node lines");
    info->host_ms += ms_since(th);

    orbx_vocabulary *v = new orbx_vocabulary();
    struct Guard { orbx_vocabulary *v; ~Guard() { if (v) orbx_vocabulary_destroy(v); } } guard{v};
    if ((rc = v->open(device)) != ORBX_OK) return rc;
    hipStream_t st = v->stream;
    const int nChunks = (int)((size + VT_CHUNK - 1) / VT_CHUNK);
    const size_t textBytes = (size_t)nChunks * VT_CHUNK + VT_OVER;
    const int capNodes = (int)(size / VT_MINLINE) + 2;
    const int tiles = (capNodes + VT_TILE - 1) / VT_TILE;
    const size_t N = (size_t)capNodes;
    VtWork wk;
    if ((rc = wk.text.ensure(textBytes / 16)) || (rc = wk.chunkBase.ensure((size_t)nChunks)) || (rc = wk.parent.ensure(N)) || (rc = wk.childCount.ensure(N)) || (rc = wk.cursor.ensure(N)) ||
        (rc = wk.arrival.ensure(N)) || (rc = wk.childList.ensure(N)) || (rc = wk.sumChild.ensure((size_t)tiles)) || (rc = wk.sumLeaf.ensure((size_t)tiles)) || (rc = wk.leaf.ensure(N)) ||
        (rc = wk.desc.ensure(2 * N)) || (rc = wk.childDesc.ensure(2 * N)) || (rc = wk.weight.ensure(N)) || (rc = wk.nodes.ensure(N)) || (rc = wk.rec.ensure(1)) ||
        (rc = wk.flags.ensure(VT_FLAGCAP)))
        return rc;
    VtEvents ev;      // 0 / 1: behind the copy out of slice buffer 0 / 1 (the buffer is free again); 2 / 3: in front of that copy; 4 / 5: around the kernels
    for (hipEvent_t &e : ev.e) if ((rc = orbx_event_create(&e)) != ORBX_OK) return rc;

    // the text in slices: slice i + 1 is read while slice i crosses the bus
    ORBX_HIP_CHECK(hipMemsetAsync((uint8_t *)wk.text.p + size, 0, textBytes - size, st));
    ORBX_HIP_CHECK(hipMemsetAsync(wk.rec.p, 0, sizeof(VtRec), st));
    ORBX_HIP_CHECK(hipMemsetAsync(wk.desc.p, 0, 32, st));      // the root: no line, descriptor 0, weight 0, parent 0
    ORBX_HIP_CHECK(hipMemsetAsync(wk.weight.p, 0, 8, st));
    ORBX_HIP_CHECK(hipMemsetAsync(wk.parent.p, 0, 4, st));
    bool used[2] = {false, false};
    auto harvest = [&](int b) -> int {      // waits for the copy out of buffer b and adds its time on the stream to upload_ms
        float t = 0.f;
        ORBX_HIP_CHECK(hipEventSynchronize(ev.e[b]));
        ORBX_HIP_CHECK(hipEventElapsedTime(&t, ev.e[2 + b], ev.e[b]));
        info->upload_ms += t;
        used[b] = false;
        return ORBX_OK;
    };
    int slice = 0;
    for (size_t off = 0; off < size; off += VT_SLICE, slice++) {
        const int b = slice & 1;
        const size_t n = size - off < VT_SLICE ? size - off : VT_SLICE;
        if (slice > 0) {      // (slice 0 is in pin[0] already)
            if (used[b] && (rc = harvest(b)) != ORBX_OK) return rc;
            tr = VtClock::now();
            if (!src.read(off, n, pin[b].p)) { (void)hipStreamSynchronize(st); orbx_set_error("reading the vocabulary file failed"); return ORBX_ERR_ARG; }
            info->read_ms += ms_since(tr);
        }
        ORBX_HIP_CHECK(hipEventRecord(ev.e[2 + b], st));
        ORBX_HIP_CHECK(hipMemcpyAsync((uint8_t *)wk.text.p + off, pin[b].p, n, hipMemcpyHostToDevice, st));
        ORBX_HIP_CHECK(hipEventRecord(ev.e[b], st));
        used[b] = true;
    }

    // the chain
    OrbxCallBox &bx = v->box;
    auto [pin_, pout] = bx.plan();
    (void)pin_;
    const auto sRec = pout.hole<VtRec>(1);
    const auto sFlags = pout.hole<VtFlag>(VT_FLAGCAP);
    OrbxStaged sg = bx.begin(st, &rc);
    if (rc != ORBX_OK) return rc;
    unsigned long long seq = bx.arm();
    ORBX_HIP_CHECK(hipEventRecord(ev.e[4], st));
    hipLaunchKernelGGL(k_vt_count, dim3((unsigned)nChunks), dim3(256), 0, st, (const uint4 *)wk.text.p, wk.chunkBase.p);
    hipLaunchKernelGGL(k_vt_scan, dim3(1), dim3(256), 0, st, wk.chunkBase.p, nChunks, info->final_newline, capNodes, wk.rec.p);
    hipLaunchKernelGGL(k_vt_parse, dim3((unsigned)nChunks), dim3(256), 0, st, (const uint4 *)wk.text.p, (unsigned)size, (const int32_t *)wk.chunkBase.p, capNodes, wk.parent.p, wk.leaf.p,
                       (uint32_t *)wk.desc.p, (unsigned long long *)wk.weight.p, wk.rec.p, wk.flags.p);
    ORBX_LAUNCH_CHECK();
    info->launches += 3;
    if ((rc = launch_structure(v, wk, capNodes, sg, sRec, sFlags, seq, &info->launches)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipEventRecord(ev.e[5], st));
    if ((rc = bx.wait(st)) != ORBX_OK) return rc;
    info->waits++;
    float kn = 0.f;
    ORBX_HIP_CHECK(hipEventSynchronize(ev.e[5]));
    for (int b = 0; b < 2; b++) if (used[b] && (rc = harvest(b)) != ORBX_OK) return rc;
    ORBX_HIP_CHECK(hipEventElapsedTime(&kn, ev.e[4], ev.e[5]));
    info->kernel_ms = kn;
    VtRec rec = *sg.host(sRec);
    if (rec.overflow || rec.flagCount > VT_FLAGCAP || rec.bigFan) return load_on_host(device, src, out, info);

    if (rec.flagCount > 0) {      // the lines the device would not vouch for: the host statement reads them, the structure stage runs again
        const VtClock::time_point tf = VtClock::now();
        std::vector<VtFlag> fl(sg.host(sFlags), sg.host(sFlags) + rec.flagCount);
        std::vector<VtPatch> patches((size_t)rec.flagCount);
        std::vector<char> line;
        int badLine = 0;
        std::string badWhy;
        for (size_t i = 0; i < fl.size(); i++) {
            line.clear();
            for (size_t off = fl[i].start; off < size;) {      // the line's bytes, up to its newline
                const size_t n = size - off < 4096 ? size - off : 4096, at = line.size();
                line.resize(at + n);
                if (!src.read(off, n, line.data() + at)) { orbx_set_error("reading the vocabulary file failed"); return ORBX_ERR_ARG; }
                const void *e = memchr(line.data() + at, '\n', n);
                if (e) { line.resize((size_t)((const char *)e - line.data())); break; }
                off += n;
            }
            VtPatch &pt = patches[i];
            memset(&pt, 0, sizeof(pt));
            pt.id = (int32_t)fl[i].id;
            const char *why = "";
            if (!host_line(line.data(), line.data() + line.size(), &pt.parent, &pt.leaf, pt.desc, &pt.weight, &why)) {
                if (!badLine || (int)fl[i].id + 1 < badLine) { badLine = (int)fl[i].id + 1; badWhy = why; }
            }
        }
        info->host_lines = rec.flagCount;
        if (badLine) return fail_line(info, badLine, "%s", badWhy.c_str());
        auto [pin2, pout2] = bx.plan();
        const auto sPatch = pin2.add(patches.data(), patches.size());
        const auto sRec2 = pout2.hole<VtRec>(1);
        const auto sFlags2 = pout2.hole<VtFlag>(VT_FLAGCAP);
        sg = bx.begin(st, &rc);
        if (rc != ORBX_OK) return rc;
        seq = bx.arm();
        info->host_ms += ms_since(tf);
        ORBX_HIP_CHECK(hipEventRecord(ev.e[4], st));
        hipLaunchKernelGGL(k_vt_patch, dim3((unsigned)((patches.size() + 255) / 256)), dim3(256), 0, st, (const VtPatch *)sg.dev(sPatch), (int)patches.size(), wk.parent.p, wk.leaf.p,
                           (uint32_t *)wk.desc.p, wk.weight.p);
        ORBX_LAUNCH_CHECK();
        info->launches++;
        if ((rc = launch_structure(v, wk, capNodes, sg, sRec2, sFlags2, seq, &info->launches)) != ORBX_OK) return rc;
        ORBX_HIP_CHECK(hipEventRecord(ev.e[5], st));
        if ((rc = bx.wait(st)) != ORBX_OK) return rc;
        info->waits++;
        ORBX_HIP_CHECK(hipEventSynchronize(ev.e[5]));
        ORBX_HIP_CHECK(hipEventElapsedTime(&kn, ev.e[4], ev.e[5]));
        info->kernel_ms += kn;
        rec = *sg.host(sRec2);
        if (rec.bigFan) return load_on_host(device, src, out, info);
    }

    // orbx_vocabulary_create's checks, in its order
    const int e1 = rec.errParent < rec.errLeaf ? rec.errParent : rec.errLeaf;
    if (e1 != INT_MAX) {
        int32_t p = 0;
        ORBX_HIP_CHECK(hipMemcpy(&p, wk.parent.p + e1, 4, hipMemcpyDeviceToHost));
        return e1 == rec.errParent ? fail_parent(info, e1, p) : fail_leaf(info, e1, p);
    }
    if (rec.errChildless != INT_MAX) return fail_childless(info, rec.errChildless);
    info->num_nodes = rec.numNodes;
    info->num_words = rec.numWords;

    // the handle keeps arrays of the tree's own size
    const size_t n = (size_t)rec.numNodes, nc = n - 1;
    v->k = info->k; v->L = info->L; v->numNodes = rec.numNodes; v->numWords = rec.numWords;
    if ((rc = v->nodes.ensure(n)) || (rc = v->childList.ensure(nc)) || (rc = v->childDesc.ensure(2 * nc)) || (rc = v->nodeWeight.ensure(n))) return rc;
    ORBX_HIP_CHECK(hipMemcpyAsync(v->nodes.p, wk.nodes.p, n * sizeof(VocNode), hipMemcpyDeviceToDevice, st));
    ORBX_HIP_CHECK(hipMemcpyAsync(v->childList.p, wk.childList.p, nc * 4, hipMemcpyDeviceToDevice, st));
    ORBX_HIP_CHECK(hipMemcpyAsync(v->childDesc.p, wk.childDesc.p, nc * 32, hipMemcpyDeviceToDevice, st));
    ORBX_HIP_CHECK(hipMemcpyAsync(v->nodeWeight.p, wk.weight.p, n * 8, hipMemcpyDeviceToDevice, st));
    ORBX_HIP_CHECK(hipStreamSynchronize(st));
    info->total_ms = ms_since(t0);
    guard.v = nullptr;
    *out = v;
    return ORBX_OK;
}

static int load_checked(int device, const VtSource &src, orbx_vocabulary **out, orbx_voc_text_info *info)
{
    orbx_voc_text_info local;
    if (!info) info = &local;
    memset(info, 0, sizeof(*info));
    const VtClock::time_point t0 = VtClock::now();
    const int rc = load_text(device, src, out, info);
    if (rc == ORBX_OK && info->total_ms == 0.f) info->total_ms = ms_since(t0);
    if (rc != ORBX_OK && *out) { orbx_vocabulary_destroy(*out); *out = nullptr; }
    return rc;
}

}  // namespace

extern "C" int orbx_vocabulary_load_text_buffer(int device, const void *text, size_t size, orbx_vocabulary **out, orbx_voc_text_info *info)
{
    if (!out || (!text && size)) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    *out = nullptr;
    VtSource src;
    static const uint8_t none = 0;
    src.mem = text ? (const uint8_t *)text : &none;
    src.size = size;
    return load_checked(device, src, out, info);
}

extern "C" int orbx_vocabulary_load_text(int device, const char *path, orbx_vocabulary **out, orbx_voc_text_info *info)
{
    if (!out || !path) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    *out = nullptr;
    if (info) memset(info, 0, sizeof(*info));
    FILE *f = fopen(path, "rb");
    if (!f) { orbx_set_error("cannot open vocabulary file %s: %s", path, strerror(errno)); return ORBX_ERR_ARG; }
    VtSource src;
    src.f = f;
    int rc;
    if (fseeko(f, 0, SEEK_END) != 0 || ftello(f) < 0) { orbx_set_error("cannot size vocabulary file %s", path); rc = ORBX_ERR_ARG; }
    else { src.size = (size_t)ftello(f); rc = load_checked(device, src, out, info); }
    fclose(f);
    return rc;
}

extern "C" int orbx_voc_text_parse_host(const void *text, size_t size, orbx_voc_text_info *info, int32_t capacity_nodes, int32_t *parent, uint8_t *is_leaf, uint8_t *descriptors,
                                        double *weights)
{
    orbx_voc_text_info local;
    if (!info) info = &local;
    if (!text && size) { orbx_set_error("NULL argument"); return ORBX_ERR_ARG; }
    const VtClock::time_point t0 = VtClock::now();
    std::vector<int32_t> par;
    std::vector<uint8_t> leaf;
    const bool arrays = parent || is_leaf || descriptors || weights;
    const int rc = parse_host(text ? (const char *)text : "", size, info, par, leaf, descriptors, weights, arrays ? capacity_nodes : 0);
    info->host_ms = info->total_ms = ms_since(t0);
    if (rc != ORBX_OK) return rc;
    if (arrays && capacity_nodes < info->num_nodes) { orbx_set_error("%d nodes, room for %d", info->num_nodes, capacity_nodes); return ORBX_ERR_CAPACITY; }
    if (parent) memcpy(parent, par.data(), par.size() * 4);
    if (is_leaf) memcpy(is_leaf, leaf.data(), leaf.size());
    return ORBX_OK;
}

extern "C" int orbx_voc_text_weight_rule(const char *token, size_t size, double *value)
{
    if (!token || size > 4096) return 0;
    int pos = 0;
    uint64_t bits = 0;
    if (!vt_weight_token((const uint8_t *)token, pos, (int)size, kPow5Host, &bits)) return 0;
    if (value) memcpy(value, &bits, 8);
    return 1;
}

extern "C" int orbx_vocabulary_tree(orbx_vocabulary *v, int32_t *k, int32_t *L, int32_t *num_nodes, int32_t *parent, uint8_t *is_leaf, uint8_t *descriptors, double *weights)
{
    if (!v) { orbx_set_error("NULL handle"); return ORBX_ERR_ARG; }
    if (k) *k = v->k;
    if (L) *L = v->L;
    if (num_nodes) *num_nodes = v->numNodes;
    if (!parent && !is_leaf && !descriptors && !weights) return ORBX_OK;
    ORBX_HIP_CHECK(hipSetDevice(v->device));
    const size_t n = (size_t)v->numNodes, nc = n - 1;
    if (weights) ORBX_HIP_CHECK(hipMemcpy(weights, v->nodeWeight.p, n * 8, hipMemcpyDeviceToHost));
    if (!parent && !is_leaf && !descriptors) return ORBX_OK;
    std::vector<VocNode> nodes(n);
    std::vector<int32_t> childList(nc);
    ORBX_HIP_CHECK(hipMemcpy(nodes.data(), v->nodes.p, n * sizeof(VocNode), hipMemcpyDeviceToHost));
    ORBX_HIP_CHECK(hipMemcpy(childList.data(), v->childList.p, nc * 4, hipMemcpyDeviceToHost));
    if (parent) parent[0] = 0;
    for (size_t i = 0; i < n; i++) {
        if (is_leaf) is_leaf[i] = nodes[i].word >= 0;
        if (parent)
            for (int c = 0; c < nodes[i].childCount; c++) parent[childList[(size_t)nodes[i].childStart + c]] = (int32_t)i;
    }
    if (descriptors) {
        std::vector<uint8_t> cdesc(nc * 32);
        ORBX_HIP_CHECK(hipMemcpy(cdesc.data(), v->childDesc.p, nc * 32, hipMemcpyDeviceToHost));
        memset(descriptors, 0, 32);      // (the root's descriptor is not part of the device tree)
        for (size_t c = 0; c < nc; c++) memcpy(descriptors + 32 * (size_t)childList[c], &cdesc[32 * c], 32);
    }
    return ORBX_OK;
}
