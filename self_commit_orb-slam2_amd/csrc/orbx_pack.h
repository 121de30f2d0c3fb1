// The packing stage of k_pyr_band's resize blend: four blend sums -> the four bytes of one output word.
// Header-only and free of HIP includes, so that tests/test_pyr_band_pack_host.py compiles the same text for the CPU (g++) and runs every pair of sums
// through both halves; on the device the shift and the permute are the instructions named beside them.
//
// A sum is m = ((b0 * h0) >> 16) + ((b1 * h1) >> 16) with row weights that add up to 2048 and horizontal values of at most (255 * 2049) >> 4: m + 2 < 1024,
// so two of them share a word as 16-bit lanes, the packed shift by 2 leaves each lane's pixel ((m + 2) >> 2 <= 255) in the lane's low byte, and one
// byte permute gathers the low bytes of four lanes.  The permute reads bytes 0 and 2 of each pair only: what a larger sum would carry into a lane's
// high byte is dropped, ((m + 2) >> 2) & 255 - the test runs every pair in 0 .. 1023.
#ifndef ORBX_PACK_H
#define ORBX_PACK_H

#include <stdint.h>

#ifdef __HIPCC__
#define ORBX_PACK_FN __device__ __forceinline__
#else
#define ORBX_PACK_FN static inline
#endif

// v_perm_b32: byte k of the result = byte sel[k] of the eight bytes (hi : lo), selectors 0 .. 7 (the constant and sign selectors are not used here)
ORBX_PACK_FN uint32_t orbx_byte_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; k++) r |= (uint32_t)((v >> (8 * ((sel >> (8 * k)) & 7u))) & 0xffu) << (8 * k);
    return r;
#endif
}

// two sums as the 16-bit lanes of one word, the rounding + 2 added to both lanes at once (no lane overflows: sums are below 2^16 - 2), then each lane
// shifted right by 2 (v_pk_lshrrev_b16)
ORBX_PACK_FN uint32_t orbx_pack2_round_shr2(uint32_t m0, uint32_t m1)
{
    const uint32_t w = (m1 << 16) + m0 + 0x00020002u;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short orbx_u16x2 __attribute__((ext_vector_type(2)));
    union { uint32_t u; orbx_u16x2 v; } x;
    x.u = w;
    x.v = x.v >> (orbx_u16x2)(2);
    return x.u;
#else
    return ((w & 0xffffu) >> 2) | ((w >> 16) >> 2 << 16);
#endif
}

// the output word of four sums: pixel k = ((m_k + 2) >> 2) & 255 in byte k
ORBX_PACK_FN uint32_t orbx_pack4_round_shr2(uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3)
{
    return orbx_byte_perm(orbx_pack2_round_shr2(m2, m3), orbx_pack2_round_shr2(m0, m1), 0x06040200u);
}

#endif
