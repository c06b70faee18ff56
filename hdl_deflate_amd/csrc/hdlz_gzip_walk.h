// hdlz_gzip_walk.h -- the RFC 1952 header walk of one gzip member by one wave (step 1 of the member rule of include/hdlz_gunzip.h), with
// the wave's CRC-32 of the header bytes that FHCRC asks for.  Shared by hdlz_gunzip.hip (a member per stream) and hdlz_gzip_members.hip
// (the members of one file).  Loads: only bytes of z[0 .. len).
#pragma once
#include "hdlz_device.h"
#include "hdlz_crc32.h"

namespace hdlz {
namespace gunzip {

constexpr uint32_t FHCRC = 2u, FEXTRA = 4u, FNAME = 8u, FCOMMENT = 16u, FRESERVED = 0xE0u;      // (FTEXT, bit 0, is ignored)

// the crc32 of z[0 .. H) by one wave -> every lane's return value.  Lane l runs the strip [l S, (l + 1) S) of the bytes RIGHT-aligned
// in 64 S (the zero bytes in front are free), a bit a step; the tree multiplies the earlier neighbour by x^(8 S 2^k), as crc_tile_word does
__device__ __forceinline__ uint32_t wave_crc32(const uint8_t* __restrict__ z, uint32_t H) {
    const uint32_t lane = threadIdx.x & 63u, S = (H + 63u) >> 6, pad = 64u * S - H;
    uint32_t c = 0;
    for (uint32_t v = lane * S; v < (lane + 1u) * S; v++)
        if (v >= pad) c = crc_byte(c, z[v - pad]);
    uint32_t m = crc_xpow(8ull * S);
#pragma unroll
    for (uint32_t k = 0; k < 6u; k++) {
        c = crc_mul(c, m) ^ (uint32_t)__shfl_down((int)c, 1u << k, 64);
        m = crc_mul(m, m);
    }
    c = (uint32_t)__shfl((int)c, 0, 64);
    return c ^ crc_mul(CRC_INIT, crc_xpow(8ull * H)) ^ CRC_INIT;
}

// the header walk of one member: z[0 .. len) -> the verdict; p = the offset of the first payload byte when it is HDLZ_OK
__device__ __forceinline__ uint32_t walk(const uint8_t* __restrict__ z, uint64_t len, uint64_t& p) {
    const uint32_t lane = threadIdx.x & 63u;
    if (len < 10u) return HDLZ_E_NO_EOF;
    const uint32_t flg = z[3];
    if (z[0] != 0x1Fu || z[1] != 0x8Bu || z[2] != 8u || (flg & FRESERVED)) return HDLZ_E_BAD_HEADER;
    uint64_t pos = 10u;                                   // (MTIME, XFL, OS: skipped)
    if (flg & FEXTRA) {
        if (pos + 2u > len) return HDLZ_E_NO_EOF;
        const uint32_t xlen = (uint32_t)z[pos] | ((uint32_t)z[pos + 1u] << 8);
        pos += 2u;
        if (pos + xlen > len) return HDLZ_E_NO_EOF;
        pos += xlen;
    }
#pragma unroll 1
    for (uint32_t field = FNAME; field <= FCOMMENT; field <<= 1) {
        if (!(flg & field)) continue;
        for (;;) {                                        // 64 bytes a step; nothing at or behind len is loaded
            if (pos >= len) return HDLZ_E_NO_EOF;         // unterminated
            const uint64_t q = pos + lane;
            const uint64_t zero = ballot64(q < len && z[q] == 0u);
            if (zero) { pos += (uint32_t)__builtin_ctzll(zero) + 1u; break; }
            pos += 64u;
        }
    }
    if (flg & FHCRC) {
        if (pos + 2u > len) return HDLZ_E_NO_EOF;
        const uint32_t want = (uint32_t)z[pos] | ((uint32_t)z[pos + 1u] << 8);
        if ((wave_crc32(z, (uint32_t)pos) & 0xFFFFu) != want) return HDLZ_E_BAD_HEADER;
        pos += 2u;
    }
    p = pos;
    return HDLZ_OK;
}

}  // namespace gunzip
}  // namespace hdlz
