// hdlz_adler.h -- Adler-32 from order-free sums, and the zlib frame test: the one copy that the judging pass of hdlz_inflate_checked
// (hdlz_checksum.hip) and the judgement of hdlz_unjoin_ws (hdlz_unjoin.hip) share; the modulus is every kernel's.
// Shared only where the kernel stays the code object it was (profiles/adler_shared.txt).  What did not, as an inline function, is
// written out in its kernels and follows this comment: the eight-step tile loop (k_adler_tiles, rotated by the tile index, and
// k_unjoin_tiles), and adler32_from's two lines in k_unjoin_finish and in hdlz_compress_chunk's final step.
//
// Arithmetic.  With A = sum x_p and C = sum p * x_p over the n bytes of the data (p = 0 .. n-1),
//     s1 = (1 + A) mod 65521,   s2 = (n + n * A - C) mod 65521                    (byte p is counted n - p times in s2)
// Both sums are order-free: the 16-byte chunks are summed by whatever lane gets them and added, no ordered combine.  Per chunk at
// position p0: Sx = sum of its bytes (4 x v_sad_u8), W = sum j * x_j (4 x v_dot4_u32_u8 against the weights 0 .. 15), and
// C += p0 * Sx + W with p0 taken relative to a base that is folded in mod 65521 later (base * A_part).
//
// Bounds (all-FF data is the worst case of every line):
//   a chunk:          Sx <= 16 * 255 = 4080, W <= 255 * 120 = 30600
//   a tile loop:      positions relative to the 32 KiB tile, q < 32768: a term is <= 32767 * 4080 + 30600 < 1.34e8, a lane adds 8 of them:
//                     < 1.07e9 < 2^32; Sx: 8 * 4080.  C reduced mod 65521 per lane, then 64 lanes and 4 waves of values < 65521 (C) and
//                     < 2.1e6 (A) added in 32 bits.
//   rows mapping:     positions relative to a 64 KiB segment, q < 65536: a term is <= 65535 * 4080 + 30600 < 2^28 (q and Sx below 2^24: the
//                     24-bit multiply is exact), a lane adds 256 of them per segment into 64 bits; Sx per segment <= 256 * 4080 < 2^21.
//                     A segment folds (base mod 65521) * A_seg + C_seg < 65521 * 2^21 + 2^36 < 2^38 into 64 bits, at most 2^16 segments
//                     per row (a row of up to 2^32 - 512 bytes, what the decoders' capacity clamp allows): < 2^54.
//   per-row finish:   fold_tile adds (32768 t mod 65521) * A_t + C_t < 2^32 per tile into 64 bits; at most 2^17 tiles per row.
//   flat finish:      the same fold for up to 2^31 tiles (an output of 2^46 bytes): < 2^63.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hdlz {

constexpr uint32_t ADLER_MOD = 65521u;
constexpr uint32_t ADLER_TILE = 32768u;       // bytes a workgroup sums at a time: 4 waves x 8 steps x 64 lanes x 16 bytes
constexpr uint32_t ADLER_TILE_WAVES = 4u, ADLER_TILE_STEPS = 8u;
static_assert(ADLER_TILE == ADLER_TILE_WAVES * ADLER_TILE_STEPS * 1024u, "a tile is what its workgroup's waves cover");
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Sx and W of one chunk
__device__ __forceinline__ void sums16(const u32x4 v, uint32_t& sx, uint32_t& w) {
    sx = __builtin_amdgcn_sad_u8(v.x, 0u, 0u);
    sx = __builtin_amdgcn_sad_u8(v.y, 0u, sx);
    sx = __builtin_amdgcn_sad_u8(v.z, 0u, sx);
    sx = __builtin_amdgcn_sad_u8(v.w, 0u, sx);
    w = __builtin_amdgcn_udot4(v.x, 0x03020100u, 0u, false);
    w = __builtin_amdgcn_udot4(v.y, 0x07060504u, w, false);
    w = __builtin_amdgcn_udot4(v.z, 0x0B0A0908u, w, false);
    w = __builtin_amdgcn_udot4(v.w, 0x0F0E0D0Cu, w, false);
}
// the low min(cnt, 4) bytes of a dword (cnt as a signed count: <= 0 keeps nothing)
__device__ __forceinline__ uint32_t keep_bytes(uint32_t d, int32_t cnt) {
    return cnt >= 4 ? d : cnt <= 0 ? 0u : d & ((1u << (8u * (uint32_t)cnt)) - 1u);
}
// the dword at p of which only `cnt` bytes (1 .. 3) may be loaded
__device__ __forceinline__ uint32_t load_tail(const uint8_t* __restrict__ p, int32_t cnt) {
    uint32_t d = p[0];
    if (cnt > 1) d |= (uint32_t)p[1] << 8;
    if (cnt > 2) d |= (uint32_t)p[2] << 16;
    return d;
}
// the chunk at byte q of `p` (q a multiple of 16, below n; p 4-byte aligned, A16: 16-byte aligned): bytes at or behind n read as zero.
// PAD4: the data ends inside memory that is the caller's up to a multiple of 4 (a row, its pitch a multiple of 4), so the dword that
// holds byte n - 1 is loaded whole and masked.  Otherwise nothing at or behind n is loaded: the last dword comes in by bytes.
template <bool A16, bool PAD4>
__device__ __forceinline__ u32x4 load_chunk(const uint8_t* __restrict__ p, uint32_t q, uint32_t n) {
    u32x4 v = {0u, 0u, 0u, 0u};
    const uint32_t* d = reinterpret_cast<const uint32_t*>(p + q);
    if (q + 16u <= n) {
        if constexpr (A16) v = *reinterpret_cast<const u32x4*>(d);
        else { v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3]; }
    } else {
        const int32_t cnt = (int32_t)(n - q);                 // 1 .. 15
        if constexpr (PAD4) {
            v.x = keep_bytes(d[0], cnt);
            if (cnt > 4) v.y = keep_bytes(d[1], cnt - 4);
            if (cnt > 8) v.z = keep_bytes(d[2], cnt - 8);
            if (cnt > 12) v.w = keep_bytes(d[3], cnt - 12);
        } else {
            auto part = [&](int32_t k) -> uint32_t {
                const int32_t c = cnt - 4 * k;
                return c >= 4 ? d[k] : c > 0 ? load_tail(p + q + 4 * k, c) : 0u;
            };
            v.x = part(0); v.y = part(1); v.z = part(2); v.w = part(3);
        }
    }
    return v;
}

// (A, C) += the sums (At, Ct) of tile t, both below 65521 (t < 2^31: t mod 65521 times 32768 stays below 2^32)
__host__ __device__ __forceinline__ constexpr void fold_tile(uint64_t& A, uint64_t& C, uint32_t t, uint32_t At, uint32_t Ct) {
    const uint32_t base = ((t % ADLER_MOD) * (ADLER_TILE % ADLER_MOD)) % ADLER_MOD;
    A += At;
    C += (uint64_t)base * At + Ct;
}
// the checksum of n bytes from their residues A and C
template <class N>
__host__ __device__ __forceinline__ constexpr uint32_t adler32_from(uint32_t A, uint32_t C, N n) {
    const uint32_t nm = (uint32_t)(n % ADLER_MOD);
    const uint32_t s1 = (1u + A) % ADLER_MOD;
    const uint32_t s2 = (uint32_t)(((uint64_t)nm + (uint64_t)nm * A + ADLER_MOD - C) % ADLER_MOD);
    return (s2 << 16) | s1;
}
// RFC 1950's two header bytes as this library accepts them: deflate, a window of at most 32 KiB, FCHECK, no preset dictionary.
// The kernels test HDLZ_ZLIB_HEADER_BAD in place: through a function's bool the compiler folds the four tests another way, and
// k_adler_rows, k_adler_finish and k_unjoin_finish stop being the code objects they were (profiles/adler_shared.txt).
#define HDLZ_ZLIB_HEADER_BAD(cmf, flg) (((cmf) & 15u) != 8u || ((cmf) >> 4) > 7u || ((cmf) * 256u + (flg)) % 31u != 0u || ((flg) & 0x20u) != 0u)
__host__ __device__ __forceinline__ constexpr bool zlib_header_ok(uint32_t cmf, uint32_t flg) { return !HDLZ_ZLIB_HEADER_BAD(cmf, flg); }
__host__ __device__ __forceinline__ uint32_t load_be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// Pinned against zlib.adler32 and zlib.decompressobj (values computed there, A and C from their definitions above).
static_assert(adler32_from(0u, 0u, 0u) == 0x00000001u, "the empty input");
static_assert(adler32_from(919u, 3698u, 9u) == 0x11E60398u, "Wikipedia");
static_assert(adler32_from(14035u, 61651u, 70001u) == 0xC54F36D4u, "70001 bytes (7 p + 3) & 255: n is reduced");
static_assert(adler32_from(39773u, 51965u, 98309u) == 0xE67D9B5Eu, "98309 bytes of FF");
static_assert(adler32_from(0u, 0u, 65521u) == 0x00000001u, "65521 bytes of FF: every residue is 0");
// (a full tile of FF: A_t = 32768 * 255 = 34673, C_t = 255 * (0 + .. + 32767) = 30786 mod 65521)
static_assert([] { uint64_t A = 0, C = 0; fold_tile(A, C, 0u, 34673u, 30786u); fold_tile(A, C, 1u, 34673u, 30786u);
                   return adler32_from((uint32_t)(A % ADLER_MOD), (uint32_t)(C % ADLER_MOD), 2u * ADLER_TILE); }() == 0x77970EF2u, "65536 bytes of FF as two tiles");
static_assert(zlib_header_ok(0x78u, 0x9Cu) && zlib_header_ok(0x78u, 0x01u) && zlib_header_ok(0x78u, 0xDAu), "the usual headers");
static_assert(!zlib_header_ok(0x78u, 0x9Du), "FCHECK");
static_assert(!zlib_header_ok(0x78u, 0xBBu), "FDICT (FCHECK holds)");
static_assert(!zlib_header_ok(0x88u, 0x1Cu), "CINFO 8 (FCHECK holds)");
static_assert(!zlib_header_ok(0x79u, 0x9Cu) && !zlib_header_ok(0x79u, 0x94u), "CM 9 (without and with FCHECK)");

}  // namespace hdlz
