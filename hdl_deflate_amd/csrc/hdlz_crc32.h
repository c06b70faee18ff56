// hdlz_crc32.h -- CRC-32 (the one of zlib, gzip and PNG) without a carry-less multiply: the one copy of the arithmetic, the tile loop
// and the tree that hdlz_crc32_ws (hdlz_crc32.hip), the gzip judgement of hdlz_unjoin_gzip_ws (hdlz_unjoin.hip) and the per-block
// checksums of hdlz_crc32_batch_ws (hdlz_bgzf.hip: crc_block, a workgroup per block) share.
//
// Arithmetic.  Bytes are polynomials over GF(2), lowest bit first; a 32-bit word w stands for w(x) with bit 31 = x^0 .. bit 0 = x^31
// (zlib's "reflected" register), P = x^32 + 0xEDB88320(x), `*` is the product mod P (crc_mul: 32 shift-and-xor steps; with one
// operand a compile-time constant the shifted copies fold to 32 constants).  raw(D) = D(x) * x^32 mod P is the register after the
// bytes D from a register of 0.  Three facts carry everything:
//     raw(zeros + D) = raw(D)                              leading zero bytes are free
//     raw(A + B)     = raw(A) * x^(8 |B|)  ^  raw(B)        appending L bytes multiplies by x^(8 L)
//     crc32(D)       = raw(D) ^ FFFFFFFF * x^(8 |D|) ^ FFFFFFFF        the initial register is a word IN FRONT of the data
// and P is primitive, so x^(2^32 - 1) = 1: x^(-e) = x^(2^32 - 1 - e), and x^(2^k) depends on k mod 32 only.  Every multiplier below is
// one entry of XP2[k] = x^(2^k), k = 0 .. 31.
//
// The combination rule (stated in Python in tests/gzip_ref.py and held against zlib.crc32 there):
//   a LANE   runs a contiguous strip of 128 bytes from a register of 0, a dword a step, through slice-by-4 tables in LDS;
//   a WAVE   merges its 64 strips by a tree: at level k the earlier of two neighbours is multiplied by x^(8 * 128 * 2^k) = XP2[10 + k]
//            and the later one added (k = 0 .. 5); the workgroup's four waves the same way with XP2[16], XP2[17]: one word per
//            TILE of 32 KiB.  A short last tile is padded with zero bytes BEHIND it: every tile is the same code;
//   the FINISH workgroup numbers the tile words from the END, j = 0 for the last tile, and puts one more word, FFFFFFFF (the
//            initial register), at j = ntiles: R = xor_j w_j * x^(8 * 32768 * j).  Thread i takes j = i, i + 1024, .. from the
//            far end (Horner with XP2[28]; the words in front of the data are zero and free), then the 1024 threads merge by the
//            same tree, level k with x^(8 * 32768 * 2^k) = XP2[18 + k], k = 0 .. 9.  The zero padding of the last tile,
//            pad = 32768 ntiles - n bytes, is taken back by ONE multiplication with x^(-8 pad), a product of XP2 entries picked
//            by the bits of the exponent (32 lanes, a product tree).  crc32 = R * x^(-8 pad) ^ FFFFFFFF.
//   n = 0: no tile, R = FFFFFFFF, pad = 0: crc32 = 0.
// Work per 2 GiB (65536 tiles): 64 Horner steps a thread and ten tree levels: no serial walk over the tiles.
//
// LDS.  A tile is staged by coalesced 16-byte loads (any alignment; the last piece of the data by bytes: nothing at or behind n is
// loaded, the tail rule of load_chunk<A16, false> in hdlz_adler.h) into strips of 33 dwords: lane t's dword w sits in bank
// (33 t + w) mod 64, so the 64 strip reads of a step hit 64 banks.  The four 1 KiB tables are built in the prologue from P.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hdlz {

constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t CRC_ONE = 0x80000000u;            // x^0
constexpr uint32_t CRC_INIT = 0xFFFFFFFFu;           // the initial register, and the final xor
constexpr uint32_t CRC_TILE = 32768u, CRC_TILE_LOG2 = 15u;      // bytes per workgroup and tile word
constexpr uint32_t CRC_THREADS = 256u, CRC_STRIP = CRC_TILE / CRC_THREADS, CRC_STRIP_WORDS = CRC_STRIP / 4u;
constexpr uint32_t CRC_STRIP_PITCH = CRC_STRIP_WORDS + 1u;      // dwords between two strips in LDS: odd, so a step's reads spread over all banks
constexpr uint32_t CRC_STEPS = CRC_TILE / (16u * CRC_THREADS);  // 16-byte pieces a thread stages per tile
constexpr uint32_t CRC_FIN_THREADS = 1024u, CRC_FIN_LOG2 = 10u;
constexpr uint32_t CRC_GRID_MAX = 1024u;             // workgroups of the tile kernels: four a CU (37 KiB of LDS each) on 256 CUs; the rest is the grid stride
static_assert(CRC_STRIP == 128u && CRC_STEPS == 8u && CRC_STRIP % 16u == 0u, "a 16-byte piece lies inside one strip");

// a * b mod P (zlib's multmodp): bit 31 of a is x^0
__host__ __device__ __forceinline__ constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll
    for (int i = 31; i >= 0; i--) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
// XP2.v[k] = x^(2^k) mod P
struct CrcPowers { uint32_t v[32]; };
constexpr CrcPowers crc_powers() {
    CrcPowers t{};
    t.v[0] = CRC_ONE >> 1;
    for (int k = 1; k < 32; k++) t.v[k] = crc_mul(t.v[k - 1], t.v[k - 1]);
    return t;
}
constexpr CrcPowers XP2 = crc_powers();
// x^e mod P for any e (square-and-multiply over XP2; the host's and the static_asserts' form -- the kernels spread it over 32 lanes)
__host__ __device__ constexpr uint32_t crc_xpow(uint64_t e) {
    uint32_t r = CRC_ONE;
    for (uint32_t k = 0; e; k++, e >>= 1)
        if (e & 1u) r = crc_mul(r, XP2.v[k & 31u]);
    return r;
}
// the exponent of x^(-8 pad), pad < 2^28
__host__ __device__ constexpr uint32_t crc_unpad_exponent(uint32_t pad) { return 0xFFFFFFFFu - 8u * pad; }
// the register after one more byte (the table entry's definition)
__host__ __device__ constexpr uint32_t crc_byte(uint32_t c, uint32_t b) {
    c ^= b;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
    return c;
}
__host__ __device__ constexpr uint32_t crc_raw(const char* s, uint32_t n) {
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; i++) c = crc_byte(c, (uint8_t)s[i]);
    return c;
}
// the finishing rule at compile time: the tile words of n bytes, in the data's order -> crc32, as crc_finish computes it
constexpr uint32_t crc_from_words(const uint32_t* w, uint32_t ntiles, uint64_t n) {
    uint32_t R = crc_mul(CRC_INIT, crc_xpow((uint64_t)ntiles << (CRC_TILE_LOG2 + 3u)));      // j = ntiles: the initial register
    for (uint32_t j = 0; j < ntiles; j++) R ^= crc_mul(w[ntiles - 1u - j], crc_xpow((uint64_t)j << (CRC_TILE_LOG2 + 3u)));
    return crc_mul(R, crc_xpow(crc_unpad_exponent((uint32_t)((uint64_t)ntiles * CRC_TILE - n)))) ^ CRC_INIT;
}
struct CrcWords { uint32_t w[3]; };

// Pinned against zlib.crc32 (values computed there).
static_assert(crc_xpow(0xFFFFFFFFull) == CRC_ONE, "x has an order that divides 2^32 - 1: x^-e = x^(2^32 - 1 - e)");
static_assert(XP2.v[31] != CRC_ONE && crc_mul(XP2.v[31], XP2.v[31]) == XP2.v[0], "x^(2^32) = x");
static_assert(crc_mul(0x12345678u, CRC_ONE) == 0x12345678u && crc_mul(CRC_ONE >> 31, CRC_ONE >> 1) == CRC_POLY, "1 is the unit; x^31 * x = P - x^32");
static_assert(crc_byte(0u, 1u) == 0x77073096u && crc_byte(0u, 255u) == 0x2D02EF8Du, "the byte table's entries 1 and 255");
static_assert((crc_raw("123456789", 9u) ^ crc_mul(CRC_INIT, crc_xpow(72u)) ^ CRC_INIT) == 0xCBF43926u, "\"123456789\": the initial register as a word in front");
static_assert(crc_raw("\0\0\0a", 4u) == crc_raw("a", 1u), "leading zero bytes are free");
static_assert(crc_raw("ab", 2u) == (crc_mul(crc_raw("a", 1u), crc_xpow(8u)) ^ crc_raw("b", 1u)), "appending a byte");
// (tile words from tests/gzip_ref.py's tile_word: raw() of the tile with zeros behind it)
static_assert(crc_from_words(CrcWords{}.w, 0u, 0u) == 0u, "empty");
static_assert(crc_from_words(CrcWords{{0xB016FF7Du}}.w, 1u, 9u) == 0xCBF43926u, "\"123456789\" as one short tile: 32759 bytes of padding taken back");
static_assert(crc_from_words(CrcWords{{0u}}.w, 1u, 32768u) == 0x011FFCA6u, "32768 zero bytes: only the length speaks");
static_assert(crc_from_words(CrcWords{{0x1A5C161Bu, 0x1A5C161Bu}}.w, 2u, 65536u) == 0xDEAB7E4Eu, "65536 bytes of FF as two tiles");
static_assert(crc_from_words(CrcWords{{0x77C1D66Bu, 0x77C1D66Bu, 0xB62801A5u}}.w, 3u, 70001u) == 0x5C5C297Au, "70001 bytes (7 p + 3) & 255: three tiles, the last short");

#ifdef __HIPCC__
typedef uint32_t crc_u32x4 __attribute__((ext_vector_type(4)));
typedef crc_u32x4 __attribute__((aligned(1))) crc_u32x4u;

// what a workgroup of CRC_THREADS threads needs in LDS, and one step of a strip: the register after the next dword.
// -DHDLZ_CRC_BANK_PRIVATE (build.sh crcbank) is the other layout: ONE table with a copy per lane, table[b][lane], so that a lookup
// always goes to the lane's own bank -- at 64 KiB for the one table: a byte a lookup in a chain four times as long, and one workgroup
// per CU where the sliced tables let four run.  Measured (profiles/gzip_joined.txt): 2.4 x the sliced tables' time, and
// SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of the whole kernel 0.54 against 0.57.  The sliced tables are the default.
#ifdef HDLZ_CRC_BANK_PRIVATE
struct CrcTileLds {
    uint32_t table[256][64];
    uint32_t strip[CRC_THREADS * CRC_STRIP_PITCH];
    uint32_t wave[CRC_THREADS / 64u];
};
__device__ __forceinline__ void crc_build_tables(CrcTileLds& s) {
    const uint32_t c = crc_byte(threadIdx.x, 0u);
    for (uint32_t l = 0; l < 64u; l++) s.table[threadIdx.x][l] = c;
}
__device__ __forceinline__ uint32_t crc_step(const CrcTileLds& s, uint32_t c, uint32_t word) {
    c ^= word;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) c = s.table[c & 255u][threadIdx.x & 63u] ^ (c >> 8);
    return c;
}
#else
struct CrcTileLds {
    uint32_t table[4][256];                           // table[k][b]: the register after byte b and k zero bytes
    uint32_t strip[CRC_THREADS * CRC_STRIP_PITCH];
    uint32_t wave[CRC_THREADS / 64u];
};
// the four tables, from P; the caller synchronises before the first lookup
__device__ __forceinline__ void crc_build_tables(CrcTileLds& s) {
    uint32_t c = threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        c = crc_byte(c, 0u);
        s.table[k][threadIdx.x] = c;
    }
}
__device__ __forceinline__ uint32_t crc_step(const CrcTileLds& s, uint32_t c, uint32_t word) {
    c ^= word;
    return s.table[3][c & 255u] ^ s.table[2][(c >> 8) & 255u] ^ s.table[1][(c >> 16) & 255u] ^ s.table[0][c >> 24];
}
#endif
// the 16-byte piece at byte q of a tile of tn bytes: zero at and behind tn, and nothing loaded there
__device__ __forceinline__ crc_u32x4 crc_load_piece(const uint8_t* __restrict__ p, uint32_t q, uint32_t tn) {
    crc_u32x4 v = {0u, 0u, 0u, 0u};
    if (q + 16u <= tn) v = *reinterpret_cast<const crc_u32x4u*>(p + q);
    else if (q < tn) {
        uint32_t d[4] = {0u, 0u, 0u, 0u};
        for (uint32_t i = 0; q + i < tn; i++) d[i >> 2] |= (uint32_t)p[q + i] << (8u * (i & 3u));
        v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3];
    }
    return v;
}
__device__ __forceinline__ uint32_t crc_piece_at(uint32_t k) {      // coalesced: a wave's 64 pieces are 1 KiB in a row
    return ((threadIdx.x >> 6) * CRC_STEPS + k) * 1024u + 16u * (threadIdx.x & 63u);
}

// the staged pieces of a tile -> its strips in LDS (piece k of this thread is the one crc_piece_at(k) names)
__device__ __forceinline__ void crc_stage(CrcTileLds& s, const crc_u32x4 (&piece)[CRC_STEPS]) {
#pragma unroll
    for (uint32_t k = 0; k < CRC_STEPS; k++) {
        const uint32_t q = crc_piece_at(k);
        uint32_t* d = &s.strip[(q >> 7) * CRC_STRIP_PITCH + ((q & 127u) >> 2)];
        d[0] = piece[k].x; d[1] = piece[k].y; d[2] = piece[k].z; d[3] = piece[k].w;
    }
}
// raw() of the staged tile -> the return value of thread 0 (other threads: 0).  The strips in front of `first_strip` are taken as
// zeros without being read (a register of 0 stays 0 over zero bytes).  The caller synchronises between the staging and this call;
// the synchronisation in here is behind the last read of a strip: the next tile may be staged as soon as the call returns.
__device__ __forceinline__ uint32_t crc_tile_word(CrcTileLds& s, uint32_t first_strip) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t c = 0;
    if (tid >= first_strip) {
        const uint32_t* mine = &s.strip[tid * CRC_STRIP_PITCH];
#pragma unroll 8
        for (uint32_t w = 0; w < CRC_STRIP_WORDS; w++) c = crc_step(s, c, mine[w]);
    }
    // the wave's 64 strips: lane l keeps strips l .. l + 2^(k+1) - 1 after level k
#pragma unroll
    for (uint32_t k = 0; k < 6u; k++) c = crc_mul(c, XP2.v[10u + k]) ^ (uint32_t)__shfl_down((int)c, 1u << k, 64);
    if (lane == 0u) s.wave[wave] = c;
    __syncthreads();                                  // (every strip has been read: the next tile may be staged)
    uint32_t word = 0;
    if (tid == 0u) {
        const uint32_t lo = crc_mul(s.wave[0], XP2.v[16]) ^ s.wave[1], hi = crc_mul(s.wave[2], XP2.v[16]) ^ s.wave[3];
        word = crc_mul(lo, XP2.v[17]) ^ hi;
    }
    return word;
}

// raw() of every 32 KiB tile of data[0 .. n) (the last one padded with zeros behind it) -> words[t], tiles blockIdx.x, + gridDim.x, ..
// Launched with CRC_THREADS threads.  reads: data[0 .. n) only.  writes: words[0 .. ceil(n / 32768)).
__device__ __forceinline__ void crc_tiles(const uint8_t* __restrict__ data, uint64_t n, uint32_t* __restrict__ words, CrcTileLds& s) {
    const uint32_t tid = threadIdx.x;
    const uint64_t ntiles = (n + CRC_TILE - 1u) >> CRC_TILE_LOG2;
    uint64_t t = blockIdx.x;
    if (t >= ntiles) return;
    crc_build_tables(s);
    crc_u32x4 piece[CRC_STEPS];
    auto fetch = [&](uint64_t tile) {
        const uint64_t base = tile << CRC_TILE_LOG2;
        const uint32_t tn = n - base < CRC_TILE ? (uint32_t)(n - base) : CRC_TILE;
#pragma unroll
        for (uint32_t k = 0; k < CRC_STEPS; k++) piece[k] = crc_load_piece(data + base, crc_piece_at(k), tn);
    };
    fetch(t);
    for (; t < ntiles; t += gridDim.x) {
        crc_stage(s, piece);
        __syncthreads();                              // the tile is staged (and, the first time, the tables are built)
        if (t + gridDim.x < ntiles) fetch(t + gridDim.x);      // the next tile's loads fly while this one is computed
        const uint32_t word = crc_tile_word(s, 0u);
        if (tid == 0u) words[t] = word;
    }
}

// crc32 of the L bytes at p (any alignment, L < 2^32) -> the return value of thread 0 (other threads: unspecified): ONE workgroup of
// CRC_THREADS threads walks the block tile by tile (hdlz_crc32_batch_ws: a workgroup per block of a batch).  The first tile is the
// PARTIAL one, r = L - 32768 (ntiles - 1) bytes placed RIGHT-ALIGNED: the pad = 32768 - r zero bytes stand in front of the data, where
// they are free -- no un-padding product --, and a strip that lies wholly inside them is neither staged nor run.  Every further tile
// is whole: one Horner step c * x^(8 * 32768) ^ tile (XP2[18]).  The initial register is a word in front, FFFFFFFF * x^(8 L) -- the
// exponent reduced mod 2^32 - 1 (x^(2^32 - 1) = 1) and spread over 32 lanes as in crc_finish --, and the final xor comes last.
// The tables must be built (crc_build_tables) in front of the call; the first synchronisation in here covers them.
// reads: p[0 .. L) only.
__device__ __forceinline__ uint32_t crc_block(const uint8_t* __restrict__ p, uint32_t L, CrcTileLds& s) {
    const uint32_t tid = threadIdx.x;
    if (L == 0u) return 0u;
    const uint32_t ntiles = ((L - 1u) >> CRC_TILE_LOG2) + 1u;
    const uint32_t r = L - ((ntiles - 1u) << CRC_TILE_LOG2), pad = CRC_TILE - r;      // r = 1 .. 32768
    const uint32_t first_strip = pad / CRC_STRIP;      // strips in front of it hold padding only
    uint32_t acc = 0;
    crc_u32x4 piece[CRC_STEPS];
    for (uint32_t t = 0; t < ntiles; t++) {
        if (t == 0u) {
#pragma unroll
            for (uint32_t k = 0; k < CRC_STEPS; k++) {
                const uint32_t q = crc_piece_at(k);
                crc_u32x4 v = {0u, 0u, 0u, 0u};
                if (q >= pad) v = *reinterpret_cast<const crc_u32x4u*>(p + (q - pad));      // (q + 16 <= 32768: the piece ends inside the data)
                else if (q + 16u > pad) {              // the piece the data starts in: its bytes pad - q .. 15
                    uint32_t d[4] = {0u, 0u, 0u, 0u};
                    for (uint32_t i = pad - q; i < 16u; i++) d[i >> 2] |= (uint32_t)p[q + i - pad] << (8u * (i & 3u));
                    v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3];
                }
                piece[k] = v;
            }
        } else {
            const uint8_t* __restrict__ tp = p + r + ((uint64_t)(t - 1u) << CRC_TILE_LOG2);
#pragma unroll
            for (uint32_t k = 0; k < CRC_STEPS; k++) piece[k] = *reinterpret_cast<const crc_u32x4u*>(tp + crc_piece_at(k));
        }
        crc_stage(s, piece);
        __syncthreads();
        const uint32_t word = crc_tile_word(s, t == 0u ? first_strip : 0u);
        if (tid == 0u) acc = t == 0u ? word : crc_mul(acc, XP2.v[CRC_TILE_LOG2 + 3u]) ^ word;
    }
    // FFFFFFFF * x^(8 L): 8 L = hi 2^32 + lo = hi + lo (mod 2^32 - 1)
    uint32_t e = L << 3;
    const uint32_t hi = L >> 29;
    e += hi;
    if (e < hi) e += 1u;
    uint32_t f = tid < 32u && ((e >> tid) & 1u) ? XP2.v[tid & 31u] : CRC_ONE;
    if (tid < 64u) {
#pragma unroll
        for (uint32_t o = 16u; o > 0u; o >>= 1) f = crc_mul(f, (uint32_t)__shfl_down((int)f, o, 64));
    }
    return acc ^ crc_mul(CRC_INIT, f) ^ CRC_INIT;
}

// crc32 of n bytes from their tile words -> the return value of thread 0 (other threads: unspecified).  Launched as ONE workgroup of
// CRC_FIN_THREADS threads; `s_fin`: that many words of LDS.  reads: words[0 .. ceil(n / 32768)).
__device__ __forceinline__ uint32_t crc_finish(const uint32_t* __restrict__ words, uint64_t n, uint32_t* s_fin) {
    const uint32_t tid = threadIdx.x;
    const uint64_t ntiles = (n + CRC_TILE - 1u) >> CRC_TILE_LOG2;      // word j from the end is words[ntiles - 1 - j]; j = ntiles: the initial register
    uint32_t v = 0;
    if ((uint64_t)tid <= ntiles) {
        uint64_t j = tid + ((ntiles - tid) >> CRC_FIN_LOG2 << CRC_FIN_LOG2);      // this thread's farthest word
        for (;;) {
            v = crc_mul(v, XP2.v[(CRC_TILE_LOG2 + 3u + CRC_FIN_LOG2) & 31u]) ^ (j == ntiles ? CRC_INIT : words[ntiles - 1u - j]);
            if (j < CRC_FIN_THREADS) break;
            j -= CRC_FIN_THREADS;
        }
    }
    s_fin[tid] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < CRC_FIN_LOG2; k++) {     // thread i keeps words i .. i + 2^(k+1) - 1: the FARTHER neighbour is multiplied
        if ((tid & ((2u << k) - 1u)) == 0u) s_fin[tid] ^= crc_mul(s_fin[tid + (1u << k)], XP2.v[CRC_TILE_LOG2 + 3u + k]);
        __syncthreads();
    }
    // x^(-8 pad): the product of the XP2 entries the exponent's bits pick, by a tree over the first 32 lanes
    const uint32_t pad = (uint32_t)((ntiles << CRC_TILE_LOG2) - n);
    uint32_t f = tid < 32u && ((crc_unpad_exponent(pad) >> tid) & 1u) ? XP2.v[tid & 31u] : CRC_ONE;
    if (tid < 64u) {
#pragma unroll
        for (uint32_t o = 16u; o > 0u; o >>= 1) f = crc_mul(f, (uint32_t)__shfl_down((int)f, o, 64));
    }
    return crc_mul(s_fin[0], f) ^ CRC_INIT;
}
#endif  // __HIPCC__

}  // namespace hdlz
