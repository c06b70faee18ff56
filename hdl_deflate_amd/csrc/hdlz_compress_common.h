// hdlz_compress_common.h -- constants, device helpers and THE TILE PHASES shared by all compress kernels
// (hdlz_compress.hip: one block per wave, any size; hdlz_compress_small.hip: several small blocks per wave-tile;
//  hdlz_compress_stream.hip: one large stream / a few large blocks spread over the whole GPU)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_adler.h"                  // ADLER_MOD

namespace hdlz {

// waves per SIMD the CWINDOW <= 32 kernels are register-capped for (96 VGPRs at 5)
#ifndef HDLZ_W1
#define HDLZ_W1 5
#endif

#ifndef HDLZ_EXT_GROUP
#define HDLZ_EXT_GROUP 4
#endif
#ifndef HDLZ_CODE_GROUP
#define HDLZ_CODE_GROUP 4
#endif
constexpr int RUN = 32;             // positions per lane
constexpr int TILE = 64 * RUN;      // 2048 positions per wave-tile
constexpr int HALO = 256;           // bytes kept in front of the tile (max CWINDOW)
constexpr int LOOKAHEAD = 16;       // bytes staged behind the tile (need p+9 and p+2)
constexpr int IN_BYTES = HALO + TILE + LOOKAHEAD;   // 2320
constexpr int OUT_WORDS = 592;      // 9 bits * 2048 = 576 words + carry word + slack
constexpr int LUT_LIT = 256;        // [byte]                                  at LUT word 0
constexpr int LUT_MATCH = 256;      // [len-3][dist-1] (CWINDOW <= 32) or [dist-1]  at LUT word 256
constexpr uint32_t LUT_MATCH_BYTE = 4u * LUT_LIT;
constexpr int LUT_LEN = 16;         // [len-1] -> the length code (wide windows: the match LUT is [dist-1] only)   at LUT word 512
constexpr uint32_t LUT_LEN_BYTE = 4u * (LUT_LIT + LUT_MATCH);
// LUT entry = code << CODE_SHIFT | nbits << NB_SHIFT: the bit count in the LOW bits (0..4; 5..8 are zero), the code from bit 9 up.  A sum of
// entries then carries the sum of their counts in its low 9 bits -- carries of the code field go upward only -- so token_codes adds
// whole entries and masks once per lane instead of shifting and adding per position.  A lane's counts sum to at most 32 * 9 = 288 bits
// (32 nine-bit literals; a match's 18 bits -- the widest, CWINDOW 256 -- cover at least three positions, 6 bits per position).
// One entry's code is at most 18 bits: 9 + 18 = 27 bits of the word.
constexpr uint32_t NB_SHIFT = 0;
constexpr uint32_t CODE_SHIFT = 9;
constexpr uint32_t NB_MASK = 31u << NB_SHIFT;                   // a count is at most 18
constexpr uint32_t NB_SUM_MASK = ((1u << CODE_SHIFT) - 1u) << NB_SHIFT;      // the field a lane's sum of counts lives in
static_assert(NB_SHIFT == 0 && 32u * 9u <= NB_SUM_MASK && 18u <= NB_MASK, "a lane's 288 bits at most fit below the code field; carries of the codes leave them alone");
static_assert(CODE_SHIFT + 18u <= 32u, "the widest code (7 + 5 + 6 bits) inside the entry");

struct __attribute__((aligned(16))) WaveLds {
    uint32_t in[IN_BYTES / 4];      // byte index = position - tile_start + HALO
    uint32_t out[OUT_WORDS];        // bit buffer of the current tile
    uint32_t lut[LUT_LIT + LUT_MATCH + LUT_LEN];
};

constexpr uint32_t GATHER_SPAN = 4u * (0x3FFu + 3u);      // bytes behind `in` that make_tokens' masked gather may touch (GMASK = 0x3FF)
static_assert(sizeof(WaveLds) >= GATHER_SPAN, "make_tokens: masked gather inside the LDS block");

// ---- the one-tile kernels with the bit-sliced search (k_compress<1, ., true>): THE SEARCH'S MISMATCH WORDS are the extension.
// For every distance d match_search_bits computes neq_d -- bit j = byte j of the lane's run differs from the byte d positions earlier --
// and the match length at position i is the run of zero bits of (neq_d of the next lane : neq_d) from bit i + 3 on.  The search keeps the
// words: NEQ[(d & 31) * 64 + lane], one ds_write_b32 per distance at a fixed address register + immediate offset; make_tokens_bits reads
// the word of the position's distance back (column = lane: bank = lane, conflict-free whatever the rows) instead of gathering and
// comparing bytes.  d = 32 aliases row 0 (no distance 0 exists); "none" (result byte 0xFF) reads row 31, inside the array, and is discarded.
// The LDS timeline of a tile:   stage: in | own bytes -> registers | search: NEQ | extend: NEQ | fixed LUT -> lut (LDS-DMA), zero: out |
// parse, chain | codes: lut | scatter, flush: out.   NEQ is the whole LDS budget of a wave (8192 bytes.  A CU holds 18 such waves, not the 20 its
// registers allow: the LDS of a workgroup is granted in steps of 1280 bytes, 8192 occupy 8960 and 18 x 8960 fill the 160 KB.  7680 bytes
// would give 20; workgroups of five or ten waves, whose LDS is a whole number of steps, hold 12 and 10 -- tools/ubench/wave_launch.hip,
// profiles/wave_groups.txt), so the staged
// tile in front of the search and the bit buffer + the LUT behind the extension share its memory.
constexpr int NEQ_ROWS = 32;                              // row = d & 31
constexpr int NEQ_WORDS = NEQ_ROWS * 64;                  // [row][lane]
constexpr int FIXED_LUT_WORDS = LUT_LIT + LUT_MATCH;      // the 512 entries these kernels use (LUT_LEN belongs to the wide windows)
constexpr bool search_bits() {                            // -DHDLZ_SEARCH_KEYS: the key search + WaveLds + the byte-gather make_tokens, for A/B
#ifdef HDLZ_SEARCH_KEYS
    return false;
#else
    return true;
#endif
}
struct __attribute__((aligned(16))) WaveLdsBits {
    union {
        uint32_t in[IN_BYTES / 4];      // the staged tile, until load_own has read the runs
        uint32_t neq[NEQ_WORDS];        // the mismatch words, from the search to the end of the extension
        struct {
            uint32_t out[OUT_WORDS];    // bit buffer of the tile, zeroed once the extension is through
            uint32_t gap[NEQ_WORDS - OUT_WORDS - FIXED_LUT_WORDS];
            uint32_t lut[FIXED_LUT_WORDS];      // FIXED_LUT, fetched once the extension is through
        };
    };
};
// make_tokens_bits reads byte (d4 & 0x7C) * 64 + 4 * column, d4 = 4 d (d = 1 .. 32) or 0xFF, column = lane or min(lane + 1, 63)
static_assert((0x7C << 6) + 4 * 63 + 4 <= 4 * NEQ_WORDS && ((0xFF & 0x7C) << 6) == 4 * 64 * 31, "every read of the extension inside NEQ; none -> row 31");
static_assert(((4 * 32) & 0x7C) == 0 && (31 * 64 + 63) < NEQ_WORDS, "d = 32 aliases row 0; the search's last row ends inside NEQ");
static_assert(sizeof(WaveLdsBits) == 8192 && 4 * NEQ_WORDS >= IN_BYTES, "seven allocation steps of 1280 bytes: 18 waves per CU; the staged tile inside the block");
static_assert(offsetof(WaveLdsBits, lut) >= 4 * OUT_WORDS && offsetof(WaveLdsBits, lut) % 16 == 0 && 4 * FIXED_LUT_WORDS == 2 * 64 * 16,
              "zero_bit_buffer leaves the LUT alone; the LUT is two 16-byte LDS-DMA requests per lane");

struct __attribute__((aligned(16))) WaveLdsNoOut {       // kernels with the hash finder: the bit buffer lives in HashLds::D's memory
    uint32_t in[IN_BYTES / 4];
    uint32_t lut[LUT_LIT + LUT_MATCH + LUT_LEN];
};

// fence for the instruction scheduler + value fences: keep independent phases from being overlapped
// (that blew the VGPR budget to 239 and spilled ~200 SGPR lane masks in the first version)
#define PHASE_FENCE() __builtin_amdgcn_sched_barrier(0)
// a comment in the ISA at a phase boundary (tools/phase_count.py counts the instructions between two marks)
#define HDLZ_MARK(name) do { PHASE_FENCE(); asm volatile("; @@PHASE " name ::: "memory"); PHASE_FENCE(); } while (0)
template <int N>
__device__ __forceinline__ void pin(uint32_t (&a)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++) asm volatile("" : "+v"(a[i]));
}
template <int B, int E, int N>
__device__ __forceinline__ void pin_range(uint32_t (&a)[N]) {
#pragma unroll
    for (int i = B; i < E; i++) asm volatile("" : "+v"(a[i]));
}

__device__ __forceinline__ uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
    return __builtin_amdgcn_alignbyte(hi, lo, sh);      // bytes [sh, sh+4) of hi:lo
}
__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t t = a < b ? a : b;
    return t < c ? t : c;
}
// index of the lowest set bit, 0xFFFFFFFF for 0 (v_ffbl_b32)
__device__ __forceinline__ uint32_t ffbl(uint32_t x) { return (uint32_t)(__builtin_ffs((int)x) - 1); }

// key of the 3-byte string at byte J of d[]: bytes 1..3 = the string, byte 0 = tag (4 * window index)
template <int J>
__device__ __forceinline__ uint32_t key3(const uint32_t* d, uint32_t tag) {
    constexpr int w = J >> 2, sh = J & 3;
    if constexpr (sh == 0) return (d[w] << 8) | tag;
    else if constexpr (sh == 1) return (d[w] & 0xFFFFFF00u) | tag;
    else return (alignbyte(d[w + 1], d[w], sh - 1) & 0xFFFFFF00u) | tag;
}

// ---- fixed Huffman token bits (used to fill the LUTs) ---------------------------------------
// literal (R7, deflate.py:1005-1016 + out_codes :112-149): sym<144 -> 8 bits rev8(0x30+sym),
// else 9 bits rev9(0x100+sym)
__host__ __device__ constexpr uint32_t literal_entry(uint32_t b) {
    const bool big = b >= 144u;
    const uint32_t v = big ? (0x100u + b) : (0x30u + b);
    const uint32_t nb = big ? 9u : 8u;
    return ((__builtin_bitreverse32(v) >> (32u - nb)) << CODE_SHIFT) | (nb << NB_SHIFT);
}
// distance part of a match token (R6, deflate.py:836-882): rev5(dist code) | extra<<5 in 5+eb bits,
// placed behind the 7-bit length code; nbits = 12 + eb
__host__ __device__ constexpr uint32_t dist_entry(uint32_t d) {
    const uint32_t dd = d - 1u;
    uint32_t c = dd, eb = 0, extra = 0;
    if (dd >= 4u) {
        const uint32_t hb = 31u - (uint32_t)__builtin_clz(dd);
        eb = hb - 1u;
        c = 2u * hb + ((dd >> eb) & 1u);
        extra = dd & ((1u << eb) - 1u);
    }
    const uint32_t dcode = __builtin_bitreverse32(c) >> 27;
    return (((dcode | (extra << 5)) << 7) << CODE_SHIFT) | ((12u + eb) << NB_SHIFT);
}
// 7-bit code of length symbol 254+m (no extra bits for m <= 10), in the code field; it carries no count (dist_entry's covers it)
__host__ __device__ constexpr uint32_t length_code(uint32_t m) { return (__builtin_bitreverse32(m - 2u) >> 25) << CODE_SHIFT; }
// pinned against RFC 1951 3.2.5 / 3.2.6 (codes go out LSB first, so a Huffman code is stored bit-reversed; extra bits are not):
static_assert(literal_entry(0) == (0x0Cu << CODE_SHIFT | 8u << NB_SHIFT), "literal 0: 8 bits, 00110000 reversed");
static_assert(literal_entry(143) == (0xFDu << CODE_SHIFT | 8u << NB_SHIFT), "literal 143: 8 bits, 10111111 reversed");
static_assert(literal_entry(144) == (0x13u << CODE_SHIFT | 9u << NB_SHIFT), "literal 144: 9 bits, 110010000 reversed");
static_assert(literal_entry(255) == (0x1FFu << CODE_SHIFT | 9u << NB_SHIFT), "literal 255: 9 bits, all ones");
static_assert(length_code(3) == 0x40u << CODE_SHIFT && length_code(10) == 0x08u << CODE_SHIFT, "lengths 3 / 10: symbols 257 / 264 = 7-bit codes 0000001 / 0001000 reversed");
static_assert(dist_entry(1) == (12u << NB_SHIFT), "distance 1: code 0, no extra bits: 7 + 5 bits");
static_assert(dist_entry(5) == ((0x04u << 7) << CODE_SHIFT | 13u << NB_SHIFT), "distance 5: code 4 (00100), one extra bit 0");
static_assert(dist_entry(32) == (((0x12u | 7u << 5) << 7) << CODE_SHIFT | 15u << NB_SHIFT), "distance 32: code 9 (01001 reversed), three extra bits 111");
static_assert(dist_entry(256) == (((0x1Eu | 63u << 5) << 7) << CODE_SHIFT | 18u << NB_SHIFT), "distance 256: code 15 (01111 reversed), six extra bits 111111: the widest entry");

// the LUT of the CWINDOW <= 32 kernels -- literal [byte] at word 0, match [len-3][dist-1] at word 256 -- depends on nothing: ONE constant
// table.  The one-tile kernels with the bit search fetch it into LDS per tile (their LDS is the mismatch words until the extension is
// through: WaveLdsBits); fill_luts computes the same entries per wave for the kernels that keep a resident LUT.
__host__ __device__ constexpr uint32_t match_entry32(uint32_t e) { return dist_entry((e & 31u) + 1u) | length_code((e >> 5) + 3u); }
struct __attribute__((aligned(16))) FixedLut { uint32_t e[LUT_LIT + LUT_MATCH]; };
constexpr FixedLut make_fixed_lut() {
    FixedLut t{};
    for (uint32_t k = 0; k < (uint32_t)LUT_LIT; k++) t.e[k] = literal_entry(k);
    for (uint32_t k = 0; k < (uint32_t)LUT_MATCH; k++) t.e[LUT_LIT + k] = match_entry32(k);
    return t;
}
static __device__ const FixedLut FIXED_LUT = make_fixed_lut();
static_assert(make_fixed_lut().e[LUT_LIT + 32 * 7 + 31] == (dist_entry(32) | length_code(10)), "match [len - 3][dist - 1]");

// =====================================================================================================================
// The tile phases.  ONE source for all compress kernels: k_compress (one block per wave, hdlz_compress.hip),
// k_compress_small (several small blocks per wave-tile, hdlz_compress_small.hip) and the multi-wave stream passes
// k_stream_tails / _xfer / _tile (hdlz_compress_stream.hip).  A wave-tile is 2048 positions, lane l owns the RUN of 32
// consecutive positions [32l, 32l+32); `in` is the staged input (byte index = position - tile start + halo).
// Everything is forced inline: the phases are straight-line code over register arrays, and the value fences (pin) and
// scheduling barriers (PHASE_FENCE) inside them are what keeps hipcc from overlapping the phases.
// =====================================================================================================================

// ---- the lane's own 32 bytes + 16 bytes of look-ahead
__device__ __forceinline__ void load_own(const uint32_t* in, uint32_t run_dw, uint32_t (&ow)[12]) {
    const uint4 v0 = *reinterpret_cast<const uint4*>(&in[run_dw]);
    const uint4 v1 = *reinterpret_cast<const uint4*>(&in[run_dw + 4]);
    const uint4 v2 = *reinterpret_cast<const uint4*>(&in[run_dw + 8]);
    ow[0] = v0.x; ow[1] = v0.y; ow[2] = v0.z; ow[3] = v0.w;
    ow[4] = v1.x; ow[5] = v1.y; ow[6] = v1.z; ow[7] = v1.w;
    ow[8] = v2.x; ow[9] = v2.y; ow[10] = v2.z; ow[11] = v2.w;
}

// ---- phase 2, match search (R3/R4; the reference's matcher3 x CWINDOW + first-set-bit pick, deflate.py:407-421, :975-994):
// best[i] = 4 * (nearest distance d in [1, 32*NCH] with x[p-d .. p-d+2] == x[p .. p+2]) for own position i; a value > 128 * NCH
// (NCH > 1: NO_MATCH4) = none.
// Keys K = (3-byte string) << 8 | 4 * window index: Ko - Kc (u32 wrap) is 4*distance (<= 128) iff the strings are equal and
// > 256 otherwise, so the MIN over a chunk of 32 candidates is four times the nearest matching distance: one v_sub and
// half a v_min3 per compare.  Windows > 32 iterate chunks of 32 distances far -> near.
// (The lane's own bytes are loaded here and die with the keys: the 32 own keys + 32 running minima + the candidate
// bytes are the register peak of the whole kernel; later phases reload the 48 bytes from LDS, three ds_read_b128.)
// wide windows (NCH > 1), "no candidate": a value every eligibility test rejects (> 4 * 256 + 124) whose distance field -- bits
// 2..10, what make_tokens gathers with -- reads 1: one v_bfe instead of compare + select + shift per position
constexpr uint32_t NO_MATCH4 = 0x8004u;
// PREV_DPP (NCH == 1, a tile that starts its block): the 32 candidates in front of the run are the own positions of the PREVIOUS lane, so
// their keys are that lane's own keys minus 128 (tag 4 (j + 32) -> 4 j): one DPP add each instead of two 16-byte LDS loads and ~1.5
// shift / align / mask instructions per key.  The DPP is a ROTATE (wave_ror:1): lane 0 has no previous lane and takes lane 63's keys --
// real keys with candidate tags, so whatever they match lies i + 32 - j > i = p positions back: in front of the block's first byte.  A
// nearer in-block candidate always wins the minimum, and a result from out there fails the position test of make_tokens like "none" does.
// (wave_shr with bound_ctrl would feed lane 0 the constant -128, which an own key FF FF FF | tag turns into a distance <= p: wrong.)
template <int NCH, bool PREV_DPP = false>
__device__ __forceinline__ void match_search(const uint32_t* in, uint32_t run_dw, uint32_t (&best)[RUN]) {
    uint32_t ko[RUN];
    uint32_t ow0;
    {
        uint32_t ow[12];
        load_own(in, run_dw, ow);
        static_for<0, RUN>([&](auto I) { constexpr int i = decltype(I)::value; ko[i] = key3<i>(ow, (uint32_t)(4 * (i + 32))); });
        ow0 = ow[0];
    }
    pin(ko); asm volatile("" : "+v"(ow0));
    PHASE_FENCE();
#pragma unroll
    for (int i = 0; i < RUN; i++) best[i] = NCH == 1 ? 0xFFFFFFFFu : NO_MATCH4;

#pragma unroll 1
    for (int k = NCH - 1; k >= 0; k--) {                      // far chunks first, nearer ones overwrite
        uint32_t cd[17];                                      // 64 candidate positions + 2 bytes
        const uint32_t cdw = run_dw - 8u * (uint32_t)(k + 1);
        [[maybe_unused]] uint32_t m128 = 0xFFFFFF80u;         // (-128 in a register: the DPP form takes no literal)
        if constexpr (PREV_DPP) {
            static_assert(NCH == 1, "own keys double as the next lane's candidates only for a 32-wide window");
            asm volatile("" : "+v"(m128));
#pragma unroll
            for (int j = 0; j < 17; j++) cd[j] = 0;
        } else {
            const uint4 c0 = *reinterpret_cast<const uint4*>(&in[cdw]);
            const uint4 c1 = *reinterpret_cast<const uint4*>(&in[cdw + 4]);
            cd[0] = c0.x; cd[1] = c0.y; cd[2] = c0.z; cd[3] = c0.w;
            cd[4] = c1.x; cd[5] = c1.y; cd[6] = c1.z; cd[7] = c1.w;
            if (NCH == 1) {
                cd[8] = ow0;                                  // candidate 31 needs the first own bytes
#pragma unroll
                for (int j = 9; j < 17; j++) cd[j] = 0;      // unused: own keys double as candidates
            } else {
                const uint4 c2 = *reinterpret_cast<const uint4*>(&in[cdw + 8]);
                const uint4 c3 = *reinterpret_cast<const uint4*>(&in[cdw + 12]);
                cd[8] = c2.x; cd[9] = c2.y; cd[10] = c2.z; cd[11] = c2.w;
                cd[12] = c3.x; cd[13] = c3.y; cd[14] = c3.z; cd[15] = c3.w;
                cd[16] = in[cdw + 16];
            }
        }
        uint32_t m[RUN];
#pragma unroll
        for (int i = 0; i < RUN; i++) m[i] = 0xFFFFFFFFu;
        // candidate-major order: two candidate keys live at a time, 32 running minima.  (Round 4: pairing the odd rows as (j+1, j+2) puts
        // their 32 single v_min_u32 into v_min3 as well, -12 instructions -- but the third live key spills 8 bytes per lane: not adopted)
        static_for<0, 63>([&](auto J) {
            constexpr int j = decltype(J)::value;             // handles candidates j and j+1 (j even)
            if constexpr ((j & 1) == 0) {
                uint32_t kc0, kc1;
                if constexpr (NCH == 1 && j >= 32) {          // own position j-32 IS candidate j (same tag 4j)
                    // pin in place: without it the scheduler precomputes all ~500 own-vs-own differences
                    asm volatile("" : "+v"(ko[j - 32]), "+v"(ko[j - 31]));
                    kc0 = ko[j - 32];
                    kc1 = ko[j - 31];
                } else if constexpr (PREV_DPP) {
                    // (the builtin, not inline asm: hipcc folds the move into v_add_u32_dpp and keeps the DPP read-after-write wait states)
                    kc0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ko[j], 0x13C, 0xF, 0xF, false) + m128;          // wave_ror:1
                    kc1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ko[j + 1], 0x13C, 0xF, 0xF, false) + m128;
                } else {
                    kc0 = key3<j>(cd, (uint32_t)(4 * j));
                    kc1 = key3<j + 1>(cd, (uint32_t)(4 * (j + 1)));
                }
                // own index i pairs with candidates j in [i, i+31]
                static_for<0, RUN>([&](auto I) {
                    constexpr int i = decltype(I)::value;
                    constexpr bool use0 = (j >= i) && (j <= i + 31);
                    constexpr bool use1 = (j + 1 >= i) && (j + 1 <= i + 31);
                    if constexpr (use0 && use1) m[i] = umin3(m[i], ko[i] - kc0, ko[i] - kc1);
                    else if constexpr (use0) m[i] = min(m[i], ko[i] - kc0);
                    else if constexpr (use1) m[i] = min(m[i], ko[i] - kc1);
                });
                if constexpr ((j & 7) == 6) { pin(m); PHASE_FENCE(); }
            }
        });
        // NCH == 1: the raw minimum IS the result (>= 256 = "none"; make_tokens' position test rejects those values)
#pragma unroll
        for (int i = 0; i < RUN; i++) {
            if (NCH == 1) best[i] = m[i];
            else if (m[i] < 256u) best[i] = m[i] + 128u * (uint32_t)k;
        }
    }
}

// ---- phase 2, BIT-SLICED (NCH == 1 with the candidates of the previous lane by DPP: the PREV_DPP case of match_search; the same best[]).
// The key form above is built around one (position, distance) pair per lane and instruction: 1.5 instructions, ~3.96 cycles per pair.
// Here a lane's 32 bytes are held as 8 BIT PLANES -- O_b bit i = bit b of own byte i -- and one instruction covers all 32 positions of
// the run for one distance:
//   C_b   = the candidate bytes at distance d: (O_b : P_b) >> (32 - d), one v_alignbit per plane (P_b = the previous lane's O_b)
//   neq   = OR_b (O_b ^ C_b): bit i = x[p] != x[p-d]                        (one xor + seven v_bitop3)
//   n3    = neq | neq >> 1 | neq >> 2, the bits 32, 33 from the NEXT lane's neq (one DPP move, two v_alignbit, one v_bitop3):
//           bit i = no 3-byte match at distance d
//   G     = positions without a match so far (distances ascend: the first one found is the nearest); D_k |= G & ~n3 for every set bit k
//           of d (one v_bitop3 each), G &= n3
// ~23 instructions per distance for 32 pairs.  Lane 0 takes lane 63's planes as history (the DPP is a rotate): a "match" from there lies
// d > i = p positions back and fails make_tokens' position test, and a real one (d <= p) is always nearer -- found first (the PREV_DPP
// argument above).  Lane 63 has no next lane (its bits 32, 33 read 0): they only feed positions 2046 and 2047, which R3 never makes eligible.
// Planes in and out are transposes of 32 x 8 bit matrices: a 4 x 4 byte transpose (v_perm) + three exchanges of a register-index bit
// with a bit-index bit (two shifts + two v_bitop3 per register pair).  Result byte = 4 d (found; d <= 32), 0xFF (none: above 252, and
// above every 4 * cwindow -- make_tokens' tests reject it like the key form's raw minima >= 256).
// v_bitop3_b32 (gfx950): any function of three words at the rate of a v_xor; its table is the function applied to 0xF0, 0xCC, 0xAA.
constexpr uint32_t B3_SEL = 0xE4;         // c ? a : b
constexpr uint32_t B3_OR_XOR = 0xF6;      // a | (b ^ c)
constexpr uint32_t B3_OR3 = 0xFE;         // a | b | c
constexpr uint32_t B3_OR_ANDN = 0xF4;     // a | (b & ~c)
template <uint32_t F>
__device__ __forceinline__ uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, F); }
// a constant in an SGPR, set where it is used (hoisted out of the block loop, the search's masks and selectors cost the kernel SGPR spills)
__device__ __forceinline__ uint32_t sconst(uint32_t v) { asm volatile("" : "+s"(v)); return v; }
// w[k] bit 8 m + b <-> w[b] bit 8 m + k (b, k = 0..7, m = 0..3): exchange bit j of the register index with bit j of the bit index,
// j = 0, 1, 2.  An involution: the same network takes bytes to planes and planes to bytes.
__device__ __forceinline__ void exchange8(uint32_t (&w)[8]) {
    static_for<0, 3>([&](auto J) {
        constexpr int s = 1 << decltype(J)::value;
        const uint32_t m0 = sconst(s == 1 ? 0x55555555u : s == 2 ? 0x33333333u : 0x0F0F0F0Fu);   // bits whose index has bit j clear
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (k & s) continue;
            const uint32_t x = w[k], y = w[k + s];
            w[k] = bitop3<B3_SEL>(x, y << s, m0);
            w[k + s] = bitop3<B3_SEL>(x >> s, y, m0);
        }
    });
}
// 4 x 4 byte transpose: t[k] byte m = r[m] byte k
__device__ __forceinline__ void transpose4x4_bytes(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t& t0, uint32_t& t1,
                                                   uint32_t& t2, uint32_t& t3) {
    const uint32_t zip_lo = sconst(0x05010400u), zip_hi = sconst(0x07030602u), cat_lo = sconst(0x05040100u), cat_hi = sconst(0x07060302u);
    const uint32_t a01 = __builtin_amdgcn_perm(r1, r0, zip_lo), b01 = __builtin_amdgcn_perm(r1, r0, zip_hi);     // r0.0 r1.0 r0.1 r1.1 | .2 .3
    const uint32_t a23 = __builtin_amdgcn_perm(r3, r2, zip_lo), b23 = __builtin_amdgcn_perm(r3, r2, zip_hi);
    t0 = __builtin_amdgcn_perm(a23, a01, cat_lo); t1 = __builtin_amdgcn_perm(a23, a01, cat_hi);
    t2 = __builtin_amdgcn_perm(b23, b01, cat_lo); t3 = __builtin_amdgcn_perm(b23, b01, cat_hi);
}
// (x0 .. x7: the lane's own 32 bytes as dwords, in registers)
// KEEP: neq_d of every distance goes to neq_col[(d & 31) * 64] (neq_col = NEQ + lane: one ds_write_b32 at a fixed address register +
// immediate offset, where neq is complete and before the DPP for nx) -- what make_tokens_bits reads instead of comparing bytes again
// (Measured and dropped, profiles/tile_diet.txt: nx read back from that row -- ds_read_b32 at NEQ + min(lane + 1, 63), the reads of four
// distances issued a group ahead -- instead of the DPP move: 32 slow instructions fewer, -0.01 .. -0.02 ms, inside the run-to-run spread.)
// WORK THE DATA DOES NOT NEED is skipped by wave-uniform branches (the result is the same bit for bit):
//   a DEAD PLANE  O_b is the same word s = 0 or 0xFFFFFFFF in all 64 lanes (bit 7 of ASCII text; three planes of decimal digits; seven of
//           '0' / '1' text): then P_b = s and every candidate word C_b = s, so the plane adds nothing to any neq.  The planes are the
//           OUTER loop -- the 32 mismatch words accumulate in registers, plane 0 starts them -- and a plane b >= 1 is tested first (one
//           v_readfirstlane, one compare + ballot) and its 31 v_alignbit + 32 v_bitop3 jumped over; P_b is fetched inside the live
//           branch.  A second pass over the distances does what follows neq: row store, n3, D, G.  (-DHDLZ_PLANES_ALL_LIVE: no test.)
//   a MATCH-FREE TILE  G is all ones in every lane (random, compressed or encrypted bytes): every result byte would be 0xFF and every
//           token a literal.  The function returns false; the kernel then does not transpose the result, runs neither the extension
//           nor the parse nor the skip chain and emits the literals' codes straight from the own bytes (literal_codes; the token form,
//           literal_tokens + token_codes: -DHDLZ_LITERAL_TOKENS).  Lane 0's false history and lane 63's zero bits
//           32, 33 can only CLEAR bits of G: such a tile takes the normal path, which rejects them.  A short block is no exception: the
//           end cap (below) keeps the zero bytes behind its end from matching each other.  (-DHDLZ_NO_LITERAL_TILE: always true.)
constexpr bool skip_dead_planes() {
#ifdef HDLZ_PLANES_ALL_LIVE
    return false;
#else
    return true;
#endif
}
constexpr bool literal_tiles() {
#ifdef HDLZ_NO_LITERAL_TILE
    return false;
#else
    return true;
#endif
}
// THE DISTANCE PLANES BY GROUPS OF FOUR.  Inside an aligned group of four distances (d >> 2 fixed: 1..3, 4..7, .. 28..31, 32) only bits 0
// and 1 of d change, so only D_0 and D_1 are updated distance by distance.  The positions that took a distance of the group are the bits G
// lost inside it: D_k |= G_at_group_start & ~G_at_group_end for the set bits k >= 2 of d, ONCE per group -- 13 v_bitop3 where the per-
// distance form has 49 (32 + 32 + 13 = 77 against 113 for D and G together).  G itself is still narrowed distance by distance: nearest
// first is untouched.  One more live register (G at the group's start).  (-DHDLZ_PLANES_PER_DISTANCE: every plane at every distance.)
constexpr bool grouped_planes() {
#ifdef HDLZ_PLANES_PER_DISTANCE
    return false;
#else
    return true;
#endif
}
// A MATCH-FREE TILE EMITS ITS LITERALS ITSELF (literal_codes, next to token_codes) instead of forming literal tokens for the generic
// token_codes to read back.  (-DHDLZ_LITERAL_TOKENS: the token form.)
constexpr bool literal_emit() {
#ifdef HDLZ_LITERAL_TOKENS
    return false;
#else
    return literal_tiles();
#endif
}
// ONE-TILE BLOCKS SUM THEIR ADLER WEIGHTS PLAINLY: see the static_assert next to adler_finish.  (-DHDLZ_ADLER_TILE_MOD: one modulo per
// tile and the carried weight, as the multi-tile kernels need them.)
constexpr bool adler_plain_one_tile() {
#ifdef HDLZ_ADLER_TILE_MOD
    return false;
#else
    return true;
#endif
}
// THE END OF THE BLOCK is part of the mismatch words: E (end_cap_word) has bit j set for every position j of the run at or behind N - 2 and is
// OR-ed into every neq_d with plane 0's xor.  Read from bit i + 3 on, such a word shows a difference at bit N - 2 - p_run at the latest,
// that is after at most N - 5 - p equal bytes: R5's "a match ends at N - 2" needs no minimum of its own in make_tokens_bits.  Nothing
// else changes: the forced bits reach n3 only at positions >= N - 4, which R3 never makes eligible (make_tokens_bits' okm rejects them), and
// they only SET bits of G -- the zero bytes behind the end no longer match each other at distance 1, so a short block without a
// candidate is a match-free tile like a full one.
// R: the result as planes -- R[0] = G, R[1 + k] = D_k; search_result_bytes() turns them into best[], inside the branch that reads it (as
// one function with a branch of its own around the transposition, best[] was live across both arms of the extension's branch: 26 spills)
// returns: some position of the tile has a candidate
// bit j = position p_run + j lies at or behind N - 2: the bits from N - 2 - p_run on, all of them when that is <= 0, none when it is >= 32
__device__ __forceinline__ uint32_t end_cap_word(int32_t n_m2, uint32_t p_run) {
    const int32_t first = min(max(n_m2 - (int32_t)p_run, 0), 32);      // (v_med3_i32)
    return (uint32_t)(~0ull << first);
}
template <bool KEEP>
__device__ __forceinline__ bool match_search_bits(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t x4, uint32_t x5, uint32_t x6,
                                                  uint32_t x7, uint32_t (&R)[7], [[maybe_unused]] uint32_t* neq_col = nullptr, uint32_t E = 0u) {
    uint32_t O[8];
    // O[k] byte m = own byte k + 8 m (k = 0..7): bytes k, k + 8, k + 16, k + 24 are byte k & 3 of dwords k >> 2, +2, +4, +6
    transpose4x4_bytes(x0, x2, x4, x6, O[0], O[1], O[2], O[3]);
    transpose4x4_bytes(x1, x3, x5, x7, O[4], O[5], O[6], O[7]);
    exchange8(O);                                             // O[b] bit i = bit b of own byte i
    pin(O);
    PHASE_FENCE();
    uint32_t nq[RUN];                                         // nq[d - 1] = neq_d, over the planes seen so far
    static_for<0, 8>([&](auto B) {
        constexpr int b = decltype(B)::value;
        bool live = true;
        if constexpr (b != 0 && skip_dead_planes()) {
            const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)O[b]);
            live = !((s0 == 0u || s0 == 0xFFFFFFFFu) && ballot64(O[b] != s0) == 0ull);
        }
        if (live) {
            const uint32_t Pb = (uint32_t)__builtin_amdgcn_mov_dpp((int)O[b], 0x13C, 0xF, 0xF, false);                // wave_ror:1
            static_for<1, RUN + 1>([&](auto Dd) {
                constexpr int d = decltype(Dd)::value;
                const uint32_t c = d == 32 ? Pb : __builtin_amdgcn_alignbit(O[b], Pb, (uint32_t)(32 - d));
                if constexpr (b == 0) nq[d - 1] = bitop3<B3_OR_XOR>(E, O[0], c);        // (the end cap rides along: as cheap as the xor)
                else nq[d - 1] = bitop3<B3_OR_XOR>(nq[d - 1], O[b], c);
                if constexpr ((d & 3) == 0) { pin_range<d - 4, d>(nq); PHASE_FENCE(); }       // (else hipcc hoists the alignbits of all distances)
            });
        }
        pin(nq);
        PHASE_FENCE();
    });
    uint32_t G = 0xFFFFFFFFu, D[6] = {0, 0, 0, 0, 0, 0};
    [[maybe_unused]] uint32_t Gs = 0xFFFFFFFFu;              // G in front of the aligned group of four distances that d lies in
    constexpr int KD = grouped_planes() ? 2 : 6;             // planes updated distance by distance
    static_for<1, RUN + 1>([&](auto Dd) {
        constexpr int d = decltype(Dd)::value;
        const uint32_t neq = nq[d - 1];
        if constexpr (KEEP) neq_col[(d & (NEQ_ROWS - 1)) * 64] = neq;
        const uint32_t nx = (uint32_t)__builtin_amdgcn_mov_dpp((int)neq, 0x130, 0xF, 0xF, true);                      // wave_shl:1 (lane 63: 0)
        const uint32_t n3 = bitop3<B3_OR3>(neq, __builtin_amdgcn_alignbit(nx, neq, 1u), __builtin_amdgcn_alignbit(nx, neq, 2u));
        static_for<0, KD>([&](auto K) {
            constexpr int k = decltype(K)::value;
            if constexpr ((d >> k) & 1) D[k] = bitop3<B3_OR_ANDN>(D[k], G, n3);
        });
        G &= n3;
        if constexpr (grouped_planes() && ((d & 3) == 3 || d == RUN)) {      // the group's last distance: what G lost inside it took d >> 2
            static_for<2, 6>([&](auto K) {
                constexpr int k = decltype(K)::value;
                if constexpr ((d >> k) & 1) D[k] = bitop3<B3_OR_ANDN>(D[k], Gs, G);
            });
            Gs = G;
        }
        if constexpr ((d & 3) == 0) { pin(D); asm volatile("" : "+v"(G)); if constexpr (grouped_planes()) asm volatile("" : "+v"(Gs)); PHASE_FENCE(); }
    });
    R[0] = G;
#pragma unroll
    for (int k = 0; k < 6; k++) R[k + 1] = D[k];
    if constexpr (literal_tiles()) return ballot64(G != 0xFFFFFFFFu) != 0ull;
    else return true;
}
// the search's result planes -> Q[k] byte m = result byte of own position k + 8 m (not for a match-free tile: nothing would read it)
__device__ __forceinline__ void search_result_packed(const uint32_t (&R)[7], uint32_t (&Q)[8]) {
    // planes of the result byte: bits 0, 1 = none, bits 2..7 = d | none
    const uint32_t G = R[0];
    Q[0] = G; Q[1] = G;
#pragma unroll
    for (int k = 2; k < 8; k++) Q[k] = R[k - 1] | G;
    exchange8(Q);
}
// ... -> best[], one register per position
__device__ __forceinline__ void search_result_bytes(const uint32_t (&R)[7], uint32_t (&best)[RUN]) {
    uint32_t Q[8];
    search_result_packed(R, Q);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        best[k] = Q[k] & 0xFFu;
        best[k + 8] = __builtin_amdgcn_ubfe(Q[k], 8u, 8u);
        best[k + 16] = __builtin_amdgcn_ubfe(Q[k], 16u, 8u);
        best[k + 24] = Q[k] >> 24;
    }
}
// ---- phase 2 for WIDE windows: a window-independent match finder ------------------------------------------
// "Nearest previous occurrence of the same 3-byte string" (matcher3 x CWINDOW + first-set-bit pick, deflate.py:407-421, :966-1016)
// is a predecessor query; its cost need not grow with the window.  match_search pays 1.5 VALU instructions per (position,
// distance) pair -- 48 per position at CWINDOW = 32, 384 at 256.  Here the tile is walked in ROUNDS of 64 consecutive positions,
// one lane per position, through three LDS structures:
//   T[h]    last position with hash h so far.  ONE returning atomic per position -- old = ds_max_rtn_u32(T[h], own position) -- both
//           inserts the position and answers "previous position of my hash class", INCLUDING the up to 63 nearer members of the
//           same round, if the LDS applies the lanes of a wave instruction to one address in lane order: the positions of a round
//           rise with the lane.  That order is not architected, so it is CHECKED instead of assumed: if a later lane b is applied
//           before an earlier lane a of the same class, a reads back a value >= position(b) > its own position -- every inversion
//           shows up as a negative distance in some lane.  A group of rounds that saw one is redone by a 64-step readlane loop (the
//           minimum of the values a class got back is the table entry before the round; the nearest lower lane of the class the
//           candidate inside the round): exact whatever the hardware does, and T's final content (a maximum) never depends on the
//           order.  (Round 3 read T, ds_max-ed, read the class's LEADER back and kept a 64-bit lane map per leader slot -- six LDS
//           operations and ~15 VALU instructions per round instead of one and two: the LDS was 65 % busy, VERDICT r3 #2.)
//   E[p]    (distance from p to the previous position with the same HASH) - 1 as one byte, 255 = none or >= 256: every hash class
//           is a chain in descending position order.
// h = the top HB bits of (K * odd) mod 2^24 (K = the three bytes): a bijection of the key, well mixed in its high bits.  A lane
// follows its chain, nearest first, comparing the exact three bytes, until they are equal (the answer), or the window is left;
// positions with the same hash and another key are the only wasted steps (about CWINDOW / 2^HB per query).
// Result: best[i] = 4 * distance for own position i of the lane's RUN (the layout of all later phases; transposed through LDS),
// NO_MATCH4 = none.  The zero halo in front of a block's first tile only yields distances > p (rejected by
// make_tokens' position test; a valid candidate is always nearer and therefore found first).
template <int NCH> struct HashCfg {
#ifndef HDLZ_HASH_BITS
#define HDLZ_HASH_BITS 10
#endif
    static constexpr int HB = HDLZ_HASH_BITS;
    static constexpr int NT = 1 << HB;
    static constexpr int PRE = 64 * ((32 * NCH + 63) / 64);     // positions in front of the tile that are inserted first
    static_assert(PRE <= HALO && HB >= 8 && HB <= 16, "halo / tag position");
    // E[] is only written from byte index HALO - PRE on and an empty T[] entry reads as index 0.  A query of a tile position
    // (index >= HALO) walks at most cwindow <= 32 * NCH entries back, i.e. never below HALO - PRE -- as long as this holds:
    static_assert(32 * NCH <= PRE, "cwindow <= PRE: chain walks must stay inside the entries this tile has written (ADVICE r3)");
};
template <int NCH> struct __attribute__((aligned(16))) HashLds {
    union {
        uint32_t T[HashCfg<NCH>::NT];
        uint16_t D[TILE];                   // the results on their way from the round layout to the run layout
    };
    uint16_t E[HALO + TILE];                // per position: eight tag bits of the key << 8 | link
    static_assert(sizeof(uint32_t) * HashCfg<NCH>::NT >= sizeof(uint16_t) * TILE, "D overlays T");
};

__device__ __forceinline__ uint32_t* lds_out(WaveLds& l, uint32_t&) { return l.out; }
__device__ __forceinline__ uint32_t* lds_out(WaveLdsBits& l, uint32_t&) { return l.out; }
template <int NCH> __device__ __forceinline__ uint32_t* lds_out(WaveLdsNoOut&, HashLds<NCH>& h) {
    static_assert(sizeof(h.T) >= sizeof(uint32_t) * OUT_WORDS, "the bit buffer overlays T / D");
    return h.T;
}

template <int NCH>
__device__ __forceinline__ void match_search_hash(const uint32_t* in, HashLds<NCH>& hl, uint32_t lane, uint32_t cw, uint32_t (&best)[RUN]) {
    constexpr int HB = HashCfg<NCH>::HB, NT = HashCfg<NCH>::NT, PRE = HashCfg<NCH>::PRE;
    constexpr uint32_t base = HALO - PRE;
    // empty table (it was the transposition buffer and the bit buffer of the previous tile)
    for (uint32_t k = lane * 4u; k < (uint32_t)NT; k += 256u) *reinterpret_cast<uint4*>(&hl.T[k]) = make_uint4(0, 0, 0, 0);
    __syncthreads();

    // Rounds are batched in groups of G: the LDS executes a wave's instructions in order, so the table operations of G rounds
    // are ISSUED back to back (round r+1's T read behind round r's ds_max) and their results are consumed afterwards -- one
    // LDS round trip per group instead of four dependent ones per round (a first version that finished a round before it
    // started the next was latency-bound at 5 waves per CU: 63 k cycles per tile).
    // Costs in CU cycles per wave instruction (tools/ubench/lds_ops.hip): random ds_read_b32 7, ds_max_u32 7, ds_or_b64 11,
    // ds_read_b64 7..10, ds_write_b64 11 -- and 65 for an UNALIGNED ds_read_b32 (one lane per cycle), 11..22 for ds_write_b8: the key
    // therefore comes from two aligned dwords + v_alignbyte, and the chain entries are dwords that carry the key themselves
    constexpr int G = 8;
    static_assert(RUN % G == 0 && PRE / 64 <= G, "groups");
    uint32_t res2[RUN / 2];                  // round layout, two rounds per register: 4 * distance of position 64 r + lane, 16 bits each
    // A group's work comes in three pieces: issue (key, hash, the table operations), consume (first candidate, chain entry) and
    // walk (the chain steps of its queries).  (Issuing group g+1 before walking group g changed nothing measurable.)
    struct Grp { uint32_t kw[G], ow[G], c0[G], dd[G]; };
    auto hash_of = [&](uint32_t kw, uint32_t& tag) -> uint32_t {
        uint32_t mix;
        asm("v_mul_u32_u24 %0, %1, %2" : "=v"(mix) : "v"(kw), "v"(0x9E3779u));     // (ignores the top byte; hipcc picks the quarter-rate v_mul_lo_u32)
        tag = (mix << (HB - 8)) & 0xFF00u;                    // the eight bits BELOW the hash bits of (K * odd) mod 2^24, as the entry's tag
        return __builtin_amdgcn_ubfe(mix, 24 - HB, HB);
    };
    auto issue = [&](auto G0, auto CNT, Grp& q) {             // rounds [g0, g0 + cnt), counted from position `base`
        constexpr int g0 = decltype(G0)::value, cnt = decltype(CNT)::value;
        uint32_t w0_[cnt], w1_[cnt];
        static_for<0, cnt>([&](auto J) {
            constexpr int j = decltype(J)::value;
            const uint32_t idx = base + 64u * (uint32_t)(g0 + j) + lane;      // byte index of the position in `in`
            w0_[j] = in[idx >> 2]; w1_[j] = in[(idx >> 2) + 1u];
        });
        static_for<0, cnt>([&](auto J) {
            constexpr int j = decltype(J)::value;
            constexpr uint32_t rbase = base + 64u * (uint32_t)(g0 + j);
            q.kw[j] = alignbyte(w1_[j], w0_[j], lane);                        // (rbase is a multiple of 4) the key is its low three bytes
            const uint32_t h = hash_of(q.kw[j], q.ow[j]);
            // insert the position and get the previous one of the hash class back (the rounds of a group back to back: the LDS
            // executes a wave's instructions in order)
            q.c0[j] = __hip_atomic_fetch_max(&hl.T[h], rbase + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        });
    };
    // (never taken on this hardware so far: see the head of this section) the previous position of the hash class of every lane of
    // one round, from the values the atomics returned, whatever order they were applied in
    auto reorder = [&](uint32_t rbase, uint32_t kw, uint32_t got) -> uint32_t {
        uint32_t tag;
        const uint32_t h = hash_of(kw, tag);
        uint32_t before = got, nearer = 0u;
        bool has = false;
#pragma unroll 1
        for (uint32_t s_ = 0; s_ < 64u; s_++) {
            const uint32_t hs = (uint32_t)__builtin_amdgcn_readlane((int)h, (int)s_), gs = (uint32_t)__builtin_amdgcn_readlane((int)got, (int)s_);
            if (hs == h) {
                before = min(before, gs);
                if (s_ < lane) { nearer = rbase + s_; has = true; }
            }
        }
        return has ? nearer : before;
    };
    auto consume = [&](auto G0, auto CNT, Grp& q) {
        constexpr int g0 = decltype(G0)::value, cnt = decltype(CNT)::value;
        uint32_t inv = 0;                                     // sign bit: some lane got a position behind its own back
        static_for<0, cnt>([&](auto J) {
            constexpr int j = decltype(J)::value;
            inv |= (base + 64u * (uint32_t)(g0 + j) + lane) - q.c0[j];
        });
#ifdef HDLZ_HASH_FORCE_REORDER                     // test build (build.sh forced, tests/test_gpu_forced_paths.py): every group takes the path the hardware never asks for
        inv = 0x80000000u;
#endif
        if (ballot64((int32_t)inv < 0) != 0ull) {
            static_for<0, cnt>([&](auto J) {
                constexpr int j = decltype(J)::value;
                q.c0[j] = reorder(base + 64u * (uint32_t)(g0 + j), q.kw[j], q.c0[j]);
            });
        }
        static_for<0, cnt>([&](auto J) {
            constexpr int j = decltype(J)::value;
            constexpr uint32_t rbase = base + 64u * (uint32_t)(g0 + j);
            const uint32_t idx = rbase + lane;
            const uint32_t d = idx - q.c0[j];                 // (an empty T entry reads as position 0: a distance that is either outside
                                                              //  the window or leads to a real position whose key is then compared)
            hl.E[idx] = (uint16_t)(q.ow[j] | min(d - 1u, 255u));
            q.dd[j] = (d - 1u) < cw ? d : 0u;                 // 0 = this lane has nothing (more) to look at
        });
    };
    // follow the chains, nearest first: the nearest position with the same three bytes inside the window.  The first step of
    // the group's rounds is issued together; the (rare) further steps run per round, branch-free in the body (the scalar unit
    // is shared by the CU's four SIMDs: a compare-and-branch ladder per step would make IT the limit).  An entry carries eight
    // tag bits of its key (a dword per entry with the whole key cost 9 KB of LDS = a wave per SIMD): a candidate whose tag agrees
    // is CONFIRMED against its three bytes, and the one in 256 wrong candidates that gets that far sends its lane back to the walk.
    auto walk = [&](auto G0, Grp& q) {
        constexpr int g0 = decltype(G0)::value;
        uint32_t ev_[G], found_[G];                           // found: 0 = none
        auto step = [&](uint32_t ev, uint32_t ow, uint32_t& dd, uint32_t& found) {
            const uint32_t nd = dd + (ev & 255u) + 1u;
            const bool live = dd != 0u;
            const bool same = (ev ^ ow) < 256u;
            found = (live & same) ? dd : found;
            dd = (live & !same & (nd <= cw)) ? nd : 0u;
        };
        // two steps for all rounds of the group, their reads in flight together (every dependent LDS round trip that is paid per
        // ROUND -- a step, the confirmation -- is paid 32 times per tile: at two to three waves per SIMD that latency is the kernel)
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            static_for<0, G>([&](auto J) {
                constexpr int j = decltype(J)::value;
                ev_[j] = hl.E[base + 64u * (uint32_t)(g0 + j) + lane - q.dd[j]];     // (a finished lane reads its own entry: in range, unused)
            });
            static_for<0, G>([&](auto J) {
                constexpr int j = decltype(J)::value;
                if (pass == 0) found_[j] = 0u;
                step(ev_[j], q.ow[j], q.dd[j], found_[j]);
            });
        }
        // the chains that are longer, round by round
        static_for<0, G>([&](auto J) {
            constexpr int j = decltype(J)::value;
            const uint32_t idx = base + 64u * (uint32_t)(g0 + j) + lane;
            while (ballot64(q.dd[j] != 0u) != 0ull) step(hl.E[idx - q.dd[j]], q.ow[j], q.dd[j], found_[j]);
        });
        // confirm the candidates: the three bytes at idx - found against the own ones (none: the own position, trivially equal)
        uint32_t c0_[G], c1_[G];
        static_for<0, G>([&](auto J) {
            constexpr int j = decltype(J)::value;
            const uint32_t a = base + 64u * (uint32_t)(g0 + j) + lane - found_[j];
            c0_[j] = in[a >> 2]; c1_[j] = in[(a >> 2) + 1u];
        });
        uint32_t anybad = 0;
        static_for<0, G>([&](auto J) {
            constexpr int j = decltype(J)::value;
            const uint32_t a = base + 64u * (uint32_t)(g0 + j) + lane - found_[j];
            ev_[j] = (alignbyte(c1_[j], c0_[j], a) ^ q.kw[j]) << 8;          // != 0: a wrong candidate with the right tag
            anybad |= ev_[j];
        });
        if (ballot64(anybad != 0u) != 0ull) {
            // (rare: one candidate in 256 wrong ones) the lane goes on behind it -- serial walk and confirmation
            static_for<0, G>([&](auto J) {
                constexpr int j = decltype(J)::value;
                const uint32_t idx = base + 64u * (uint32_t)(g0 + j) + lane;
                bool bad = ev_[j] != 0u;
                while (ballot64(bad) != 0ull) {
                    uint32_t dd = 0u;
                    if (bad) {
                        const uint32_t nd = found_[j] + ((uint32_t)hl.E[idx - found_[j]] & 255u) + 1u;
                        dd = nd <= cw ? nd : 0u;
                        found_[j] = 0u;
                    }
                    while (ballot64(dd != 0u) != 0ull) step(hl.E[idx - dd], q.ow[j], dd, found_[j]);
                    const uint32_t a = idx - found_[j];
                    bad = bad && ((alignbyte(in[(a >> 2) + 1u], in[a >> 2], a) ^ q.kw[j]) << 8) != 0u;
                }
            });
        }
        static_for<0, G>([&](auto J) {
            constexpr int j = decltype(J)::value;
            constexpr int r = g0 + j - PRE / 64;
            const uint32_t f = found_[j] ? found_[j] : (NO_MATCH4 >> 2);
            if constexpr ((r & 1) == 0) res2[r >> 1] = f << 2;
            else res2[r >> 1] |= f << 18;
        });
    };
    {
        Grp q;
        issue(std::integral_constant<int, 0>{}, std::integral_constant<int, PRE / 64>{}, q);      // the positions in front of the tile
        consume(std::integral_constant<int, 0>{}, std::integral_constant<int, PRE / 64>{}, q);
        static_for<0, RUN / G>([&](auto GI) {
            constexpr int g0 = PRE / 64 + decltype(GI)::value * G;
            issue(std::integral_constant<int, g0>{}, std::integral_constant<int, G>{}, q);
            consume(std::integral_constant<int, g0>{}, std::integral_constant<int, G>{}, q);
            walk(std::integral_constant<int, g0>{}, q);
            pin(res2);
            PHASE_FENCE();
        });
    }
    // round layout -> run layout.  res2[k] holds rounds 2k (low half) and 2k+1 of this lane: written as ONE dword at [k][lane]
    // (16 conflict-free ds_write_b32 instead of 32 ds_write_b16); position p = 64 r + j sits in dword (r >> 1) * 64 + j, half r & 1,
    // so the run of lane l -- positions 32 l .. 32 l + 31, all of round l >> 1 -- is 32 consecutive dwords and one half of each
    __syncthreads();
    uint32_t* D32 = reinterpret_cast<uint32_t*>(hl.D);
#pragma unroll
    for (int k = 0; k < RUN / 2; k++) D32[64 * k + lane] = res2[k];
    __syncthreads();
    const uint32_t dbase = (lane >> 2) * 64u + 32u * (lane & 1u), hsh = 16u * ((lane >> 1) & 1u);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint4 v = *reinterpret_cast<const uint4*>(&D32[dbase + 4u * q]);
        best[4 * q + 0] = __builtin_amdgcn_ubfe(v.x, hsh, 16u); best[4 * q + 1] = __builtin_amdgcn_ubfe(v.y, hsh, 16u);
        best[4 * q + 2] = __builtin_amdgcn_ubfe(v.z, hsh, 16u); best[4 * q + 3] = __builtin_amdgcn_ubfe(v.w, hsh, 16u);
    }
    __syncthreads();
}

// which kernels use the hash finder, and the waves per SIMD they are register-capped for
#ifndef HDLZ_WH
#define HDLZ_WH 3                               // waves per SIMD of the kernels with the hash finder (13.6 KB of LDS per wave: 12 per CU)
#endif
template <int NCH> constexpr bool wide_hash() { return NCH > 1; }      // every window > 32 (round 4: CWINDOW = 64 too, 279 against 246 GB/s for the one-pass brute force, which is gone)
template <int NCH> constexpr int waves_eu() { return NCH == 1 ? HDLZ_W1 : HDLZ_WH; }

// ---- THE window rule of every compress launcher (host): cwindow (1 .. 256) -> NCH = 1, 2 or 8 chunks of 32 candidate distances and
// FULLWIN = "cwindow == 32 * NCH" (the reference's own windows 32 and 256, and 64), handed to f as types: f(std::integral_constant<int,
// NCH>{}, std::bool_constant<FULLWIN>{}).  Two things rest on it: cwindow <= 32 * NCH <= HashCfg<NCH>::PRE (the hash finder's chain walks
// stay inside the entries a tile wrote), and FULLWIN only where make_tokens may drop its window compare (kernels built without it ignore it).
template <int NCH, class F> inline void window_case(int cwindow, F& f) {
    static_assert(32 * NCH <= HashCfg<NCH>::PRE && 32 * NCH <= HALO, "the window of this NCH inside what a tile stages and inserts");
    if (cwindow == 32 * NCH) f(std::integral_constant<int, NCH>{}, std::true_type{});
    else f(std::integral_constant<int, NCH>{}, std::false_type{});
}
template <class F> inline void with_window(int cwindow, F&& f) {
    if (cwindow <= 32) window_case<1>(cwindow, f);
    else if (cwindow <= 64) window_case<2>(cwindow, f);
    else window_case<8>(cwindow, f);
}

// ---- phase 3, eligibility + extension (R3/R5; SEARCHF / SEARCH10, deflate.py:899-964, :1018-1062):
// tok[i] = 4 * (len-1) << 16 | LUT byte offset of the token  (len-1 = 0 for a literal).
//   lds_run  byte offset of the run in `in`;  nrem = positions of the block from the run's first position on (0 = none)
//   p4_run   4 * min(block-relative position of the run, 32 * NCH): with that clamp `d4 <= p4_run + 4i` is at once R4's
//            d <= p, the "a candidate exists" test AND -- for NCH == 1, where best[] holds raw minima -- the rejection of
//            the >= 256 values that stand for "no match" (p4_run + 4i <= 128 + 124)
//   FULLWIN  cwindow == 32 * NCH: every distance the search can return is inside the window (no cw4 compare)
// Measured and dropped (profiles/r02_tokens_ab.txt): the candidate's 8 bytes from ONE unaligned ds_read_b64 -- 8 VALU
// instructions fewer per position, but gfx950's LDS splits unaligned 64-bit reads: LDS busy 57 -> 82 %, 1 % slower.
//   SCALAR_TAIL: the lane runs are consecutive pieces of ONE block and tile_rem = positions of the block from the tile's first
//            position on: R3's "p <= N-5" then holds for a PREFIX of the lanes, so it is evaluated on the scalar unit --
//            at most two different lane masks per tile -- and and-ed into the compare's lane mask (else: per lane, from nrem)
//   GMASK    dword-index mask of the extension's gather: the gather of a position WITHOUT a candidate (NCH == 1: a raw minimum up to
//            2^32 - 1 stands for "none") would address LDS far outside `in`; masked, it stays inside the first 4 (GMASK + 3) bytes behind
//            `in` -- which every caller's LDS block covers (static_assert there) -- and its result is discarded as before.  The mask
//            replaces the ~3 of the dword address: no instruction more.  (an out-of-allocation LDS read.)
template <int NCH, bool FULLWIN, bool SCALAR_TAIL = false, uint32_t GMASK = 0x3FFu>
__device__ __forceinline__ void make_tokens(const uint32_t* in, uint32_t lds_run, uint32_t (&ow)[12], uint32_t (&best)[RUN],
                                            uint32_t cw4, uint32_t kmax, uint32_t p4_run, uint32_t nrem, uint32_t (&tok)[RUN],
                                            int32_t tile_rem = 0) {
    pin(best); pin(ow);
    PHASE_FENCE();
    const uint32_t nrem_m5 = nrem - 5u;                       // (wraps when nrem < 5: then nothing is eligible)
    const uint32_t kmax_m3 = kmax - 3u;
    // lanes l with tile_rem - 32 l >= i + 5  <=>  l < cnt_i,  cnt_i = ((tile_rem - 5 - i) >> 5) + 1: two values over i = 0..31
    const int32_t rem5 = tile_rem - 5;
    const uint32_t thr = rem5 >= 0 ? ((uint32_t)rem5 & 31u) : 0u;                        // i <= thr: the larger count
    const int32_t cnt_hi = rem5 >= 0 ? (rem5 >> 5) + 1 : 0, cnt_lo = rem5 >= 0 ? (rem5 >> 5) : 0;
    const uint64_t m_hi = cnt_hi >= 64 ? ~0ull : ((1ull << cnt_hi) - 1ull), m_lo = cnt_lo >= 64 ? ~0ull : ((1ull << cnt_lo) - 1ull);
    // token word of a match of length len = l3 + 3 at distance d:  4 * (len-1) << 16 | LUT offset
    //   CWINDOW <= 32: LUT [len-3][d-1] -> l3 * (4 * 65536 + 128) + 4d + K;   wider: LUT [d-1] -> l3 * 4 * 65536 + 4d + K
    // (the upper half holds 4 * (len-1): the parse shifts its nibble table by exactly that, the LUT_LEN offset is exactly that, and a plain
    //  v_lshrrev is a full-rate instruction where the shift-and-scale forms are not)
    const uint32_t tok_k = (2u << 18) + LUT_MATCH_BYTE - 4u;
    const uint32_t tok_mul = NCH == 1 ? (4u * 65536u + 128u) : 4u * 65536u;
    static_for<0, RUN>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const uint32_t d4 = best[i];
        // R3: 1 <= p <= N-5;  R4: d <= min(CWINDOW, p)   ('&': no short-circuit branches)
        uint64_t okm = __builtin_amdgcn_ballot_w64(d4 <= p4_run + (uint32_t)(4 * i));      // (the compare's own lane mask)
        if constexpr (!FULLWIN) okm &= __builtin_amdgcn_ballot_w64(d4 <= cw4);
        if constexpr (SCALAR_TAIL) okm &= ((uint32_t)i <= thr ? m_hi : m_lo);
        else okm &= __builtin_amdgcn_ballot_w64(nrem >= (uint32_t)(i + 5));
        // distance for the gather; for "no match" any in-range value will do (the result is discarded)
        // (NCH == 1: a plain shift -- v_lshrrev is a full-rate instruction, v_bfe / v_and + shift are not, profiles/r04_ubench/ubench_valu_cycles2.txt;
        //  a raw minimum that means "none" then gathers at some masked address inside the caller's LDS block, see GMASK; the result is discarded)
        const uint32_t d = (NCH == 1) ? (d4 >> 2) : __builtin_amdgcn_ubfe(d4, 2u, 9u);      // (NO_MATCH4 reads as 1)
        // R5: common prefix of x[p+3..p+10] and x[p-d+3..p-d+10]
        const uint32_t q = lds_run + (uint32_t)(i + 3) - d;   // byte offset of the candidate's 4th byte
        const uint32_t qd = (q >> 2) & GMASK;
        const uint32_t a0 = in[qd], a1 = in[qd + 1], a2 = in[qd + 2];
        const uint32_t clo = alignbyte(a1, a0, q), chi = alignbyte(a2, a1, q);      // (v_alignbyte takes the shift from q[1:0])
        constexpr int o = i + 3;
        uint32_t olo, ohi;
        if constexpr ((o & 3) == 0) { olo = ow[o >> 2]; ohi = ow[(o >> 2) + 1]; }
        else { olo = alignbyte(ow[(o >> 2) + 1], ow[o >> 2], o & 3); ohi = alignbyte(ow[(o >> 2) + 2], ow[(o >> 2) + 1], o & 3); }
        // equal low BITS of the two 8-byte windows.  Only 7 bytes can matter (len <= 10): a sentinel in the top bit of
        // the eighth bounds the count at 63 (-> 7 bytes) and keeps ffbl away from its "no bit set" value
        const uint32_t zhi = ffbl((chi ^ ohi) | 0x80000000u) | 32u;
        uint32_t zlo;                                            // v_ffbl_b32(0) = 0xFFFFFFFF: "no difference in the low half"
        asm("v_ffbl_b32 %0, %1" : "=v"(zlo) : "v"(clo ^ olo));   // (asm: hipcc turns ffs()-1 + min into a compare and a select)
        uint32_t zb;                                             // min(zlo, zhi): zhi <= 63 and zlo is a bit index or 0xFFFFFFFF, so the 16-bit
        asm("v_min_u16 %0, %1, %2" : "=v"(zb) : "v"(zlo), "v"(zhi));   // minimum is the minimum (full rate; v_min_u32 is not), upper half zero
        // len - 3 = min(equal bytes, Kmax - 3, N-2-p - 3): a match never covers the last two bytes
        const uint32_t l3 = umin3(zb >> 3, kmax_m3, nrem_m5 - (uint32_t)i);
        // literal byte -> LUT offset 4*byte
        constexpr int bsh = 8 * (i & 3);
        uint32_t lit;
        if constexpr (bsh == 0) lit = (ow[i >> 2] << 2) & 0x3FCu;
        else lit = (ow[i >> 2] >> (bsh - 2)) & 0x3FCu;
        uint32_t mt;     // l3 * tok_mul + d4 + tok_k  (hipcc folds the C form into a quarter-rate v_mul_lo_u32)
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(mt) : "v"(l3), "s"(tok_mul), "v"(d4 + tok_k));
        asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(tok[i]) : "v"(lit), "v"(mt), "s"(okm));      // tok = ok ? mt : lit
        // (positions per scheduling group: the gathers of a group are in flight together; profiles/r05_tile_timing.txt)
        constexpr int EG = HDLZ_EXT_GROUP;
        if constexpr ((i & (EG - 1)) == EG - 1) { pin_range<(i & ~(EG - 1)), (i & ~(EG - 1)) + EG>(tok); PHASE_FENCE(); }
    });
}

// ---- phase 3 of the one-tile kernels with the bit search: the same tok[] and the same eligibility test, the LENGTH from the mismatch
// words the search kept (WaveLdsBits::neq) instead of a byte compare.  For position i of the lane and its distance d, bit j of neq_d says
// x[32 l + j] != x[32 l + j - d], so len - 3 = the zero bits of (neq_d of lane l + 1 : neq_d) from bit i + 3 on, capped like the byte form:
//   word   NEQ[(d & 31) * 64 + l]: byte offset (d4 & 0x7C) << 6 + 4 l.  d = 32 reads row 0, "none" (0xFF) row 31 (discarded)
//   i <= 22: bits i + 3 .. i + 9 lie in the lane's own word -- a plain shift (at most Kmax - 3 <= 7 bits count);  i = 23 .. 28: the
//          next lane's word of the same row too, one v_alignbit;  i >= 29: bit i + 3 is bit i - 29 of the next lane's word -- that word
//          alone, a plain shift.  Lane 63 has no next lane: it reads its own word in that place (col_hi = 4 * min(l + 1, 63)); its own
//          word has the end cap's bit at N - 2 - p_run <= 30, so the count stops inside the own word before those bits are reached
//          (i >= 28 is not eligible there)
//   l3     min(ffbl(x), Kmax - 3): v_ffbl_b32(0) = 0xFFFFFFFF needs no sentinel under the cap; the block's end is a set bit of the
//          words themselves (end_cap_word: bit N - 2 - p_run of the lane that holds it, so ffbl(x) <= N - 5 - p wherever p is eligible;
//          a lane whose word has no such bit has N - 2 - p_run >= 32 and N - 5 - p >= 7 >= Kmax - 3 for its i <= 22, and its i >= 23
//          read on into the next lane's word, which carries the bit or leaves at least 7 again)
//          (Measured and dropped, profiles/tile_diet.txt: the cap as a sentinel bit, ffbl(x | 1 << (Kmax - 3)), a v_or_b32 in place of the
//          v_min_u32: 30 slow instructions fewer per tile and no difference in time)
// Lane 0's bits j < d compare against lane 63's bytes (the search's rotate): a position i of lane 0 is eligible only for d <= i, and its
// bits j >= i + 3 > d look at the block's own bytes.  11 VALU instructions per position (12 for i >= 23) against 22, one or two
// conflict-free ds_read_b32 (bank = column, whatever the row) against three gathered dwords.
// token word of the literal at own position I: the LUT offset 4 * byte (upper half 0: length 1)
template <int I>
__device__ __forceinline__ uint32_t literal_token(const uint32_t (&ow)[12]) {
    constexpr int bsh = 8 * (I & 3);
    if constexpr (bsh == 0) return (ow[I >> 2] << 2) & 0x3FCu;
    else return (ow[I >> 2] >> (bsh - 2)) & 0x3FCu;
}
// a match-free tile (match_search_bits returned false): every token is its literal.  The -DHDLZ_LITERAL_TOKENS form only: two
// instructions per position that token_codes then reads back; literal_codes (below token_codes) needs no token at all
__device__ __forceinline__ void literal_tokens(const uint32_t (&ow)[12], uint32_t (&tok)[RUN]) {
    static_for<0, RUN>([&](auto I) { tok[decltype(I)::value] = literal_token<decltype(I)::value>(ow); });
}
// SUB-DWORD OPERANDS (-DHDLZ_EXT_SDWA=0: off, for A/B).  The result byte of a position has three readers -- the eligibility compare, the row
// mask and the token's distance term -- and the literal's LUT offset is one byte of the own bytes times four.  The SDWA forms of v_cmp,
// v_and, v_add and v_lshlrev take a byte of a register as their operand.  Measured (tools/ubench/valu_cycles4.hip, profiles/
// wave_groups.txt): the compare and the shift cost what their plain forms cost (3.1 / 3.25 cycles), v_and and v_add move from the 1.97- to
// the 3.25-cycle class -- 2.6 cycles more per position, which is what the extract (v_bfe 3.25, v_and / v_lshr 1.97) cost: even in cycles,
// one instruction and one live register per position less.  What the packed form GAINS comes with it: thresholds packed like the result
// bytes (one v_add per four positions instead of one v_or each) and a literal that needs no mask in byte 0 either.  (Inline asm with whole-dword destinations: no instruction here writes part of a register,
// which is the one SDWA case with a read-after-write rule of its own.)
#ifndef HDLZ_EXT_SDWA
#define HDLZ_EXT_SDWA 1
#endif
#define HDLZ_SDWA_SRC0_BYTE(op, M) op " %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_" #M " src1_sel:DWORD"
template <int M> __device__ __forceinline__ uint32_t and_byte(uint32_t q, uint32_t s) {             // ((q >> 8 M) & 0xFF) & s
    uint32_t r;
    if constexpr (M == 0) asm(HDLZ_SDWA_SRC0_BYTE("v_and_b32_sdwa", 0) : "=v"(r) : "v"(q), "s"(s));
    else if constexpr (M == 1) asm(HDLZ_SDWA_SRC0_BYTE("v_and_b32_sdwa", 1) : "=v"(r) : "v"(q), "s"(s));
    else if constexpr (M == 2) asm(HDLZ_SDWA_SRC0_BYTE("v_and_b32_sdwa", 2) : "=v"(r) : "v"(q), "s"(s));
    else asm(HDLZ_SDWA_SRC0_BYTE("v_and_b32_sdwa", 3) : "=v"(r) : "v"(q), "s"(s));
    return r;
}
template <int M> __device__ __forceinline__ uint32_t add_byte(uint32_t q, uint32_t s) {             // ((q >> 8 M) & 0xFF) + s
    uint32_t r;
    if constexpr (M == 0) asm(HDLZ_SDWA_SRC0_BYTE("v_add_u32_sdwa", 0) : "=v"(r) : "v"(q), "s"(s));
    else if constexpr (M == 1) asm(HDLZ_SDWA_SRC0_BYTE("v_add_u32_sdwa", 1) : "=v"(r) : "v"(q), "s"(s));
    else if constexpr (M == 2) asm(HDLZ_SDWA_SRC0_BYTE("v_add_u32_sdwa", 2) : "=v"(r) : "v"(q), "s"(s));
    else asm(HDLZ_SDWA_SRC0_BYTE("v_add_u32_sdwa", 3) : "=v"(r) : "v"(q), "s"(s));
    return r;
}
#define HDLZ_SDWA_CMP_BYTE(M, S1) "v_cmp_le_u32_sdwa %0, %1, %2 src0_sel:BYTE_" #M " src1_sel:" S1
template <int M, bool BOTH> __device__ __forceinline__ uint64_t le_byte(uint32_t q, uint32_t s) {   // lanes with byte M of q <= s (BOTH: <= byte M of s)
    uint64_t r;
    if constexpr (BOTH) {
        if constexpr (M == 0) asm(HDLZ_SDWA_CMP_BYTE(0, "BYTE_0") : "=s"(r) : "v"(q), "v"(s));
        else if constexpr (M == 1) asm(HDLZ_SDWA_CMP_BYTE(1, "BYTE_1") : "=s"(r) : "v"(q), "v"(s));
        else if constexpr (M == 2) asm(HDLZ_SDWA_CMP_BYTE(2, "BYTE_2") : "=s"(r) : "v"(q), "v"(s));
        else asm(HDLZ_SDWA_CMP_BYTE(3, "BYTE_3") : "=s"(r) : "v"(q), "v"(s));
    } else {
        if constexpr (M == 0) asm(HDLZ_SDWA_CMP_BYTE(0, "DWORD") : "=s"(r) : "v"(q), "s"(s));
        else if constexpr (M == 1) asm(HDLZ_SDWA_CMP_BYTE(1, "DWORD") : "=s"(r) : "v"(q), "s"(s));
        else if constexpr (M == 2) asm(HDLZ_SDWA_CMP_BYTE(2, "DWORD") : "=s"(r) : "v"(q), "s"(s));
        else asm(HDLZ_SDWA_CMP_BYTE(3, "DWORD") : "=s"(r) : "v"(q), "s"(s));
    }
    return r;
}
#define HDLZ_SDWA_SHL_BYTE(M) "v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_" #M
template <int M> __device__ __forceinline__ uint32_t shl_byte(uint32_t sh, uint32_t w) {            // ((w >> 8 M) & 0xFF) << sh
    uint32_t r;
    if constexpr (M == 0) asm(HDLZ_SDWA_SHL_BYTE(0) : "=v"(r) : "s"(sh), "v"(w));
    else if constexpr (M == 1) asm(HDLZ_SDWA_SHL_BYTE(1) : "=v"(r) : "s"(sh), "v"(w));
    else if constexpr (M == 2) asm(HDLZ_SDWA_SHL_BYTE(2) : "=v"(r) : "s"(sh), "v"(w));
    else asm(HDLZ_SDWA_SHL_BYTE(3) : "=v"(r) : "s"(sh), "v"(w));
    return r;
}
// make_tokens_bits on the packed result bytes (a ONE-TILE block: the tile starts at position 0).  Position i = k + 8 m reads byte m of
// Q[k]; the positions are taken register by register (k outer) -- tok[] does not care about the order -- so that the eligibility
// thresholds can be packed the same way: d4 <= 4 p is  d4 <= 4 i  in lane 0 and "d4 is a distance at all" (d4 <= 128 < 0xFF) in every
// other lane, where ANY threshold in [128, 254] will do.  T_k byte m = 4 (k + 8 m) in lane 0, 0x80 + 32 m + 4 k elsewhere (at most 0xFC):
// T_k = T_0 + 0x04040404 k without a carry between the bytes, one v_add per FOUR positions, compared byte against byte.
template <bool FULLWIN>
__device__ __forceinline__ void make_tokens_bits_packed(const uint32_t* neq, uint32_t lane, uint32_t (&ow)[12], uint32_t (&Q)[8], uint32_t cw4,
                                                        uint32_t kmax, uint32_t (&tok)[RUN], int32_t tile_rem) {
    pin(Q);
    PHASE_FENCE();
    const uint32_t kmax_m3 = min(kmax - 3u, 7u);              // (MAXMATCH is 5 or 10: the clamp keeps the single-word shift exact whatever comes in)
    const int32_t rem5 = tile_rem - 5;                        // R3's "p <= N - 5" as lane masks: see make_tokens (SCALAR_TAIL)
    const uint32_t thr = rem5 >= 0 ? ((uint32_t)rem5 & 31u) : 0u;
    const int32_t cnt_hi = rem5 >= 0 ? (rem5 >> 5) + 1 : 0, cnt_lo = rem5 >= 0 ? (rem5 >> 5) : 0;
    const uint64_t m_hi = cnt_hi >= 64 ? ~0ull : ((1ull << cnt_hi) - 1ull), m_lo = cnt_lo >= 64 ? ~0ull : ((1ull << cnt_lo) - 1ull);
    const uint32_t tok_mul = 4u * 65536u + 128u;
    const uint8_t* neq8 = reinterpret_cast<const uint8_t*>(neq);
    const uint32_t col_lo = 4u * lane, dcol = min(252u - col_lo, 4u);                 // col_hi = col_lo + dcol = 4 * min(lane + 1, 63)
    // the constant operands of the sub-dword forms live in SGPRs (they take no literal constant)
    const uint32_t tok_k = sconst((2u << 18) + LUT_MATCH_BYTE - 4u), row_mask = sconst(0x7Cu), two = sconst(2u), cw4v = cw4;
    uint32_t T = lane == 0u ? 0x60402000u : 0xE0C0A080u;
    asm volatile("" : "+v"(T));
    static_for<0, RUN>([&](auto J) {
        constexpr int k = decltype(J)::value >> 2, m = decltype(J)::value & 3, i = k + 8 * m;
        if constexpr (m == 0 && k != 0) T += 0x04040404u;
        uint64_t okm = le_byte<m, true>(Q[k], T);
        if constexpr (!FULLWIN) okm &= le_byte<m, false>(Q[k], cw4v);
        okm &= ((uint32_t)i <= thr ? m_hi : m_lo);
        uint32_t a0;     // ((d4 & 0x7C) << 6) + col_lo
        asm("v_lshl_add_u32 %0, %1, 6, %2" : "=v"(a0) : "v"(and_byte<m>(Q[k], row_mask)), "v"(col_lo));
        uint32_t x;      // (next lane's word : own word) >> (i + 3)
        if constexpr (i + 3 + 7 <= 32) x = *reinterpret_cast<const uint32_t*>(neq8 + a0) >> (i + 3);
        else if constexpr (i + 3 >= 32) x = *reinterpret_cast<const uint32_t*>(neq8 + (a0 + dcol)) >> (i + 3 - 32);      // (v_alignbit shifts by 0 .. 31)
        else x = __builtin_amdgcn_alignbit(*reinterpret_cast<const uint32_t*>(neq8 + (a0 + dcol)), *reinterpret_cast<const uint32_t*>(neq8 + a0), (uint32_t)(i + 3));
        uint32_t z;
        asm("v_ffbl_b32 %0, %1" : "=v"(z) : "v"(x));
        const uint32_t l3 = min(z, kmax_m3);                     // (N - 5 - p: the end cap in the word)
        const uint32_t lit = shl_byte<(i & 3)>(two, ow[i >> 2]); // the LUT offset 4 * byte
        uint32_t mt;     // l3 * tok_mul + d4 + tok_k
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(mt) : "v"(l3), "s"(tok_mul), "v"(add_byte<m>(Q[k], tok_k)));
        asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(tok[i]) : "v"(lit), "v"(mt), "s"(okm));      // tok = ok ? mt : lit
        if constexpr (m == 3) { asm volatile("" : "+v"(tok[k]), "+v"(tok[k + 8]), "+v"(tok[k + 16]), "+v"(tok[k + 24]), "+v"(T)); PHASE_FENCE(); }
    });
}
template <bool FULLWIN>
__device__ __forceinline__ void make_tokens_bits(const uint32_t* neq, uint32_t lane, uint32_t (&ow)[12], uint32_t (&best)[RUN], uint32_t cw4,
                                                 uint32_t kmax, uint32_t p4_run, uint32_t (&tok)[RUN], int32_t tile_rem) {
    pin(best); pin_range<0, 8>(ow);
    PHASE_FENCE();
    const uint32_t kmax_m3 = min(kmax - 3u, 7u);              // (MAXMATCH is 5 or 10: the clamp keeps the single-word shift exact whatever comes in)
    const int32_t rem5 = tile_rem - 5;                        // R3's "p <= N - 5" as lane masks: see make_tokens (SCALAR_TAIL)
    const uint32_t thr = rem5 >= 0 ? ((uint32_t)rem5 & 31u) : 0u;
    const int32_t cnt_hi = rem5 >= 0 ? (rem5 >> 5) + 1 : 0, cnt_lo = rem5 >= 0 ? (rem5 >> 5) : 0;
    const uint64_t m_hi = cnt_hi >= 64 ? ~0ull : ((1ull << cnt_hi) - 1ull), m_lo = cnt_lo >= 64 ? ~0ull : ((1ull << cnt_lo) - 1ull);
    const uint32_t tok_k = (2u << 18) + LUT_MATCH_BYTE - 4u;  // token word of a match: l3 * tok_mul + 4 d + tok_k (make_tokens)
    const uint32_t tok_mul = 4u * 65536u + 128u;
    const uint8_t* neq8 = reinterpret_cast<const uint8_t*>(neq);
    const uint32_t col_lo = 4u * lane, dcol = 4u * min(lane + 1u, 63u) - col_lo;      // col_hi = col_lo + dcol
    static_for<0, RUN>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const uint32_t d4 = best[i];
        uint64_t okm = __builtin_amdgcn_ballot_w64(d4 <= p4_run + (uint32_t)(4 * i));
        if constexpr (!FULLWIN) okm &= __builtin_amdgcn_ballot_w64(d4 <= cw4);
        okm &= ((uint32_t)i <= thr ? m_hi : m_lo);
        uint32_t a0;     // ((d4 & 0x7C) << 6) + col_lo  (hipcc shifts first, masks and adds: three instructions)
        asm("v_lshl_add_u32 %0, %1, 6, %2" : "=v"(a0) : "v"(d4 & 0x7Cu), "v"(col_lo));
        uint32_t x;      // (next lane's word : own word) >> (i + 3)
        if constexpr (i + 3 + 7 <= 32) x = *reinterpret_cast<const uint32_t*>(neq8 + a0) >> (i + 3);
        else if constexpr (i + 3 >= 32) x = *reinterpret_cast<const uint32_t*>(neq8 + (a0 + dcol)) >> (i + 3 - 32);      // (v_alignbit shifts by 0 .. 31)
        else x = __builtin_amdgcn_alignbit(*reinterpret_cast<const uint32_t*>(neq8 + (a0 + dcol)), *reinterpret_cast<const uint32_t*>(neq8 + a0), (uint32_t)(i + 3));
        uint32_t z;                                              // v_ffbl_b32(0) = 0xFFFFFFFF: "no difference in sight"
        asm("v_ffbl_b32 %0, %1" : "=v"(z) : "v"(x));             // (asm: hipcc turns ffs()-1 + min into a compare and a select)
        const uint32_t l3 = min(z, kmax_m3);                     // (N - 5 - p: the end cap in the word, see above)
        const uint32_t lit = literal_token<i>(ow);
        uint32_t mt;     // l3 * tok_mul + d4 + tok_k  (hipcc folds the C form into a quarter-rate v_mul_lo_u32)
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(mt) : "v"(l3), "s"(tok_mul), "v"(d4 + tok_k));
        asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(tok[i]) : "v"(lit), "v"(mt), "s"(okm));      // tok = ok ? mt : lit
        constexpr int EG = HDLZ_EXT_GROUP;
        if constexpr ((i & (EG - 1)) == EG - 1) { pin_range<(i & ~(EG - 1)), (i & ~(EG - 1)) + EG>(tok); PHASE_FENCE(); }
    });
}

// ---- phase 4a, greedy parse of one run ("di += m / di += 1", deflate.py:960,1008 -- a serial chain in the reference) folded
// into a TRANSFER FUNCTION "entry skip (0..9) -> exit skip": nibble s of the result = exit skip for entry skip s.
// Backward pass: E[i] = exit skip if a token starts at local index i; nibbles of P hold E[i+1..i+10].
__device__ __forceinline__ uint64_t run_transfer(const uint32_t (&tok)[RUN]) {
    uint64_t P = 0x9876543210ull;
#pragma unroll
    for (int i = RUN - 1; i >= 0; i--) {
        const uint32_t sh = tok[i] >> 16;                     // 4 * (len-1)
        const uint32_t e = (uint32_t)(P >> sh) & 15u;
        P = (P << 4) | e;
    }
    return P;
}

// ---- phase 4b: compose the 64 run functions across the wave.  s: in = entry skip of lane 0, out = exit skip of lane 63; returns this
// lane's entry skip.
// Round 5: a run function is almost always CONSTANT -- whatever the entry skip, the parse of 32 positions falls into step at the first
// literal or cut-short match (0 / 0 / 0 / 4 % of the runs of the four bench families are not constant; data whose matches follow each
// other at full length through the whole run -- zeros, short periods -- is what keeps a function a rotation).  A lane behind a constant
// function knows its entry skip at once, a lane behind a chain of k others after k steps of "take the previous lane's exit through my own
// function" (one DPP move + a nibble pick per step, all lanes at once).  Up to CHAIN_STEPS such steps; a wave that still has an open lane
// then takes the serial composition on the scalar unit, which is exact for every input (64 steps of ~6 dependent scalar instructions:
// 7.7 k of the 52.6 k cycles a wave spent per tile, profiles/r05_tile_timing.txt -- a wave in that loop issues nothing else).
constexpr int CHAIN_STEPS = 4;
__device__ __forceinline__ uint32_t chain_skips_serial(uint64_t P, uint32_t lane, uint32_t& s);
__device__ __forceinline__ uint32_t chain_skips(uint64_t P, uint32_t lane, uint32_t& s) {
    const uint32_t plo = (uint32_t)P, phi = (uint32_t)(P >> 32) & 0xFFu;
#ifndef HDLZ_CHAIN_SERIAL_ONLY
    // all ten nibbles equal  <=>  P ^ (P >> 4) has no bit in its low 36
    const uint32_t dl = plo ^ __builtin_amdgcn_alignbit(phi, plo, 4u), dh = (phi ^ (phi >> 4)) & 15u;
    uint32_t x = (dl | dh) == 0u ? (plo & 15u) : 16u;           // this lane's EXIT skip, 16 = not known yet
#ifdef HDLZ_CHAIN_FORCE_SERIAL                                   // test build: every wave takes the scalar composition
    x = 16u;
#endif
    bool open = ballot64(x >= 16u) != 0ull;
#pragma unroll 1
    for (int it = 0; it < CHAIN_STEPS && open; it++) {
        const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp((int)s, (int)x, 0x138, 0xF, 0xF, false);      // wave_shr:1; lane 0 keeps s
        const uint32_t via = (uint32_t)(P >> (4u * (prev & 15u))) & 15u;
        x = (x >= 16u && prev < 16u) ? via : x;
        open = ballot64(x >= 16u) != 0ull;
    }
    if (!open) {
        const uint32_t e = (uint32_t)__builtin_amdgcn_update_dpp((int)s, (int)x, 0x138, 0xF, 0xF, false);
        s = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
        return e;
    }
#endif
    return chain_skips_serial(P, lane, s);
}
__device__ __forceinline__ uint32_t chain_skips_serial(uint64_t P, uint32_t lane, uint32_t& s) {
    const uint32_t plo = (uint32_t)P;
    // the upper part of a function is 8 bits (entry skips 8 and 9): the four of a quad of lanes are packed into ONE register first (two
    // quad-permute moves), so the scalar chain reads 64 + 16 lanes instead of 2 x 64 (v_readlane is a 3.25-cycle instruction)
    uint32_t ph4 = (uint32_t)(P >> 32) & 0xFFu;
    ph4 |= (uint32_t)__builtin_amdgcn_mov_dpp((int)ph4, 0xB1, 0xF, 0xF, true) << 8;      // quad_perm [1,0,3,2]: lanes 0 / 2 of a quad get their neighbour
    ph4 |= (uint32_t)__builtin_amdgcn_mov_dpp((int)ph4, 0x4E, 0xF, 0xF, true) << 16;     // quad_perm [2,3,0,1]: lane 0 gets the pair of lanes 2, 3
    uint64_t sv[4] = {0, 0, 0, 0};     // entry skips of all 64 lanes, one nibble each (scalar regs)
    // 4 segments of 16 lanes; the scheduling barriers keep the compiler from hoisting all the
    // readlanes to the top (that needed ~260 SGPR spills = v_writelane/v_readlane traffic)
    static_for<0, 4>([&](auto G) {
        constexpr int g = decltype(G)::value;
        uint64_t acc = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            // NB: readlane returns a signed int -- cast before widening or bit 31 smears into the high half
            const uint32_t hi4 = (uint32_t)__builtin_amdgcn_readlane((int)ph4, g * 16 + q * 4);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int l = q * 4 + k;
                acc |= (uint64_t)s << (4 * l);
                const uint64_t f = ((uint64_t)((hi4 >> (8 * k)) & 0xFFu) << 32) |
                                   (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)plo, g * 16 + l);
                s = (uint32_t)(f >> (4u * s)) & 15u;
            }
        }
        sv[g] = acc;
        __builtin_amdgcn_sched_barrier(0);
    });
    const uint32_t g = lane >> 4;
    const uint64_t mine = g == 0 ? sv[0] : g == 1 ? sv[1] : g == 2 ? sv[2] : sv[3];
    return (uint32_t)(mine >> (4u * (lane & 15u))) & 15u;
}

// ---- phase 5a, token bits (R6/R7; DISTANCE deflate.py:836-882, literal emit :1005-1016) from the per-wave LDS LUTs:
// code[i] = LUT entry (code << CODE_SHIFT | nbits) of every token START, 0 elsewhere; returns the lane's bit count.
//   c0      this lane's entry skip (a value >= 32 = the lane starts no token at all)
//   LIMIT   only positions i < nlimit may start a token (padding positions of a packed small block)
// The bit count is the sum of the ENTRIES, masked once: the counts sit in the entries' low bits (NB_SUM_MASK), one v_add per position
// (half a v_add3) where a count in the top bits cost a shift as well.
// (Measured and dropped, profiles/tile_diet.txt: the start flag as a mask in a register -- (c - 4) >> 31, v_bitop3 select, v_and: 5.5
// instructions per position, all of the 1.96-cycle class, where hipcc turns the selects below into a v_cmp and an exec-masked region
// with five scalar instructions per position -- was 0.03 ms SLOWER on the headline, three runs against three.)
// (A match-free tile of the one-tile bit-search kernels does not come here: every position starts a literal, literal_codes below.)
template <int NCH, bool LIMIT>
__device__ __forceinline__ uint32_t token_codes(const uint8_t* lut8, uint32_t (&tok)[RUN], uint32_t c0, uint32_t nlimit,
                                                uint32_t (&code)[RUN]) {
    uint32_t acc = 0;                                         // sum of the entries: its NB_SUM_MASK field is the lane's bit count
    uint32_t c = 4u * c0;                                     // positions still covered by the last token, times four (the token word's unit)
    static_for<0, RUN>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const uint32_t e = *reinterpret_cast<const uint32_t*>(lut8 + (tok[i] & 0xFFFFu));
        bool start = (c == 0u);
        if constexpr (LIMIT) start = start & ((uint32_t)i < nlimit);
        const uint32_t lenm1x4 = tok[i] >> 16;
        c = start ? lenm1x4 : (c - 4u);
        uint32_t ee = e;
        if constexpr (NCH != 1)                               // wide windows: [dist] LUT + the length code from its own small LUT
            ee |= *reinterpret_cast<const uint32_t*>(lut8 + LUT_LEN_BYTE + lenm1x4);        // (computed: six VALU instructions per position)
        code[i] = start ? ee : 0u;
        acc += code[i];
        constexpr int CG = HDLZ_CODE_GROUP;
        if constexpr ((i & (CG - 1)) == CG - 1) { pin_range<(i & ~(CG - 1)), (i & ~(CG - 1)) + CG>(code); asm volatile("" : "+v"(c), "+v"(acc)); PHASE_FENCE(); }
    });
    return (acc & NB_SUM_MASK) >> NB_SHIFT;
}
// ... of a MATCH-FREE tile: every position starts a one-byte token (entry skip 0, padding positions behind a short block's end
// included: 8-bit literals that wipe_behind removes), so there is no start flag, no count and no token word -- code[i] is the LUT entry
// at 4 * byte, the address one sub-dword shift of the own bytes (as the extension forms its literal), the bit count the sum of the
// entries masked once.  Two VALU instructions per position where literal_tokens + token_codes had about eight, and the 32 LUT reads
// run under no exec mask.
__device__ __forceinline__ uint32_t literal_codes(const uint8_t* lut8, const uint32_t (&ow)[12], uint32_t (&code)[RUN]) {
    static_assert(4u * 255u + 4u <= 4u * (uint32_t)LUT_LIT, "every byte's offset inside the literal LUT");
    uint32_t acc = 0;
    const uint32_t two = sconst(2u);
    static_for<0, RUN>([&](auto I) {
        constexpr int i = decltype(I)::value;
        code[i] = *reinterpret_cast<const uint32_t*>(lut8 + shl_byte<(i & 3)>(two, ow[i >> 2]));
        acc += code[i];
        constexpr int CG = HDLZ_CODE_GROUP;
        if constexpr ((i & (CG - 1)) == CG - 1) { pin_range<(i & ~(CG - 1)), (i & ~(CG - 1)) + CG>(code); asm volatile("" : "+v"(acc)); PHASE_FENCE(); }
    });
    return (acc & NB_SUM_MASK) >> NB_SHIFT;
}

// inclusive wave scan (all 64 lanes must call it): Hillis-Steele inside the rows of 16 (row_shr 1, 2, 4, 8; a lane without a source adds 0),
// then the row totals across (row_bcast15 into rows 1 and 3, row_bcast31 into rows 2 and 3) -- six DPP adds; the shuffle form
// (__shfl_up = ds_bpermute + compare + select per step) was 38 VALU + 6 LDS instructions
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);      // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);      // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);      // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);      // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);     // row_bcast15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);     // row_bcast31 -> rows 2, 3
    return v;
}

// ---- phase 5b, the bit writer (put / do_flush, deflate.py:535-567): OR every token into the LDS bit buffer at its own
// bit offset (ds_or_b32), the lane's first token at bit `bp`.
// The codes of two consecutive positions are joined first and go out as ONE value: 32 ds_or pairs per run instead of 64, 11 instead
// of 14 VALU instructions per pair.  A pair never holds two match tokens -- a match covers at least three positions, so the position
// behind a match start starts nothing --: at most a 9-bit literal and a match of 7 + 5 + 6 bits (CWINDOW 256), 27 bits in a 32-bit
// word.  (Round 4, first half: CWINDOW <= 32 only, reasoned from two 15-bit tokens; the bound above holds for every window.)
__device__ __forceinline__ void scatter_codes(uint8_t* out8, const uint32_t (&code)[RUN], uint32_t bp) {
#pragma unroll
    for (int i = 0; i < RUN; i += 2) {
        const uint32_t n0 = (code[i] & NB_MASK) >> NB_SHIFT;
        const uint32_t c = ((code[i + 1] >> CODE_SHIFT) << n0) | (code[i] >> CODE_SHIFT);
        const uint64_t v = (uint64_t)c << (bp & 31u);
        uint32_t* w = reinterpret_cast<uint32_t*>(out8 + ((bp >> 3) & ~3u));
        __hip_atomic_fetch_or(w, (uint32_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_or(w + 1, (uint32_t)(v >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        bp += n0 + ((code[i + 1] & NB_MASK) >> NB_SHIFT);
        if ((i & 6) == 6) { asm volatile("" : "+v"(bp)); PHASE_FENCE(); }
    }
}

// ---- phase 6, Adler-32 partials of the run (deflate.py:826-831, :888-897): sa = sum x_i, sc = sum i * x_i (i = 0..31)
__device__ __forceinline__ void adler_run(const uint32_t (&ow)[12], uint32_t& sa, uint32_t& sc) {
    sa = 0; sc = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        sa = __builtin_amdgcn_sad_u8(ow[k], 0u, sa);
        const uint32_t wts = (uint32_t)(4 * k) | ((uint32_t)(4 * k + 1) << 8) | ((uint32_t)(4 * k + 2) << 16) | ((uint32_t)(4 * k + 3) << 24);
        sc = __builtin_amdgcn_udot4(ow[k], wts, sc, false);
    }
}

// sum of v over the 64 lanes, as a wave-uniform value: four DPP adds inside the rows of 16 (quad permutes, half mirror, mirror: every lane
// then holds its row's sum) and four v_readlane -- the xor butterfly through ds_bpermute was 36 VALU + 12 LDS instructions for two sums
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);       // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);       // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);      // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);      // row_mirror
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// ---- the framing of a zlib block (R1, R8, R9): ONE source for the four drivers (k_compress, k_compress_small, k_compress_chunk and
// k_stream_place with the scans that feed it)
constexpr uint32_t HEADER_WORD = 0x78u | (0x9Cu << 8) | (0x3u << 16);      // R1: 78 9C + bits 1,1,0 (BFINAL, BTYPE = 01) ...
constexpr uint32_t HEADER_BITS = 19;                                         // ... the first token starts at this bit
// Positions >= N of a block's last tile are zero bytes: they never match (R3), each is parsed as one 8-bit literal, and the bits of
// all of them sit behind the real end of the block -- which is therefore PAD_BITS * (t0 + TILE - n) bits in front of the tile's last bit
constexpr uint32_t PAD_BITS = 8;
// wipe what was written behind the real end (bit end_bits), word k counted from the one the end lies in: that word masked, the ones
// behind it zeroed.  (How far: the driver's extent -- k_compress the four words that can still go out, k_compress_chunk its whole buffer.)
__device__ __forceinline__ void wipe_behind(uint32_t* lout, uint32_t end_bits, uint32_t k) {
    const uint32_t ew = end_bits >> 5, rb = end_bits & 31u;
    lout[ew + k] = (k == 0u) ? (lout[ew] & ((1u << rb) - 1u)) : 0u;
}
// R8: bytes of the block up to the trailer = the tokens, EOB (7 zero bits), zero padding to a byte (32- and 64-bit bit counts)
template <class U> __device__ __forceinline__ U block_nbytes(U end_bits) { return (end_bits + 7u + 7u) >> 3; }
// |M_b|, the member a row of n bytes that ends at bit E becomes in a joined stream (hdlz_join.h), and in `body` the bytes of it that
// come from the row; 0: the row's length, its end bit and the pitch contradict each other
__device__ __forceinline__ uint32_t member_len(uint32_t n, uint64_t E, uint64_t pitch, uint32_t& body) {
    body = 0u;
    if (E < HEADER_BITS || block_nbytes(E) + 4u != (uint64_t)n || (uint64_t)n > pitch) return 0u;
    const uint32_t nbytes = n - 4u;
    const uint32_t p = (uint32_t)(8ull * nbytes - E) - 7u;       // pad bits behind the end-of-block code
    body = nbytes - 2u;
    return body + (p >= 3u ? 4u : 5u);
}
// R8: Adler-32 of the block from A = sum x_p and W = sum (N - p) x_p (any residues mod 65521, 32 or 64 bits wide)
// (A ONE-TILE block needs no reduction in front of this one: a lane's weight N - p_run is at most TILE, its run sums to at most 32 * 255, so
// its term sum (N - p) x_p = (N - p_run) * sa - sc is at most TILE * 8160, and the wave's 64 terms stay below 2^31 -- k_compress sums
// them plainly, without the modulo per tile and the carried weight of the multi-tile kernels.)
static_assert(64ull * TILE * (RUN * 255ull) < (1ull << 31) && 64ull * (RUN * 255ull) + 1ull < (1ull << 31) && (uint64_t)TILE < (uint64_t)ADLER_MOD,
              "one-tile blocks: the plain Adler sums of a wave fit 31 bits");
template <class U> __device__ __forceinline__ void adler_finish(U A, U W, uint32_t n, uint32_t& s1, uint32_t& s2) {
    s1 = (uint32_t)((A + 1u) % ADLER_MOD);
    s2 = (uint32_t)((W + n % ADLER_MOD) % ADLER_MOD);
}
// R8: byte k (0 .. 3) of the trailer -- big-endian, s2 then s1 -- and the four of them behind the block's nbytes bytes
__device__ __forceinline__ uint32_t adler_byte(uint32_t k, uint32_t s1, uint32_t s2) {
    const uint32_t s = k < 2u ? s2 : s1;
    return (k & 1u) ? (s & 255u) : (s >> 8);
}
__device__ __forceinline__ void put_adler(uint8_t* out8, uint32_t nbytes, uint32_t s1, uint32_t s2) {
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) out8[nbytes + k] = (uint8_t)adler_byte(k, s1, s2);
}

// zero the bit buffer of a tile and seed its first word (16-byte stores: 3 LDS instructions per lane instead of 10)
__device__ __forceinline__ void zero_bit_buffer(uint32_t* lout, uint32_t lane, uint32_t carry_word) {
    static_assert(OUT_WORDS % 4 == 0, "16-byte stores");
    for (uint32_t q = lane; q < (uint32_t)OUT_WORDS / 4u; q += 64u)
        *reinterpret_cast<uint4*>(lout + 4u * q) = make_uint4(q == 0u ? carry_word : 0u, 0u, 0u, 0u);
}

// fill the per-wave LUTs (literal: [byte] -> code|nbits; match: [len-3][dist-1] (CWINDOW <= 32) or [dist-1])
template <int NCH>
__device__ __forceinline__ void fill_luts(uint32_t* lut, uint32_t lane) {
    for (uint32_t e = lane; e < (uint32_t)LUT_LIT; e += 64) lut[e] = literal_entry(e);
    for (uint32_t e = lane; e < (uint32_t)LUT_MATCH; e += 64) {
        if (NCH == 1) lut[LUT_LIT + e] = match_entry32(e);
        else lut[LUT_LIT + e] = dist_entry(e + 1u);
    }
    if (lane < (uint32_t)LUT_LEN) lut[LUT_LIT + LUT_MATCH + lane] = lane ? length_code(lane + 1u) : 0u;      // index len-1; 0: a literal
}

// bytes at or beyond `valid` of a 16-byte chunk in registers read as zero (valid >= 16: the chunk as it is)
__device__ __forceinline__ void zero_tail16(uint4& v, uint32_t valid) {
    uint32_t* vv = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t lo = 4u * k;
        const uint32_t m = valid <= lo ? 0u : (valid >= lo + 4u ? 0xFFFFFFFFu : ((1u << (8u * (valid - lo))) - 1u));
        vv[k] &= m;
    }
}

// one 16-byte chunk of a block at position p (p < n), from a source of any alignment; bytes at or beyond n read as zero
__device__ __forceinline__ uint4 load_chunk16(const uint8_t* __restrict__ src, uint32_t p, uint32_t n, bool aligned16, uint32_t mis) {
    uint4 v;
    if (aligned16) {
        v = *reinterpret_cast<const uint4*>(src + p);
    } else {
        // realign with aligned dword loads + v_alignbyte
        const uint32_t* q = reinterpret_cast<const uint32_t*>(src + p - mis);
        const uint32_t nd = (n - p + mis + 3u) >> 2;      // dwords that hold valid bytes
        uint32_t d0 = q[0];
        uint32_t d1 = nd > 1 ? q[1] : 0, d2 = nd > 2 ? q[2] : 0, d3 = nd > 3 ? q[3] : 0, d4 = nd > 4 ? q[4] : 0;
        v.x = alignbyte(d1, d0, mis);
        v.y = alignbyte(d2, d1, mis);
        v.z = alignbyte(d3, d2, mis);
        v.w = alignbyte(d4, d3, mis);
    }
    const uint32_t valid = n - p;                // bytes of this chunk inside the block
    if (valid < 16u) zero_tail16(v, valid);      // positions >= N must read as zero bytes
    return v;
}

// ---- stage the tile that starts at position t0: [t0 - 256, t0 + 2048 + 16) straight from HBM (no carried halo: tiles are independent)
__device__ __forceinline__ void stage_tile(uint8_t* lin8, const uint8_t* __restrict__ src, uint32_t t0, uint32_t n, bool aligned16,
                                           uint32_t mis, uint32_t lane) {
    __syncthreads();
    const uint32_t nchunk = (HALO + TILE + LOOKAHEAD) / 16;          // 145 16-byte chunks
    for (uint32_t c = lane; c < nchunk; c += 64) {
        const int64_t p = (int64_t)t0 - HALO + (int64_t)c * 16;       // first position of the chunk
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p >= 0 && p < (int64_t)n) v = load_chunk16(src, (uint32_t)p, n, aligned16, mis);
        *reinterpret_cast<uint4*>(lin8 + c * 16u) = v;
    }
}

}  // namespace hdlz
