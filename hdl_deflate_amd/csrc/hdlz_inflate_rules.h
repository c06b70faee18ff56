// hdlz_inflate_rules.h -- the deflate block rules that every inflate decoder applies, stated ONCE: RFC 1951 and the reference's order of
// checks (deflate.py) as plain functions over integers, one order table, and the serial path of the lane and group kernels.
// The five mappings (hdlz_inflate_tok / _grp / _dyn / _par / _any .hip) keep their own bit readers, data layouts, loops and order of
// evaluation; what they share is the predicates and the arithmetic inside those forms.  A rule changes here or nowhere
// (tests/test_cabi_load.py: test_inflate_rules_have_one_source).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hdlz {
namespace rules {

// ---- input: 4 stream bytes at position ip of z (zn bytes long), any alignment; bytes at or beyond zn read as zero
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
__device__ __forceinline__ uint32_t load32(const uint8_t* __restrict__ z, uint32_t ip, uint32_t zn) {
    if (ip + 4u <= zn) return *reinterpret_cast<const u32_unaligned*>(z + ip);
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4u; k++)
        if (ip + k < zn) v |= (uint32_t)z[ip + k] << (8u * k);
    return v;
}

// ---- stream constants: the reference's isize (deflate.py:605) and the mask its OBSIZE-wide registers put on a stored LEN (:329, :714)
__forceinline__ constexpr int32_t isize_of(uint32_t zn) { return (int32_t)zn - 1; }
__forceinline__ constexpr uint32_t stored_len_mask(uint32_t obsize) { return obsize ? ((1u << (31u - (uint32_t)__builtin_clz(obsize))) - 1u) : 0xFFFFu; }

// ---- end-of-input margins; endbit = the first bit behind what was just read.  NO_EOF behind a literal/length code (deflate.py:1535-1539,
// and behind a dynamic header), and the hold in front of a COPY (:1600), which the whole stream turns into NO_EOF
__forceinline__ constexpr bool no_eof_behind_code(uint32_t endbit, int32_t isize) { return (int32_t)(endbit >> 3) > isize - 3; }
__forceinline__ constexpr bool copy_hold(uint32_t endbit, int32_t isize) { return (int32_t)(endbit >> 3) >= isize - 2; }

// ---- stored blocks (deflate.py:709-717): LEN sits this many bits behind the header's first bit, which is bit `dio` of its byte
__forceinline__ constexpr uint32_t stored_len_skip(uint32_t dio) { const uint32_t skip = 8u - dio; return skip <= 2u ? 16u - dio : skip; }
static_assert(stored_len_skip(0) == 8 && stored_len_skip(5) == 3 && stored_len_skip(6) == 10 && stored_len_skip(7) == 9, "deflate.py:709-717");

// ---- RFC 1951 3.2.5 in closed form (deflate.py:100-110): length code `token` = symbol - 257 (0..28), distance code dc (0..29).  TWO
// spellings, because the kernels' register counts need both: with branches for the table fills and the serial decoders, as selects
// (*_sel) where every lane of a wave computes the fields of a token that may not be there (k_inflate_dyn's window decode, the closed-form
// distance of k_inflate_grp and k_par_tokens).  One spelling for all moved a VGPR count either way; the assert below keeps them one table.
__forceinline__ constexpr void length_info(uint32_t token, uint32_t& base, uint32_t& eb) {
    if (token < 8u) { base = 3u + token; eb = 0; }
    else if (token == 28u) { base = 258u; eb = 0; }
    else { eb = (token >> 2) - 1u; base = 3u + ((4u + (token & 3u)) << eb); }
}
__forceinline__ constexpr void dist_info(uint32_t dc, uint32_t& base, uint32_t& eb) {
    if (dc < 4u) { base = 1u + dc; eb = 0; }
    else { eb = (dc >> 1) - 1u; base = 1u + ((2u + (dc & 1u)) << eb); }
}
__forceinline__ constexpr void length_info_sel(uint32_t token, uint32_t& base, uint32_t& eb) {
    const uint32_t e = (token >> 2 > 1u ? token >> 2 : 1u) - 1u;               // 0 for token < 8
    const uint32_t b = token < 8u ? token : ((4u + (token & 3u)) << e);
    eb = token == 28u ? 0u : e;
    base = token == 28u ? 258u : 3u + b;
}
__forceinline__ constexpr uint32_t dist_extra_bits(uint32_t dc) { return (dc >> 1 > 1u ? dc >> 1 : 1u) - 1u; }                 // 0 for dc < 4
__forceinline__ constexpr uint32_t dist_base(uint32_t dc, uint32_t eb) { return 1u + (dc < 4u ? dc : ((2u + (dc & 1u)) << eb)); }
__forceinline__ constexpr void dist_info_sel(uint32_t dc, uint32_t& base, uint32_t& eb) { eb = dist_extra_bits(dc); base = dist_base(dc, eb); }
__forceinline__ constexpr bool closed_form_is(bool dist, uint32_t code, uint32_t base, uint32_t eb) {
    uint32_t b0 = 0, e0 = 0, b1 = 0, e1 = 0;
    if (dist) { dist_info(code, b0, e0); dist_info_sel(code, b1, e1); } else { length_info(code, b0, e0); length_info_sel(code, b1, e1); }
    return b0 == base && e0 == eb && b1 == base && e1 == eb;
}
__forceinline__ constexpr bool closed_forms_agree() {
    for (uint32_t c = 0; c < 30u; c++) {
        uint32_t b = 0, e = 0, lb = 0, le = 0;
        dist_info(c, b, e); length_info(c, lb, le);
        if (!closed_form_is(true, c, b, e) || (c < 29u && !closed_form_is(false, c, lb, le))) return false;
    }
    return true;
}
static_assert(closed_forms_agree(), "both spellings, every code");
static_assert(closed_form_is(false, 0, 3, 0) && closed_form_is(false, 8, 11, 1) && closed_form_is(false, 27, 227, 5) && closed_form_is(false, 28, 258, 0), "lengths");
static_assert(closed_form_is(true, 0, 1, 0) && closed_form_is(true, 3, 4, 0) && closed_form_is(true, 4, 5, 1) && closed_form_is(true, 29, 24577, 13), "distances");

// ---- dynamic header, the fields (BL, deflate.py:1090-1114): the 14 bits behind BTYPE -> HLIT + 257, HDIST + 1, HCLEN + 4; legal counts?
__forceinline__ constexpr bool dyn_header_fields(uint32_t bits14, uint32_t& nlen, uint32_t& ndist, uint32_t& ncode) {
    nlen = (bits14 & 31u) + 257u; ndist = ((bits14 >> 5) & 31u) + 1u; ncode = ((bits14 >> 10) & 15u) + 4u;
    return !(nlen > 286u || ndist > 30u);
}
// the order of the code-length code's 3-bit lengths (RFC 1951 3.2.7)
static __device__ constexpr uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---- dynamic header, one code-length symbol (READBL / REPEAT, deflate.py:1116-1164, :1190-1202): the extra bits behind its code, the
// run it stands for (ev: the value of those extra bits) and the length the run repeats
__forceinline__ constexpr uint32_t cl_extra_bits(uint32_t sym) { return sym < 16u ? 0u : sym == 16u ? 2u : sym == 17u ? 3u : 7u; }
__forceinline__ constexpr uint32_t cl_repeat(uint32_t sym, uint32_t ev) { return sym < 16u ? 1u : sym == 18u ? 11u + ev : 3u + ev; }
__forceinline__ constexpr uint32_t cl_value(uint32_t sym, uint32_t prev) { return sym < 16u ? sym : sym == 16u ? prev : 0u; }
// a 16 needs a length in front of it, and no run passes the end of the list (idx of total lengths are read)
__forceinline__ constexpr bool cl_step_ok(uint32_t sym, uint32_t idx, uint32_t rep, uint32_t total) { return !(sym == 16u && idx == 0u) && idx + rep <= total; }
// the run [idx, idx + rep) gives symbol 256, the end-of-block code, its length: a block whose 256 has length 0 is refused
__forceinline__ constexpr bool cl_run_covers_eob(uint32_t idx, uint32_t rep) { return idx <= 256u && idx + rep > 256u; }
static_assert(cl_extra_bits(18) == 7 && cl_repeat(18, 127) == 138 && cl_value(18, 9) == 0, "18: 11..138 zeros");
static_assert(cl_extra_bits(16) == 2 && cl_repeat(16, 3) == 6 && cl_value(16, 9) == 9, "16: the previous length 3..6 times");
static_assert(cl_extra_bits(17) == 3 && cl_repeat(17, 0) == 3 && cl_value(17, 9) == 0 && cl_repeat(7, 0) == 1 && cl_value(7, 9) == 7, "17: 3..10 zeros; 0..15: itself");
static_assert(!cl_step_ok(16, 0, 3, 300) && cl_step_ok(16, 1, 3, 300) && cl_step_ok(18, 162, 138, 300) && !cl_step_ok(18, 163, 138, 300), "");

// ---- dynamic header, acceptance (zlib's inflate_table, puff).  `left` is the completeness count of a code set: what is left of the code
// space, 0 = complete, < 0 = over-subscribed -- in any unit: the counting decoders shift it up per length, k_any_headers keeps the Kraft
// sum kr in units of 2^-15 and passes 32768 - kr; the meaning is the same.  The code-length code must be complete.  A literal/length or
// distance set may be incomplete only as exactly ONE code, of length 1; the distance set may also be empty (RFC 1951 3.2.7).
__forceinline__ constexpr bool cl_code_ok(int32_t left) { return left == 0; }
__forceinline__ constexpr bool code_set_ok(int32_t left, uint32_t ncodes, uint32_t ncodes_of_length_1, bool is_distance) {
    return left == 0 || (left > 0 && ((ncodes == 1u && ncodes_of_length_1 == 1u) || (is_distance && ncodes == 0u)));
}
static_assert(code_set_ok(0, 286, 0, false) && code_set_ok(0, 2, 2, true), "complete");
static_assert(!code_set_ok(-1, 3, 3, false) && !code_set_ok(-16384, 3, 3, true), "over-subscribed");
static_assert(code_set_ok(16384, 1, 1, false) && code_set_ok(1, 1, 1, true), "one code of length 1");
static_assert(!code_set_ok(24576, 1, 0, false) && !code_set_ok(24576, 1, 0, true), "one code of length 2");
static_assert(!code_set_ok(8192, 2, 1, false) && !code_set_ok(8192, 2, 1, true), "two codes, incomplete");
static_assert(code_set_ok(32768, 0, 0, true) && !code_set_ok(32768, 0, 0, false), "an empty distance set, but no empty literal/length set");

}  // namespace rules
}  // namespace hdlz

// ---- the serial path of the lane kernel (k_inflate_tok) and the group kernel (k_inflate_grp): the next item of a stream -- HEADER
// (deflate.py:677-732) with the stored LEN, NEXT (:1409-1445; DYN: D_NEXT :1447-1517), the INFLATE checks in the reference's order
// (:1519-1591) -- until something is pending, and one byte of a stored block's COPY (:1603-1626).  ONE text, a macro like
// TOK_FIXED_GROUP; the including kernel has the decoder state under these names (bb, bc, o, cap, obsize, isize, len_mask, assume_fixed,
// oneblock, final_, need_header, srem, rem, dist, litv, litn, slow, active, out_len) and its own steps as macros behind its prefix K:
//   K_REFILL()  K_BITPOS()  K_FAIL(code)         its bit reader and how it fails
//   K_LIT_AT(bits)                               the literal/length code in front of the bits, as a lit_entry word
//   K_DIST_CODE(bits, nbits, dbase, deb)         the distance code in front of the bits: its length, base and extra-bit count -- or, in
//                                                this order, HDLZ_E_BAD_SYMBOL (no such code) / HDLZ_E_BAD_DISTANCE (symbols 30, 31) and break
//   K_NO_DYNAMIC                                 a dynamic-tree block is left to another pass (HDLZ_E_DYNAMIC_UNSUPPORTED)
//   K_BLOCK_TABLES(hm)                           behind the header of a fixed / dynamic block (may fail and break)
//   K_DIST_REFILL()                              between the length's extra bits and the distance code
//   K_MATCH_TAKEN(distance)                      a match passed every check
//   K_NEXT_BLOCK                                 `continue` or `break` behind a block header or an end-of-block code
#define HDLZ_SERIAL_ITEMS(K)                                                                                 \
    while (slow && active && rem == 0u && srem == 0u && litn == 0u) {                                       \
        K##_REFILL();                                                                                       \
        if (need_header) {                                                                                  \
            /* HEADER (deflate.py:677-732) */                                                               \
            final_ = ((uint32_t)bb & 1u) | oneblock;                                                        \
            const uint32_t hm = assume_fixed ? 1u : ((uint32_t)(bb >> 1) & 3u);                             \
            if (hm == 3u) { K##_FAIL(HDLZ_E_BAD_BTYPE); break; }                                            \
            if (K##_NO_DYNAMIC && hm == 2u) { K##_FAIL(HDLZ_E_DYNAMIC_UNSUPPORTED); break; }                \
            need_header = false;                                                                            \
            if (hm == 0u) {                                                                                 \
                /* stored (deflate.py:709-717) */                                                           \
                const uint32_t skip = rules::stored_len_skip(K##_BITPOS() & 7u);                            \
                const uint32_t length = (uint32_t)(bb >> skip) & 0xFFFFu & len_mask;                        \
                bb >>= (skip + 16u); bc -= (skip + 16u);          /* now at NLEN = the reference's di */    \
                K##_REFILL();                                                                               \
                bb >>= 16; bc -= 16u;                             /* NLEN unchecked (D2); data follows */   \
                srem = length;                                                                              \
                if (length == 0u) {                                                                         \
                    /* COPY with nothing to copy (deflate.py:1617-1626) */                                  \
                    if ((int32_t)(K##_BITPOS() >> 3) >= isize) { K##_FAIL(HDLZ_E_NO_EOF); break; }          \
                    if (final_) { out_len = o; active = false; break; }                                     \
                    need_header = true;                                                                     \
                }                                                                                           \
            } else {                                                                                        \
                bb >>= 3; bc -= 3u;                                                                         \
                K##_BLOCK_TABLES(hm);                                                                       \
            }                                                                                               \
            K##_NEXT_BLOCK;                                                                                 \
        }                                                                                                   \
        /* NEXT (deflate.py:1409-1445) */                                                                   \
        const uint32_t e = K##_LIT_AT((uint32_t)bb);                                                        \
        const uint32_t nb = e & 15u, code = (e >> 4) & 0x1FFu;                                              \
        if (nb < 1u) { K##_FAIL(HDLZ_E_BAD_SYMBOL); break; }                                                \
        bb >>= nb; bc -= nb;                                                                                \
        /* INFLATE (deflate.py:1519-1591) */                                                                \
        if (rules::no_eof_behind_code(K##_BITPOS(), isize)) { K##_FAIL(HDLZ_E_NO_EOF); break; }             \
        if (code == 256u) {                                                                                 \
            if (final_) { out_len = o; active = false; break; }   /* D6 */                                  \
            need_header = true;                                                                             \
            K##_NEXT_BLOCK;                                                                                 \
        }                                                                                                   \
        if (code < 256u) {                                                                                  \
            if (o >= cap) { K##_FAIL(HDLZ_E_OUT_CAPACITY); break; }                                         \
            litv = code; litn = 1;                                                                          \
            break;                                                                                          \
        }                                                                                                   \
        const uint32_t token = code - 257u;                                                                 \
        if (token >= 29u) { K##_FAIL(HDLZ_E_BAD_SYMBOL); break; }                                           \
        uint32_t lbase, leb, dnb, dbase, deb;                                                               \
        rules::length_info(token, lbase, leb);                                                              \
        const uint32_t tlength = lbase + ((uint32_t)bb & ((1u << leb) - 1u));                               \
        bb >>= leb; bc -= leb;                                                                              \
        K##_DIST_REFILL();                                                                                  \
        K##_DIST_CODE((uint32_t)bb, dnb, dbase, deb);                                                       \
        bb >>= dnb;                                                                                         \
        const uint32_t distance = dbase + ((uint32_t)bb & ((1u << deb) - 1u));                              \
        bb >>= deb;                                                                                         \
        bc -= dnb + deb;                                                                                    \
        if (distance > o || distance > obsize) { K##_FAIL(HDLZ_E_BAD_DISTANCE); break; }        /* D8 */    \
        if (rules::copy_hold(K##_BITPOS(), isize)) { K##_FAIL(HDLZ_E_NO_EOF); break; }                      \
        if ((uint64_t)o + tlength > cap) { K##_FAIL(HDLZ_E_OUT_CAPACITY); break; }                          \
        rem = tlength;                                                                                      \
        dist = distance;                                                                                    \
        K##_MATCH_TAKEN(distance);                                                                          \
    }
// stored COPY (deflate.py:1603-1616): one byte per round (rare: level-0 streams, incompressible blocks)
#define HDLZ_SERIAL_STORED_BYTE(K)                                                                           \
    if (active && srem != 0u && litn == 0u && rem == 0u) {                                                  \
        K##_REFILL();                                                                                       \
        if ((int32_t)(K##_BITPOS() >> 3) >= isize) { K##_FAIL(HDLZ_E_NO_EOF); }                             \
        else if (o >= cap) { K##_FAIL(HDLZ_E_OUT_CAPACITY); }                                               \
        else {                                                                                              \
            litv = (uint32_t)bb & 0xFFu; litn = 1;                                                          \
            bb >>= 8; bc -= 8u;                                                                             \
            srem--;                                                                                         \
            if (srem == 0u) {                              /* the block ends with this byte (deflate.py:1617-1626) */ \
                if ((int32_t)(K##_BITPOS() >> 3) >= isize) { K##_FAIL(HDLZ_E_NO_EOF); litn = 0; }           \
                else if (final_) { out_len = o + 1u; active = false; }      /* (the byte is still emitted below) */ \
                else need_header = true;                                                                    \
            }                                                                                               \
        }                                                                                                   \
    }
