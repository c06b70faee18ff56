/*
 * hdlz_unjoin.h -- extension of hdlz_join.h: read a joined stream back member by member, in parallel.
 *
 * hdlz_join_batch_ws writes ONE zlib stream and the index of its members (d_off).  The members are independent by construction -- each
 * is a byte-aligned, non-final fixed block whose back-references never leave it, followed by the sync marker of an empty stored block --
 * so the index is all a batch decoder needs: hdlz_unjoin_ws decodes every member with the batch kernels of hdlz_inflate_batch_ws (one
 * lane, sixteen lanes or one wave per member), straight into the flat output, and checks the stream as zlib would: the marker behind
 * every member, the final empty block, the Adler-32 of the whole output.  Additive: HDLZ_VERSION and every declaration of hdlz.h and
 * hdlz_join.h stay as they are; the conventions of hdlz.h (device pointers, ownership, extents, "writes" / "reads", return values)
 * hold here too.
 *
 * THE MEMBERS.  Member b is d_stream[d_off[b] .. d_off[b+1]).  It is decoded into d_out[o_b .. o_b + n_b): with d_out_off
 * o_b = d_out_off[b] and n_b = d_out_off[b+1] - d_out_off[b], without it o_b = b * out_len and n_b = out_len -- the pair the compress
 * call was given as d_in_off / in_len, the same pair the join takes.  The output is the original flat buffer, contiguous from byte 0.
 *
 * The whole-GPU chains of hdlz_inflate_batch_ws (k_par_*, k_any_*) are not part of this: a handful of very large members run one wave
 * each.  Members of other writers (dynamic or stored first blocks, members found without an index) are out of scope.
 */
#ifndef HDLZ_UNJOIN_H
#define HDLZ_UNJOIN_H
#include "hdlz_join.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hdlz_unjoin_result {
    uint64_t out_len;    /* bytes written to d_out (= d_out_off[nmembers] resp. the sum of the member lengths); 0 unless status == HDLZ_OK */
    uint64_t first_bad;  /* lowest index of a member that failed; nmembers for a failure of the stream's own frame; ~0 when OK */
    uint32_t status;
    uint32_t adler;      /* Adler-32 computed over the output; 0 when a member failed to decode */
} hdlz_unjoin_result;

/*
 * scratch of hdlz_unjoin_ws, host arithmetic: with r256(x) = x rounded up to a multiple of 256,
 *     r256(12 * nmembers)                      three words per member: decoded length, status, end bit
 *   + r256(8 * ceil(total_out / 32768))        the checksum's partial sums, 8 bytes per 32 KiB tile of the output
 *   + r256(hdlz_inflate_work_bytes(nmembers, 0, 0, flags, 1))      what the batch decode of a ragged batch of nmembers streams asks for
 * total_out is the out_cap the call will be given.  0 for nmembers >= 2^31.
 */
size_t hdlz_unjoin_work_bytes(uint64_t nmembers, uint64_t total_out, uint32_t flags);

/*
 * The call: four steps on the caller's stream, nothing forks to a side stream, the host reads nothing back -- every length and offset
 * is checked on the device: the index checks, the decode, the partial checksums of the output, the judgement and the record.
 *
 * PER MEMBER, in this order of precedence (d_member_status[b], and the record's status when b is the lowest member that failed):
 *   1. reject with HDLZ_E_BAD_PARAM when the index is unusable: d_off[b+1] < d_off[b] + 5, d_off[b+1] > stream_len, a member of
 *      256 MiB or more, o_b not a multiple of 4, d_out_off decreasing, d_out_off[0] != 0, or o_b + n_b > out_cap.  Such a member is
 *      not decoded: the rest of its index words may be garbage.  (A stream cut inside its last six bytes still holds every member
 *      whole: that is the stream's HDLZ_E_NO_EOF below, as zlib would say, not an unusable index.)
 *   2. the decoder's own status, as the batch calls give it: reject with HDLZ_E_BAD_BTYPE when the member's first block is not
 *      BTYPE 01 (BFINAL is not read, as under HDLZ_INFLATE_ONEBLOCK; such a member is not decoded either), HDLZ_E_BAD_SYMBOL,
 *      HDLZ_E_BAD_DISTANCE (a back-reference that leaves the member included), HDLZ_E_NO_EOF when the block does not end inside the
 *      member, HDLZ_E_OUT_CAPACITY when the member holds more than n_b bytes.  HDLZ_E_DYNAMIC_UNSUPPORTED is never returned.
 *   3. reject with HDLZ_E_BAD_PARAM when fewer than n_b bytes were decoded: the index contradicts the stream.
 *   4. reject with HDLZ_E_NO_EOF when the member does not end where the index says.  With e = the first bit behind the end-of-block
 *      code: bits e .. e+2 must be 0 (BFINAL = 0, BTYPE = 00); the bits up to the next byte boundary are ignored, as zlib does; the
 *      four bytes behind that must be 00 00 FF FF, and the byte behind them must be byte d_off[b+1].
 * THE STREAM (first_bad = nmembers), judged only when no member failed; d_off[0] and the header first, the rest in the order written:
 *   reject with HDLZ_E_BAD_HEADER when d_off[0] != 2 or the two header bytes fail the test of hdlz_inflate_checked (CM = 8, window at
 *      most 32 KiB, FCHECK, no preset dictionary);
 *   reject with HDLZ_E_NO_EOF when stream_len < d_off[nmembers] + 6 or the two bytes at d_off[nmembers] are not 03 00;
 *   reject with HDLZ_E_BAD_CHECKSUM when the big-endian word behind them is not the Adler-32 of the output; adler is still reported.
 * nmembers = 0 reads 78 9C 03 00 00 00 00 01 (d_off[0] = 2) and answers HDLZ_OK with out_len = 0.  Bytes behind d_off[nmembers] + 6
 * are no error.
 *
 *   flags              at most one of HDLZ_INFLATE_LANE_PER_STREAM, HDLZ_INFLATE_WAVE_PER_STREAM, HDLZ_INFLATE_GROUP_PER_STREAM: the
 *                      mapping, otherwise chosen from nmembers by the thresholds of hdlz_inflate_batch_ws.  Results are identical
 *                      under every mapping.  Any other bit: HDLZ_E_BAD_PARAM.
 *   d_member_status    nullable: nmembers words, the status of every member (for diagnosis; the record names the first failure).
 *   d_work/work_bytes  at least hdlz_unjoin_work_bytes(nmembers, out_cap, flags) bytes, 256-byte aligned.
 * THE CAPACITY A DECODER SEES is min(n_b, out_cap - o_b) -- after check 1 that is n_b.  Every global store of the three mappings,
 * 16-byte and dword stores included, lies wholly below the output position the capacity has already admitted (lines are stored once
 * complete, the rest byte by byte up to the decoded length), and o_b is a multiple of 4, so a member that overflows its slot fails
 * with HDLZ_E_OUT_CAPACITY before a byte leaves the slot: nothing spills into a neighbour, and nothing past out_cap for the last member
 * whatever n_b modulo 4 is.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_stream, d_off or d_result NULL; d_out NULL with out_cap > 0;
 * nmembers >= 2^31; a flag other than the three mapping hints, or two of them; d_out not 4-byte aligned; d_off, d_out_off or d_result
 * not 8-byte aligned; d_work not 256-byte aligned; d_work NULL or work_bytes below the query when that is not 0.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_out[0 .. out_len) when HDLZ_OK; otherwise the bytes inside d_out[0 .. out_cap) are unspecified -- never a byte at or behind
 *         out_cap; d_member_status[0 .. nmembers) when given; the result record; d_work[0 .. work_bytes).  The initial contents of
 *         d_out, d_member_status, d_result and d_work never reach a result.
 * reads:  d_stream[0 .. stream_len) only -- of member b the bytes d_off[b] .. d_off[b+1) (bounds-checked as in hdlz_inflate_batch_ws:
 *         no load reaches past the member), the two header bytes and, when no member failed, the six bytes at d_off[nmembers] --;
 *         d_off[0 .. nmembers]; d_out_off[0 .. nmembers] when given; d_out[0 .. min(out_len, out_cap)) for the checksum.
 */
int hdlz_unjoin_ws(const uint8_t* d_stream, uint64_t stream_len,
                   const uint64_t* d_off,          /* nmembers + 1 words, as hdlz_join_batch_ws wrote them */
                   const uint64_t* d_out_off, uint32_t out_len,   /* what the compress call was given as d_in_off / in_len: the same pair the join takes */
                   uint64_t nmembers, uint32_t flags,
                   uint8_t* d_out, uint64_t out_cap,
                   uint32_t* d_member_status,      /* nullable: per-member status, for diagnosis */
                   hdlz_unjoin_result* d_result,
                   void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_UNJOIN_H */
