/*
 * hdlz_gzip_members.h -- extension of hdlz_gunzip.h: a gzip FILE of many members (cat a.gz b.gz, WARC, dictzip / mgzip / pgzip output, a
 * BGZF file without its BC field) found, decoded and verified in parallel from nothing but the file.  hdlz_gunzip.h leaves this out of
 * scope ("several members of one stream decoded in one call"): a member has no size field, so the index below is a GUESS, stated as a
 * purely syntactic rule, and the read behind it VERIFIES every member of the guess.  Additive: HDLZ_VERSION and every declaration of
 * the headers in front stay as they are, and their conventions (device pointers, ownership, extents, "writes" / "reads", return
 * values) hold here too.
 *
 * THE INDEX RULE (hdlz_gzip_members_index_ws).  With z the file and n = file_len:
 *   candidates     every p with p + 4 <= n, z[p .. p + 3) = 1F 8B 08 and z[p + 3] & 0xE0 == 0; and p = 0 when n > 0
 *   sorted         c_0 < ... < c_{M-1}, c_M = n;  span_b = c_{b+1} - c_b
 *   guess_b        0 when span_b < 18, else min(the little-endian word at c_{b+1} - 4, 1032 span_b + 258) in 64-bit arithmetic: the
 *                  ISIZE word a back-to-back member would have, held to deflate's largest expansion
 *   d_off[b] = c_b, d_off[M] = n; d_out_off = the exclusive scan of the guesses (d_out_off[M] = total_out)
 * The record: nmembers = M, total_out, status, a reserved word (0).  M > member_cap: status HDLZ_E_OUT_CAPACITY, the record still holds
 * the true counts and only the words [0 .. member_cap] of the two arrays are written (hdlz_bgzf_index_ws's convention).  n = 0:
 * HDLZ_OK, no member, d_off[0] = d_out_off[0] = 0.  The result equals the rule on EVERY file: bytes that only look like a header (one
 * in 2^27 positions of random bytes; a .gz stored inside a member) are candidates like any other, and the read tells them apart.
 * The call: the file is read once, 16 bytes a lane, a wave per window of 32 KiB with a 3-byte halo over the window's seam -> per
 * window the count, the first and last candidate, the guesses between its own candidates, and one word per KiB that says which lanes
 * saw a candidate; one workgroup scans the windows (counts, guesses, the guess across every seam, all in 64 bits) and writes the
 * record; an emit pass loads again only the 16-byte pieces the words name.  Three launches, capturable, no host read.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: one of d_off, d_out_off, d_result NULL, or d_file
 * NULL with file_len > 0; member_cap >= 2^40; d_work NULL or work_bytes below hdlz_gzip_members_index_work_bytes(file_len) where that
 * is not 0; one of d_off, d_out_off, d_result, d_work not 8-byte aligned.
 * hdlz_gzip_members_index_work_bytes(file_len) is a closed form: 0 for an empty file, else r256(64 + 308 W), W = ceil(file_len / 32768),
 * r256 = rounded up to 256.
 * writes: d_off and d_out_off [0 .. min(M, member_cap)]; *d_result; d_work[0 .. work_bytes).  Their initial contents never reach a result.
 * reads:  d_file[0 .. file_len) only, at any alignment.
 *
 * THE VERIFIED READ (hdlz_gzip_members_inflate_ws).  Sub-ranges as in hdlz_bgzf_inflate_ws: pass d_off + b0, d_out_off + b0, b1 - b0;
 * member b decodes to d_out + (d_out_off[b] - d_out_off[0]).  Per member, with s = d_off[b], e = d_off[b + 1], span = e - s and
 * n_slot = d_out_off[b + 1] - d_out_off[b], in this order of precedence:
 *   1  the index checks   e < s, e > file_len, span >= 2^28, d_out_off[b] < d_out_off[0], d_out_off[b + 1] < d_out_off[b],
 *                         n_slot >= 2^32 - 512, or d_out_off[b + 1] - d_out_off[0] > out_cap: HDLZ_E_BAD_PARAM, the member is not decoded
 *   2  the header walk    step 1 of the member rule of hdlz_gunzip.h over z[s .. e) -> p
 *   3  the decode         raw deflate from z[s + p], a wave per member (the member view of hdlz_unjoin.h's decoder): blocks of any type
 *                         until BFINAL, stores bytewise (slots need no alignment), input bounded by e, capacity n_slot; a failure is
 *                         the decoder's status, as in hdlz_gunzip.h, step 2
 *   4  the CRC-32         of the n_slot bytes of the slot
 *   5  the verdict        with `end` as in hdlz_gunzip.h, step 3:
 *                           end + 8 != span                     HDLZ_E_NO_EOF      (the member is cut, or it stops in front of the next
 *                                                                                  candidate: padding, or the guess split a member)
 *                           the decoded length != n_slot        HDLZ_E_BAD_CHECKSUM
 *                           the word at z[s + end] != the CRC-32, or the word at z[s + end + 4] != n_slot mod 2^32: HDLZ_E_BAD_CHECKSUM
 *                         otherwise HDLZ_OK
 * A member whose status is HDLZ_OK is by construction one that a serial reader arriving at s accepts, with in_used = span, and its slot
 * holds its bytes.  The record: out_len (d_out_off[nmembers] - d_out_off[0] when every member is OK, else 0), first_bad and status of
 * the lowest failed member (first_bad = 2^64 - 1 when there is none), as in hdlz_bgzf_inflate_result.  d_member_status, when given,
 * receives every member's status.
 * The call: the checks and the header walk (a wave per member), the member decode, hdlz_crc32_batch_ws's kernel over the slots, the
 * verdict, the record.  Capturable, no host read.  Parameter errors, in this order: d_result NULL, or with nmembers > 0 one of d_file,
 * d_off, d_out_off NULL, or d_out NULL with out_cap > 0; nmembers >= 2^31; one of d_off, d_out_off, d_result not 8-byte aligned;
 * d_member_status not 4-byte aligned; d_work not 256-byte aligned; d_work NULL or work_bytes below
 * hdlz_gzip_members_inflate_work_bytes(nmembers) where that is not 0.
 * hdlz_gzip_members_inflate_work_bytes(nmembers) is a closed form: 0 for no members and for 2^31 and more, else
 * r256(20 nmembers) + r256(24 nmembers + 8).
 * writes: the slots of the members that passed check 1, never outside them (a failed member's slot may hold anything); d_member_status
 *         [0 .. nmembers) when given; *d_result; d_work[0 .. work_bytes).  Their initial contents never reach a result.
 * reads:  d_off and d_out_off [0 .. nmembers]; of the file only bytes of the spans that passed check 1, so nothing behind file_len; of a
 *         slot only its own bytes.
 *
 * Out of scope: the whole-GPU batch chains and the lane / group mappings for members (a member of many MiB is one wave's work here:
 * the caller sends such a span to hdlz_gunzip_ws with one stream, as Engine.read_gzip does from `big_member` bytes on); members or slots
 * past the limits of check 1; members that decode past 4 GiB (ISIZE is the length mod 2^32); writing such files; and REPAIR on the
 * device -- where a run of members did not verify (a look-alike split a member, padding stands between two), the caller decodes one
 * member serially at that position (hdlz_gunzip_ws) and resumes at the candidate where it ended.
 */
#ifndef HDLZ_GZIP_MEMBERS_H
#define HDLZ_GZIP_MEMBERS_H
#include "hdlz_gunzip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hdlz_gzip_members_index_result {
    uint64_t nmembers;      /* M: the candidates of the file, whatever member_cap is */
    uint64_t total_out;     /* the sum of the M guesses */
    uint32_t status;        /* HDLZ_OK, or HDLZ_E_OUT_CAPACITY: M > member_cap */
    uint32_t reserved;      /* 0 */
} hdlz_gzip_members_index_result;

typedef struct hdlz_gzip_members_inflate_result {
    uint64_t out_len;
    uint64_t first_bad;
    uint32_t status;
    uint32_t reserved;      /* 0 */
} hdlz_gzip_members_inflate_result;

size_t hdlz_gzip_members_index_work_bytes(uint64_t file_len);

int hdlz_gzip_members_index_ws(const uint8_t* d_file, uint64_t file_len, uint64_t member_cap,
                               uint64_t* d_off,       /* member_cap + 1 words */
                               uint64_t* d_out_off,   /* member_cap + 1 words */
                               hdlz_gzip_members_index_result* d_result,
                               void* d_work, size_t work_bytes, void* stream);

size_t hdlz_gzip_members_inflate_work_bytes(uint64_t nmembers);

int hdlz_gzip_members_inflate_ws(const uint8_t* d_file, uint64_t file_len, const uint64_t* d_off, const uint64_t* d_out_off,
                                 uint64_t nmembers, uint8_t* d_out, uint64_t out_cap,
                                 uint32_t* d_member_status,   /* nullable */
                                 hdlz_gzip_members_inflate_result* d_result,
                                 void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_GZIP_MEMBERS_H */
