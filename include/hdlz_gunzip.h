/*
 * hdlz_gunzip.h -- extension of hdlz_gzip.h: read gzip members of ANY writer -- gzip, pigz, zlib, Python --, one per stream, with the
 * CRC-32 and ISIZE of the trailer verified on the device.  hdlz_unjoin_gzip_ws reads only this library's own joined form (its 10-byte
 * header and the member index), hdlz_bgzf_inflate_ws needs BGZF's BSIZE field and hdlz_inflate_checked judges zlib framing; this
 * header takes up the line hdlz_gzip.h leaves out of scope: "headers of other writers (FEXTRA, FNAME, FCOMMENT, FHCRC)", and gives the
 * caller what a file of several members needs -- where the member ended.  Additive: HDLZ_VERSION and every declaration of hdlz.h,
 * hdlz_join.h, hdlz_unjoin.h, hdlz_gzip.h, hdlz_bgzf.h, hdlz_bgzf_range.h and hdlz_bgzf_stored.h stay as they are, and their
 * conventions (device pointers, ownership, extents, "writes" / "reads", return values) hold here too.
 *
 * THE MEMBER RULE.  The input shapes are those of hdlz_inflate_checked: rows of one pitch, or a flat buffer with d_in_off[B + 1] and
 * in_len as the optional bound on the lengths.  Every stream is ONE member of RFC 1952 followed by anything.  With z the stream and
 * len its length (d_in_off[b + 1] - d_in_off[b], or in_len), a serial reader does, in this order of precedence:
 *   1  the header walk
 *        len < 10                                            HDLZ_E_NO_EOF
 *        z[0..2] != 1F 8B 08, or FLG & 0xE0 != 0 (FLG = z[3]) HDLZ_E_BAD_HEADER
 *        pos = 10                                            (MTIME, XFL and OS are skipped; FTEXT, FLG & 1, is ignored)
 *        FEXTRA (FLG & 4):   pos + 2 > len: HDLZ_E_NO_EOF; XLEN = z[pos] + 256 z[pos + 1]; pos += 2; pos + XLEN > len: HDLZ_E_NO_EOF;
 *                            pos += XLEN
 *        FNAME (FLG & 8), then FCOMMENT (FLG & 16): the bytes from pos up to and including the first zero byte are skipped; no zero
 *                            byte in front of len: HDLZ_E_NO_EOF
 *        FHCRC (FLG & 2):    pos + 2 > len: HDLZ_E_NO_EOF; z[pos] + 256 z[pos + 1] != the low 16 bits of the CRC-32 of z[0 .. pos):
 *                            HDLZ_E_BAD_HEADER (verified, as zlib does); pos += 2
 *        p = pos                                             the offset of the first payload byte; p >= 10
 *   2  the decode            raw deflate from z[p]: blocks of any type until BFINAL, RFC 1951 history (obsize = 0), bounded by len.  A
 *                            failure is the decoder's status, exactly what hdlz_inflate_batch_ws gives a stream of len - p + 2 bytes
 *                            whose payload starts at its third byte (so a payload of fewer than 3 bytes is HDLZ_E_SHORT_INPUT, output
 *                            beyond out_pitch HDLZ_E_OUT_CAPACITY, and a payload that is cut what that decoder makes of it)
 *   3  the trailer           end = the index of the first byte behind the final block's last bit, counted from z[0];
 *                            end + 8 > len: HDLZ_E_NO_EOF
 *   4  the checks            the little-endian word at z[end] != CRC-32 of the n decoded bytes: HDLZ_E_BAD_CHECKSUM
 *                            the little-endian word at z[end + 4] != n mod 2^32: HDLZ_E_BAD_CHECKSUM
 *   5  otherwise             HDLZ_OK: d_out_len[b] = n, d_in_used[b] = end + 8, d_crc[b] = the computed CRC-32
 * A failed stream has d_out_len[b] = 0; d_in_used[b] and d_crc[b] are 0 for a failure of steps 1 to 3 and end + 8 and the computed word
 * for a failure of step 4 (as hdlz_inflate_checked does for Adler-32); its row may hold anything inside the row.  Bytes behind
 * d_in_used[b] are no error: that is where the next member of a file starts (tests/gunzip_ref.py states this rule in Python).
 * Streams are limited to 256 MiB - 1 bytes, as in hdlz_inflate_batch_ws.
 *
 * THE CALL.  The header walk (a wave per stream), the decode by an existing decoder -- nstreams >= 2: a wave per stream, the member view
 * of hdlz_unjoin.h's decoder; nstreams == 1, the .gz file: the path of hdlz_inflate_batch_ws, so a large stream is decoded by the whole
 * GPU, in_len being the bound that path sizes itself from --, the CRC-32 of every row (a workgroup per row for out_pitch < 65536, else
 * 32 KiB tiles over the whole GPU), the verdict.  The host reads nothing back in between.
 * d_in_used is REQUIRED, d_crc may be NULL.  Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order:
 * d_in_used NULL; nstreams >= 2^31; with nstreams > 0 one of d_in, d_out, d_out_len, d_status NULL; without d_in_off: in_len >= 2^28,
 * or nstreams > 1 and in_pitch < in_len; nstreams > 1 and out_pitch >= 2^32; out_pitch not a multiple of 4 or d_out not 4-byte
 * aligned; d_in_off not 8-byte aligned; one of the four result arrays not 4-byte aligned; d_work not 256-byte aligned; with
 * nstreams > 0, d_work NULL or work_bytes below hdlz_gunzip_work_bytes.
 * hdlz_gunzip_work_bytes(nstreams, in_len, out_pitch, ragged) is a closed form (0 where the call refuses the shape, and for no streams):
 *     r256(12 nstreams) + r256(16 nstreams) + r256(4 T) + D,   r256 = rounded up to 256
 *     T = nstreams * ceil(min(out_pitch, 2^32 - 1) / 32768) when out_pitch >= 65536 and that product is below 2^31, else 0
 *     D = r256(hdlz_inflate_work_bytes(1, in_len, out_pitch, 0, 1)) when nstreams == 1, else 0
 * and the call needs all of it (unlike hdlz_inflate_batch_ws it refuses less).  Nothing is allocated; every launch is capturable; only
 * this form exists (no pool-scratch sibling).
 * writes: d_out_len, d_status, d_in_used and, when given, d_crc [0 .. nstreams); row b as hdlz_inflate_batch_ws writes it, never outside
 *         d_out[b*out_pitch .. (b+1)*out_pitch); d_work[0 .. work_bytes).  The initial contents of all of these never reach a result.
 * reads:  only bytes of the streams themselves, at any alignment; of row b only bytes below d_out_len[b] (whole 16-byte pieces where
 *         they lie inside them, single bytes else): nothing behind the decoded length reaches a result.
 *
 * Out of scope: several members of one stream decoded in one call (the caller moves on by d_in_used; a file of many members is taken
 * up by hdlz_gzip_members.h, which finds and verifies them in parallel); the lane and group mappings for
 * batches (the member twins of k_inflate_tok and k_inflate_grp have no dynamic-tree pass) and the whole-GPU path for more than one
 * stream per call; obsize and HDLZ_INFLATE_ASSUME_FIXED semantics; writing header fields of other writers; ZIP archives (taken up by
 * hdlz_zip.h).
 */
#ifndef HDLZ_GUNZIP_H
#define HDLZ_GUNZIP_H
#include "hdlz_gzip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t hdlz_gunzip_work_bytes(uint64_t nstreams, uint32_t in_len, uint64_t out_pitch, int ragged);

int hdlz_gunzip_ws(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len,
                   uint64_t nstreams, uint8_t* d_out, uint64_t out_pitch,
                   uint32_t* d_out_len, uint32_t* d_status,
                   uint32_t* d_in_used,   /* required */
                   uint32_t* d_crc,       /* nullable */
                   void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_GUNZIP_H */
