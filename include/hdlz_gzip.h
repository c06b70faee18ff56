/*
 * hdlz_gzip.h -- extension of hdlz_unjoin.h: the joined stream as ONE gzip member, with a CRC-32 computed and verified on the device.
 *
 * hdlz_join_batch_ws writes a zlib stream (78 9C .. Adler-32); what is stored and exchanged is .gz.  The three calls here give the
 * same members the gzip frame of RFC 1952 -- gzip -d, pigz -d, Python's gzip and every HTTP stack read the result -- and read that
 * frame back.  Additive: HDLZ_VERSION and every declaration of hdlz.h, hdlz_join.h and hdlz_unjoin.h stay as they are; the conventions
 * of hdlz.h (device pointers, ownership, extents, "writes" / "reads", return values) hold here too.
 *
 * THE STREAM.  With the members M_0 .. M_{B-1} exactly as hdlz_join.h defines them, X the concatenated input and N its length:
 *   1F 8B 08 00  00 00 00 00  00 FF        the header: CM = 8, FLG = 0, MTIME = 0, XFL = 0, OS = 255 (unknown); always these 10 bytes
 *   M_0 .. M_{B-1}
 *   03 00                                  a final empty fixed block
 *   CRC-32(X) little-endian, N mod 2^32 little-endian
 * stream_len is the zlib form's length plus 12; d_off[0] = 10 and d_off[B] is where 03 00 starts; B = 0: the header followed by
 * 03 00 00 00 00 00 00 00 00 00 (20 bytes).  The member bytes and the index are those of the zlib form, moved by 8.
 * Out of scope: gzip in hdlz_inflate_checked, headers of other writers (FEXTRA, FNAME, FCOMMENT, FHCRC), files of several gzip
 * members, the CRC-32 of a pitched or gapped batch.  (hdlz_gunzip.h, the extension of this header, reads members with such headers and
 * says where each one ended, which is what a file of several members needs.)
 */
#ifndef HDLZ_GZIP_H
#define HDLZ_GZIP_H
#include "hdlz_unjoin.h"

#ifdef __cplusplus
extern "C" {
#endif

/* scratch of hdlz_crc32_ws: 0 for n = 0, else 4 bytes per 32 KiB tile of the data, rounded up to 256 */
size_t hdlz_crc32_work_bytes(uint64_t n);

/*
 * CRC-32 as zlib computes it (reflected polynomial EDB88320, initial register and final xor FFFFFFFF) of d_data[0 .. n) -> d_crc[0],
 * in two launches: one raw word per 32 KiB tile over the whole GPU, then one workgroup that combines the words by a tree.  n = 0
 * gives 0.  d_data may have any alignment; d_crc and d_work are 4-byte aligned.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_crc NULL; d_data NULL with n > 0; d_work NULL or work_bytes
 * below the query when that is not 0; d_crc or d_work not 4-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_crc[0], d_work[0 .. work_bytes).  The initial contents of d_crc and d_work never reach the result.
 * reads:  d_data[0 .. n) only: nothing at or behind n and nothing in front of d_data -- whole 16-byte pieces are loaded where they
 *         lie inside the data, the last piece byte by byte.
 */
int hdlz_crc32_ws(const uint8_t* d_data, uint64_t n, uint32_t* d_crc, void* d_work, size_t work_bytes, void* stream);

/* bytes that hold the gzip form of the joined stream: hdlz_join_bound(nblocks, in_len) + 12 */
size_t hdlz_join_gzip_bound(uint64_t nblocks, uint32_t in_len);

/* scratch of hdlz_join_gzip_ws: the same as hdlz_join_work_bytes(nblocks) */
size_t hdlz_join_gzip_work_bytes(uint64_t nblocks);

typedef struct hdlz_join_gzip_result {
    uint64_t stream_len;   /* length of the gzip stream; 0 when a block failed */
    uint32_t status;       /* HDLZ_OK, HDLZ_E_OUT_CAPACITY or the worst status of a block */
    uint32_t crc;          /* the word *d_crc, as it went into the trailer; 0 when a block failed */
} hdlz_join_gzip_result;

/*
 * The gzip join: the parameters of hdlz_join_batch_ws, and
 *   d_crc              REQUIRED: a device word that holds CRC-32(X) when the call's kernels run -- put there earlier on the same stream,
 *                      normally by hdlz_crc32_ws over the flat input the compress call was given.  The join reads no input byte, so a
 *                      pitched or gapped batch, whose X is not one buffer, has to supply the word some other way; combining per-row
 *                      CRCs is out of scope.  4-byte aligned.
 *   d_off              nblocks + 1 words, WRITTEN: d_off[b] = where member b starts (d_off[0] = 10), d_off[nblocks] = where 03 00
 *                      starts; stream_len = d_off[nblocks] + 10.  (A failed block counts as a member of length 0.)
 *   d_result           the result record, WRITTEN.  status, in this order of precedence:
 *                        the numerically largest status of any failed block (a row whose length, end bit and row_pitch contradict each
 *                        other counts as failed with HDLZ_E_BAD_PARAM); then stream_len = crc = 0 and the bytes of d_stream inside
 *                        [0, stream_cap) are unspecified;
 *                        HDLZ_E_OUT_CAPACITY when stream_len > stream_cap: stream_len and crc are still reported, members that
 *                        would end beyond stream_cap are not copied, and neither is the trailer;
 *                        otherwise HDLZ_OK.
 *   d_work / work_bytes at least hdlz_join_gzip_work_bytes(nblocks) bytes, 8-byte aligned (NULL allowed when that is 0).
 * ISIZE is N mod 2^32 with N from d_in_off / in_len, as in hdlz_join_batch_ws.  The members are placed by that call's own kernel
 * (the header is 10 = 8 + 2 bytes), so gz[10 .. d_off[B]) equals z[2 .. d_off_z[B]) of the zlib join of the same rows, byte for byte.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_crc, d_stream, d_off or d_result NULL; with nblocks > 0 any
 * of d_rows, d_len, d_end_bits, d_status, d_work NULL; nblocks >= 2^31; work_bytes below the query; d_work, d_off or d_result not
 * 8-byte aligned; d_crc not 4-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_stream[0 .. min(stream_len, stream_cap)) -- never a byte at or behind stream_cap --, d_off[0 .. nblocks], the result
 *         record, d_work[0 .. work_bytes).
 * reads:  d_crc[0]; d_len, d_end_bits, d_status [0 .. nblocks); d_in_off[0 .. nblocks] when given; of row b only bytes below d_len[b],
 *         as hdlz_join_batch_ws states it.  The initial contents of d_stream, d_off, d_result and d_work never reach a result.
 */
int hdlz_join_gzip_ws(const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_end_bits,
                      const uint32_t* d_status, const uint64_t* d_in_off, uint32_t in_len, uint64_t nblocks,
                      const uint32_t* d_crc,   /* required */
                      uint8_t* d_stream, uint64_t stream_cap, uint64_t* d_off, hdlz_join_gzip_result* d_result,
                      void* d_work, size_t work_bytes, void* stream);

typedef struct hdlz_unjoin_gzip_result {
    uint64_t out_len;    /* bytes written to d_out; 0 unless status == HDLZ_OK */
    uint64_t first_bad;  /* lowest index of a member that failed; nmembers for a failure of the stream's own frame; ~0 when OK */
    uint32_t status;
    uint32_t crc;        /* CRC-32 computed over the output; 0 when a member failed to decode */
} hdlz_unjoin_gzip_result;

/*
 * scratch of hdlz_unjoin_gzip_ws: as hdlz_unjoin_work_bytes, with 4 bytes per 32 KiB tile of the output where that has 8:
 *     r256(12 * nmembers) + r256(4 * ceil(total_out / 32768)) + r256(hdlz_inflate_work_bytes(nmembers, 0, 0, flags, 1))
 * 0 for nmembers >= 2^31.
 */
size_t hdlz_unjoin_gzip_work_bytes(uint64_t nmembers, uint64_t total_out, uint32_t flags);

/*
 * hdlz_unjoin_ws for the gzip form: the same parameters, scratch rule (with the query above), per-member rules 1 .. 4, mapping flags,
 * capacity rule, parameter errors, "writes" and "reads" -- the index checks, the three member decoders and the judgement of the
 * members work on absolute offsets and are that call's own kernels.  What differs is the checksum (CRC-32 tiles of the output in
 * place of the Adler sums) and THE STREAM's frame (first_bad = nmembers), judged only when no member failed, in this order:
 *   reject with HDLZ_E_BAD_HEADER when d_off[0] != 10, stream_len < 10 or bytes 0 .. 3 are not 1F 8B 08 00 -- FLG must be 0: this
 *      call reads the header its own writer makes, not gzip at large; MTIME, XFL and OS are not looked at;
 *   reject with HDLZ_E_NO_EOF when stream_len < d_off[nmembers] + 10 or the two bytes at d_off[nmembers] are not 03 00;
 *   reject with HDLZ_E_BAD_CHECKSUM when the little-endian word behind them is not the CRC-32 of the output, or the next one is not
 *      out_len mod 2^32; crc is still reported.
 * nmembers = 0 reads the 20-byte stream (d_off[0] = 10) and answers HDLZ_OK with out_len = 0.  Bytes behind the trailer are no error.
 * reads, of the frame: bytes 0 .. 3 of the stream and, when no member failed, the ten bytes at d_off[nmembers].
 */
int hdlz_unjoin_gzip_ws(const uint8_t* d_stream, uint64_t stream_len,
                        const uint64_t* d_off,          /* nmembers + 1 words, as hdlz_join_gzip_ws wrote them */
                        const uint64_t* d_out_off, uint32_t out_len,
                        uint64_t nmembers, uint32_t flags,
                        uint8_t* d_out, uint64_t out_cap,
                        uint32_t* d_member_status,      /* nullable */
                        hdlz_unjoin_gzip_result* d_result,
                        void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_GZIP_H */
