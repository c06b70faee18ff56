/*
 * hdlz_join.h -- extension of hdlz.h: a batch of blocks as ONE standard zlib stream.
 *
 * hdlz_compress_batch hands back one zlib stream per block.  The two calls here turn such a batch into a single stream that
 * zlib.decompress, pigz -d or any other inflater reads back as the concatenation of the blocks: hdlz_compress_batch_bits is the
 * batch call with one more output -- where every block ended, to the bit --, hdlz_join_batch_ws joins its rows.  The per-block
 * parallelism stays an internal detail, as in pigz.  Additive: HDLZ_VERSION and every declaration of hdlz.h stay as they are; the
 * conventions of hdlz.h (device pointers, ownership, extents, "writes" / "reads", return values) hold here too.
 *
 * THE STREAM.  Blocks 0 .. B-1 with input lengths n_b, X = their concatenation (N bytes), R_b = the row hdlz_compress_batch writes
 * for block b (78 9C, one final fixed block, Adler-32), nbytes_b = d_out_len[b] - 4, E_b = the bit index, from the row's first bit,
 * of the first bit of the block's end-of-block code (E_b >= 19, nbytes_b = (E_b + 14) >> 3), p_b = 8 nbytes_b - E_b - 7 pad bits (0 .. 7):
 *   member M_b = R_b[2 .. nbytes_b) with bit 0 of its first byte cleared (BFINAL = 0), followed by the sync marker of an empty stored
 *                block: 00 00 FF FF when p_b >= 3 (the three header bits fall inside the padding), else 00 00 00 FF FF
 *   stream     = 78 9C, M_0 .. M_{B-1}, 03 00 (a final empty fixed block), Adler-32(X) big-endian; B = 0: 78 9C 03 00 00 00 00 01
 * E_b cannot be recovered from the row: a literal's code may end in zero bits, so the pad bits cannot be told from data.
 */
#ifndef HDLZ_JOIN_H
#define HDLZ_JOIN_H
#include "hdlz.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes that hold the joined stream of nblocks blocks of at most in_len bytes: 8 + nblocks * (hdlz_out_bound(in_len) - 1) */
size_t hdlz_join_bound(uint64_t nblocks, uint32_t in_len);

/* scratch of hdlz_join_batch_ws: 0 for nblocks = 0 (or >= 2^31), else 8 + 24 bytes per tile of 256 rows, rounded up to 256 */
size_t hdlz_join_work_bytes(uint64_t nblocks);

typedef struct hdlz_join_result {
    uint64_t stream_len;   /* length of the joined stream; 0 when a block failed */
    uint32_t status;       /* HDLZ_OK, HDLZ_E_OUT_CAPACITY or the worst status of a block */
    uint32_t adler;        /* Adler-32 of the concatenated input (the stream's trailer); 0 when a block failed */
} hdlz_join_result;

/*
 * hdlz_compress_batch with the end bits: same parameters, same checks, the same bytes in d_out, d_out_len and d_status -- and
 * d_end_bits[b] = E_b for every block whose status is HDLZ_OK, 0 for a block that fails.  d_end_bits is REQUIRED (NULL or not 8-byte
 * aligned: HDLZ_E_BAD_PARAM).  Every block goes through the wave-per-block kernels, batches of small blocks included (the mapping
 * that packs several small blocks per wave does not report end bits); the bytes are the same either way.
 * writes: as hdlz_compress_batch, plus d_end_bits[0 .. nblocks).  reads: as hdlz_compress_batch.
 */
int hdlz_compress_batch_bits(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len,
                             uint64_t nblocks, int cwindow, int maxmatch, uint8_t* d_out, uint64_t out_pitch,
                             uint32_t* d_out_len, uint32_t* d_status,
                             uint64_t* d_end_bits,   /* required */
                             void* stream);

/*
 * The join: rows, lengths, end bits and statuses as hdlz_compress_batch_bits left them (row b at d_rows + b * row_pitch) -> the
 * stream above in d_stream, in two launches (a ticketed decoupled look-back over tiles of 256 rows that scans the member lengths and
 * copies the members, as hdlz_archive_batch does; one workgroup that finishes the checksum).
 *   d_in_off / in_len  the INPUT lengths of the blocks, for the combined Adler-32 (no input byte is read): with d_in_off block b has
 *                      in_off[b+1] - in_off[b] bytes, otherwise every block has in_len bytes.  Pass what the compress call was given.
 *   d_off              nblocks + 1 words, WRITTEN: d_off[b] = where member b starts (d_off[0] = 2), d_off[nblocks] = where 03 00
 *                      starts; stream_len = d_off[nblocks] + 6.  (A failed block counts as a member of length 0.)
 *   d_result           the result record, WRITTEN.  status, in this order of precedence:
 *                        the numerically largest status of any failed block (a row whose length, end bit and row_pitch contradict each
 *                        other counts as failed with HDLZ_E_BAD_PARAM); then stream_len = adler = 0 and the bytes of d_stream inside
 *                        [0, stream_cap) are unspecified;
 *                        HDLZ_E_OUT_CAPACITY when stream_len > stream_cap: stream_len and adler are still reported, members that
 *                        would end beyond stream_cap are not copied, and neither is the trailer;
 *                        otherwise HDLZ_OK.
 *   d_work / work_bytes at least hdlz_join_work_bytes(nblocks) bytes, 8-byte aligned (NULL allowed when that is 0).
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_stream, d_off or d_result NULL; with nblocks > 0 any of d_rows,
 * d_len, d_end_bits, d_status, d_work NULL; nblocks >= 2^31; work_bytes below the query; d_work, d_off or d_result not 8-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_stream[0 .. min(stream_len, stream_cap)) -- never a byte at or behind stream_cap --, d_off[0 .. nblocks], the result
 *         record, d_work[0 .. work_bytes).
 * reads:  d_len, d_end_bits, d_status [0 .. nblocks); d_in_off[0 .. nblocks] when given; of row b only bytes below d_len[b]: the
 *         members are loaded 16 bytes at a time counted from row + 2, whole 16-byte pieces of row[2 .. d_len[b] - 4) only, the rest
 *         and the four trailer bytes singly -- so no load reaches past d_len[b], and none outside the row: a row with
 *         d_len[b] > row_pitch is not read at all (it counts as failed).  The initial contents of d_stream, d_off, d_result and d_work
 *         never reach a result.
 */
int hdlz_join_batch_ws(const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_end_bits,
                       const uint32_t* d_status, const uint64_t* d_in_off, uint32_t in_len, uint64_t nblocks,
                       uint8_t* d_stream, uint64_t stream_cap, uint64_t* d_off, hdlz_join_result* d_result,
                       void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_JOIN_H */
