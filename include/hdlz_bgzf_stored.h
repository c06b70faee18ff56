/*
 * hdlz_bgzf_stored.h -- extension of hdlz_bgzf.h: a BGZF writer that can fall back to a STORED member.  hdlz_bgzf_join_ws frames every
 * block as one fixed-Huffman member; bytes that do not compress grow by 9/8 there, so it guarantees only blocks of up to 58230 bytes
 * and fails a 65280-byte block (bgzip's and htslib's block size) of random, compressed or encrypted bytes.  hdlz_bgzf.h leaves "a
 * stored-block fallback for incompressible blocks" out of scope; this header takes that line up.  The join below chooses per block
 * between the row's fixed block and the input bytes behind a stored block's five header bytes, whichever member is shorter -- so it has
 * to be given the input, which hdlz_bgzf_join_ws never reads.  With it
 *   - a file in which every block takes the fixed form is byte-identical to hdlz_bgzf_join_ws's,
 *   - a member never exceeds n_b + 31 bytes (n_b: the block's input length): the writer expands no data beyond its framing,
 *   - blocks of up to 65505 bytes never fail for their content, and blocks of 0 to 4 bytes (HDLZ_E_SHORT_INPUT in the compressor: the
 *     reference never starts below 5 bytes) are written stored.
 * The read side needs nothing new: hdlz_bgzf_index_ws, hdlz_bgzf_inflate_ws and hdlz_bgzf_read_ranges_ws decode stored members.
 * Additive: HDLZ_VERSION and every declaration of hdlz.h, hdlz_join.h, hdlz_unjoin.h, hdlz_gzip.h, hdlz_bgzf.h and hdlz_bgzf_range.h
 * stay as they are, and their conventions (device pointers, ownership, extents, "writes" / "reads", return values) hold here too.
 *
 * Out of scope: a stored form in the joined zlib / gzip streams (their member view refuses a first block that is not fixed), skipping
 * the compressor for blocks known not to compress, a faster stored copy in the reader, fusing the CRC-32 into the compressor.
 */
#ifndef HDLZ_BGZF_STORED_H
#define HDLZ_BGZF_STORED_H
#include "hdlz_bgzf.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * bytes that hold the file hdlz_bgzf_join_stored_ws writes from nblocks blocks of at most in_len bytes:
 *     28 + nblocks * min(hdlz_out_bound(in_len) + 20, in_len + 31)
 * (per block the shorter of the two forms' worst cases; the EOF member behind them)
 */
size_t hdlz_bgzf_stored_bound(uint64_t nblocks, uint32_t in_len);

/* scratch of hdlz_bgzf_join_stored_ws: the same as hdlz_join_work_bytes(nblocks) */
size_t hdlz_bgzf_join_stored_work_bytes(uint64_t nblocks);

typedef struct hdlz_bgzf_stored_result {
    uint64_t file_len;    /* length of the file, the EOF member included; 0 when a block failed */
    uint64_t nstored;     /* members written in the stored form; 0 when a block failed */
    uint32_t status;      /* HDLZ_OK, HDLZ_E_OUT_CAPACITY or the worst status of a block */
    uint32_t first_bad;   /* lowest index of a block that failed; 0xFFFFFFFF when none did */
} hdlz_bgzf_stored_result;

/*
 * The BGZF writer with the stored fallback.  d_in, d_in_off, in_pitch, in_len: the input exactly as hdlz_compress_batch was given it,
 * ragged or pitched, with the same addressing rule (block b is d_in[d_in_off[b] .. d_in_off[b + 1]) when d_in_off is given, else the
 * in_len bytes at d_in + b * in_pitch); d_rows, row_pitch, d_len, d_status: the rows, lengths and statuses exactly as that call left
 * them; d_crc[0 .. nblocks): the CRC-32 of every input block, put there earlier on the same stream by hdlz_crc32_batch_ws.
 *
 * THE MEMBER RULE is this serial statement; the file equals it for every input.  For block b with n_b input bytes, status st =
 * d_status[b] and row length L = d_len[b]:
 *   1. st is neither HDLZ_OK nor HDLZ_E_SHORT_INPUT: the block fails with st.
 *   2. st == HDLZ_OK and (L < 8 or L > row_pitch): the block fails with HDLZ_E_BAD_PARAM (the length and the pitch contradict each
 *      other: hdlz_bgzf_join_ws's rule).
 *   3. n_b > 65505: the block fails with HDLZ_E_OUT_CAPACITY (a stored member is n_b + 31 bytes, and a member holds 65536).
 *   4. The fixed form is USABLE iff st == HDLZ_OK and L + 20 <= 65536.  Its member is L + 20 bytes, byte for byte what
 *      hdlz_bgzf_join_ws writes: HEADER(16) | BSIZE = L + 19 (LE16) | row b's bytes [2, L - 4) | d_crc[b] (LE32) | n_b (LE32).
 *   5. The fixed form is CHOSEN iff it is usable and L + 20 <= n_b + 31; a tie goes to the fixed form.  Otherwise the stored form is
 *      chosen, n_b + 31 bytes:
 *        HEADER(16) | BSIZE = n_b + 30 (LE16) | 01 | n_b (LE16) | ~n_b (LE16) | the n_b input bytes | d_crc[b] (LE32) | n_b (LE32)
 *      (HEADER(16): the first sixteen bytes of hdlz_bgzf.h's HEADER; 01: BFINAL = 1, BTYPE = 00 and five pad bits.)  n_b = 0 is a legal
 *      stored member of 31 bytes; a block with HDLZ_E_SHORT_INPUT is always stored.
 *   6. A failed block counts as a member of length 0.
 *   7. The precedence of the record's status, first_bad, the behaviour at file_cap, d_off and the EOF member are those of
 *      hdlz_bgzf_join_ws: d_off[b] = where member b starts (d_off[0] = 0), d_off[nblocks] = where the EOF member starts, file_len =
 *      d_off[nblocks] + 28; the numerically largest status of any failed block comes first -- then file_len = 0, nstored = 0 and the
 *      bytes of d_file inside [0, file_cap) are unspecified --; else HDLZ_E_OUT_CAPACITY when file_len > file_cap: file_len and nstored
 *      are still reported, members that would end beyond file_cap are not copied and neither is the EOF member; otherwise HDLZ_OK.
 *      nblocks = 0 writes the EOF member alone.
 *   d_kind      nullable, nblocks bytes, WRITTEN: 0 where the fixed form was chosen (and for a failed block), 1 where the stored form was.
 *   d_work      at least hdlz_bgzf_join_stored_work_bytes(nblocks) bytes, 8-byte aligned (NULL allowed when that is 0).
 * Two launches behind the zeroing of the scratch: the ticketed tile, look-back scan and wave-per-row gather of hdlz_bgzf_join_ws in a
 * kernel of its own that decides length and source per row, then the EOF member and the record.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_file, d_off or d_result NULL; with nblocks > 0 any of d_in,
 * d_rows, d_len, d_status, d_crc, d_work NULL; nblocks >= 2^31; work_bytes below the query; d_work, d_off, d_in_off or d_result not
 * 8-byte aligned; d_crc not 4-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_file[0 .. min(file_len, file_cap)) -- never a byte at or behind file_cap --, d_off[0 .. nblocks], d_kind[0 .. nblocks) when
 *         given, the result record, d_work[0 .. work_bytes).
 * reads:  d_len, d_status, d_crc [0 .. nblocks); d_in_off[0 .. nblocks] when given; of row b only bytes [2, d_len[b] - 4), and only
 *         when the fixed form is chosen; of input block b exactly its n_b bytes, and only when the stored form is chosen -- no load
 *         outside them, at any alignment of source or destination.  The initial contents of d_file, d_off, d_kind, d_result and d_work
 *         never reach a result.
 */
int hdlz_bgzf_join_stored_ws(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len,
                             const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint32_t* d_status,
                             uint64_t nblocks, const uint32_t* d_crc,
                             uint8_t* d_file, uint64_t file_cap, uint64_t* d_off,
                             uint8_t* d_kind,                       /* nullable, nblocks bytes, WRITTEN: 0 fixed, 1 stored */
                             hdlz_bgzf_stored_result* d_result, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_BGZF_STORED_H */
