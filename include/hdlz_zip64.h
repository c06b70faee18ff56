/*
 * hdlz_zip64.h -- extension of hdlz_zip_write.h: ZIP64, the form a ZIP file takes once it passes 4 GiB or 65535 entries (what
 * numpy.savez, zipfile, Info-ZIP, Java and Go switch to without a word), indexed, read and written on the device.  Additive: HDLZ_VERSION and
 * every declaration, struct and refusal of the headers in front of it stay as they are -- hdlz_zip_index_ws still refuses the locator
 * --, and their conventions (device pointers, ownership, extents, "writes" / "reads", return values) hold here too.  The two result
 * records are those of hdlz_zip.h; the entry record is this header's.
 *
 * Sizes, CRC-32 and method come from the CENTRAL DIRECTORY only, as in hdlz_zip.h.  All words of the format are little-endian; a
 * "word" below is 16, 32 or 64 bits as the format has it; "all ones" is FFFF or FFFFFFFF.
 *
 * THE INDEX RULE (hdlz_zip64_index_ws), a serial text; every result equals it for every file (tests/zip64_ref.py states it in Python):
 *   1  the end record
 *        file_len < 22                                               HDLZ_E_NO_EOF
 *        p = the LARGEST offset in [max(0, file_len - 22 - 65535), file_len - 22] whose bytes are 50 4B 05 06 and for which
 *            p + 22 + comment_len(p) == file_len (comment_len: the 16-bit word at p + 20).  No such p: HDLZ_E_BAD_HEADER
 *        WITH A LOCATOR -- p >= 20 and the bytes at p - 20 are 50 4B 06 07 -- the file is ZIP64; each line is HDLZ_E_BAD_HEADER:
 *          the locator's disk (the 32-bit word at p - 16) is not 0, or its disk count (p - 4) is above 1
 *          r = the 64-bit word at p - 12; r + 56 > p - 20, or the bytes at r are not 50 4B 06 06
 *          s = the 64-bit word at r + 4; s < 44 or r + 12 + s != p - 20 -- the ZIP64 end record must fit exactly, as the comment
 *              must; an extensible data sector (s > 44) is allowed and skipped
 *          the disk (32 bits at r + 16) or the directory's disk (r + 20) is not 0, or the entries on this disk (64 bits at r + 24)
 *              differ from the total (r + 32)
 *          cd_size = the 64-bit word at r + 40, cd_off = the one at r + 48; cd_off + cd_size != r
 *          total > cd_size / 46
 *          one of the classic record's six values -- the two disk numbers (p + 4, p + 6), the two counts (p + 8, p + 10), cd_size
 *              (p + 12), cd_off (p + 16) -- is neither equal to the ZIP64 value nor all ones
 *          The directory ends at D = r.
 *        WITHOUT A LOCATOR the rule of hdlz_zip.h holds word for word: the disk number (p + 4) or the directory's disk (p + 6) is
 *          not 0, entries on this disk (p + 8) != total entries (p + 10), or cd_off + cd_size != p (the 32-bit words at p + 16 and
 *          p + 12): HDLZ_E_BAD_HEADER.  The directory ends at D = p.
 *        A failure of step 1 ends the call: nentries = total_out = cd_off = cd_size = 0 and no record is written.
 *   2  the directory walk    q = cd_off; for e = 0 .. total - 1:
 *        q + 46 > D, or the bytes at q are not 50 4B 01 02: stop with HDLZ_E_BAD_HEADER
 *        q' = q + 46 + n + m + k (the name, extra and comment lengths at q + 28, q + 30, q + 32); q' > D: stop with HDLZ_E_BAD_HEADER
 *        entry e is PASSED: its central record starts at q; q = q'
 *      after the last entry q != D: HDLZ_E_BAD_HEADER (all entries passed).  At a stop nentries is the number of entries passed.
 *   3  per passed entry      method (q + 10), flags (q + 8), crc (q + 16), name_len (q + 28) are the central record's; csize
 *      (q + 20), usize (q + 24), the disk start (q + 34) and the local offset L (q + 42) are its classic words, zero-extended, unless
 *      the ZIP64 field replaces them.  The first line that applies sets the entry's status; none stops the walk:
 *        flags & 0x41 (encrypted, strong encryption)                 HDLZ_E_BAD_BTYPE
 *        method not 0 (stored) or 8 (deflated)                       HDLZ_E_BAD_BTYPE
 *        THE ZIP64 FIELD, with and without a locator: the record's m extra bytes (behind the name) are walked as fields
 *          (id16, len16, data); the walk ends where fewer than 4 bytes remain or a field overruns m.  X is the first field whose id
 *          is 0001.  Values are taken from the front of X's data in this order, each ONLY IF its classic word is all ones: usize
 *          (8 bytes), csize (8), L (8), the disk start (4).  A value X cannot supply (no X, or X too short) keeps its all-ones
 *          word, no later value is taken, and the entry is                                     HDLZ_E_BAD_HEADER
 *          a disk start that is not 0                                HDLZ_E_BAD_HEADER
 *        method == 0 and csize != usize                              HDLZ_E_BAD_HEADER
 *        L + 30 > cd_off, or the bytes at L are not 50 4B 03 04      HDLZ_E_BAD_HEADER
 *        payload_off = L + 30 + the LOCAL header's own name and extra lengths (L + 26, L + 28)
 *        payload_off + csize > cd_off                                HDLZ_E_BAD_HEADER
 *      All of it in 64 bits.  No other local field is compared.  payload_off is 0 when the status is not HDLZ_OK.
 *   4  offsets               as in hdlz_zip.h: out_off[0] = 0; out_off[e + 1] = out_off[e] + s_e rounded up to a multiple of
 *      out_align, s_e being usize for an entry whose status is HDLZ_OK and 0 for a failed one; total_out = out_off[last] + s_last.
 *   5  capacity              nentries > entry_cap: HDLZ_E_OUT_CAPACITY in front of the walk's own status; nentries, cd_off and cd_size
 *      are the true ones, only d_entries[0 .. entry_cap) is written, and total_out counts the entries [0, entry_cap) ONLY -- so it
 *      is 0 in the sizing call (entry_cap = 0, d_entries NULL), which tells the caller the entry_cap to repeat the call with.
 * The record's status is that of step 1, else HDLZ_E_OUT_CAPACITY (step 5), else that of step 2; the statuses of step 3 stand in the
 * entries only.
 * EQUALITY WITH hdlz_zip_index_ws: for every file without a locator in which no entry has an all-ones size, offset or disk word, the
 * records and the result are those of hdlz_zip_index_ws, widened (with entry_cap >= nentries: step 5 differs in total_out).
 *
 *
 * THE FILE RULE (hdlz_zip64_write_ws), a serial text; the file equals it for every input (tests/zip64_ref.py states it in Python).
 * THE INPUT is that of hdlz_zip_write.h; nentries may be anything below 2^31.  zip64_from: a size or an offset that is >= zip64_from
 * goes into a ZIP64 field -- FFFFFFFF is the standard value ("only where the format needs it"), 0 means "always", any value between
 * is legal.
 *   1  failing entries       the first cause that applies wins
 *        F_e > F_{e+1} or F_{e+1} > B                                                           HDLZ_E_BAD_PARAM
 *        a block of e whose status is not HDLZ_OK                       the numerically largest such status
 *        a row of e whose length, end bit and row_pitch contradict each other (hdlz_join.h), or whose block has a negative
 *        length                                                                                 HDLZ_E_BAD_PARAM
 *        e has blocks and in_off[F_{e+1}] - in_off[F_e] != u_e                                  HDLZ_E_BAD_PARAM
 *        n_e > 65535                                                                            HDLZ_E_BAD_PARAM
 *      (no cause hangs on u_e any more)
 *   2  entries without blocks   F_e == F_{e+1}: the entry is STORED, whatever its length.
 *   3  the choice of form    as in hdlz_zip_write.h: the deflated payload is the members M_b of the entry's rows followed by 03 00,
 *      c_e its length; it is CHOSEN iff c_e < u_e; otherwise the entry is stored and c_e = u_e.
 *   4  the entry's bytes     L_e: where its local header starts.
 *        the LOCAL header has a ZIP64 extra iff u_e >= zip64_from or c_e >= zip64_from: 30 + n_e + 20 bytes
 *          50 4B 03 04 | 2D 00 | flags | method | time | date | crc | FFFFFFFF | FFFFFFFF | n_e | 14 00 | name | 01 00 10 00 | u_e | c_e
 *        (u_e and c_e 64-bit words); without it the 30 + n_e bytes of hdlz_zip_write.h, version 14 00 unless the central record has an
 *        extra.  The payload behind it, the next entry behind that.
 *        the CENTRAL record: usize, csize and L_e, in this order, go into the extra 01 00 | 8k | the k values (64-bit words), each
 *        iff it is >= zip64_from, and its 32-bit word is then FFFFFFFF; never a disk word.  46 + n_e + (k ? 4 + 8k : 0) bytes:
 *          50 4B 01 02 | version | version | flags | method | time | date | crc | csize | usize | n_e | extra length | comment 0 |
 *          disk 0 | internal 0 | external 0 | local offset | name | the extra
 *        version: 2D 00 in all three version words of an entry with a ZIP64 extra in either header (a local one implies a central
 *        one), 14 00 in the others.  The form, the members, the flags, the times and the names are those of hdlz_zip_write.h.
 *        BEHIND THE DIRECTORY, iff E > 65535, cd_off >= zip64_from or cd_size >= zip64_from, the 56-byte ZIP64 end record
 *          50 4B 06 06 | 44 (64 bits) | 2D 00 | 2D 00 | 0 | 0 (32 bits each) | E | E | cd_size | cd_off (64 bits each)
 *        and the 20-byte locator 50 4B 06 07 | 0 | the offset of that record (64 bits) | 1.  Then the classic end record
 *          50 4B 05 06 | 0 | 0 | min(E, FFFF) twice | cd_size | cd_off | 0
 *        cd_size and cd_off as FFFFFFFF when they are >= zip64_from.  E = 0 at zip64_from > 0 gives the 22-byte file.
 *   5  limits                none but file_cap.
 *   6  the record's status   as in hdlz_zip_write.h: the largest status of any failed entry (first_bad the lowest such entry;
 *      file_len = cd_off = cd_size = nstored = 0), else HDLZ_E_OUT_CAPACITY when file_len > file_cap -- the lengths are the true ones, a
 *      call with file_cap = 0 is the sizing call, and no byte of d_file is written --, else HDLZ_OK.
 *   7  d_entries             when given: the records hdlz_zip64_index_ws would write for this file with the same out_align, also when
 *      the file did not fit.  When an entry failed: every record is zero but its status, which is the entry's own.
 * IDENTITY WITH hdlz_zip_write_ws: with zip64_from = FFFFFFFF every input for which hdlz_zip_write_ws answers HDLZ_OK gives the same
 * file byte for byte.
 *
 * Not there: deflated entries above 2^28 - 7 compressed bytes or 2^32 - 512 bytes of output READ (the decoders' limits, below; they
 * are written); a speculative directory walk (the walk is the one serial part: a hop per entry); data descriptors written; appending
 * to an archive; encryption; what hdlz_zip.h and hdlz_zip_write.h leave out.
 */
#ifndef HDLZ_ZIP64_H
#define HDLZ_ZIP64_H
#include "hdlz_zip_write.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hdlz_zip64_entry {   /* 64 bytes; the members of hdlz_zip_entry, sizes in 64 bits */
    uint64_t cd_off, payload_off, out_off, csize, usize;
    uint32_t crc, status;
    uint16_t method, flags, name_len, reserved;   /* reserved: 0 */
    uint64_t reserved2;                           /* 0 */
} hdlz_zip64_entry;

/*
 * scratch of hdlz_zip64_index_ws: 0 for entry_cap >= 2^31, else
 *     256 + r256(16 entry_cap),   r256 = rounded up to 256
 * (a 256-byte summary; for each of the entry_cap entries that get a record the 64-bit offset of its central record and the 64-bit
 * size it counts in the output).  It does not depend on file_len.
 */
size_t hdlz_zip64_index_work_bytes(uint64_t file_len, uint64_t entry_cap);

/*
 * Index a ZIP or ZIP64 file on the device: THE INDEX RULE above.  The host reads nothing inside the call.  The four launches of
 * hdlz_zip_index_ws, generalised: (a) one workgroup finds the end record and, behind a locator, reads the ZIP64 end record; (b) one
 * workgroup walks the directory through LDS in pieces of 16 KiB, one hop per LDS round trip, offsets in 64 bits -- it stores the
 * offsets of the first entry_cap central records and counts the entries behind them --; (c) a thread per entry below entry_cap
 * parses the 46 bytes, walks the extra fields for the ZIP64 one, loads the local header's two lengths and makes the checks of
 * step 3; (d) one workgroup scans the sizes of those entries for out_off, each thread a run of ceil(n / 1024) of them, and writes
 * the record.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: d_result NULL, or d_file NULL with file_len > 0;
 * d_entries NULL with entry_cap > 0; entry_cap >= 2^31; out_align not a power of two in [1, 256]; d_work NULL or work_bytes below
 * the query; d_entries, d_result or d_work not 8-byte aligned.  file_len may be any value.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_entries[0 .. min(nentries, entry_cap)), the record, d_work[0 .. work_bytes).
 * reads:  d_file[0 .. file_len) only -- never a load outside it.  The initial contents of the outputs and of d_work never reach a
 *         result.
 */
int hdlz_zip64_index_ws(const uint8_t* d_file, uint64_t file_len, uint64_t entry_cap, uint32_t out_align,
                        hdlz_zip64_entry* d_entries,    /* entry_cap records, WRITTEN; NULL allowed with entry_cap = 0 */
                        hdlz_zip_index_result* d_result, void* d_work, size_t work_bytes, void* stream);

/*
 * scratch of hdlz_zip64_inflate_ws: 0 for count = 0 or count >= 2^31, else
 *     2 * r256(24 count) + T + D
 *     T = r256(4 ceil(out_cap / 32768)) and D = r256(hdlz_inflate_work_bytes(1, in_len, R, 0, 1)) when count == 1, else both 0;
 *     R = min(out_cap rounded down to 4, 2^32 - 512): the row the one-stream path is given
 * (the layout of hdlz_zip_inflate_work_bytes; for out_cap <= 2^32 - 512 the same number.)
 */
size_t hdlz_zip64_inflate_work_bytes(uint64_t count, uint32_t in_len, uint64_t out_cap);

/*
 * hdlz_zip_inflate_ws over the records of this header: entries [first, first + count) of an index, entry e decoded to its SLOT
 * d_out + (out_off[e] - out_off[first]).  THE ROUTES and THE JUDGEMENT are those of hdlz_zip.h, run by the same kernels; file_len may
 * be any value, all offsets are 64-bit, and a stored entry may have any size.  The checks in front of the decode, the first line
 * that applies wins, and a refused entry is not decoded:
 *     the record's status is not HDLZ_OK                                          that status
 *     method not 0 or 8, or method == 0 and csize != usize                        HDLZ_E_BAD_PARAM
 *     payload_off < 30, or payload_off + csize + 4 > file_len                     HDLZ_E_BAD_PARAM
 *     out_off[e] < out_off[first], or the slot ends behind out_cap                HDLZ_E_BAD_PARAM
 *     deflated and usize > 2^32 - 512 (the decoders' room)                        HDLZ_E_OUT_CAPACITY
 *     deflated and csize > 2^28 - 7 (the decoders count bits in 32)               HDLZ_E_BAD_PARAM
 *     usize >= 2^32 off the one-stream path -- count >= 2, or count == 1 at a d_out that path does not take -- (crc_block takes
 *         32-bit lengths; the caller gives such an entry a call of its own, as it does for large entries)      HDLZ_E_BAD_PARAM
 *     in_len != 0 and: count > 1 and csize > in_len; count == 1, deflated and csize + 6 > in_len      HDLZ_E_BAD_PARAM
 * With count == 1 on the one-stream path a stored entry of any size is a flat copy over the whole GPU and its CRC-32 comes from
 * the 32 KiB tile kernels, both 64-bit; the decoder is given the row d_out[0 .. R), R as in the scratch query.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: d_result NULL; with count > 0 any of d_file,
 * d_entries NULL; d_out NULL with out_cap > 0; first + count >= 2^31; d_entries or d_result not 8-byte aligned; d_entry_status not
 * 4-byte aligned; d_work not 256-byte aligned; with count > 0, d_work NULL or work_bytes below the query.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_out inside the slots of the entries that passed the checks, never a byte at or behind out_cap (count == 1 on the
 *         one-stream path: inside the row, as hdlz_zip_inflate_ws); d_entry_status[0 .. count) when given, the record,
 *         d_work[0 .. work_bytes).
 * reads:  d_entries[first .. first + count); d_file[0 .. file_len) only -- never a load outside it; of a slot only its usize bytes.
 *         The initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_zip64_inflate_ws(const uint8_t* d_file, uint64_t file_len, const hdlz_zip64_entry* d_entries, uint64_t first, uint64_t count,
                          uint32_t in_len, uint8_t* d_out, uint64_t out_cap,
                          uint32_t* d_entry_status,   /* nullable */
                          hdlz_zip_inflate_result* d_result, void* d_work, size_t work_bytes, void* stream);

/*
 * bytes that hold the file whatever zip64_from is:
 *     98 + 124 nentries + 2 names_len + total_in
 * (22 + 56 + 20 behind the directory; 30 + 20 + 46 + 28 bytes and the name twice per entry; nblocks and block_len do not enter.)
 */
size_t hdlz_zip64_write_bound(uint64_t nentries, uint64_t nblocks, uint32_t block_len, uint64_t total_in, uint64_t names_len);

/*
 * scratch of hdlz_zip64_write_ws: 0 for nentries >= 2^31 or nblocks >= 2^31, else
 *     r256(8 + 16 ceil(nblocks / 256)) + 2 r256(8 (nblocks + 1)) + 256 + 4 r256(8 (nentries + 1)) + 2 r256(4 (nentries + 1))
 * (the layout of hdlz_zip_write_work_bytes with c_e in a 64-bit word.)
 */
size_t hdlz_zip64_write_work_bytes(uint64_t nentries, uint64_t nblocks);

/*
 * Write the file: THE FILE RULE above.  The host reads nothing inside the call.  The four launches of hdlz_zip_write_ws: (z) and (a),
 * the zeroing and the tile scan over the blocks, are the same kernels; (b) ONE workgroup of 1024 threads plans any number of entries,
 * each thread a run of ceil(nentries / 1024): a local record's size hangs on u_e and c_e alone, a central record's on L_e too, so the
 * offsets take two scans one behind the other -- the local records, then the central ones -- and thread 0 writes the end records and
 * the result record; (c) the gather: its rows and its tiles of the stored copy are the code of hdlz_zip_write_ws, and the wave that
 * writes an entry's two headers writes the ZIP64 extras behind the names and d_entries[e].  All bulk stores are 16 bytes to 16-byte
 * aligned addresses of d_file.
 *   flags, dos_datetime, out_align, total_in    as in hdlz_zip_write_ws
 *   zip64_from    at most FFFFFFFF
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: d_result NULL; nentries >= 2^31; nblocks >= 2^31,
 * or nblocks > 0 with nentries = 0; with nentries > 0 any of d_in, d_ent_off, d_names, d_name_off, d_blk_first, d_crc NULL; with
 * nblocks > 0 any of d_in_off, d_rows, d_len, d_end_bits, d_status NULL; d_file NULL with file_cap > 0; a bit of flags other than
 * HDLZ_ZIP_FLAG_UTF8; out_align not a power of two in [1, 256]; zip64_from > FFFFFFFF; d_work NULL or work_bytes below the query;
 * d_ent_off, d_name_off, d_in_off, d_end_bits, d_blk_first, d_entries, d_result or d_work not 8-byte aligned; d_len, d_status or d_crc
 * not 4-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_file[0 .. min(file_len, file_cap)), d_entries[0 .. nentries) when given, the record, d_work[0 .. work_bytes).
 * reads:  as hdlz_zip_write_ws: the index arrays, the names exactly, of row b only the bytes [2, d_len[b] - 4) and only when its
 *         entry is deflated, of entry e exactly its u_e bytes and only when it is stored.  The initial contents of the outputs and
 *         of d_work never reach a result.
 */
int hdlz_zip64_write_ws(const uint8_t* d_in, const uint64_t* d_ent_off, const uint8_t* d_names, const uint64_t* d_name_off, uint64_t nentries,
                        const uint64_t* d_in_off, const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_end_bits,
                        const uint32_t* d_status, uint64_t nblocks, const uint64_t* d_blk_first, const uint32_t* d_crc, uint32_t flags,
                        uint32_t dos_datetime, uint32_t out_align, uint64_t zip64_from, uint64_t total_in, uint8_t* d_file, uint64_t file_cap,
                        hdlz_zip64_entry* d_entries,    /* nullable: nentries records, WRITTEN */
                        hdlz_zip_write_result* d_result, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_ZIP64_H */
