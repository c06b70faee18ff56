/*
 * hdlz_zip_write.h -- extension of hdlz_zip.h: a ZIP archive (.zip, .npz) WRITTEN on the device from the rows of one compress batch:
 * local headers with their names, every entry's payload deflated or stored, whichever is shorter, the central directory and the end
 * record, in one file that zipfile, unzip, numpy.load and hdlz_zip_index_ws read.  hdlz_zip.h reads the container; this header closes
 * the pair, as hdlz_bgzf.h did for BGZF.  Additive: HDLZ_VERSION and every declaration of hdlz.h and of the extension headers in
 * front of this one stay as they are, and their conventions (device pointers, ownership, extents, "writes" / "reads", return values)
 * hold here too.  All words of the format are little-endian.
 *
 * THE INPUT.  E entries; entry e is d_in[ent_off[e] .. ent_off[e + 1]), u_e bytes, its name d_names[name_off[e] .. name_off[e + 1]),
 * n_e bytes.  B blocks, as ONE hdlz_compress_batch_bits call was given them (d_in_off) and left them (rows, lengths, end bits,
 * statuses); entry e owns the blocks [F_e, F_{e+1}), F = d_blk_first (ascending, F_0 = 0, F_E = B), and block b of entry e holds the
 * in_off[b + 1] - in_off[b] bytes of the entry that start at byte in_off[b] - in_off[F_e] of it: only DIFFERENCES of d_in_off are
 * used, so the compress call may have been given the blocked entries in a buffer of its own.  d_crc[e]: the CRC-32 of entry e.
 *
 * THE FILE RULE, a serial text; the file equals it for every input (tests/zip_write_ref.py states it in Python):
 *   1  failing entries       the first cause that applies wins
 *        F_e > F_{e+1} or F_{e+1} > B (the entry's blocks are no range of the batch)            HDLZ_E_BAD_PARAM
 *        a block of e whose status is not HDLZ_OK                       the numerically largest such status
 *        a row of e whose length, end bit and row_pitch contradict each other (hdlz_join.h: E_b < 19, or
 *        ((E_b + 14) >> 3) + 4 != d_len[b], or d_len[b] > row_pitch), or whose block has a negative length
 *        (in_off[b + 1] < in_off[b])                                                            HDLZ_E_BAD_PARAM
 *        e has blocks and in_off[F_{e+1}] - in_off[F_e] != u_e                                  HDLZ_E_BAD_PARAM
 *        n_e > 65535                                                                            HDLZ_E_BAD_PARAM
 *        u_e >= 2^32 - 1 (no ZIP64)                                                             HDLZ_E_OUT_CAPACITY
 *   2  entries without blocks   F_e == F_{e+1}: the entry is STORED, whatever its length.  This is how the caller says "do not
 *      compress", and how entries under 5 bytes are written (the compressor never starts below 5).
 *   3  the choice of form    otherwise the deflated payload is M_{F_e} .. M_{F_{e+1} - 1} followed by 03 00 (a final empty fixed block),
 *      M_b exactly the member of hdlz_join.h: the row's bytes [2, nbytes_b) with BFINAL cleared, then the 4- or 5-byte sync marker the
 *      pad bits choose; c_e = the payload's length.  The deflated form is CHOSEN iff c_e < u_e; otherwise the entry is stored: the
 *      payload is the u_e input bytes and c_e = u_e.
 *   4  the entry's bytes     the local header, 30 + n_e bytes:
 *        50 4B 03 04 | 14 00 | flags | method (8 or 0) | time | date | crc | csize | usize | n_e | 00 00 | name
 *      -- no extra field and no data descriptor (flag bit 3 is clear) --, the payload behind it, the next entry behind that.  Behind
 *      the last payload the directory, one central record of 46 + n_e bytes per entry:
 *        50 4B 01 02 | 14 00 (made by: 2.0, host 0) | 14 00 | flags | method | time | date | crc | csize | usize | n_e | extra 0 |
 *        comment 0 | disk 0 | internal 0 | external 0 (4 bytes) | local offset | name
 *      (host 0 with zero attributes is a plain file; a Unix host byte with mode 0 would extract unreadable files), then the 22-byte
 *      end record 50 4B 05 06 | 0 | 0 | E | E | cd_size | cd_off | 0: no comment.  E = 0 gives the 22-byte file.
 *   5  limits                no ZIP64: E > 65535 is HDLZ_E_BAD_PARAM in front of the device; a local offset or cd_off >= 2^32 - 1, or a
 *      file of 2^32 bytes or more, gives the record HDLZ_E_OUT_CAPACITY: the lengths are reported and no byte of d_file is written.
 *   6  the record's status, in order of precedence
 *        the largest status of any failed entry: first_bad = the lowest failed entry; file_len = cd_off = cd_size = nstored = 0 and the
 *        bytes inside [0, file_cap) are unspecified;
 *        HDLZ_E_OUT_CAPACITY when file_len > file_cap (or step 5): the true file_len, cd_off, cd_size and nstored are still reported --
 *        a call with file_cap = 0 is the sizing call -- and no byte of d_file is written, so none at or behind file_cap ever is;
 *        otherwise HDLZ_OK.  first_bad is FFFFFFFF when no entry failed.
 *   7  d_entries             when given: the records hdlz_zip_index_ws would write for this file with the same out_align (cd_off,
 *      payload_off, out_off, csize, usize, crc, method, flags, name_len, status = HDLZ_OK; reserved = 0) -- the writer hands back a
 *      ready index --, also when the file did not fit.  When an entry failed: every record is zero but its status, which is the
 *      entry's own (HDLZ_OK for a sound one).
 *
 * Out of scope: ZIP64 (hdlz_zip64.h, the extension of this header, reads and writes it: hdlz_zip64_write_ws); data descriptors; extra fields
 * and payload alignment (zipalign); comments; per-entry times or attributes; encryption; appending to an existing archive;
 * dynamic-tree blocks; a member-parallel read of this writer's own entries (the ZIP carries no block index: hdlz_zip_inflate_ws
 * reads an entry as any inflater does).
 */
#ifndef HDLZ_ZIP_WRITE_H
#define HDLZ_ZIP_WRITE_H
#include "hdlz_zip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HDLZ_ZIP_FLAG_UTF8 0x0800u      /* general purpose bit 11: the names are UTF-8 */

/*
 * bytes that hold the file of nentries entries of total_in bytes with names of names_len bytes in all:
 *     22 + 76 nentries + 2 names_len + total_in
 * (30 + 46 bytes and the name twice per entry; a payload is never longer than its entry, which is why nblocks and block_len -- the
 * bound the compress call was given -- do not enter: they are taken so that a later form of the rule may use them).
 */
size_t hdlz_zip_write_bound(uint64_t nentries, uint64_t nblocks, uint32_t block_len, uint64_t total_in, uint64_t names_len);

/*
 * scratch of hdlz_zip_write_ws: 0 for nentries > 65535 or nblocks >= 2^31, else
 *     r256(8 + 16 ceil(nblocks / 256)) + 2 r256(8 (nblocks + 1)) + 256 + 3 r256(8 (nentries + 1)) + 3 r256(4 (nentries + 1))
 * r256 = rounded up to 256 (the ticket and two look-back words per tile of 256 blocks; per block the prefix of the member lengths and
 * of the failure counts; a summary; per entry three 64-bit and three 32-bit words of the plan).
 */
size_t hdlz_zip_write_work_bytes(uint64_t nentries, uint64_t nblocks);

typedef struct hdlz_zip_write_result {      /* 40 bytes */
    uint64_t file_len;      /* the file's length; 0 when an entry failed */
    uint64_t cd_off;        /* where the directory starts */
    uint64_t cd_size;       /* its length */
    uint64_t nstored;       /* entries written stored (step 2 and the ties of step 3) */
    uint32_t status;
    uint32_t first_bad;     /* the lowest failed entry; FFFFFFFF when none failed */
} hdlz_zip_write_result;

/*
 * Write the file: THE FILE RULE above.  The host reads nothing inside the call.  Four launches: (z) the scan's ticket and look-back
 * words are zeroed; (a) a tile scan with decoupled look-back over the blocks: the exclusive prefix of the member lengths and of the
 * counts of failed and of contradictory rows; (b) ONE workgroup over the entries: c_e from two prefix words, the form, the checks of
 * step 1, the scans of the record sizes for the local offsets, the directory offsets, out_off and the tiles of the stored copy -- it
 * leaves the plan in the scratch and writes the end record and the result record; (c) the gather over the whole GPU, in one grid:
 * a wave per block moves M_b to its place (BFINAL cleared, the marker appended, 03 00 behind an entry's last member; for a stored
 * entry that has blocks the same wave moves the block's input bytes) -- a workgroup takes 16 consecutive blocks, 256 from 65536
 * blocks on, and every wave finds the entries of its quarter by one search in d_blk_first --, workgroups that cut the stored entries without blocks into
 * tiles of 64 KiB (their number sized from total_in and nentries, never from a device word: a workgroup finds its entry by a search in
 * the plan, and strides when total_in understated the bytes), and a wave per entry that writes the local header, the central record,
 * the name behind both and d_entries[e].  All bulk stores are 16 bytes to 16-byte aligned addresses of d_file.  nblocks = 0: (z) and
 * (a) are not launched.
 *   flags         only HDLZ_ZIP_FLAG_UTF8 may be set; it goes into both headers of every entry
 *   dos_datetime  date << 16 | time (MS-DOS), the same for all entries
 *   out_align     a power of two from 1 to 256, as in hdlz_zip_index_ws: for out_off of d_entries
 *   total_in      what hdlz_zip_write_bound was given: sizes the grid of the stored copy and nothing else -- any value gives the same file
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: d_result NULL; nentries > 65535; nblocks >= 2^31,
 * or nblocks > 0 with nentries = 0; with nentries > 0 any of d_in, d_ent_off, d_names, d_name_off, d_blk_first, d_crc NULL; with
 * nblocks > 0 any of d_in_off, d_rows, d_len, d_end_bits, d_status NULL; d_file NULL with file_cap > 0; a bit of flags other than
 * HDLZ_ZIP_FLAG_UTF8; out_align not a power of two in [1, 256]; d_work NULL or work_bytes below the query; d_ent_off, d_name_off,
 * d_in_off, d_end_bits, d_blk_first, d_entries, d_result or d_work not 8-byte aligned; d_len, d_status or d_crc not 4-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_file[0 .. min(file_len, file_cap)), d_entries[0 .. nentries) when given, the record, d_work[0 .. work_bytes).
 * reads:  d_ent_off, d_name_off, d_blk_first [0 .. nentries]; d_crc[0 .. nentries); d_in_off[0 .. nblocks]; d_len, d_end_bits, d_status
 *         [0 .. nblocks); the names, exactly their bytes; of row b only the bytes [2, d_len[b] - 4), and only when its entry is
 *         deflated; of entry e exactly its u_e bytes, and only when it is stored -- no load outside these, at any alignment of source
 *         or destination.  The initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_zip_write_ws(const uint8_t* d_in, const uint64_t* d_ent_off, const uint8_t* d_names, const uint64_t* d_name_off, uint64_t nentries,
                      const uint64_t* d_in_off, const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_end_bits,
                      const uint32_t* d_status, uint64_t nblocks, const uint64_t* d_blk_first, const uint32_t* d_crc, uint32_t flags,
                      uint32_t dos_datetime, uint32_t out_align, uint64_t total_in, uint8_t* d_file, uint64_t file_cap,
                      hdlz_zip_entry* d_entries,      /* nullable: nentries records, WRITTEN */
                      hdlz_zip_write_result* d_result, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_ZIP_WRITE_H */
