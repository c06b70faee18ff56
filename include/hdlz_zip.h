/*
 * hdlz_zip.h -- extension of hdlz_gzip.h: ZIP archives (.zip, .npz, .jar, .whl, .docx) of any writer, the directory indexed and the
 * entries read on the device, every entry judged against the central directory (CRC-32, sizes).  hdlz_gunzip.h reads gzip members,
 * hdlz_bgzf.h BGZF files; this header takes up the one deflate container they leave.  Additive: HDLZ_VERSION and every declaration of
 * hdlz.h, hdlz_join.h, hdlz_unjoin.h, hdlz_gzip.h, hdlz_bgzf.h, hdlz_bgzf_range.h, hdlz_bgzf_stored.h and hdlz_gunzip.h stay as they
 * are, and their conventions (device pointers, ownership, extents, "writes" / "reads", return values) hold here too.
 *
 * Sizes, CRC-32 and method come from the CENTRAL DIRECTORY only; an entry's local header is used to find its payload and for nothing
 * else (writers on unseekable streams leave its CRC and sizes zero and set flag bit 3; numpy.savez_compressed gives it a 20-byte ZIP64
 * extra field the central record does not have).  All words of the format are little-endian.
 *
 * THE INDEX RULE (hdlz_zip_index_ws), a serial text; every result equals it for every file (tests/zip_ref.py states it in Python):
 *   1  the end record
 *        file_len < 22                                               HDLZ_E_NO_EOF
 *        p = the LARGEST offset in [max(0, file_len - 22 - 65535), file_len - 22] whose bytes are 50 4B 05 06 and for which
 *            p + 22 + comment_len(p) == file_len (comment_len: the 16-bit word at p + 20) -- the comment must fit exactly, so a
 *            look-alike inside a comment or a nested archive is not taken.  No such p: HDLZ_E_BAD_HEADER
 *        p >= 20 and the bytes at p - 20 are 50 4B 06 07 (the ZIP64 locator)    HDLZ_E_BAD_HEADER
 *        the disk number (p + 4) or the directory's disk (p + 6) is not 0, entries on this disk (p + 8) != total entries (p + 10),
 *        or cd_off + cd_size != p (cd_size: the word at p + 12, cd_off: the word at p + 16)      HDLZ_E_BAD_HEADER
 *        A failure of step 1 ends the call: nentries = total_out = cd_off = cd_size = 0 and no record is written.
 *   2  the directory walk    q = cd_off; for e = 0 .. total - 1:
 *        q + 46 > p, or the bytes at q are not 50 4B 01 02: stop with HDLZ_E_BAD_HEADER
 *        q' = q + 46 + n + m + k (the name, extra and comment lengths at q + 28, q + 30, q + 32); q' > p: stop with HDLZ_E_BAD_HEADER
 *        entry e is PASSED: its central record starts at q; q = q'
 *      after the last entry q != p: HDLZ_E_BAD_HEADER (all entries passed).  At a stop nentries is the number of entries passed:
 *      the entries in front of the stop stay valid and indexed, as in hdlz_bgzf_index_ws.
 *   3  per passed entry      method (q + 10), flags (q + 8), crc (q + 16), csize (q + 20), usize (q + 24), name_len (q + 28), the disk
 *      start (q + 34) and the local offset L (q + 42) are the central record's.  These checks set the entry's status and do not stop the
 *      walk; the first that applies wins:
 *        flags & 0x41 (encrypted, strong encryption)                 HDLZ_E_BAD_BTYPE
 *        method not 0 (stored) or 8 (deflated)                       HDLZ_E_BAD_BTYPE
 *        csize, usize or L is FFFFFFFF, or the disk start is not 0   HDLZ_E_BAD_HEADER
 *        method == 0 and csize != usize                              HDLZ_E_BAD_HEADER
 *        L + 30 > cd_off, or the bytes at L are not 50 4B 03 04      HDLZ_E_BAD_HEADER
 *        payload_off = L + 30 + the LOCAL header's own name and extra lengths (L + 26, L + 28)
 *        payload_off + csize > cd_off                                HDLZ_E_BAD_HEADER
 *      No other local field is compared.  payload_off is 0 when the status is not HDLZ_OK.
 *   4  offsets               out_off[0] = 0; out_off[e + 1] = out_off[e] + s_e rounded up to a multiple of out_align, where s_e is
 *      usize for an entry whose status is HDLZ_OK and 0 for a failed one; total_out = out_off[last] + s_last (0 without entries): the
 *      end of the last slot.  out_align is a power of two from 1 to 256.
 *   5  capacity              nentries > entry_cap: HDLZ_E_OUT_CAPACITY in front of the walk's own status -- the true nentries,
 *      total_out, cd_off and cd_size are still reported and only d_entries[0 .. entry_cap) is written: a call with entry_cap = 0 (and
 *      d_entries NULL) is the sizing call.
 * The record's status is that of step 1, else HDLZ_E_OUT_CAPACITY (step 5), else that of step 2; the statuses of step 3 stand in the
 * entries only.
 *
 * Out of scope: writing ZIP files (hdlz_zip_write.h, the extension of this header, does); ZIP64 (the locator is refused, FFFFFFFF sizes
 * and offsets fail the entry: hdlz_zip64.h, the extension behind hdlz_zip_write.h, reads such files); encryption; methods other than
 * 0 and 8; self-extracting prefixes (offsets count from the file's first byte) and multi-disk archives; the lane and group mappings
 * of the batch decoders; several large entries on the whole-GPU path in one call (the caller makes one call per large entry:
 * Engine.inflate_zip does).
 */
#ifndef HDLZ_ZIP_H
#define HDLZ_ZIP_H
#include "hdlz_gzip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* an entry of at least this many compressed bytes is worth a call of its own (count == 1: the whole-GPU path); below it, entries are
 * read together, a wave each.  (INTEGRATION.md section 4 records where the number comes from.) */
#define HDLZ_ZIP_LARGE_MIN 16384u

typedef struct hdlz_zip_entry {     /* 48 bytes */
    uint64_t cd_off;        /* start of the entry's central record; its name is at cd_off + 46 */
    uint64_t payload_off;   /* first byte of the entry's data; 0 when status != HDLZ_OK */
    uint64_t out_off;       /* where the entry's bytes go in the flat output (see out_align) */
    uint32_t csize, usize, crc;
    uint16_t method, flags, name_len, reserved;   /* reserved: 0 */
    uint32_t status;
} hdlz_zip_entry;

typedef struct hdlz_zip_index_result {
    uint64_t nentries, total_out, cd_off, cd_size;
    uint32_t status, reserved;                    /* reserved: 0 */
} hdlz_zip_index_result;

/*
 * scratch of hdlz_zip_index_ws: 0 for file_len >= 2^32, else
 *     256 + 2 * 262144 = 524544
 * (a 256-byte summary; for each of the at most 65535 entries of a directory the 32-bit offset of its central record and the 32-bit
 * size it counts in the output).  It does not depend on entry_cap: total_out needs every entry, in the sizing call too.
 */
size_t hdlz_zip_index_work_bytes(uint64_t file_len, uint64_t entry_cap);

/*
 * Index a ZIP file on the device: THE INDEX RULE above.  The host reads nothing inside the call.  Four launches: (a) one workgroup
 * finds the end record -- each lane tests positions from the file's end down, 256 a step, and the workgroup takes the largest that
 * fits --; (b) one workgroup walks the directory: it stages the directory through LDS in pieces of 16 KiB with coalesced 16-byte
 * loads and follows the hops there (six bytes a record), writing only the offset of every central record; a piece starts at the record
 * the last one could not hold whole, so a record may straddle any piece boundary or be longer than a piece (46 + 3 * 65535 bytes);
 * (c) a thread per entry parses the 46 bytes, loads the local header's two lengths and makes the checks of step 3; (d) one workgroup
 * scans the sizes for out_off and writes the record.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: d_result NULL, or d_file NULL with file_len > 0;
 * d_entries NULL with entry_cap > 0; file_len >= 2^32; entry_cap >= 2^32; out_align not a power of two in [1, 256]; d_work NULL or
 * work_bytes below the query; d_entries, d_result or d_work not 8-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_entries[0 .. min(nentries, entry_cap)), the record, d_work[0 .. work_bytes).
 * reads:  d_file[0 .. file_len) only -- never a load outside it.  The initial contents of the outputs and of d_work never reach a
 *         result.
 */
int hdlz_zip_index_ws(const uint8_t* d_file, uint64_t file_len, uint64_t entry_cap, uint32_t out_align,
                      hdlz_zip_entry* d_entries,      /* entry_cap records, WRITTEN; NULL allowed with entry_cap = 0 */
                      hdlz_zip_index_result* d_result, void* d_work, size_t work_bytes, void* stream);

/*
 * scratch of hdlz_zip_inflate_ws: 0 for count = 0 or count >= 2^31, else
 *     2 * r256(24 count) + T + D,   r256 = rounded up to 256
 *     T = r256(4 ceil(out_cap / 32768)) and D = r256(hdlz_inflate_work_bytes(1, in_len, out_cap rounded down to 4, 0, 1)) when
 *         count == 1, else both 0
 * (six 32-bit and three 64-bit words per entry; one entry: a CRC word per 32 KiB tile and the share of the batch call's path.)
 */
size_t hdlz_zip_inflate_work_bytes(uint64_t count, uint32_t in_len, uint64_t out_cap);

typedef struct hdlz_zip_inflate_result {
    uint64_t out_len;     /* out_off[first + count - 1] - out_off[first] + the last entry's usize; 0 unless status == HDLZ_OK */
    uint64_t first_bad;   /* lowest index (within this call's range) of an entry that failed; ~0 when OK */
    uint32_t status;      /* HDLZ_OK, or the status of that entry */
    uint32_t reserved;    /* 0 */
} hdlz_zip_inflate_result;

/*
 * Read entries [first, first + count) of an index: entry e decodes to its SLOT d_out + (out_off[e] - out_off[first]), usize bytes, so
 * any sub-range decodes without the rest.  d_entries: the records of hdlz_zip_index_ws -- or of anyone else: every entry is checked
 * again on the device before it is decoded, the first line that applies wins, and a refused entry is not decoded:
 *     the record's status is not HDLZ_OK                                          that status
 *     method not 0 or 8, or method == 0 and csize != usize                        HDLZ_E_BAD_PARAM
 *     payload_off < 30, or payload_off + csize + 4 > file_len                     HDLZ_E_BAD_PARAM
 *     out_off[e] < out_off[first], or the slot ends behind out_cap                HDLZ_E_BAD_PARAM
 *     deflated and csize > 2^28 - 7                                               HDLZ_E_BAD_PARAM
 *     in_len != 0 and: count > 1 and csize > in_len; count == 1, deflated and csize + 6 > in_len      HDLZ_E_BAD_PARAM
 * THE ROUTES, the split of hdlz_gunzip_ws:
 *   count >= 2   deflated entries by the task view of the wave-per-member decoder (k_inflate_dyn<false, true>): the stream of entry e
 *                is d_file[payload_off - 2 .. payload_off + csize + 4) -- the four bytes behind the payload are always inside the file
 *                (a directory stands there) and supply what the end-of-input rules want --, its room usize bytes (at most
 *                2^32 - 512: a larger slot is HDLZ_E_OUT_CAPACITY); stored entries by a copy kernel, a workgroup per entry, at any
 *                alignment; then the CRC-32 of every slot, a workgroup per entry (crc_block, the loop of hdlz_crc32_batch_ws -- the
 *                slots of an aligned index are not neighbours, so the kernel is this call's own).
 *   count == 1   a large entry: the path of hdlz_inflate_batch_ws over the two-word ragged index {payload_off - 2,
 *                payload_off + csize + 4} built on the device, in_len being the bound that path sizes itself from (0: not stated -- the
 *                entry is then decoded by one wave), so a large payload is decoded by the whole GPU; a stored entry is a flat copy
 *                over the whole GPU, its grid sized from out_cap; the CRC-32 by the 32 KiB tile kernels.  That path stores words: it
 *                is taken when d_out is 4-byte aligned and out_cap >= 4 and is given the row d_out[0 .. out_cap rounded down to 4) --
 *                an entry whose usize is larger is HDLZ_E_BAD_PARAM; a single entry at any other d_out takes the route above.
 * THE JUDGEMENT per entry, behind the decoder's own status, the same on both routes: decoded length > usize: HDLZ_E_OUT_CAPACITY (the
 * decoder's own word where usize is its room); decoded length != usize: HDLZ_E_BAD_CHECKSUM; the end of the final block, rounded up to
 * a byte, != payload_off + csize: HDLZ_E_NO_EOF; CRC-32 of the slot != the record's: HDLZ_E_BAD_CHECKSUM.  A stored entry has only
 * the last check.  The record holds the status and the index of the lowest failed entry.
 * d_entry_status (nullable): count words, WRITTEN: every entry's status.  in_len: the caller's bound on the entries' csize (count >= 2:
 * checked only) or on csize + 6 (count == 1: what the one-stream path sizes itself from).
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: d_result NULL; with count > 0 any of d_file,
 * d_entries NULL; d_out NULL with out_cap > 0; first + count >= 2^31; file_len >= 2^32; d_entries or d_result not 8-byte aligned;
 * d_entry_status not 4-byte aligned; d_work not 256-byte aligned; with count > 0, d_work NULL or work_bytes below the query.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_out inside the slots of the entries that passed the checks, never a byte at or behind out_cap (count == 1 on the
 *         one-stream path: inside the row, as hdlz_inflate_batch_ws writes a row -- an entry that decodes to more than usize bytes may
 *         leave bytes behind its slot there); d_entry_status[0 .. count) when given, the record, d_work[0 .. work_bytes).
 * reads:  d_entries[first .. first + count); d_file[0 .. file_len) only -- never a load outside it; of a slot only its usize bytes.
 *         The initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_zip_inflate_ws(const uint8_t* d_file, uint64_t file_len, const hdlz_zip_entry* d_entries, uint64_t first, uint64_t count,
                        uint32_t in_len, uint8_t* d_out, uint64_t out_cap,
                        uint32_t* d_entry_status,     /* nullable */
                        hdlz_zip_inflate_result* d_result, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_ZIP_H */
