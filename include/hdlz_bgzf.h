/*
 * hdlz_bgzf.h -- extension of hdlz_gzip.h: BGZF, the self-indexing blocked gzip of htslib, bgzip, BAM and tabix, written and read on
 * the device.
 *
 * The joined streams of hdlz_join.h and hdlz_gzip.h are read back in parallel only by a caller that still holds the member index the
 * join wrote, the block size and the length of the data: the stream itself says none of it.  A BGZF file is a series of gzip members
 * of at most 64 KiB, each with its own compressed size in the header and its own CRC-32 and length in the trailer: the file is its own
 * index, any range of members decodes without the rest, and gzip -d, Python's gzip, bgzip -d and every htslib tool read it.  This
 * header takes up two lines that hdlz_gzip.h leaves out of scope: "files of several gzip members" (of this one kind) and "the CRC-32
 * of a pitched or gapped batch" (hdlz_crc32_batch_ws: one word per block).  Additive: HDLZ_VERSION and every declaration of hdlz.h,
 * hdlz_join.h, hdlz_unjoin.h and hdlz_gzip.h stay as they are; the conventions of hdlz.h (device pointers, ownership, extents,
 * "writes" / "reads", return values) hold here too.
 *
 * THE FORMAT.  A member of `size` bytes is
 *   1F 8B 08 04 | MTIME(4) | XFL | OS | 06 00 | 42 43 02 00 | BSIZE(2, LE) | deflate data | CRC-32(4, LE) | ISIZE(4, LE)
 * with size = BSIZE + 1, size - 26 bytes of deflate data and ISIZE <= 65536.  A HEADER here is these 18 bytes: XLEN = 6, the BC
 * subfield and nothing else -- what bgzip, htslib and this writer make; MTIME, XFL and OS may be anything.  Any other header is
 * HDLZ_E_BAD_HEADER.  The writer emits MTIME = 0, XFL = 0, OS = FF and closes the file with the standard 28-byte EOF member
 *   1F 8B 08 04 00 00 00 00 00 FF 06 00 42 43 02 00 1B 00 03 00 00 00 00 00 00 00 00 00
 * Out of scope: .gzi index files, headers with other extra subfields, a stored-block fallback for incompressible blocks (taken up by
 * hdlz_bgzf_stored.h), the lane and group mappings in the reader, the whole-GPU chains, the port adapter.
 */
#ifndef HDLZ_BGZF_H
#define HDLZ_BGZF_H
#include "hdlz_gzip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * CRC-32 (as zlib computes it) of every block of a batch -> d_crc[b], one workgroup per block.  Block b is
 * d_data[d_off[b] - d_off[0] .. d_off[b + 1] - d_off[0]) when d_off (nblocks + 1 ascending words) is given, else the `len` bytes at
 * d_data + b * pitch.  Any alignment; any block length below 2^32; a block of length 0 gives 0.  No scratch.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_crc NULL with nblocks > 0; d_data NULL with nblocks > 0 (and,
 * without d_off, len > 0); nblocks >= 2^31; d_crc not 4-byte aligned; d_off not 8-byte aligned.
 * Nothing is allocated; the launch is capturable.
 * writes: d_crc[0 .. nblocks).  reads: d_off[0 .. nblocks] when given, and the bytes of the blocks only.
 */
int hdlz_crc32_batch_ws(const uint8_t* d_data, const uint64_t* d_off, uint64_t pitch, uint32_t len,
                        uint64_t nblocks, uint32_t* d_crc, void* stream);

/*
 * bytes that hold the BGZF file of nblocks blocks of at most in_len bytes: 28 + nblocks * (hdlz_out_bound(in_len) + 20).
 * (A member is its row without the six bytes of the zlib frame, with 18 bytes in front and 8 behind.)  A block of at most
 * 58230 input bytes always fits a member: 6 + ((9 n + 17) >> 3) <= 65516.
 */
size_t hdlz_bgzf_bound(uint64_t nblocks, uint32_t in_len);

/* scratch of hdlz_bgzf_join_ws: the same as hdlz_join_work_bytes(nblocks) */
size_t hdlz_bgzf_join_work_bytes(uint64_t nblocks);

typedef struct hdlz_bgzf_join_result {
    uint64_t file_len;    /* length of the file, the EOF member included; 0 when a block failed */
    uint32_t status;      /* HDLZ_OK, HDLZ_E_OUT_CAPACITY or the worst status of a block */
    uint32_t first_bad;   /* lowest index of a block that failed; 0xFFFFFFFF when none did */
} hdlz_bgzf_join_result;

/*
 * The BGZF writer.  d_rows, row_pitch, d_len, d_status: the rows, lengths and statuses exactly as hdlz_compress_batch left them (no end
 * bits: the packed small-block mapping stays usable); d_in_off / in_len: the input lengths, as the compress call was given them, for
 * ISIZE; d_crc[0 .. nblocks): the CRC-32 of every input block, put there earlier on the same stream by hdlz_crc32_batch_ws.
 * Member b is the header with BSIZE = d_len[b] + 19, then row b's bytes [2, d_len[b] - 4) -- its one final fixed block, a complete
 * byte-padded deflate stream; BFINAL stays 1 --, then d_crc[b] and the block's input length n_b.  Behind the last member comes the EOF
 * member; nblocks = 0 writes the EOF member alone.
 * A block fails here with HDLZ_E_OUT_CAPACITY when d_len[b] + 20 > 65536 or n_b > 65536, and with HDLZ_E_BAD_PARAM when d_len[b] < 8
 * or d_len[b] > row_pitch (the length and the pitch contradict each other); a failed block counts as a member of length 0.
 *   d_off       nblocks + 1 words, WRITTEN: d_off[b] = where member b starts (d_off[0] = 0), d_off[nblocks] = where the EOF member
 *               starts; file_len = d_off[nblocks] + 28.
 *   d_result    WRITTEN.  status, in this order of precedence (hdlz_join_result's): the numerically largest status of any failed
 *               block -- then file_len = 0 and the bytes of d_file inside [0, file_cap) are unspecified; HDLZ_E_OUT_CAPACITY when
 *               file_len > file_cap: file_len is still reported, members that would end beyond file_cap are not copied and neither
 *               is the EOF member; otherwise HDLZ_OK.
 *   d_work      at least hdlz_bgzf_join_work_bytes(nblocks) bytes, 8-byte aligned (NULL allowed when that is 0).
 * Two launches behind the zeroing of the scratch: the look-back scan and gather of hdlz_join_batch_ws (its own kernel, in another
 * instance) with header and trailer written in the same pass, then the EOF member and the record.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_file, d_off or d_result NULL; with nblocks > 0 any of d_rows,
 * d_len, d_status, d_crc, d_work NULL; nblocks >= 2^31; work_bytes below the query; d_work, d_off, d_in_off or d_result not 8-byte
 * aligned; d_crc not 4-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_file[0 .. min(file_len, file_cap)) -- never a byte at or behind file_cap --, d_off[0 .. nblocks], the result record,
 *         d_work[0 .. work_bytes).
 * reads:  d_len, d_status, d_crc [0 .. nblocks); d_in_off[0 .. nblocks] when given; of row b only bytes [2, d_len[b] - 4).  The
 *         initial contents of d_file, d_off, d_result and d_work never reach a result.
 */
int hdlz_bgzf_join_ws(const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint32_t* d_status,
                      const uint64_t* d_in_off, uint32_t in_len, uint64_t nblocks, const uint32_t* d_crc,
                      uint8_t* d_file, uint64_t file_cap, uint64_t* d_off, hdlz_bgzf_join_result* d_result,
                      void* d_work, size_t work_bytes, void* stream);

/*
 * scratch of hdlz_bgzf_index_ws: 0 for file_len = 0, else with W = ceil(file_len / 65536) windows
 *     r256(64 + 48 * W)       (a 64-byte summary; per window four 64-bit and four 32-bit words)
 * where r256 rounds up to a multiple of 256.
 */
size_t hdlz_bgzf_index_work_bytes(uint64_t file_len);

typedef struct hdlz_bgzf_index_result {
    uint64_t nmembers;    /* members the walk passed */
    uint64_t total_out;   /* the sum of their ISIZE words */
    uint64_t file_used;   /* where the walk stopped */
    uint32_t status;
    uint32_t eof_marker;  /* 1 iff status == HDLZ_OK and the last member has size 28 and ISIZE 0 */
} hdlz_bgzf_index_result;

/*
 * Find the members of a BGZF file on the device.  THE CONTRACT is this serial walk; the result equals it for every file.  Start with
 * p = 0, b = 0, o = 0 and loop:
 *   1. p == file_len: stop with HDLZ_OK.
 *   2. file_len - p < 18: stop with HDLZ_E_NO_EOF.
 *   3. the 18 bytes at p are not a HEADER, or size < 28: stop with HDLZ_E_BAD_HEADER.
 *   4. p + size > file_len: stop with HDLZ_E_NO_EOF.
 *   5. the ISIZE at p + size - 4 is above 65536: stop with HDLZ_E_BAD_HEADER.
 *   6. d_off[b] = p, d_out_off[b] = o; p += size, o += ISIZE, b += 1.
 * At the stop nmembers = b, total_out = o, file_used = p, d_off[b] = p and d_out_off[b] = o: the members in front of a failure stay
 * valid and indexed.  A missing EOF marker is no error (eof_marker = 0).  When b > member_cap the status is HDLZ_E_OUT_CAPACITY --
 * nmembers, total_out and file_used are still the true values, so the caller can call again -- and only the words [0 .. member_cap]
 * of the two arrays are written.  file_len = 0 gives HDLZ_OK with no member.  The host reads nothing inside the call.
 * Three launches: (a) a workgroup per 64 KiB WINDOW of the file reads it once, finds the window's first header-shaped 16 bytes (a
 * window of a well-formed file holds a member start, size <= 65536; a header may straddle into the next window's first 17 bytes),
 * takes it for a true start, hops to the window's end and records (entry, exit, count, ISIZE sum); (b) one wave checks
 * exit[w] == entry[w + 1], 64 seams a step, re-walks a window whose guess was wrong (a look-alike header inside a stored block's
 * payload in front of the true start) from the true entry, finds the stop and scans the counts; (c) a thread per window re-walks
 * it and writes the two arrays.  Only files with look-alike headers in front of a window's true start pay a serial part.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_off, d_out_off or d_result NULL; d_file NULL with
 * file_len > 0; d_work NULL or work_bytes below the query when that is not 0; member_cap >= 2^40; d_off, d_out_off, d_result or d_work
 * not 8-byte aligned.
 * Nothing is allocated; every launch is capturable.
 * writes: d_off and d_out_off [0 .. min(nmembers, member_cap)], the record, d_work[0 .. work_bytes).
 * reads:  d_file[0 .. file_len) only.  The initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_bgzf_index_ws(const uint8_t* d_file, uint64_t file_len, uint64_t member_cap,
                       uint64_t* d_off, uint64_t* d_out_off,   /* member_cap + 1 words each, WRITTEN */
                       hdlz_bgzf_index_result* d_result, void* d_work, size_t work_bytes, void* stream);

/*
 * scratch of hdlz_bgzf_inflate_ws: 0 for nmembers = 0 or nmembers >= 2^31, else
 *     r256(12 * nmembers) + r256(16 * (nmembers + 1)) + r256(4 * nmembers)
 * (length, status and end bit per member; the decoder's private offsets; one CRC word per member).  flags must be 0.
 */
size_t hdlz_bgzf_inflate_work_bytes(uint64_t nmembers, uint32_t flags);

typedef struct hdlz_bgzf_inflate_result {
    uint64_t out_len;     /* d_out_off[nmembers] - d_out_off[0]; 0 unless status == HDLZ_OK */
    uint64_t first_bad;   /* lowest index (within this call's range) of a member that failed; ~0 when OK */
    uint32_t status;
    uint32_t reserved;    /* 0 */
} hdlz_bgzf_inflate_result;

/*
 * Read members of a BGZF file, every member judged by its own trailer.  d_off and d_out_off: nmembers + 1 words each, as
 * hdlz_bgzf_index_ws wrote them -- or ANY SUB-RANGE of them: member b is d_file[d_off[b] .. d_off[b + 1]) and decodes to
 * d_out + (d_out_off[b] - d_out_off[0]), so a range of members decodes without the rest (pass d_off + b0, d_out_off + b0, b1 - b0).
 * All on the caller's stream, nothing read back:
 *   1. index checks per member (the index may come from elsewhere): HDLZ_E_BAD_PARAM when d_off[b + 1] - d_off[b] is not in
 *      [28, 65536] or the member does not lie inside file_len; HDLZ_E_BAD_HEADER when the 18 bytes at d_off[b] are not a HEADER;
 *      HDLZ_E_BAD_PARAM when d_off[b + 1] - d_off[b] != BSIZE + 1, when the slot's length is not the member's ISIZE or is above 65536,
 *      or when the slot ends behind out_cap.  Such a member is not decoded.
 *   2. the decode: one wave per member, every block type (stored, fixed, dynamic: files of bgzip and htslib), BFINAL honoured,
 *      bytewise stores: slots need no alignment.  The decoder's stream ends at the member's trailer: it never runs into the next
 *      header or past the file.  flags must be 0: the lane and group mappings are out of scope and the mapping hints are
 *      HDLZ_E_BAD_PARAM here.
 *   3. the CRC-32 of every output slot (the kernel of hdlz_crc32_batch_ws).
 *   4. the judgement per member, behind the decoder's own status: decoded length != ISIZE: HDLZ_E_BAD_CHECKSUM; the end of the final
 *      block, rounded up to a byte, is not the trailer's first byte: HDLZ_E_NO_EOF; CRC-32 != the trailer's: HDLZ_E_BAD_CHECKSUM.
 *   5. the record: status and first_bad of the lowest failed member.
 * d_member_status (nullable): nmembers words, WRITTEN: every member's status.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_result NULL; with nmembers > 0 any of d_file, d_off, d_out_off,
 * d_work NULL; d_out NULL with out_cap > 0; nmembers >= 2^31; flags != 0; work_bytes below the query; d_off, d_out_off or d_result not
 * 8-byte aligned; d_work not 256-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_out[0 .. out_cap) inside the slots of members that passed check 1 -- never a byte at or behind out_cap --,
 *         d_member_status[0 .. nmembers) when given, the record, d_work[0 .. work_bytes).
 * reads:  d_off, d_out_off [0 .. nmembers]; d_file[0 .. file_len) only -- never a load outside it.  The initial contents of the
 *         outputs and of d_work never reach a result.
 */
int hdlz_bgzf_inflate_ws(const uint8_t* d_file, uint64_t file_len, const uint64_t* d_off, const uint64_t* d_out_off,
                         uint64_t nmembers, uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                         uint32_t* d_member_status,      /* nullable */
                         hdlz_bgzf_inflate_result* d_result, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_BGZF_H */
