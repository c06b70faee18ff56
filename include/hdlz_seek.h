/*
 * hdlz_seek.h -- random access into ANY gzip or zlib stream.  hdlz_bgzf_range.h, hdlz_unjoin.h and hdlz_zip.h seek in files whose
 * writer planned for it; an ordinary .gz (gzip, pigz, Python, zlib) or one large zlib stream can only be decoded from its first bit.
 * This header adds what zran, indexed_gzip and rapidgzip keep on the host: an index of SEEK POINTS -- a block boundary's bit position
 * and output offset, and the 32 KiB of output in front of it -- that the first full read leaves behind (hdlz_seek_index_ws), and a
 * batched ranged read through it (hdlz_seek_read_ranges_ws) that costs the decode of the segments the ranges touch.
 * Additive: HDLZ_VERSION and every declaration of the other headers stay as they are, and their conventions (device pointers,
 * caller-owned scratch, "writes" / "reads", return values, a result record on the device) hold here too.
 *
 * THE INDEX of a stream with n points is four device arrays:
 *   d_bit[n + 1]   (uint64) the absolute bit position in the file -- 8 * byte + bit, bit 0 the byte's lowest -- of the first header bit
 *                  (BFINAL) of the block at point k; d_bit[n] is the bit behind the last bit of the final block
 *   d_pos[n + 1]   (uint64) the output offset at that boundary; d_pos[0] = 0, d_pos[n] = the length of the data
 *   d_crc[n]       (uint32) the CRC-32 of SEGMENT k, the output bytes [d_pos[k], d_pos[k + 1])
 *   d_win[n][32768]         the h = min(32768, d_pos[k]) output bytes in front of d_pos[k], right-aligned in slot k; the 32768 - h
 *                  bytes in front of them are zero, so an index is deterministic and comparable byte for byte
 * THE POINT RULE.  Let S be a set of true block boundaries (bit, pos) of the stream, in stream order, that contains the first block's
 * header.  Point 0 is the first header.  Another boundary b of S, with predecessor a in S, is a point iff
 *     floor(pos_b / span) > floor(pos_a / span)
 * -- the first known boundary at or behind a multiple of span.  Boundaries that share an output position select only the first of
 * them, so d_pos is strictly ascending, and only the last segment of a stream can be empty.  Each route of the index call states its S;
 * every consumer of an index relies on the rule alone.  (A route that does not know every boundary may select, of several that share
 * a position, one that is not the stream's first there: the blocks in front of it at that position are empty and belong to the
 * segment in front.)
 *
 * Not there: files past the decoders' limits (2^28 bytes compressed, 2^32 - 512 bytes of output; the index is 64-bit throughout so
 * that a later build can lift this); gzip files of several members in one index (the first member is indexed; hdlz_gzip_members.h
 * reads the others); points from the fixed-block chain's end-of-block list (a stream that chain delivers is decoded once more by one
 * wave for its points); several streams per index call (ZIP entries); windows trimmed to the bytes a segment really references, or stored compressed;
 * decoding a segment once when ranges share it; the lane / group mappings and the whole-GPU chains for a segment; importing other
 * tools' index files; the port adapter.
 */
#ifndef HDLZ_SEEK_H
#define HDLZ_SEEK_H
#include "hdlz_bgzf_range.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HDLZ_SEEK_ZLIB 1u         /* RFC 1950: two header bytes, deflate, Adler-32 */
#define HDLZ_SEEK_GZIP 2u         /* RFC 1952: the first member of the file */
#define HDLZ_SEEK_WINDOW 32768u   /* bytes of a slot of d_win */

typedef struct hdlz_seek_result {
    uint64_t npoints;     /* n, the TRUE count -- also when point_cap is too small; 0 for a stream that fails */
    uint64_t total_out;   /* the length of the data; 0 for a stream that fails */
    uint64_t end_bit;     /* d_bit[n]; 0 for a stream that fails */
    uint64_t max_seg;     /* the largest d_pos[k + 1] - d_pos[k]; 0 when the arrays are not written */
    uint32_t status;
    uint32_t route;       /* who filled the points: 1 = the chain route, 2 = the wave route */
} hdlz_seek_result;

/*
 * scratch of hdlz_seek_index_ws: 0 where the call refuses the shape (flags, span = 0, file_len >= 2^28, point_cap >= 2^31), else with
 * P = point_cap, row = min(out_cap rounded DOWN to a multiple of 4, 2^32 - 512) and r256 = rounded up to a multiple of 256
 *     768 + 2 * r256(8 * P) + r256(8 * ceil(row / 32768)) + r256(hdlz_inflate_work_bytes(1, file_len, row, 0, gzip ? 1 : 0))
 * -- a head, the one stream's result words and header walk, the points as the decode records them (two 64-bit words each), the
 * checksum's word per 32 KiB tile of row, and the share of the one-stream decode path (the whole-GPU chains).
 */
size_t hdlz_seek_index_work_bytes(uint64_t file_len, uint32_t flags, uint64_t out_cap, uint64_t point_cap);

/*
 * Decode one stream whole into d_out, judge it, and leave its seek index behind.
 * flags: HDLZ_SEEK_ZLIB or HDLZ_SEEK_GZIP, nothing else.  DECODE AND JUDGEMENT are those of the one-stream calls, unchanged: zlib --
 * hdlz_inflate_checked with one stream of file_len bytes (the two header bytes, the decode, Adler-32, the trailer; its statuses);
 * gzip -- hdlz_gunzip_ws with one stream (the member rule of hdlz_gunzip.h: header walk, decode, CRC-32, ISIZE; the first member
 * only, bytes behind it are no error).  The bytes in d_out and the record's status and total_out are what those calls give, with
 * out_pitch = row (see the scratch formula: the decoder's room is out_cap rounded down to a multiple of 4, as in hdlz_zip_inflate_ws).
 * RFC behaviour only: no obsize, no HDLZ_INFLATE_ASSUME_FIXED.
 * ROUTES.  Two fill the points; which one did is decided on the device from the chains' control words and reported in the record.
 *   1, the chain route: where the whole-GPU chain for any block types delivered the stream (what those calls decode a stream of 4 KiB
 *      and more with, unless it starts with a fixed block), a kernel behind the chains' verdict takes S = the stream's first header and
 *      every header of a dynamic block on the true chain, with the output offsets the chain computed, applies the rule a thread per
 *      block and orders the selected ones.  It costs nothing in the decode kernels.  Stored and fixed blocks behind the first header
 *      are not in this S: a stream of stored blocks alone has one point.
 *   2, the wave route, everything else -- streams below the chains' gate, streams the chains give up on, streams the fixed-block
 *      chain delivered: the recording view of the wave decoder, ONE wave; at every block header, where the header's bit and the output
 *      offset are known, it applies the rule against the previous header and appends; S = every block boundary.  Where the serial
 *      decoder would run anyway (below the gate, after a give-up) the recording instance IS that run; where the fixed-block chain
 *      delivered, the recording instance decodes the stream once more.
 * Behind the judgement: a workgroup per point copies its window out of d_out (16 bytes a lane), and a workgroup per point takes the
 * CRC-32 of its segment.
 * THE RECORD.  status: the judged call's status when that is not HDLZ_OK -- then npoints, total_out, end_bit and max_seg are 0 and none
 * of the four arrays is written.  Else npoints is the true count; npoints > point_cap is HDLZ_E_OUT_CAPACITY: total_out and end_bit
 * are reported, max_seg is 0 and none of the four arrays is written (point_cap = 0 is the SIZING CALL for the points; it still
 * decodes).  Else HDLZ_OK and the arrays are written as stated above.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_result NULL; flags not exactly one of the two; span = 0;
 * file_len >= 2^28; point_cap >= 2^31; d_file NULL with file_len > 0; d_out NULL with out_cap > 0; with point_cap > 0 one of d_bit,
 * d_pos, d_crc, d_win NULL; d_bit, d_pos or d_result not 8-byte aligned; d_crc or d_out not 4-byte aligned; d_win not 16-byte
 * aligned; d_work not 256-byte aligned; d_work NULL or work_bytes below the query.
 * Nothing is allocated; every launch is capturable; the host reads nothing inside the call; only this form exists.
 * writes: d_out[0 .. row) as the judged call writes its row; on HDLZ_OK d_bit, d_pos [0 .. n], d_crc [0 .. n), d_win[0 .. 32768 n) --
 *         never a word at or behind point_cap + 1 (d_bit, d_pos) or point_cap (d_crc, d_win) --; the record; d_work[0 .. work_bytes).
 * reads:  d_file[0 .. file_len) only.  The initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_seek_index_ws(const uint8_t* d_file, uint64_t file_len, uint32_t flags, uint32_t span,
                       uint8_t* d_out, uint64_t out_cap,
                       uint64_t* d_bit, uint64_t* d_pos,     /* point_cap + 1 words each, WRITTEN */
                       uint32_t* d_crc, uint8_t* d_win,      /* point_cap words; point_cap slots of 32768 bytes, WRITTEN */
                       uint64_t point_cap, hdlz_seek_result* d_result,
                       void* d_work, size_t work_bytes, void* stream);

/* the record of a ranged read: the layout and meaning of hdlz_bgzf_ranges_result (a task is a segment touched by a range) */
typedef hdlz_bgzf_ranges_result hdlz_seek_ranges_result;

/*
 * scratch of hdlz_seek_read_ranges_ws: 0 for nranges = 0 (and for nranges or task_cap >= 2^31, flags != 0, seg_cap > 2^32 - 512),
 * else with R = nranges, T = task_cap and slot = r256(seg_cap)
 *     256 + 4 * r256(8 * (R + 1)) + 3 * r256(4 * R) + 3 * r256(8 * T) + 9 * r256(4 * T) + 2 * slot * R
 * -- the scratch of hdlz_bgzf_read_ranges_ws with slots of `slot` bytes, and three more words per task (start bit, history, segment).
 */
size_t hdlz_seek_ranges_work_bytes(uint64_t nranges, uint64_t task_cap, uint64_t seg_cap, uint32_t flags);

/*
 * Read a batch of ranges of the data through a seek index.  The contract is that of hdlz_bgzf_read_ranges_ws in plain (byte offset)
 * mode, with segment k of the index where that call has member b -- steps 1 to 4, 6 and 7 of its serial statement word for word with
 * O = d_pos and M = npoints: d_ranges holds (begin, end) pairs, clamped to [0, d_pos[npoints]] (reading past the end is short, not an
 * error; begin > end is HDLZ_E_BAD_PARAM for that range only); d_range_off is the exclusive scan of the lengths and the output is in
 * range order; ranges may overlap, repeat and come in any order; total_out > out_cap or ntasks > task_cap is HDLZ_E_OUT_CAPACITY with
 * both true values reported and nothing decoded (out_cap = 0 and task_cap = 0: the SIZING CALL).  flags must be 0.
 * A TASK is one segment touched by one range: from lo = the last k with d_pos[k] <= p0 through the segment that holds p1 - 1.  Step 5
 * here, per task with segment k:
 *   a  the index words are checked: d_pos[k] <= d_pos[k + 1]; the expected length d_pos[k + 1] - d_pos[k] <= seg_cap;
 *      d_bit[k] < d_bit[k + 1] <= 8 * file_len; else HDLZ_E_BAD_PARAM for the range.  No decoder starts from an unchecked word.
 *   b  the segment is decoded WHOLE by the segment view of the wave decoder, one wave: from bit d_bit[k] & 7 of byte d_bit[k] >> 3,
 *      o = 0 in its destination -- d_out where the range covers the segment whole, else one of the range's two slots of seg_cap
 *      bytes --, history from slot k of d_win (a distance beyond d_pos[k]'s own min(32768, d_pos[k]) bytes is HDLZ_E_BAD_DISTANCE, as
 *      in the whole-stream decode).  A segment that is not the last stops at the first block header at or behind d_bit[k + 1] --
 *      empty blocks in front of that bit are decoded with the segment --; the last one stops at BFINAL.  The input view of an inner segment ends 8 bytes behind the byte of d_bit[k + 1], or at the file's
 *      end, which keeps a valid segment clear of the decoder's end-of-input rules.  A decoder failure is the task's status; output
 *      beyond the expected length, or any failure with the expected length out, in front of d_bit[k + 1] is HDLZ_E_NO_EOF: the
 *      segment does not end where the index says.
 *   c  the judgement, in this order: decoded length != expected: HDLZ_E_BAD_CHECKSUM; the bit where the decode stopped != d_bit[k + 1]:
 *      HDLZ_E_NO_EOF; CRC-32 of the decoded segment != d_crc[k]: HDLZ_E_BAD_CHECKSUM -- also when only a slice is delivered.
 * seg_cap is normally the index call's max_seg.  A failed range leaves only its own piece of d_out unspecified.
 * One wave decodes a whole segment, so the latency of a range grows with the span the index was built with (profiles/seek.txt).
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_result or d_range_off NULL; with nranges > 0 any of d_ranges,
 * d_file, d_bit, d_pos, d_crc, d_win NULL; d_out NULL with out_cap > 0; nranges, npoints or task_cap >= 2^31; npoints = 0 with
 * nranges > 0; file_len >= 2^28; seg_cap > 2^32 - 512; flags != 0; d_bit, d_pos, d_ranges, d_range_off or d_result not 8-byte
 * aligned; d_crc or d_range_status not 4-byte aligned; d_work not 256-byte aligned; d_work NULL or work_bytes below the query when
 * that is not 0.
 * Nothing is allocated; every launch is capturable; the host reads nothing inside the call; only this form exists.
 * writes: d_out[0 .. min(total_out, out_cap)) -- never a byte at or behind out_cap --, d_range_off[0 .. nranges],
 *         d_range_status[0 .. nranges) when given, the record, d_work[0 .. work_bytes).
 * reads:  d_bit, d_pos [0 .. npoints]; d_crc[0 .. npoints); d_win[0 .. 32768 npoints); d_ranges[0 .. 2 * nranges);
 *         d_file[0 .. file_len) only.  The initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_seek_read_ranges_ws(const uint8_t* d_file, uint64_t file_len,
                             const uint64_t* d_bit, const uint64_t* d_pos, const uint32_t* d_crc, const uint8_t* d_win, uint64_t npoints,
                             const uint64_t* d_ranges, uint64_t nranges, uint32_t flags, uint64_t seg_cap,
                             uint8_t* d_out, uint64_t out_cap,
                             uint64_t* d_range_off,        /* nranges + 1 words, WRITTEN */
                             uint32_t* d_range_status,     /* nullable, nranges words, WRITTEN */
                             uint64_t task_cap, hdlz_seek_ranges_result* d_result,
                             void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_SEEK_H */
