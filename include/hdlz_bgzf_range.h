/*
 * hdlz_bgzf_range.h -- extension of hdlz_bgzf.h: random access into a BGZF file.  One call takes a BATCH of ranges of the data, given as
 * uncompressed byte offsets (bgzip -b / -s, bgzf_useek) or as the virtual offsets of a .bai, .tbi or .csi index, resolves them against
 * the member index on the device, decodes exactly the members they touch, judges every one of those by its own trailer and delivers
 * exactly the requested bytes, range after range -- no host work inside the call, so thousands of small regions cost one call and not a
 * round trip each.
 *
 * hdlz_bgzf.h leaves ".gzi index files" out of scope.  This header takes that line up as far as the device goes: the two arrays of
 * hdlz_bgzf_index_ws ARE a .gzi index (every member's compressed and uncompressed offset), and the call below seeks by them; writing and
 * reading the file itself is host work (hdl_deflate_amd/bgzf.py: gzi_dumps, gzi_loads).  Additive: HDLZ_VERSION and every declaration of
 * hdlz.h, hdlz_join.h, hdlz_unjoin.h, hdlz_gzip.h and hdlz_bgzf.h stay as they are, and their conventions hold here too.
 *
 * A VIRTUAL OFFSET is coffset << 16 | uoffset: the file offset of a member's first byte, and a byte position inside that member's data.
 * Virtual offsets fit a signed 64-bit word for files below 2^47 bytes.
 *
 * Out of scope: decoding a member once when several ranges share it (every range decodes the members it touches), an LDS-resident
 * decode for edge members, the lane and group mappings, a stored-block fallback in the writer, reading .bai / .tbi / .csi files, the
 * port adapter.
 */
#ifndef HDLZ_BGZF_RANGE_H
#define HDLZ_BGZF_RANGE_H
#include "hdlz_bgzf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HDLZ_BGZF_RANGE_VIRTUAL 1u   /* begin / end are virtual offsets; else uncompressed byte offsets */

typedef struct hdlz_bgzf_ranges_result {
    uint64_t total_out;   /* sum of the lengths of all ranges; the true value also under HDLZ_E_OUT_CAPACITY (held at 2^64 - 1) */
    uint64_t ntasks;      /* members touched, counted once per range that touches them; true value likewise */
    uint64_t first_bad;   /* lowest index of a range whose status is not OK; ~0 when none */
    uint32_t status;
    uint32_t reserved;    /* 0 */
} hdlz_bgzf_ranges_result;

/*
 * scratch of hdlz_bgzf_read_ranges_ws: 0 for nranges = 0 (and for nranges or task_cap >= 2^31, or flag bits other than bit 0), else
 * with R = nranges and T = task_cap
 *     256 + 4 * r256(8 * (R + 1)) + 3 * r256(4 * R) + 3 * r256(8 * T) + 6 * r256(4 * T) + 131072 * R
 * where r256 rounds up to a multiple of 256: a head; per range two positions, the task base and two edge tasks (64 bits each, the
 * last as two words), first member, status and lowest failed task (32 bits each); per task the member's two file offsets and its
 * destination (64 bits each), room, decoded length, status, end bit, CRC-32 and range (32 bits each); and per range two slots of
 * 65536 bytes.  That is 131072 bytes of slots per range, at most 44 bytes of words per range and 48 per task, and below 6 KiB besides.
 */
size_t hdlz_bgzf_ranges_work_bytes(uint64_t nranges, uint64_t task_cap, uint32_t flags);

/*
 * Read a batch of ranges of the data of a BGZF file.  d_off and d_out_off: the index, nmembers + 1 words each, as hdlz_bgzf_index_ws
 * wrote them (or as a .gzi file gives them, with the 0 in front and the file's last member and total length behind).  d_ranges:
 * 2 * nranges words, (begin, end) of range r at [2r] and [2r + 1].
 * THE CONTRACT is this serial statement; the result equals it for every ascending index.  Let M = nmembers, O[b] = d_out_off[b] and
 * C[b] = d_off[b].  For range r with (x, y) = its two words:
 *   1. Resolve to positions p0, p1 in the coordinates of O.
 *      Plain mode: x > y is HDLZ_E_BAD_PARAM for this range; else p0 = clamp(x, O[0], O[M]) and p1 likewise from y -- reading past
 *      the end is short, not an error.
 *      Virtual mode (HDLZ_BGZF_RANGE_VIRTUAL): each word splits into (c, u) = (v >> 16, v & 0xFFFF); c must equal C[b] for some b in
 *      [0, M]; for b < M, u <= O[b + 1] - O[b] is required -- so (C[b], ISIZE_b) and (C[b + 1], 0) name the same position --, for b = M,
 *      u = 0; then p = O[b] + u.  (A member of 65536 bytes is addressable only up to u = 65535, as in htslib.)  Anything else, or
 *      p0 > p1, is HDLZ_E_BAD_PARAM for this range.
 *      A range with HDLZ_E_BAD_PARAM has length 0 and no tasks.
 *   2. The range's length is p1 - p0.  d_range_off is the exclusive scan of the lengths: d_range_off[0] = 0,
 *      d_range_off[nranges] = total_out, and range r's bytes go to d_out[d_range_off[r] .. d_range_off[r + 1]).  Ranges may overlap,
 *      repeat and come in any order; the output is in range order.
 *   3. Tasks.  p0 == p1: none.  Else lo = the lowest b with O[b + 1] > p0, hi = the lowest b >= lo with O[b] >= p1, or M; the tasks
 *      are members lo .. hi - 1 and ntasks += hi - lo.  Empty members strictly inside the span are tasks and are judged like any
 *      other; the two edge members are never empty.
 *   4. Capacity.  total_out > out_cap or ntasks > task_cap: the record's status is HDLZ_E_OUT_CAPACITY, both true values are reported,
 *      d_range_off is fully written, first_bad is ~0, nothing is decoded and d_out is not written; every d_range_status word of a
 *      range whose step 1 succeeded is HDLZ_E_OUT_CAPACITY.  The caller sizes its buffers and calls again: a call with out_cap = 0 and
 *      task_cap = 0 is the SIZING CALL.
 *   5. Every task passes check 1 of hdlz_bgzf_inflate_ws (the index may come from elsewhere): the member's size in [28, 65536], the
 *      member inside file_len, HEADER, BSIZE + 1, O[b + 1] - O[b] equal to its ISIZE and at most 65536.  It is then decoded WHOLE, one
 *      wave per member, every block type; its CRC-32 is taken over the whole decoded member; and it is judged as in steps 4 and 5 of
 *      hdlz_bgzf_inflate_ws -- also when only a slice of it is delivered, which is what htslib does.
 *   6. A range's status is that of its lowest failing task, or HDLZ_OK.  A failed range leaves the bytes of ITS OWN slot of d_out
 *      unspecified and touches nothing else; all other ranges are delivered byte-exact.  The record's status and first_bad are those of
 *      the lowest failed range; total_out and ntasks are always the true values.
 *   7. nranges = 0 writes d_range_off[0] = 0 and an OK record.
 * With an index that is not ascending the statuses are unspecified, but the extents below still hold: no decoder starts from a word
 * that was not checked, and a member that is neither a range's first nor its last and is not covered whole is HDLZ_E_BAD_PARAM.  Such
 * an index can make the lengths add up to more than 64 bits hold: the sum is held at 2^64 - 1, and that value is HDLZ_E_OUT_CAPACITY
 * whatever out_cap says (d_range_off is then held likewise); and every task's check 1 includes that its range's piece
 * d_range_off[r] .. d_range_off[r + 1] has the range's length and ends at or in front of out_cap, else HDLZ_E_BAD_PARAM.
 *
 * All on the caller's stream, nothing read back: (a) a thread per range: the binary searches and checks of step 1, and of step 3;
 * (b) ONE workgroup scans lengths and task counts, a strip of ceil(nranges / 256) ranges per thread -- linear in nranges on 256
 * threads, which is what limits a call to some 10^6 ranges before the scan shows; (c) a thread per task finds its range (binary
 * search in the scanned counts), checks the member and writes its file span and destination: d_out for a member that is covered
 * whole, else one of the range's two slots; (d) the decode through the task view of the member decoder; (e) CRC-32, a workgroup
 * per task; (f) the judgement per task, the lowest failed task per range; (g) a workgroup per slot copies the slice out of it, 16 bytes
 * a lane, bytewise at both ends; (h) the statuses per range, the lowest failed range, the record.  The grids of (c) .. (f) are sized
 * by task_cap, so a task_cap far above ntasks costs launches of idle threads.
 *
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at): d_result or d_range_off NULL; with nranges > 0 any of d_ranges,
 * d_file, d_off, d_out_off NULL; d_out NULL with out_cap > 0; nranges, nmembers or task_cap >= 2^31; flag bits other than bit 0; d_off,
 * d_out_off, d_ranges, d_range_off or d_result not 8-byte aligned; d_range_status not 4-byte aligned; d_work not 256-byte aligned;
 * d_work NULL or work_bytes below the query when that is not 0.
 * Nothing is allocated; every launch is capturable; the host reads nothing inside the call; only this form exists.
 * writes: d_out[0 .. min(total_out, out_cap)) -- never a byte at or behind out_cap --, d_range_off[0 .. nranges],
 *         d_range_status[0 .. nranges) when given, the record, d_work[0 .. work_bytes).
 * reads:  d_off, d_out_off [0 .. nmembers]; d_ranges[0 .. 2 * nranges); d_file[0 .. file_len) only -- never a load outside it.  The
 *         initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_bgzf_read_ranges_ws(const uint8_t* d_file, uint64_t file_len,
                             const uint64_t* d_off, const uint64_t* d_out_off, uint64_t nmembers,   /* the index, nmembers + 1 words each */
                             const uint64_t* d_ranges, uint64_t nranges, uint32_t flags,            /* 2 * nranges words: begin, end */
                             uint8_t* d_out, uint64_t out_cap,
                             uint64_t* d_range_off,        /* nranges + 1 words, WRITTEN */
                             uint32_t* d_range_status,     /* nullable, nranges words, WRITTEN */
                             uint64_t task_cap, hdlz_bgzf_ranges_result* d_result,
                             void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_BGZF_RANGE_H */
