// hdlz_device.h -- shared declarations of the HIP side of libhdlz.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>
#include "../../include/hdlz_bgzf_range.h"   // (includes hdlz_bgzf.h, hdlz_gzip.h, hdlz_unjoin.h, hdlz_join.h and hdlz.h)
#include "../../include/hdlz_bgzf_stored.h"
#include "../../include/hdlz_gunzip.h"
#include "../../include/hdlz_gzip_members.h"
#include "../../include/hdlz_zip.h"
#include "../../include/hdlz_zip_write.h"
#include "../../include/hdlz_zip64.h"
#include "../../include/hdlz_seek.h"
#include "../../include/hdlz_png.h"
#include "../../include/hdlz_png_write.h"
#include "../../include/hdlz_tiff.h"

namespace hdlz {

struct CompressArgs {
    const uint8_t* in;
    const uint64_t* in_off;   // nullable: then fixed pitch / length
    uint64_t in_pitch;
    uint32_t in_len;
    uint64_t nblocks;
    int cwindow;
    int maxmatch;
    uint8_t* out;
    uint64_t out_pitch;
    uint32_t* out_len;
    uint32_t* status;
    uint64_t* end_bits = nullptr;  // nullable (hdlz_compress_batch_bits): per block, the bit index -- from the row's first bit -- of the first bit of the
                                   // end-of-block code; 0 for a block that fails.  Moves with out_len / status.  k_compress only: a call that asks
                                   // for it never takes k_compress_small.
};

// The POINT SINK of hdlz_seek_index_ws (include/hdlz_seek.h): where the recording view of k_inflate_dyn leaves the seek
// points of the ONE stream it decodes.  bit == nullptr: no sink, which is what every other caller passes.
struct PointSink {
    uint64_t* head = nullptr;    // [0] the count of points, true also past cap; [1] the absolute bit behind the final block's last bit;
                                 // [2] zeroed by the entry point; 1: the chain route filled the sink (k_any_points), the wave has nothing to do
    uint64_t* bit = nullptr;     // cap words: the absolute bit of the header in front of point k (8 * the stream's first byte + its own bit)
    uint64_t* pos = nullptr;     // cap words: the output offset there
    uint32_t cap = 0;
    uint32_t span = 1;
};

struct InflateArgs {
    const uint8_t* in;
    const uint64_t* in_off;
    uint64_t in_pitch;
    uint32_t in_len;
    uint64_t nstreams;
    uint32_t flags;
    uint32_t obsize;
    uint8_t* out;
    uint64_t out_pitch;
    uint32_t* out_len;
    uint32_t* status;
    uint32_t* in_used = nullptr;   // nullable (hdlz_inflate_checked): per stream, the index of the first byte behind the last bit of the final
                                   // block, counted from the stream's first byte; 0 for a stream whose decode fails.  Moves with out_len / status.
    PointSink sink{};              // hdlz_seek_index_ws only (k_inflate_dyn's recording view); no other kernel looks at it
};

// The MEMBER VIEW of the batch decoders (hdlz_unjoin_ws): stream b is member b of a joined stream, its output slot a
// piece of one flat buffer.  The <..., MEMBERS = true> twins of k_inflate_tok, k_inflate_grp and k_inflate_dyn take this record in place
// of InflateArgs; of the base they use in, out, nstreams, flags (HDLZ_INFLATE_ONEBLOCK: BFINAL is not read), obsize and the three
// result arrays -- status[b] is READ first: a member the index checks refused (status != HDLZ_OK) is not touched --, and in_used[b]
// receives the END BIT, the bit behind the end-of-block code counted from byte m_off[b] - 2, instead of a rounded byte.
struct MemberArgs : InflateArgs {
    const uint64_t* m_off;       // nmembers + 1 words: member b is in[m_off[b] .. m_off[b + 1])
    const uint64_t* m_out_off;   // nullable: then member b decodes to out + b * m_out_len, m_out_len bytes
    uint32_t m_out_len;
    uint64_t m_out_cap;          // no store at or behind out + m_out_cap
    uint32_t m_gap = 0;          // bytes at the end of [m_off[b], m_off[b + 1]) that are NOT the member's: 0 for a joined stream; 18 for BGZF
                                 // (hdlz_bgzf_inflate_ws: m_off[b] = the member's start + 18, so the gap is the next member's header)
    // The TASK VIEW (hdlz_bgzf_read_ranges_ws): the members of a launch are not neighbours, and each has a destination
    // of its own.  All three are null for every other caller, which the view then leaves exactly as it was.
    const uint64_t* m_end = nullptr;      // nullable: member b is in[m_off[b] .. m_end[b]) -- m_off[b + 1] is not read
    uint8_t* const* m_dst = nullptr;      // nullable, k_inflate_dyn<false, true> only: member b decodes to m_dst[b], m_dst_cap[b] bytes of room;
    const uint32_t* m_dst_cap = nullptr;  //   out, m_out_off, m_out_len and m_out_cap are not used then.  The launchers of the other two
                                          //   twins refuse a record with m_dst set (hipErrorInvalidValue): they would decode to out + 0
};
// The SEGMENT VIEW of k_inflate_dyn (hdlz_seek_read_ranges_ws): task t is one segment of a seek index -- the blocks
// between two seek points.  It starts at bit (t_sbit[t] & 7) of byte t_off[t], its input ends in front of byte t_end[t], it decodes to
// t_dst[t] with exactly t_cap[t] bytes of room, and the t_hist[t] bytes of history in front of it are the last ones of the 32 KiB
// window win + 32768 * t_k[t].  Bit 31 of t_sbit: the stream's last segment, which ends at BFINAL; every other one stops at the first
// block header at or behind bit[t_k[t] + 1], the next point's.  Of the base: in, nstreams (the task slots), out_len, status (READ first, as in the member view)
// and in_used, which receives the absolute bit in the file where the task stopped.
struct SegArgs : InflateArgs {
    const uint64_t* t_off;
    const uint64_t* t_end;
    uint8_t* const* t_dst;
    const uint32_t* t_cap;
    const uint32_t* t_sbit;
    const uint32_t* t_hist;
    const uint32_t* t_k;
    const uint8_t* win;
    const uint64_t* bit;         // the index's d_bit
};
// the stream a decoder sees is in[m_off[b] - 2 .. m_off[b + 1]): it skips two bytes unvalidated (never loaded: the FF FF of the marker in
// front, or 78 9C; BGZF: the BSIZE field), and the member's own marker (BGZF: its 8-byte trailer) supplies the bytes the end-of-input
// rules want behind the end-of-block code
__device__ __forceinline__ void member_view(const MemberArgs& a, uint64_t b, uint64_t& off, uint32_t& zn, uint64_t& o, uint32_t& cap) {
    const uint64_t lo = a.m_off[b];
    off = lo - 2u;
    zn = (uint32_t)((a.m_end ? a.m_end[b] : a.m_off[b + 1]) - lo) + 2u - a.m_gap;
    if (a.m_dst) { o = 0; cap = a.m_dst_cap[b]; return; }     // (the task view: the caller takes m_dst[b]; its checks hold cap <= 65536)
    uint64_t n;
    if (a.m_out_off) { o = a.m_out_off[b]; n = a.m_out_off[b + 1] - o; }
    else { o = b * (uint64_t)a.m_out_len; n = a.m_out_len; }
    const uint64_t room = a.m_out_cap - o;                    // (the index checks: o + n <= m_out_cap)
    n = n < room ? n : room;
    cap = n > 0xFFFFFE00ull ? 0xFFFFFE00u : (uint32_t)n;     // o + 258 never wraps
}

__host__ __device__ inline uint32_t out_bound(uint32_t n) {
    return 6u + (uint32_t)((9ull * n + 10ull + 7ull) >> 3);
}
// scratch is handed out in pieces of 256 bytes
constexpr size_t round256(size_t x) { return (x + 255u) & ~(size_t)255u; }

// 16 bytes as four words: v4 at a multiple of 16, v4u at any address
typedef uint32_t v4 __attribute__((ext_vector_type(4)));
typedef v4 __attribute__((aligned(1))) v4u;

// wave64 ballot straight from the compare.  (HIP's __ballot(int) takes the predicate through a 0/1 VGPR: v_cndmask + v_cmp_ne per
// call -- 19 such pairs in a round of k_inflate_tok.)
__device__ __forceinline__ uint64_t ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// LDS-DMA: every active lane's 16 bytes at gptr (any alignment) go to LDS byte address lds_base + 16 * lane, no VGPR in between
// (global_load_lds_dwordx4, M0 = the wave-uniform LDS base; semantics checked by tools/ubench/lds_dma.hip).  The request is a VMEM
// load: it retires in order with the wave's other loads and stores, and only an s_waitcnt vmcnt covers it.
__device__ __forceinline__ void lds_dma16(const uint8_t* gptr, uint32_t lds_base) {
    uint32_t save;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(save) : "v"(gptr), "s"(lds_base) : "memory");
}
// ordering point between the LDS accesses of ONE wave (single-wave workgroups): the LDS executes a wave's instructions in order, so
// all it takes is that the compiler keeps them in order.  (__syncthreads() also waits vmcnt(0) -- for output stores issued a moment ago.)
__device__ __forceinline__ void wave_lds_order() { asm volatile("" ::: "memory"); }

// compile-time counted loop: body(std::integral_constant<int, I>{}) for I in [B, E)
template <int B, int E, class F>
__host__ __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

hipError_t launch_compress(const CompressArgs& a, hipStream_t stream);
hipError_t launch_compress_small(const CompressArgs& a, hipStream_t stream, int ncu);
// The scratch of ONE call.  caller == true (the hdlz_*_ws entry points): [base, base + bytes) is the caller's device buffer and
// nothing is allocated -- a request that does not fit FAILS and the call takes a path that needs less (same results).  caller == false
// (the entry points without d_work): requests go to the library's stream-ordered pool (scratch_alloc / hipFreeAsync).
struct Work {
    uint8_t* base;
    size_t bytes;
    bool caller;
    hipError_t get(size_t need, hipStream_t stream, uint8_t** p) const;
    hipError_t put(uint8_t* p, hipStream_t stream) const;
};
size_t inflate_tok_work_bytes(uint64_t nstreams, bool ragged);              // pass 1's ordered list / pass 2's lists (max of the two)
size_t inflate_par_work_bytes(uint32_t in_len, uint64_t nstreams, uint64_t out_pitch, uint32_t flags);    // all streams at once (0: the path does not apply)
size_t archive_work_bytes(uint64_t nblocks);
hipError_t launch_inflate_tok(const InflateArgs& a, hipStream_t stream, const Work& w);
hipError_t launch_inflate_grp(const InflateArgs& a, hipStream_t stream);
hipError_t launch_inflate_tok_dyn(const InflateArgs& a, hipStream_t stream, bool all, const Work& w);
hipError_t launch_inflate_par(const InflateArgs& a, hipStream_t stream, bool* used, const Work& w);
hipError_t launch_inflate_dyn(const InflateArgs& a, hipStream_t stream, bool all, const uint32_t* few_n = nullptr, uint32_t lane_min = 0);
hipError_t launch_inflate_dyn_flagged(const InflateArgs& a, hipStream_t stream);
hipError_t launch_inflate_dyn_record(const InflateArgs& a, hipStream_t stream, const uint32_t* done = nullptr);   // ONE stream, a.sink set: the recording view
hipError_t launch_inflate_dyn_segments(const SegArgs& a, hipStream_t stream);        // the segment view, a wave per task
// the judging pass of hdlz_inflate_checked (hdlz_checksum.hip): behind a decode that stored in_used, on the same stream
struct JudgeArgs {
    const uint8_t* in;
    const uint64_t* in_off;     // nullable, as in InflateArgs
    uint64_t in_pitch;
    uint32_t in_len;
    uint64_t nstreams;
    const uint8_t* out;
    uint64_t out_pitch;
    uint32_t* out_len;          // read; set to 0 for a stream that fails the judgement
    uint32_t* status;           // read; the verdict
    uint32_t* in_used;          // read: the decoder's end position; written: end + 4, or 0
    uint32_t* adler;            // nullable
    uint2* work;                // judge_work_bytes(nstreams, out_pitch) bytes (per-tile sums; null when that is 0)
};
// hdlz_unjoin_ws: the member twins of the three batch mappings (a.in_off is not used: the lane mapping orders its lists by a.m_off)
hipError_t launch_inflate_tok_members(const MemberArgs& a, hipStream_t stream, const Work& w);
hipError_t launch_inflate_grp_members(const MemberArgs& a, hipStream_t stream);
hipError_t launch_inflate_dyn_members(const MemberArgs& a, hipStream_t stream);
// hdlz_unjoin.hip: the index checks in front of the decode, the checksum tiles, the judgement and the record behind it
struct UnjoinArgs {
    const uint8_t* in;
    uint64_t in_len;
    const uint64_t* off;
    const uint64_t* out_off;     // nullable
    uint32_t out_len;
    uint64_t nmembers;
    uint8_t* out;
    uint64_t out_cap;
    uint32_t* member_status;     // nullable
    hdlz_unjoin_result* result;
    uint32_t* len;               // scratch, per member: the decoded length; behind the judgement word 256 g holds workgroup g's lowest failed member
    uint32_t* status;            // ... the status: written by the index checks, then by the decode, then by the judgement
    uint32_t* end_bit;           // ... the end bit
    uint2* tiles;                // scratch: (A, C) per 32 KiB tile of out[0 .. out_cap)
};
hipError_t launch_unjoin_index(const UnjoinArgs& a, hipStream_t stream);
hipError_t launch_unjoin_judge(const UnjoinArgs& a, hipStream_t stream);
size_t unjoin_tiles(uint64_t total_out);
// ... and the gzip form's twin of launch_unjoin_judge (hdlz_unjoin_gzip_ws): a.tiles holds ONE word per 32 KiB tile, a.result is a
// hdlz_unjoin_gzip_result (the same layout)
hipError_t launch_unjoin_gzip_judge(const UnjoinArgs& a, hipStream_t stream);
size_t judge_work_bytes(uint64_t nstreams, uint64_t out_pitch);
hipError_t launch_judge(const JudgeArgs& a, hipStream_t stream);
size_t stream_work_bytes(uint32_t n, uint32_t nblocks);
hipError_t launch_compress_streams(const uint8_t* in, uint64_t in_pitch, uint32_t n, uint32_t nblocks, int cwindow, int maxmatch,
                                   uint8_t* out, uint64_t out_pitch, uint32_t* out_len, uint32_t* status, void* work,
                                   hipStream_t stream);
typedef hdlz_cstate ChunkState;     // resumable compress session (include/hdlz.h)
hipError_t launch_compress_chunk(const uint8_t* in, uint32_t n, uint32_t q_end, int final_, int cwindow, int maxmatch, uint8_t* out,
                                 uint64_t out_cap, void* state, hipStream_t stream);
hipError_t launch_inflate_chunk(const uint8_t* in, uint32_t in_len, int final_, uint32_t flags, uint32_t obsize, uint8_t* out,
                                uint64_t out_cap, uint32_t out_limit, void* state, hipStream_t stream);
// stream-ordered scratch memory from the library's OWN per-device memory pool (release threshold 256 MiB -- with the default
// pool's threshold of 0 every call paid a fresh device allocation: 10..40 ms for the 8 MB of a 1 MiB single-stream inflate; with
// "keep everything" one large single-stream inflate held gigabytes of HBM for the life of the process)
hipError_t scratch_alloc(void** p, size_t bytes, hipStream_t stream);
hipError_t scratch_release();          // give the cached scratch of the current device back (hdlz_release_scratch)
// p[0 .. n) = 0 by a kernel.  (Not hipMemsetAsync: captured into a HIP graph, a memset node on memory that a mem-alloc node of the
// same graph hands out was seen to leave the words unchanged on ROCm 7.2 -- the device-side counters then started from garbage.)
hipError_t zero_words(uint32_t* p, uint32_t n, hipStream_t stream);

hipError_t launch_compact(const uint8_t* rows, uint64_t pitch, const uint32_t* len, const uint64_t* off,
                          uint64_t nblocks, uint8_t* archive, hipStream_t stream);

hipError_t launch_archive(const uint8_t* rows, uint64_t pitch, const uint32_t* len, uint64_t nblocks, uint8_t* archive, uint64_t cap,
                          uint64_t* off, hipStream_t stream, const Work& w);

// The tile joins (hdlz_join.hip, hdlz_bgzf_stored.hip; hdlz_frame.h has their shared steps).  `work`: join_work_bytes(nblocks) bytes
// (null when that is 0), carved into a JoinWork by the launcher; the entry point fills in the rest of the record.
struct JoinWork {
    uint32_t* ticket;            // ticket (+ pad), ...
    unsigned long long* desc;    // ... one look-back word per tile, ...
    uint32_t* part;              // ... PARTS words per tile
};
size_t join_work_bytes(uint64_t nblocks);
// the rows of hdlz_compress_batch_bits -> one zlib stream (hdlz_join_batch_ws) or one gzip member (hdlz_join_gzip_ws)
struct JoinArgs {
    const uint8_t* rows;
    uint64_t pitch;
    const uint32_t* len;
    const uint64_t* end_bits;
    const uint32_t* status;
    const uint64_t* in_off;      // nullable: then every block has in_len bytes
    uint32_t in_len;
    uint64_t nblocks;
    uint8_t* stream;
    uint64_t cap;
    uint64_t* off;
    hdlz_join_result* result;    // the zlib form's record (the gzip form has its own)
    JoinWork w;
};
hipError_t launch_join(JoinArgs a, void* work, hipStream_t stream);
// `crc`: the device word that holds the CRC-32 of the input; a.stream / a.cap: the whole gzip stream
hipError_t launch_join_gzip(JoinArgs a, const uint32_t* crc, hdlz_join_gzip_result* result, void* work, hipStream_t stream);
// the rows of hdlz_compress_batch -> a BGZF file: every member the row's fixed block (hdlz_bgzf_join_ws), or fixed or stored, whichever
// is shorter (hdlz_bgzf_join_stored_ws: `in` ... as the compress call was given them, `kind`)
struct BgzfJoinArgs {
    const uint8_t* in;           // the stored form only
    const uint64_t* in_off;      // nullable: then block b is the in_len bytes at in + b * in_pitch
    uint64_t in_pitch;           // the stored form only
    uint32_t in_len;
    const uint8_t* rows;
    uint64_t pitch;
    const uint32_t* len;
    const uint32_t* status;
    uint64_t nblocks;
    const uint32_t* crc;         // the CRC-32 of every input block
    uint8_t* file;
    uint64_t cap;
    uint64_t* off;
    uint8_t* kind;               // nullable; the stored form only
    JoinWork w;
};
hipError_t launch_bgzf_join(BgzfJoinArgs a, hdlz_bgzf_join_result* result, void* work, hipStream_t stream);
hipError_t launch_bgzf_join_stored(BgzfJoinArgs a, hdlz_bgzf_stored_result* result, void* work, hipStream_t stream);

// hdlz_bgzf.hip: the CRC-32 of every block of a batch (`skip`: nullable, per block: a status that is not HDLZ_OK leaves the block
// unread and its word unwritten), the member index of a BGZF file, and what runs around the member decode of hdlz_bgzf_inflate_ws
hipError_t launch_crc32_batch(const uint8_t* data, const uint64_t* off, uint64_t pitch, uint32_t len, uint64_t nblocks, uint32_t* crc,
                              const uint32_t* skip, hipStream_t stream);
size_t bgzf_index_work_bytes(uint64_t file_len);
hipError_t launch_bgzf_index(const uint8_t* file, uint64_t file_len, uint64_t member_cap, uint64_t* off, uint64_t* out_off,
                             hdlz_bgzf_index_result* result, void* work, hipStream_t stream);
struct BgzfArgs {
    const uint8_t* in;
    uint64_t in_len;
    const uint64_t* off;
    const uint64_t* out_off;
    uint64_t nmembers;
    uint8_t* out;
    uint64_t out_cap;
    uint32_t* member_status;     // nullable
    hdlz_bgzf_inflate_result* result;
    uint32_t* len;               // scratch, per member, as in UnjoinArgs: the decoded length / the workgroup's lowest failed member
    uint32_t* status;
    uint32_t* end_bit;
    uint64_t* m_off;             // scratch, nmembers + 1 words: off[b] + 18 (MemberArgs::m_off with m_gap = 18)
    uint64_t* m_out_off;         // scratch, nmembers + 1 words: out_off[b] - out_off[0]
    uint32_t* crc;               // scratch, per member: the CRC-32 of its slot
};
hipError_t launch_bgzf_check(const BgzfArgs& a, hipStream_t stream);
hipError_t launch_bgzf_judge(const BgzfArgs& a, hipStream_t stream);

// hdlz_bgzf_range.hip: hdlz_bgzf_read_ranges_ws (include/hdlz_bgzf_range.h).  The scratch, in this order -- every piece
// a multiple of 256 bytes; R = nranges, T = task_cap:
//   head      256 bytes: total_out, ntasks, the capacity flag (64 bits each), the lowest failed range (32 bits)
//   per range p0, p1 (8 R each), tbase (8 (R + 1): the task counts, then their exclusive scan), lo, status, first (the lowest failed task,
//             counted inside the range), edge[2] (the tasks that decode into the range's two slots) (4 R each)
//   per task  off (the member's start + 18), end (the member's end), dst (8 T each), cap (its ISIZE), len, status, end_bit, crc,
//             range (4 T each)
//   slots     2 R slots of 65536 bytes: slot 2r holds range r's first member, slot 2r + 1 its last, when only a slice of it is delivered
struct RangeArgs {
    const uint8_t* in;
    uint64_t in_len;
    const uint64_t* off;
    const uint64_t* out_off;
    uint64_t nmembers;
    const uint64_t* ranges;
    uint64_t nranges;
    uint32_t flags;
    uint8_t* out;
    uint64_t out_cap;
    uint64_t* range_off;
    uint32_t* range_status;      // nullable
    uint64_t task_cap;
    hdlz_bgzf_ranges_result* result;
    uint64_t* head;
    uint64_t *r_p0, *r_p1, *r_tbase;
    uint32_t *r_lo, *r_status, *r_first, *r_edge;
    uint64_t *t_off, *t_end;
    uint8_t** t_dst;
    uint32_t *t_cap, *t_len, *t_status, *t_end_bit, *t_crc, *t_range;
    uint8_t* slots;
    uint64_t slot_bytes;         // the size of a slot: 65536 for BGZF; hdlz_seek_read_ranges_ws: its seg_cap, rounded up to 256
};
size_t bgzf_ranges_work_bytes(uint64_t nranges, uint64_t task_cap, uint64_t slot_bytes = 65536u);
RangeArgs bgzf_ranges_args(void* work, uint64_t nranges, uint64_t task_cap, uint64_t slot_bytes = 65536u);   // the pieces of the scratch; the caller fills in the rest
hipError_t launch_bgzf_ranges_plan(const RangeArgs& a, hipStream_t stream);        // resolve, scan, expand and check: in front of the decode
hipError_t launch_bgzf_ranges_finish(const RangeArgs& a, hipStream_t stream);      // CRC words, judgement, edge slices, statuses, the record
// ... and the steps of the two that know nothing of a BGZF member, for hdlz_seek_read_ranges_ws (hdlz_seek.hip has its own expand and judge)
hipError_t launch_ranges_resolve_scan(const RangeArgs& a, hipStream_t stream);     // k_ranges_resolve (plain mode), k_ranges_scan
hipError_t launch_ranges_crc(const RangeArgs& a, hipStream_t stream);              // k_ranges_crc
hipError_t launch_ranges_deliver(const RangeArgs& a, hipStream_t stream);          // k_ranges_slice, k_ranges_finish, k_ranges_record

// hdlz_seek.hip: hdlz_seek_index_ws and hdlz_seek_read_ranges_ws (include/hdlz_seek.h)
struct SeekIndexArgs {
    const uint8_t* out;          // the decoded stream
    const uint32_t* out_len;     // the judged call's words for the ONE stream
    const uint32_t* status;
    PointSink sink;              // as the decoder filled it
    uint64_t* bit;               // the caller's four arrays
    uint64_t* pos;
    uint32_t* crc;
    uint8_t* win;
    uint64_t point_cap;
    hdlz_seek_result* result;
    uint64_t* head;              // scratch, 256 bytes: [0] the points the arrays hold (0 when they are not written)
};
hipError_t launch_seek_index_finish(const SeekIndexArgs& a, hipStream_t stream);    // k_seek_points, k_seek_windows, k_seek_crc
struct SeekRangeArgs {
    RangeArgs r;                 // r.out_off: d_pos; r.nmembers: npoints; r.off is not used
    const uint64_t* bit;
    const uint32_t* crc;
    const uint8_t* win;
    uint64_t seg_cap;
    uint32_t *t_sbit, *t_hist, *t_k;      // scratch, task_cap words each: SegArgs
};
hipError_t launch_seek_expand(const SeekRangeArgs& a, hipStream_t stream);
hipError_t launch_seek_judge(const SeekRangeArgs& a, hipStream_t stream);

// hdlz_crc32.hip: CRC-32 of data[0 .. n) -> crc[0].  `words`: one word per 32 KiB tile (crc32_tiles(n) of them; null when n is 0).
size_t crc32_tiles(uint64_t n);
hipError_t launch_crc32(const uint8_t* data, uint64_t n, uint32_t* crc, uint32_t* words, hipStream_t stream);

// hdlz_gunzip.hip: hdlz_gunzip_ws (include/hdlz_gunzip.h) -- the header walk in front of the decode, the CRC-32 of the
// rows and the verdict behind it.  The input and the five result arrays are the caller's; the rest is scratch.
struct GunzipArgs {
    const uint8_t* in;
    const uint64_t* in_off;     // nullable, as in InflateArgs
    uint64_t in_pitch;
    uint32_t in_len;
    uint64_t nstreams;
    const uint8_t* out;
    uint64_t out_pitch;
    uint32_t* out_len;
    uint32_t* status;
    uint32_t* in_used;
    uint32_t* crc;              // nullable
    uint32_t* p;                // scratch, per stream: the offset of the first payload byte
    uint32_t* verdict;          // ... the header's verdict
    uint32_t* crcw;             // ... the CRC-32 of the row
    uint64_t* idx;              // scratch, 2 nstreams words: MemberArgs::m_off, then m_end; single: the ragged index {start + p - 2, end}
    uint32_t* tiles;            // scratch: gunzip_tile_words(nstreams, out_pitch) words (null when that is 0)
    bool single;                // nstreams == 1: the decode is the batch call's, and in_used holds a byte where the member view stores a bit
};
size_t gunzip_tile_words(uint64_t nstreams, uint64_t out_pitch);
hipError_t launch_gunzip_heads(const GunzipArgs& a, hipStream_t stream);
hipError_t launch_gunzip_crc(const GunzipArgs& a, hipStream_t stream);
hipError_t launch_gunzip_judge(const GunzipArgs& a, hipStream_t stream);

// hdlz_gzip_members.hip: the member index of a plain gzip file and what hdlz_gzip_members_inflate_ws runs around the member decode
// (include/hdlz_gzip_members.h)
size_t gzip_members_index_work_bytes(uint64_t file_len);
hipError_t launch_gzip_members_index(const uint8_t* file, uint64_t file_len, uint64_t member_cap, uint64_t* off, uint64_t* out_off,
                                     hdlz_gzip_members_index_result* result, void* work, hipStream_t stream);
struct GzipMembersArgs {
    const uint8_t* in;
    uint64_t in_len;             // file_len
    const uint64_t* off;
    const uint64_t* out_off;
    uint64_t nmembers;
    uint64_t out_cap;
    uint32_t* member_status;     // nullable
    hdlz_gzip_members_inflate_result* result;
    uint32_t* len;               // scratch, per member, as in BgzfArgs: the decoded length / the workgroup's lowest failed member
    uint32_t* status;            // ... the index checks and the header's verdict, then the decoder's status, then the verdict
    uint32_t* end_bit;
    uint32_t* p;                 // ... the offset of the first payload byte
    uint32_t* crc;               // ... the CRC-32 of the slot
    uint64_t* m_off;             // scratch, per member: MemberArgs::m_off (off[b] + p)
    uint64_t* m_end;             // ... MemberArgs::m_end (off[b + 1])
    uint64_t* m_out_off;         // scratch, nmembers + 1 words: out_off[b] - out_off[0]
};
hipError_t launch_gzip_members_heads(const GzipMembersArgs& a, hipStream_t stream);
hipError_t launch_gzip_members_judge(const GzipMembersArgs& a, hipStream_t stream);

// hdlz_zip.hip: hdlz_zip_index_ws and what hdlz_zip_inflate_ws runs around the decode (include/hdlz_zip.h)
size_t zip_index_work_bytes();
hipError_t launch_zip_index(const uint8_t* file, uint64_t file_len, uint64_t entry_cap, uint32_t out_align, hdlz_zip_entry* entries,
                            hdlz_zip_index_result* result, void* work, hipStream_t stream);
// (Rec: hdlz_zip_entry, or hdlz_zip64_entry for hdlz_zip64_inflate_ws -- the same kernels, instantiated for either record)
template <class Rec> struct ZipArgsT {
    const uint8_t* in;
    uint64_t in_len;                  // file_len
    const Rec* entries;               // the call's d_entries + first
    uint64_t count;
    uint32_t bound;                   // the call's in_len
    uint8_t* out;
    uint64_t out_cap;
    uint32_t* entry_status;           // nullable
    hdlz_zip_inflate_result* result;
    uint32_t* len;                    // scratch, per entry, as in BgzfArgs: the decoded length / the workgroup's lowest failed entry
    uint32_t* status;                 // ... the decoder's status word (a stored entry: FFFFFFFF, left alone), then the verdict
    uint32_t* end_bit;                // ... where the final block ended: a bit (the task view) or, single, a byte
    uint32_t* cap;                    // ... MemberArgs::m_dst_cap
    uint32_t* crc;                    // ... the CRC-32 of the slot
    uint32_t* verdict;                // ... the checks in front of the decode
    uint64_t* m_off;                  // scratch, per entry: MemberArgs::m_off; single: with m_end[0] the ragged index of one stream
    uint64_t* m_end;                  // ... MemberArgs::m_end (the word behind m_off[count - 1])
    uint8_t** m_dst;                  // ... MemberArgs::m_dst
    uint32_t* tiles;                  // scratch, single: one word per 32 KiB tile of out_cap (else null)
    bool single;                      // count == 1 on the batch call's path
};
using ZipArgs = ZipArgsT<hdlz_zip_entry>;
using ZipArgs64 = ZipArgsT<hdlz_zip64_entry>;
hipError_t launch_zip_check(const ZipArgs& a, hipStream_t stream);
hipError_t launch_zip_copy(const ZipArgs& a, hipStream_t stream);
hipError_t launch_zip_crc(const ZipArgs& a, hipStream_t stream);
hipError_t launch_zip_judge(const ZipArgs& a, hipStream_t stream);
hipError_t launch_zip_check(const ZipArgs64& a, hipStream_t stream);
hipError_t launch_zip_copy(const ZipArgs64& a, hipStream_t stream);
hipError_t launch_zip_crc(const ZipArgs64& a, hipStream_t stream);
hipError_t launch_zip_judge(const ZipArgs64& a, hipStream_t stream);

// hdlz_zip.hip again: hdlz_zip64_index_ws (include/hdlz_zip64.h)
size_t zip64_index_work_bytes(uint64_t entry_cap);
hipError_t launch_zip64_index(const uint8_t* file, uint64_t file_len, uint64_t entry_cap, uint32_t out_align, hdlz_zip64_entry* entries,
                              hdlz_zip_index_result* result, void* work, hipStream_t stream);

// hdlz_png.hip: hdlz_png_index_ws and what hdlz_png_decode_ws runs around the decode (include/hdlz_png.h)
size_t png_index_work_bytes(uint64_t n);
hipError_t launch_png_index(const uint8_t* files, uint64_t files_len, const uint64_t* file_off, const uint64_t* file_len, uint64_t n, uint32_t flags,
                            uint32_t out_align, uint64_t image_cap, hdlz_png_image* images, hdlz_png_index_result* result, void* work, hipStream_t stream);
struct PngArgs {
    const uint8_t* in;
    uint64_t in_len;                  // files_len
    const hdlz_png_image* images;     // the call's d_images + first
    uint64_t count;
    uint32_t flags;
    uint64_t list_cap, tile_cap;      // the chunk list's entries (idat_cap + 4 count); the Adler tile words
    uint64_t z_bytes, raw_bytes;
    uint8_t* out;
    uint64_t out_cap;
    uint32_t* image_status;           // nullable
    hdlz_png_decode_result* result;
    uint32_t* len;                    // scratch, per image: the decoded length
    uint32_t* status;                 // ... the decoder's status word (a refused image: the checks' verdict, which the decoder leaves alone)
    uint32_t* end_bit;                // ... where the final block ended: a bit (the task view) or, single, a byte
    uint32_t* cap;                    // ... MemberArgs::m_dst_cap (raw_len)
    uint32_t* verdict;                // ... the checks in front of the decode
    uint32_t* crcbad;                 // ... 1: a chunk's CRC-32 did not match
    uint32_t* fltbad;                 // ... 1: a row's filter byte was above 4
    uint32_t* fin;                    // ... the image's status
    uint64_t* m_off;                  // scratch, per image: MemberArgs::m_off; single: with m_end[0] the ragged index of one stream
    uint64_t* m_end;                  // ... MemberArgs::m_end (the word behind m_off[count - 1])
    uint8_t** m_dst;                  // ... MemberArgs::m_dst
    uint64_t *cbase, *tb, *zb, *sb;   // scratch, count + 1 words each: where an image's chunks, Adler tiles, gather tiles and bands start
    uint64_t* head;                   // scratch, 32 words: the four totals
    uint64_t *c_src, *c_dst;          // scratch, the chunk list: where the chunk's type stands in `in`; an IDAT's place in its zlib stream
    uint32_t *c_len, *c_img;          // ... its data length; NONE: the entry is not used
    uint2* tiles;                     // scratch: (A, C) per 32 KiB tile of the decoded streams
    uint8_t *z, *raw;                 // scratch: the gathered zlib streams, the decoded streams
    bool single;                      // count == 1: the batch call's path
};
hipError_t launch_png_front(const PngArgs& a, hipStream_t stream);     // checks, chunk list, gather, chunk CRCs: in front of the decode
hipError_t launch_png_back(const PngArgs& a, hipStream_t stream);      // Adler tiles, unfilter, expansion, verdicts, the record

// hdlz_tiff.hip: hdlz_tiff_index_ws and what hdlz_tiff_decode_ws runs around the decode (include/hdlz_tiff.h)
size_t tiff_index_work_bytes(uint64_t n);
hipError_t launch_tiff_index(const uint8_t* files, uint64_t files_len, const uint64_t* file_off, const uint64_t* file_len, const uint32_t* pages, uint64_t n,
                             uint32_t out_align, uint64_t image_cap, hdlz_tiff_image* images, hdlz_tiff_index_result* result, void* work, hipStream_t stream);
struct TiffArgs {
    const uint8_t* in;
    uint64_t in_len;                  // files_len
    const hdlz_tiff_image* images;    // the call's d_images + first
    uint64_t count;
    uint64_t chunk_cap, tile_cap;     // the slots of the chunk list; the Adler tile words (raw_bytes / 32768 + chunk_cap)
    uint64_t raw_bytes;
    uint8_t* out;
    uint64_t out_cap;
    uint32_t* image_status;           // nullable
    hdlz_tiff_decode_result* result;
    uint32_t* verdict;                // scratch, per image: the checks in front of the decode
    uint32_t* fin;                    // ... the image's status
    uint64_t *cb, *tb;                // scratch, count + 1 words each: where an image's chunks and Adler tiles start
    uint64_t* head;                   // scratch, 32 words: the two totals
    uint64_t* m_off;                  // scratch, per chunk: MemberArgs::m_off; single: with m_end[0] the ragged index of one stream
    uint64_t* m_end;                  // ... MemberArgs::m_end (the word behind m_off[chunk_cap - 1])
    uint8_t** m_dst;                  // ... MemberArgs::m_dst: the chunk's place among the decoded chunks
    uint32_t* cap;                    // ... MemberArgs::m_dst_cap (the chunk's decoded bytes)
    uint32_t* len;                    // ... the decoded length
    uint32_t* status;                 // ... the decoder's status word (FFFFFFFF: a chunk it is not to touch)
    uint32_t* end_bit;                // ... where the final block ended: a bit (the task view) or, single, a byte
    uint32_t* cst;                    // ... the planner's verdict on the chunk
    uint2* tiles;                     // scratch: (A, C) per 32 KiB tile of the decoded chunks
    uint8_t* raw;                     // scratch: the decoded chunks
    uint32_t bound;                   // single: the bound the batch call's path is given on the stream's length
    bool single;                      // count == 1 and chunk_cap == 1: the batch call's path
};
hipError_t launch_tiff_front(const TiffArgs& a, hipStream_t stream);    // checks, chunk list: in front of the decode
hipError_t launch_tiff_back(const TiffArgs& a, hipStream_t stream);     // Adler tiles, unpredict, verdicts, the record

// hdlz_zip_write.hip: hdlz_zip_write_ws (include/hdlz_zip_write.h).  The scratch, carved by the launcher: E = nentries
struct ZipWriteWork {
    uint32_t* ticket;                 // the scan's ticket (+ pad), ...
    unsigned long long *desc, *desc2; // ... its look-back words per tile: the member lengths; the two counts
    uint64_t *pre, *cnt;              // per row (+ 1): the exclusive prefix of |M_b|; of the failed rows (bits 0 .. 30) and the contradictory ones
    uint64_t* head;                   // the summary: is the file written, the tiles of the stored copy, did an entry fail
    uint64_t *pay, *cdrec, *out_off;  // per entry: payload_off, where its central record starts, out_off
    uint32_t *csize, *form, *tile0;   // per entry: c_e; method | status << 8; (E + 1 words) the first tile of the stored copy
    uint64_t* csize64;                // hdlz_zip64_write_ws: c_e in 64 bits, in the piece of csize (then twice as large)
};
struct ZipWriteArgs {
    const uint8_t* in;
    const uint64_t* ent_off;
    const uint8_t* names;
    const uint64_t* name_off;
    uint64_t nentries;
    const uint64_t* in_off;
    const uint8_t* rows;
    uint64_t pitch;
    const uint32_t* len;
    const uint64_t* end_bits;
    const uint32_t* status;
    uint64_t nblocks;
    const uint64_t* blk_first;
    const uint32_t* crc;
    uint32_t flags, datetime, out_align;
    uint64_t total_in;
    uint8_t* file;
    uint64_t cap;
    hdlz_zip_entry* entries;          // nullable
    hdlz_zip_write_result* result;
    ZipWriteWork w;
    hdlz_zip64_entry* entries64 = nullptr;      // hdlz_zip64_write_ws (wide): its records, nullable, and its zip64_from
    uint64_t zip64_from = 0xFFFFFFFFull;
};
size_t zip_write_work_bytes(uint64_t nentries, uint64_t nblocks, bool wide = false);
hipError_t launch_zip_write(ZipWriteArgs a, void* work, hipStream_t stream, bool wide = false);

// hdlz_png_write.hip: hdlz_png_filter_ws and hdlz_png_write_ws (include/hdlz_png_write.h)
struct PngFilterArgs {
    const uint8_t* pix;
    uint64_t pix_len;
    const hdlz_png_spec* specs;
    uint64_t n;
    uint32_t mode;
    uint64_t total_rows;
    uint8_t* raw;
    uint64_t raw_cap;
    uint8_t* row_filter;              // nullable
    uint32_t* status;
    uint64_t* raw_off;
    uint64_t *row_base, *band_base;   // scratch, n + 1 words each: where an image's rows and bands start
};
size_t png_filter_work_bytes(uint64_t n);
hipError_t launch_png_filter(PngFilterArgs a, void* work, hipStream_t stream);
struct PngWriteArgs {
    const hdlz_png_spec* specs;
    uint64_t n;
    const uint8_t* raw;
    const uint64_t* raw_off;
    const uint32_t* fstatus;          // nullable
    const uint64_t* in_off;
    const uint8_t* rows;
    uint64_t pitch;
    const uint32_t* len;
    const uint64_t* end_bits;
    const uint32_t* status;
    uint64_t nblocks;
    const uint64_t* blk_first;
    uint32_t idat, flags, out_align;
    uint8_t* file;
    uint64_t cap;
    uint64_t *file_off, *file_len;
    uint32_t* image_status;           // nullable
    hdlz_png_image* images;           // nullable
    hdlz_png_write_result* result;
    uint64_t *pre, *cnt, *pa, *pe, *ps;      // scratch, nblocks + 1 words each: the exclusive prefixes of |M_b|, the two counts, the Adler sums
    uint64_t *zlen, *cbase;           // scratch, per image (+ 1): zlen; where its chunks (IHDR and the IDATs) start in the CRC list
    uint32_t *adler, *ist;            // scratch, per image: the stream's Adler-32; the image's status
    uint64_t* head;                   // scratch, 32 words: [0] are the files written, [1] the chunks of the CRC list
};
size_t png_write_work_bytes(uint64_t n, uint64_t nblocks);
hipError_t launch_png_write(PngWriteArgs a, void* work, hipStream_t stream);

}  // namespace hdlz
