// hdlz_seek.hip -- the kernels of include/hdlz_seek.h that are not a decoder's.  The points of hdlz_seek_index_ws come
// from the decode itself, into scratch (PointSink, hdlz_device.h): from k_any_points behind the whole-GPU chain for any block types
// (hdlz_inflate_any.hip), or from the recording view of k_inflate_dyn (hdlz_inflate_dyn.hip), whose segment view decodes the tasks of
// hdlz_seek_read_ranges_ws (SegArgs).  The ranged read runs the kernels of
// hdlz_bgzf_range.hip for everything that does not know what a task is made of: k_ranges_resolve, k_ranges_scan, k_ranges_crc,
// k_ranges_slice, k_ranges_finish and k_ranges_record over the same scratch (RangeArgs), with slots of the call's own size.
//
// k_seek_points    ONE workgroup, behind the judged decode: the verdict over the recorded points -- the stream failed, or more points
//                  than point_cap: no array is written --, else d_bit and d_pos out of the scratch, their word n, the largest segment;
//                  the record.
// k_seek_windows   a workgroup per point: slot k of d_win -- zeros, then the min(32768, d_pos[k]) bytes in front of d_pos[k], 16 bytes a lane.
// k_seek_crc       a workgroup per point: crc_block of hdlz_crc32.h over segment k of d_out.
// k_seek_expand    a thread per task slot: k_ranges_expand for a segment -- the index words checked, the task's start byte and bit, its
//                  input view, window, history and expected length, and its destination.
// k_seek_judge     a thread per task: length, end bit, CRC-32, in this order; the lowest failed task of every range (atomicMin).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_crc32.h"
#include "hdlz_frame.h"
#include "hdlz_ranges.h"

namespace hdlz {
namespace seek {
using namespace bgzf;                              // RT, the head's words, upper

constexpr uint64_t WIN = HDLZ_SEEK_WINDOW;
constexpr uint32_t VIEW_TAIL = 8u;                 // bytes of an inner segment's input view behind the byte of the next point's bit
constexpr uint32_t ROUTE_CHAIN = 1u, ROUTE_WAVE = 2u;

__global__ __launch_bounds__(RT) void k_seek_points(SeekIndexArgs a) {
    __shared__ uint64_t s_max[RT];
    const uint32_t tid = threadIdx.x;
    const uint32_t st = a.status[0];
    const bool ok = st == HDLZ_OK;
    const uint64_t n = ok ? a.sink.head[0] : 0u, total = ok ? a.out_len[0] : 0u, end_bit = ok ? a.sink.head[1] : 0u;
    const bool write = ok && n <= a.point_cap;     // (n >= 1: the first header is a point)
    uint64_t mx = 0;
    if (write) {
        for (uint64_t k = tid; k < n; k += RT) {
            const uint64_t p = a.sink.pos[k], e = k + 1u < n ? a.sink.pos[k + 1u] : total;
            a.bit[k] = a.sink.bit[k]; a.pos[k] = p;
            mx = e - p > mx ? e - p : mx;
        }
        if (tid == 0u) { a.bit[n] = end_bit; a.pos[n] = total; }
    }
    s_max[tid] = mx;
    __syncthreads();
    for (uint32_t d = RT / 2u; d != 0u; d >>= 1) {
        if (tid < d) s_max[tid] = s_max[tid] > s_max[tid + d] ? s_max[tid] : s_max[tid + d];
        __syncthreads();
    }
    if (tid != 0u) return;
    a.head[0] = write ? n : 0u;
    hdlz_seek_result res;
    res.npoints = n; res.total_out = total; res.end_bit = end_bit; res.max_seg = s_max[0];
    res.status = !ok ? st : write ? (uint32_t)HDLZ_OK : (uint32_t)HDLZ_E_OUT_CAPACITY;
    res.route = a.sink.head[2] == 1u ? ROUTE_CHAIN : ROUTE_WAVE;
    *a.result = res;
}

__global__ __launch_bounds__(RT) void k_seek_windows(SeekIndexArgs a) {
    const uint32_t tid = threadIdx.x;
    const uint64_t n = a.head[0];                  // (at most point_cap)
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint64_t p = a.sink.pos[k];
        const uint32_t h = p < WIN ? (uint32_t)p : (uint32_t)WIN, z = (uint32_t)WIN - h;
        uint8_t* __restrict__ slot = a.win + WIN * k;                       // 16-byte aligned: d_win is, and WIN is a multiple of 16
        for (uint32_t i = tid; i < (z >> 4); i += RT) reinterpret_cast<v4*>(slot)[i] = v4{0u, 0u, 0u, 0u};
        if (tid < (z & 15u)) slot[(z & ~15u) + tid] = 0u;
        copy_to_aligned16(slot + z, a.out + (p - h), h, tid, RT);
    }
}

__global__ __launch_bounds__(CRC_THREADS) void k_seek_crc(SeekIndexArgs a) {
    __shared__ CrcTileLds s;
    crc_build_tables(s);
    __syncthreads();
    const uint64_t n = a.head[0];
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint64_t p = a.sink.pos[k], e = k + 1u < n ? a.sink.pos[k + 1u] : a.out_len[0];
        const uint32_t c = crc_block(a.out + p, (uint32_t)(e - p), s);
        if (threadIdx.x == 0u) a.crc[k] = c;
    }
}

__global__ __launch_bounds__(RT) void k_seek_expand(SeekRangeArgs s) {
    const RangeArgs& a = s.r;
    const uint64_t t = (uint64_t)blockIdx.x * RT + threadIdx.x;
    if (t >= a.task_cap) return;
    if (a.head[H_CAPACITY] != 0u || t >= a.head[H_NTASKS]) {      // an idle slot: no kernel behind this one touches it
        a.t_status[t] = HDLZ_E_OUT_CAPACITY; a.t_range[t] = NONE;
        return;
    }
    const uint64_t r = upper(a.r_tbase, a.nranges + 1u, t) - 1u;  // tbase[r] <= t < tbase[r + 1]
    const uint64_t tb = a.r_tbase[r], k = a.r_lo[r] + (t - tb);   // k < npoints: the resolve kept lo + count <= npoints
    const uint64_t o = a.out_off[k], e = a.out_off[k + 1], b0 = s.bit[k], b1 = s.bit[k + 1];
    const uint64_t p0 = a.r_p0[r], p1 = a.r_p1[r];
    const bool last = k + 1u == a.nmembers;
    uint32_t st = HDLZ_OK;
    if (e < o || e - o > s.seg_cap || b0 >= b1 || b1 > 8u * a.in_len) st = HDLZ_E_BAD_PARAM;
    const uint64_t piece = a.range_off[r], piece_end = a.range_off[r + 1];
    if (st == HDLZ_OK && (piece_end > a.out_cap || piece_end < piece || piece_end - piece != p1 - p0)) st = HDLZ_E_BAD_PARAM;
    uint8_t* dst = nullptr;
    if (st == HDLZ_OK) {
        if (o >= p0 && e <= p1) dst = a.out + (piece + (o - p0));     // covered whole: inside the range's piece of d_out
        else {
            const bool first = t == tb, final_ = t + 1u == a.r_tbase[r + 1];
            if (!first && !final_) st = HDLZ_E_BAD_PARAM;                         // (only with an index that is not ascending)
            else {
                const uint64_t slot = 2u * r + (first ? 0u : 1u);
                dst = a.slots + slot * a.slot_bytes;                              // seg_cap <= slot_bytes
                a.r_edge[slot] = (uint32_t)t;
            }
        }
    }
    uint64_t view_end = (b1 >> 3) + VIEW_TAIL;
    if (last || view_end > a.in_len) view_end = a.in_len;
    a.t_off[t] = b0 >> 3; a.t_end[t] = view_end; a.t_dst[t] = dst;
    a.t_cap[t] = st == HDLZ_OK ? (uint32_t)(e - o) : 0u; a.t_len[t] = 0u; a.t_status[t] = st; a.t_end_bit[t] = 0u; a.t_range[t] = (uint32_t)r;
    s.t_sbit[t] = (uint32_t)(b0 & 7u) | (last ? 0x80000000u : 0u);
    s.t_hist[t] = o < WIN ? (uint32_t)o : (uint32_t)WIN;
    s.t_k[t] = (uint32_t)k;
}

__global__ __launch_bounds__(RT) void k_seek_judge(SeekRangeArgs s) {
    const RangeArgs& a = s.r;
    const uint64_t t = (uint64_t)blockIdx.x * RT + threadIdx.x;
    if (t >= a.task_cap) return;
    const uint32_t r = a.t_range[t];
    if (r == NONE) return;
    uint32_t st = a.t_status[t];
    // (output behind the expected length in front of the next point's bit: the segment does not end where the index says)
    if (st == HDLZ_E_OUT_CAPACITY) { st = HDLZ_E_NO_EOF; a.t_status[t] = st; }
    if (st == HDLZ_OK) {
        const uint32_t k = s.t_k[t];                                              // (the expand's checks passed: k + 1 <= npoints)
        if (a.t_len[t] != a.t_cap[t]) st = HDLZ_E_BAD_CHECKSUM;
        else if ((uint64_t)a.t_end_bit[t] != s.bit[k + 1u]) st = HDLZ_E_NO_EOF;
        else if (a.t_crc[t] != s.crc[k]) st = HDLZ_E_BAD_CHECKSUM;
        if (st != HDLZ_OK) a.t_status[t] = st;
    }
    if (st != HDLZ_OK) atomicMin(&a.r_first[r], (uint32_t)(t - a.r_tbase[r]));
}

}  // namespace seek

static inline dim3 seek_capped(uint64_t n) { return dim3((unsigned)(n < 65536u ? (n ? n : 1u) : 65536u)); }
static inline dim3 seek_groups_of(uint64_t n) { return dim3((unsigned)((n + seek::RT - 1u) / seek::RT)); }

hipError_t launch_seek_index_finish(const SeekIndexArgs& a, hipStream_t stream) {
    using namespace seek;
    hipError_t e = launch(k_seek_points, dim3(1), dim3(RT), stream, a);
    if (a.point_cap == 0) return e;
    if (e == hipSuccess) e = launch(k_seek_windows, seek_capped(a.point_cap), dim3(RT), stream, a);
    if (e == hipSuccess) e = launch(k_seek_crc, seek_capped(a.point_cap), dim3(CRC_THREADS), stream, a);
    return e;
}

hipError_t launch_seek_expand(const SeekRangeArgs& a, hipStream_t stream) {
    if (a.r.nranges == 0 || a.r.task_cap == 0) return hipSuccess;
    return launch(seek::k_seek_expand, seek_groups_of(a.r.task_cap), dim3(seek::RT), stream, a);
}

hipError_t launch_seek_judge(const SeekRangeArgs& a, hipStream_t stream) {
    if (a.r.nranges == 0 || a.r.task_cap == 0) return hipSuccess;
    return launch(seek::k_seek_judge, seek_groups_of(a.r.task_cap), dim3(seek::RT), stream, a);
}

}  // namespace hdlz
