// hdlz_bgzf_range.hip -- the kernels of include/hdlz_bgzf_range.h: what hdlz_bgzf_read_ranges_ws runs around the member
// decode (k_inflate_dyn<false, true>, hdlz_inflate_dyn.hip, through the task view of MemberArgs).  A TASK is one member touched by one
// range; the scratch layout stands at RangeArgs (hdlz_device.h).
//
// k_ranges_resolve   a thread per range: steps 1 and 3 of the contract -- two binary searches per virtual offset, two for lo and hi.
// k_ranges_scan      ONE workgroup: the exclusive scans of lengths and task counts, a strip of ranges per thread; the capacity verdict.
//                    The sum of the lengths SATURATES, and a saturated sum is a capacity failure: no sum that wrapped reaches a store.
// k_ranges_expand    a thread per task slot: its range (binary search in the scanned counts), check 1 of hdlz_bgzf_inflate_ws, the
//                    member's file span and its destination -- d_out when the range covers it whole, else one of the range's two slots.
// k_ranges_crc       a workgroup per task: crc_block of hdlz_crc32.h over the decoded member (k_crc32_batch with a pointer per block).
// k_ranges_judge     a thread per task: the verdict of k_bgzf_judge; the lowest failed task of every range (atomicMin).
// k_ranges_slice     a workgroup per slot: the delivered slice of an edge member, slot -> d_out (copy_to_aligned16, hdlz_frame.h).
// k_ranges_finish    a thread per range: its status; the lowest failed range (atomicMin).
// k_ranges_record    one thread: the record.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_crc32.h"
#include "hdlz_frame.h"
#include "hdlz_ranges.h"

namespace hdlz {
namespace bgzf {

// a virtual offset -> its position in the data; false when it names none (step 1)
__device__ __forceinline__ bool resolve_virtual(const RangeArgs& a, uint64_t v, uint64_t& p) {
    const uint64_t c = v >> 16, u = v & 0xFFFFu, M = a.nmembers;
    const uint64_t b = lower(a.off, M + 1u, c);
    if (b > M || a.off[b] != c) return false;
    const uint64_t o = a.out_off[b];
    if (b == M) { if (u != 0u) return false; }
    else {
        const uint64_t e = a.out_off[b + 1];
        if (e < o || u > e - o) return false;
    }
    p = o + u;
    return true;
}

__global__ __launch_bounds__(RT) void k_ranges_resolve(RangeArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * RT + threadIdx.x;
    if (r >= a.nranges) return;
    const uint64_t x = a.ranges[2u * r], y = a.ranges[2u * r + 1u], M = a.nmembers;
    uint32_t st = HDLZ_OK;
    uint64_t p0 = 0, p1 = 0;
    if (a.flags & HDLZ_BGZF_RANGE_VIRTUAL) {
        if (!resolve_virtual(a, x, p0) || !resolve_virtual(a, y, p1) || p0 > p1) st = HDLZ_E_BAD_PARAM;
    } else if (x > y) st = HDLZ_E_BAD_PARAM;
    else {
        const uint64_t o0 = a.out_off[0], oM = a.out_off[M];
        p0 = x < o0 ? o0 : x; p0 = p0 > oM ? oM : p0;
        p1 = y < o0 ? o0 : y; p1 = p1 > oM ? oM : p1;
    }
    if (st != HDLZ_OK) p0 = p1 = 0u;
    uint64_t lo = 0, cnt = 0;
    if (p1 > p0) {
        const uint64_t ub = upper(a.out_off, M + 1u, p0);       // the lowest b with O[b + 1] > p0 is one in front of it
        lo = ub ? ub - 1u : 0u;
        uint64_t hi = lower(a.out_off, M + 1u, p1);
        hi = hi > M ? M : hi;
        cnt = hi > lo ? hi - lo : 0u;                           // (an index that is not ascending: lo + cnt <= M still holds)
    }
    a.r_p0[r] = p0; a.r_p1[r] = p1; a.r_tbase[r] = cnt;
    a.r_lo[r] = (uint32_t)lo; a.r_status[r] = st; a.r_first[r] = NONE;
    a.r_edge[2u * r] = NONE; a.r_edge[2u * r + 1u] = NONE;
}

// a + b, held at 2^64 - 1: with an index from elsewhere the lengths may add up to more than a word holds
__device__ __forceinline__ uint64_t add_sat(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// thread t owns the ranges [t * strip, (t + 1) * strip): it sums them, the 256 sums are scanned in LDS, and it walks them again.
// The lengths add with add_sat, so a total that does not fit a word reads 2^64 - 1 and is a capacity failure whatever out_cap says;
// below it no partial sum wrapped, every range_off[r] + length = range_off[r + 1] <= total <= out_cap holds in plain arithmetic, and
// that is what k_ranges_expand and k_ranges_slice rest on.  (The task counts cannot wrap: fewer than 2^31 ranges of at most 2^31 tasks.)
__global__ __launch_bounds__(RT) void k_ranges_scan(RangeArgs a) {
    __shared__ uint64_t s_len[RT], s_cnt[RT];
    const uint32_t tid = threadIdx.x;
    const uint64_t R = a.nranges, strip = (R + RT - 1u) / RT;
    const uint64_t b0 = tid * strip < R ? tid * strip : R, b1 = b0 + strip < R ? b0 + strip : R;
    uint64_t len = 0, cnt = 0;
    for (uint64_t r = b0; r < b1; r++) { len = add_sat(len, a.r_p1[r] - a.r_p0[r]); cnt += a.r_tbase[r]; }
    s_len[tid] = len; s_cnt[tid] = cnt;
    __syncthreads();
    for (uint32_t d = 1u; d < RT; d <<= 1) {
        const uint64_t tl = tid >= d ? s_len[tid - d] : 0u, tc = tid >= d ? s_cnt[tid - d] : 0u;
        __syncthreads();
        s_len[tid] = add_sat(s_len[tid], tl); s_cnt[tid] += tc;
        __syncthreads();
    }
    uint64_t run_len = tid ? s_len[tid - 1u] : 0u, run_cnt = s_cnt[tid] - cnt;      // (a saturated sum has no difference to take)
    for (uint64_t r = b0; r < b1; r++) {
        const uint64_t c = a.r_tbase[r];
        a.range_off[r] = run_len; a.r_tbase[r] = run_cnt;
        run_len = add_sat(run_len, a.r_p1[r] - a.r_p0[r]); run_cnt += c;
    }
    if (tid != RT - 1u) return;
    const uint64_t total = s_len[tid], ntasks = s_cnt[tid];
    a.range_off[R] = total; a.r_tbase[R] = ntasks;
    a.head[H_TOTAL] = total; a.head[H_NTASKS] = ntasks;
    a.head[H_CAPACITY] = total == ~0ull || total > a.out_cap || ntasks > a.task_cap ? 1u : 0u;
    a.head[H_FIRST] = NONE;
}

__global__ __launch_bounds__(RT) void k_ranges_expand(RangeArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * RT + threadIdx.x;
    if (t >= a.task_cap) return;
    if (a.head[H_CAPACITY] != 0u || t >= a.head[H_NTASKS]) {      // an idle slot: no kernel behind this one touches it
        a.t_status[t] = HDLZ_E_OUT_CAPACITY; a.t_range[t] = NONE;
        return;
    }
    const uint64_t r = upper(a.r_tbase, a.nranges + 1u, t) - 1u;  // tbase[r] <= t < tbase[r + 1]  (tbase[0] = 0, tbase[R] = ntasks > t)
    const uint64_t tb = a.r_tbase[r], b = a.r_lo[r] + (t - tb);   // b < M: the resolve kept lo + count <= M
    const uint64_t lo = a.off[b], hi = a.off[b + 1], o = a.out_off[b], e = a.out_off[b + 1];
    const uint64_t p0 = a.r_p0[r], p1 = a.r_p1[r];
    uint32_t st = HDLZ_OK, isize = 0u;
    if (hi < lo || hi - lo < MEMBER_MIN || hi - lo > MEMBER_MAX || hi > a.in_len) st = HDLZ_E_BAD_PARAM;
    else if (!is_header(a.in + lo)) st = HDLZ_E_BAD_HEADER;
    else if (le16(a.in + lo + 16u) + 1u != hi - lo) st = HDLZ_E_BAD_PARAM;
    else {
        isize = le32(a.in + hi - 4u);
        if (e < o || e - o != isize || isize > ISIZE_MAX) st = HDLZ_E_BAD_PARAM;
    }
    // the clause of k_bgzf_check (e - o0 > out_cap), here per range: its piece ends inside d_out.  The scan's verdict implies it; it
    // stands here so that no destination below rests on another kernel's arithmetic.
    const uint64_t piece = a.range_off[r], piece_end = a.range_off[r + 1];
    if (st == HDLZ_OK && (piece_end > a.out_cap || piece_end < piece || piece_end - piece != p1 - p0)) st = HDLZ_E_BAD_PARAM;
    uint8_t* dst = nullptr;
    if (st == HDLZ_OK) {
        if (o >= p0 && e <= p1) dst = a.out + (piece + (o - p0));     // covered whole: [o, e) inside [p0, p1), so inside the range's piece of d_out
        else {
            const bool first = t == tb, last = t + 1u == a.r_tbase[r + 1];
            if (!first && !last) st = HDLZ_E_BAD_PARAM;                           // (only with an index that is not ascending)
            else {
                const uint64_t slot = 2u * r + (first ? 0u : 1u);
                dst = a.slots + slot * a.slot_bytes;
                a.r_edge[slot] = (uint32_t)t;
            }
        }
    }
    a.t_off[t] = lo + HEAD; a.t_end[t] = hi; a.t_dst[t] = dst;
    a.t_cap[t] = isize; a.t_len[t] = 0u; a.t_status[t] = st; a.t_end_bit[t] = 0u; a.t_range[t] = (uint32_t)r;
}

__global__ __launch_bounds__(CRC_THREADS) void k_ranges_crc(RangeArgs a) {
    __shared__ CrcTileLds s;
    crc_build_tables(s);
    __syncthreads();
    for (uint64_t t = blockIdx.x; t < a.task_cap; t += gridDim.x) {
        if (a.t_status[t] != HDLZ_OK) continue;                 // (uniform over the workgroup; idle slots too)
        const uint32_t c = crc_block(a.t_dst[t], a.t_cap[t], s);
        if (threadIdx.x == 0u) a.t_crc[t] = c;
    }
}

__global__ __launch_bounds__(RT) void k_ranges_judge(RangeArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * RT + threadIdx.x;
    if (t >= a.task_cap) return;
    const uint32_t r = a.t_range[t];
    if (r == NONE) return;
    uint32_t st = a.t_status[t];
    if (st == HDLZ_OK) {
        const uint64_t lo = a.t_off[t] - HEAD, hi = a.t_end[t];                   // (check 1 passed: these words are sound)
        const uint32_t size = (uint32_t)(hi - lo), eb = a.t_end_bit[t];           // the end bit counts from byte lo + 16
        if (a.t_len[t] != le32(a.in + hi - 4u)) st = HDLZ_E_BAD_CHECKSUM;
        else if (((eb + 7u) >> 3) + 16u != size - TAIL) st = HDLZ_E_NO_EOF;
        else if (a.t_crc[t] != le32(a.in + hi - 8u)) st = HDLZ_E_BAD_CHECKSUM;
        if (st != HDLZ_OK) a.t_status[t] = st;
    }
    if (st != HDLZ_OK) atomicMin(&a.r_first[r], (uint32_t)(t - a.r_tbase[r]));
}

__global__ __launch_bounds__(RT) void k_ranges_slice(RangeArgs a) {
    const uint32_t tid = threadIdx.x;
    for (uint64_t slot = blockIdx.x; slot < 2u * a.nranges; slot += gridDim.x) {
        const uint32_t t = a.r_edge[slot];
        if (t == NONE || a.t_status[t] != HDLZ_OK) continue;    // (uniform; a failed range's piece stays as it is)
        const uint64_t r = slot >> 1;
        const uint64_t o = a.out_off[a.r_lo[r] + (t - a.r_tbase[r])], e = o + a.t_cap[t];       // the member holds [o, e) of the data
        const uint64_t p0 = a.r_p0[r], p1 = a.r_p1[r];
        const uint64_t s0 = o > p0 ? o : p0, s1 = e < p1 ? e : p1;
        if (s1 <= s0) continue;
        const uint8_t* __restrict__ src = a.slots + slot * a.slot_bytes + (s0 - o);
        uint8_t* __restrict__ dst = a.out + (a.range_off[r] + (s0 - p0));
        copy_to_aligned16(dst, src, (uint32_t)(s1 - s0), tid, RT);
    }
}

__global__ __launch_bounds__(RT) void k_ranges_finish(RangeArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * RT + threadIdx.x;
    const bool capacity = a.head[H_CAPACITY] != 0u;
    uint32_t st = HDLZ_OK;
    if (r < a.nranges) {
        st = a.r_status[r];
        if (st == HDLZ_OK) {
            const uint32_t f = a.r_first[r];
            if (capacity) st = HDLZ_E_OUT_CAPACITY;
            else if (f != NONE) st = a.t_status[a.r_tbase[r] + f];
            a.r_status[r] = st;
        }
        if (a.range_status) a.range_status[r] = st;
    }
    const uint64_t m = ballot64(st != HDLZ_OK && !capacity);
    if (m && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(m)) atomicMin(reinterpret_cast<uint32_t*>(a.head + H_FIRST), (uint32_t)r);
}

__global__ void k_ranges_record(RangeArgs a) {
    hdlz_bgzf_ranges_result res;
    res.total_out = a.head[H_TOTAL]; res.ntasks = a.head[H_NTASKS];
    res.first_bad = ~0ull; res.status = HDLZ_OK; res.reserved = 0u;
    const uint32_t f = (uint32_t)a.head[H_FIRST];
    if (a.head[H_CAPACITY] != 0u) res.status = HDLZ_E_OUT_CAPACITY;
    else if (f != NONE) { res.status = a.r_status[f]; res.first_bad = f; }
    *a.result = res;
}

// the record of an empty batch
__global__ void k_ranges_empty(uint64_t* range_off, hdlz_bgzf_ranges_result* result) {
    range_off[0] = 0u;
    hdlz_bgzf_ranges_result res;
    res.total_out = 0u; res.ntasks = 0u; res.first_bad = ~0ull; res.status = HDLZ_OK; res.reserved = 0u;
    *result = res;
}

}  // namespace bgzf

size_t bgzf_ranges_work_bytes(uint64_t R, uint64_t T, uint64_t slot_bytes) {
    if (R == 0) return 0;
    return 256u + 4u * round256(8u * ((size_t)R + 1u)) + 3u * round256(4u * (size_t)R) + 3u * round256(8u * (size_t)T) +
           6u * round256(4u * (size_t)T) + (size_t)(2u * slot_bytes) * (size_t)R;
}

RangeArgs bgzf_ranges_args(void* work, uint64_t R, uint64_t T, uint64_t slot_bytes) {
    RangeArgs a{};
    uint8_t* p = static_cast<uint8_t*>(work);
    const size_t r8 = round256(8u * ((size_t)R + 1u)), r4 = round256(4u * (size_t)R), t8 = round256(8u * (size_t)T), t4 = round256(4u * (size_t)T);
    auto take = [&p](size_t n) { uint8_t* q = p; p += n; return q; };
    a.head = reinterpret_cast<uint64_t*>(take(256u));
    a.r_p0 = reinterpret_cast<uint64_t*>(take(r8)); a.r_p1 = reinterpret_cast<uint64_t*>(take(r8));
    a.r_tbase = reinterpret_cast<uint64_t*>(take(r8)); a.r_edge = reinterpret_cast<uint32_t*>(take(r8));
    a.r_lo = reinterpret_cast<uint32_t*>(take(r4)); a.r_status = reinterpret_cast<uint32_t*>(take(r4)); a.r_first = reinterpret_cast<uint32_t*>(take(r4));
    a.t_off = reinterpret_cast<uint64_t*>(take(t8)); a.t_end = reinterpret_cast<uint64_t*>(take(t8)); a.t_dst = reinterpret_cast<uint8_t**>(take(t8));
    a.t_cap = reinterpret_cast<uint32_t*>(take(t4)); a.t_len = reinterpret_cast<uint32_t*>(take(t4)); a.t_status = reinterpret_cast<uint32_t*>(take(t4));
    a.t_end_bit = reinterpret_cast<uint32_t*>(take(t4)); a.t_crc = reinterpret_cast<uint32_t*>(take(t4)); a.t_range = reinterpret_cast<uint32_t*>(take(t4));
    a.slots = p;
    a.slot_bytes = slot_bytes;
    return a;
}

static inline dim3 capped(uint64_t n) { return dim3((unsigned)(n < (1u << 20) ? n : (1u << 20))); }
static inline dim3 groups_of(uint64_t n) { return dim3((unsigned)((n + bgzf::RT - 1u) / bgzf::RT)); }

// (an empty batch: the record at once, and launch_ranges_deliver has nothing left to do)
hipError_t launch_ranges_resolve_scan(const RangeArgs& a, hipStream_t stream) {
    using namespace bgzf;
    if (a.nranges == 0) return launch(k_ranges_empty, dim3(1), dim3(1), stream, a.range_off, a.result);
    hipError_t e = launch(k_ranges_resolve, groups_of(a.nranges), dim3(RT), stream, a);
    if (e == hipSuccess) e = launch(k_ranges_scan, dim3(1), dim3(RT), stream, a);
    return e;
}

hipError_t launch_bgzf_ranges_plan(const RangeArgs& a, hipStream_t stream) {
    using namespace bgzf;
    hipError_t e = launch_ranges_resolve_scan(a, stream);
    if (e == hipSuccess && a.nranges && a.task_cap) e = launch(k_ranges_expand, groups_of(a.task_cap), dim3(RT), stream, a);
    return e;
}

hipError_t launch_ranges_crc(const RangeArgs& a, hipStream_t stream) {
    using namespace bgzf;
    if (a.nranges == 0 || a.task_cap == 0) return hipSuccess;
    return launch(k_ranges_crc, capped(a.task_cap), dim3(CRC_THREADS), stream, a);
}

hipError_t launch_ranges_deliver(const RangeArgs& a, hipStream_t stream) {
    using namespace bgzf;
    if (a.nranges == 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (a.task_cap) e = launch(k_ranges_slice, capped(2u * a.nranges), dim3(RT), stream, a);
    if (e == hipSuccess) e = launch(k_ranges_finish, groups_of(a.nranges), dim3(RT), stream, a);
    if (e == hipSuccess) e = launch(k_ranges_record, dim3(1), dim3(1), stream, a);
    return e;
}

hipError_t launch_bgzf_ranges_finish(const RangeArgs& a, hipStream_t stream) {
    using namespace bgzf;
    if (a.nranges == 0) return hipSuccess;
    hipError_t e = launch_ranges_crc(a, stream);
    if (e == hipSuccess && a.task_cap) e = launch(k_ranges_judge, groups_of(a.task_cap), dim3(RT), stream, a);
    if (e == hipSuccess) e = launch_ranges_deliver(a, stream);
    return e;
}

}  // namespace hdlz
