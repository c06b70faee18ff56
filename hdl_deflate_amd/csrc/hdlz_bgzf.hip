// hdlz_bgzf.hip -- the kernels of include/hdlz_bgzf.h that are not another kernel's instance: the CRC-32 of every
// block of a batch, the member index of a BGZF file, and what hdlz_bgzf_inflate_ws runs around the member decode.  (The writer is
// k_bgzf_join, hdlz_bgzf_stored.hip; the decode is k_inflate_dyn<false, true>, hdlz_inflate_dyn.hip, through MemberArgs with m_gap = 18.
// The format's constants, the header bytes and is_header stand in hdlz_frame.h.)
//
// k_crc32_batch     a workgroup per block: crc_block of hdlz_crc32.h (first tile right-aligned, Horner over the further tiles).
// k_bgzf_scan       a workgroup per 64 KiB window: the first header-shaped 16 bytes, taken for a member start, and the hops from it
//                   to the window's end -> (entry, exit, count, ISIZE sum, stop status, EOF shape of the last member).
// k_bgzf_seam       ONE wave: exit[w] == entry[w + 1] for 64 seams a step; a window whose guess is wrong is walked again from its true
//                   entry by lane 0; the first confirmed window with a stop status ends the walk; the confirmed windows' counts and
//                   sums are scanned on the way.  Writes the record and the two arrays' last words.
// k_bgzf_emit       a thread per confirmed window: hops again and writes d_off / d_out_off.
// k_bgzf_check      a thread per member: the index checks of hdlz_bgzf_inflate_ws and the decoder's private offsets.
// k_bgzf_judge / k_bgzf_finish   the verdict per member from the decoder's results, the CRC words and the trailer; the record.  The
//                   lowest failed member travels as in hdlz_unjoin.hip: per workgroup into word 256 g, then lowest_word (hdlz_frame.h).
// The member check (k_bgzf_check, and per task k_ranges_expand), the verdict (k_bgzf_judge, k_ranges_judge) and the step into word
// 256 g (k_bgzf_judge, k_unjoin_judge) stand written out in each kernel: as functions of hdlz_frame.h they gave every one of these
// kernels another instruction sequence (profiles/framing_shared.txt, section 3).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_crc32.h"
#include "hdlz_frame.h"

namespace hdlz {
namespace bgzf {

constexpr uint32_t WIN_LOG2 = 16u, WIN = 1u << WIN_LOG2;
constexpr uint64_t NONE64 = ~0ull;

// ---- hdlz_crc32_batch_ws
__global__ __launch_bounds__(CRC_THREADS) void k_crc32_batch(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off, uint64_t pitch,
                                                             uint32_t len, uint64_t nblocks, uint32_t* __restrict__ crc,
                                                             const uint32_t* __restrict__ skip) {
    __shared__ CrcTileLds s;
    crc_build_tables(s);
    __syncthreads();
    for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        if (skip && skip[b] != HDLZ_OK) continue;            // (uniform over the workgroup)
        const uint8_t* p;
        uint32_t L;
        if (off) {
            const uint64_t lo = off[b];
            p = data + (lo - off[0]);
            L = (uint32_t)(off[b + 1] - lo);
        } else {
            p = data + b * pitch;
            L = len;
        }
        const uint32_t c = crc_block(p, L, s);
        if (threadIdx.x == 0u) crc[b] = c;
    }
}

// ---- hdlz_bgzf_index_ws.  The scratch: a summary of 8 words of 64 bits, then per window entry, exit, cbase, obase (64 bits each),
// count, isum, stat, eof (32 bits each).
struct IndexWork {
    uint64_t* sum;       // [0] = windows that take part in the walk
    uint64_t *entry, *exit, *cbase, *obase;
    uint32_t *count, *isum, *stat, *eof;
};
__host__ __device__ inline IndexWork index_work(void* work, uint64_t W) {
    IndexWork w;
    w.sum = static_cast<uint64_t*>(work);
    w.entry = w.sum + 8; w.exit = w.entry + W; w.cbase = w.exit + W; w.obase = w.cbase + W;
    w.count = reinterpret_cast<uint32_t*>(w.obase + W); w.isum = w.count + W; w.stat = w.isum + W; w.eof = w.stat + W;
    return w;
}
struct Hop { uint64_t exit; uint32_t count, isum, stat, eof; };
// steps 2 .. 6 of the contract's walk from p (< limit <= file_len) until p >= limit or a stop: no load outside file[0 .. file_len)
__device__ __forceinline__ Hop walk(const uint8_t* __restrict__ f, uint64_t file_len, uint64_t p, uint64_t limit) {
    Hop h{p, 0u, 0u, (uint32_t)HDLZ_OK, 0u};
    while (p < limit) {
        if (file_len - p < HEAD) { h.stat = HDLZ_E_NO_EOF; break; }
        const uint32_t size = le16(f + p + 16u) + 1u;
        if (!is_header(f + p) || size < MEMBER_MIN) { h.stat = HDLZ_E_BAD_HEADER; break; }
        if (size > file_len - p) { h.stat = HDLZ_E_NO_EOF; break; }
        const uint32_t isize = le32(f + p + size - 4u);
        if (isize > ISIZE_MAX) { h.stat = HDLZ_E_BAD_HEADER; break; }
        h.count += 1u; h.isum += isize; h.eof = size == MEMBER_MIN && isize == 0u ? 1u : 0u;
        p += size;
    }
    h.exit = p;
    return h;
}

__global__ __launch_bounds__(256) void k_bgzf_scan(const uint8_t* __restrict__ f, uint64_t file_len, IndexWork w) {
    __shared__ uint32_t s_found;
    const uint32_t tid = threadIdx.x;
    const uint64_t win = blockIdx.x, lo = win << WIN_LOG2;
    const uint64_t hi = file_len - lo < WIN ? file_len : lo + WIN;
    if (tid == 0u) s_found = NONE;
    __syncthreads();
    for (uint32_t step = 0; step < WIN / 4096u; step++) {
        const uint64_t q = lo + step * 4096u + 16u * tid;     // this thread's 16 positions
        uint32_t mine = NONE;
        if (q < hi) {
            uint32_t d[4] = {0u, 0u, 0u, 0u};
            if (q + 16u <= file_len) {
                const v4 v = *reinterpret_cast<const v4u*>(f + q);
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            } else {
                for (uint32_t i = 0; q + i < file_len; i++) d[i >> 2] |= (uint32_t)f[q + i] << (8u * (i & 3u));
            }
            for (uint32_t i = 0; i < 16u; i++) {
                if (((d[i >> 2] >> (8u * (i & 3u))) & 0xFFu) != 0x1Fu) continue;
                const uint64_t p = q + i;
                if (p >= hi || file_len - p < HEAD || !is_header(f + p)) continue;      // (a header may reach 17 bytes into the next window)
                mine = (uint32_t)(p - lo);
                break;
            }
        }
        if (__syncthreads_or(mine != NONE)) {
            if (mine != NONE) atomicMin(&s_found, mine);
            __syncthreads();
            break;
        }
        if (lo + (step + 1u) * 4096u >= hi) break;           // (uniform)
    }
    if (tid != 0u) return;
    const uint32_t found = s_found;
    Hop h{0u, 0u, 0u, (uint32_t)HDLZ_OK, 0u};
    if (found != NONE) h = walk(f, file_len, lo + found, hi);
    w.entry[win] = found == NONE ? NONE64 : lo + found;
    w.exit[win] = h.exit; w.count[win] = h.count; w.isum[win] = h.isum; w.stat[win] = h.stat; w.eof[win] = h.eof;
}

__global__ __launch_bounds__(64) void k_bgzf_seam(const uint8_t* __restrict__ f, uint64_t file_len, uint64_t W, uint64_t member_cap,
                                                  uint64_t* __restrict__ off, uint64_t* __restrict__ out_off,
                                                  hdlz_bgzf_index_result* __restrict__ result, IndexWork w) {
    const uint32_t lane = threadIdx.x;
    uint64_t base = 0, e = 0;            // window `base` is entered at e (both wave-uniform)
    uint64_t nm = 0, total = 0;          // members and output bytes of the confirmed windows in front of `base`
    uint64_t used = 0;                   // windows that take part
    uint32_t status = HDLZ_OK, eof = 0;
    while (e < file_len && base < W) {   // (e == file_len: step 1 of the walk, HDLZ_OK; e < file_len lies in window `base`)
        const uint64_t win = base + lane;
        const bool valid = win < W;
        const uint64_t ent = valid ? w.entry[win] : NONE64, ex = valid ? w.exit[win] : 0ull;
        const uint32_t st = valid ? w.stat[win] : 0u, cnt = valid ? w.count[win] : 0u, isz = valid ? w.isum[win] : 0u, ef = valid ? w.eof[win] : 0u;
        uint64_t prev = __shfl_up(ex, 1, 64);
        if (lane == 0u) prev = e;
        const bool ok = valid && ent == prev;
        const uint64_t badm = ballot64(!ok);
        const uint32_t fbad = badm ? (uint32_t)__builtin_ctzll(badm) : 64u;          // lanes in front of it are confirmed
        const uint64_t conf = fbad == 64u ? ~0ull : (1ull << fbad) - 1ull;
        const uint64_t stopm = ballot64(st != HDLZ_OK) & conf;
        const uint32_t take = stopm ? (uint32_t)__builtin_ctzll(stopm) + 1u : fbad;      // confirmed windows up to and with the one that stops
        // exclusive scan of the taken windows' counts and sums
        uint64_t c = lane < take ? cnt : 0u, o = lane < take ? isz : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t tc = __shfl_up(c, d, 64), to = __shfl_up(o, d, 64);
            if (lane >= (uint32_t)d) { c += tc; o += to; }
        }
        if (lane < take) { w.cbase[win] = nm + c - cnt; w.obase[win] = total + o - isz; }
        if (take != 0u) {
            nm += __shfl(c, take - 1u, 64); total += __shfl(o, take - 1u, 64);
            e = __shfl(ex, take - 1u, 64);
            eof = (uint32_t)__shfl((int)ef, take - 1u, 64);
            base += take; used = base;
        }
        if (stopm) { status = (uint32_t)__shfl((int)st, take - 1u, 64); break; }
        if (fbad == 64u || e >= file_len || base >= W) continue;
        // window `base` was guessed wrong (or holds no header-shaped bytes at all): lane 0 walks it from its true entry
        Hop h{0u, 0u, 0u, 0u, 0u};
        if (lane == 0u) {
            const uint64_t lim = file_len - (base << WIN_LOG2) < WIN ? file_len : (base + 1u) << WIN_LOG2;
            h = walk(f, file_len, e, lim);
            w.entry[base] = e; w.exit[base] = h.exit; w.count[base] = h.count; w.isum[base] = h.isum; w.stat[base] = h.stat; w.eof[base] = h.eof;
            w.cbase[base] = nm; w.obase[base] = total;
        }
        h.exit = __shfl(h.exit, 0, 64); h.count = (uint32_t)__shfl((int)h.count, 0, 64); h.isum = (uint32_t)__shfl((int)h.isum, 0, 64);
        h.stat = (uint32_t)__shfl((int)h.stat, 0, 64); h.eof = (uint32_t)__shfl((int)h.eof, 0, 64);
        nm += h.count; total += h.isum; e = h.exit; eof = h.eof;
        base += 1u; used = base;
        if (h.stat != HDLZ_OK) { status = h.stat; break; }
    }
    if (lane != 0u) return;
    w.sum[0] = used;
    if (nm <= member_cap) { off[nm] = e; out_off[nm] = total; }
    hdlz_bgzf_index_result res;
    res.nmembers = nm; res.total_out = total; res.file_used = e;
    res.status = nm > member_cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : status;
    res.eof_marker = res.status == HDLZ_OK && nm != 0u ? eof : 0u;
    *result = res;
}

__global__ __launch_bounds__(256) void k_bgzf_emit(const uint8_t* __restrict__ f, uint64_t W, uint64_t member_cap, uint64_t* __restrict__ off,
                                                   uint64_t* __restrict__ out_off, IndexWork w) {
    const uint64_t win = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (win >= W || win >= w.sum[0]) return;
    uint64_t p = w.entry[win], b = w.cbase[win], o = w.obase[win];
    for (uint32_t k = w.count[win]; k != 0u && b <= member_cap; k--, b++) {          // (every hop was checked by the walk that counted it)
        const uint32_t size = le16(f + p + 16u) + 1u;
        off[b] = p; out_off[b] = o;
        o += le32(f + p + size - 4u);
        p += size;
    }
}

// the record of an empty file
__global__ void k_bgzf_index_empty(uint64_t* off, uint64_t* out_off, hdlz_bgzf_index_result* result) {
    off[0] = 0u; out_off[0] = 0u;
    hdlz_bgzf_index_result res;
    res.nmembers = 0u; res.total_out = 0u; res.file_used = 0u; res.status = HDLZ_OK; res.eof_marker = 0u;
    *result = res;
}

// ---- hdlz_bgzf_inflate_ws: in front of the decode
__global__ __launch_bounds__(JT) void k_bgzf_check(BgzfArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * JT + threadIdx.x;
    if (b >= a.nmembers) return;
    const uint64_t lo = a.off[b], hi = a.off[b + 1];
    const uint64_t o0 = a.out_off[0], o = a.out_off[b], e = a.out_off[b + 1];
    uint32_t st = HDLZ_OK;
    if (hi < lo || hi - lo < MEMBER_MIN || hi - lo > MEMBER_MAX || hi > a.in_len) st = HDLZ_E_BAD_PARAM;
    else if (!is_header(a.in + lo)) st = HDLZ_E_BAD_HEADER;
    else if (le16(a.in + lo + 16u) + 1u != hi - lo) st = HDLZ_E_BAD_PARAM;
    else {
        const uint32_t isize = le32(a.in + hi - 4u);
        if (o < o0 || e < o || e - o != isize || isize > ISIZE_MAX || e - o0 > a.out_cap) st = HDLZ_E_BAD_PARAM;
    }
    a.status[b] = st; a.len[b] = 0u; a.end_bit[b] = 0u;
    a.m_off[b] = lo + HEAD; a.m_out_off[b] = o - o0;
    if (b + 1u == a.nmembers) { a.m_off[b + 1] = hi + HEAD; a.m_out_off[b + 1] = e - o0; }
}

// ---- behind the decode and the CRC words: one thread per member; per workgroup the lowest failed member, in the length word of the
// workgroup's first member, which every thread has read by then
__global__ __launch_bounds__(JT) void k_bgzf_judge(BgzfArgs a) {
    __shared__ uint32_t s_first[JT / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t b = (uint64_t)blockIdx.x * JT + tid;
    uint32_t st = HDLZ_OK;
    if (b < a.nmembers) {
        st = a.status[b];
        if (st == HDLZ_OK) {
            const uint64_t lo = a.off[b], hi = a.off[b + 1];                  // (the index checks passed: these words are sound)
            const uint32_t size = (uint32_t)(hi - lo), eb = a.end_bit[b];     // the end bit counts from byte lo + 16
            if (a.len[b] != le32(a.in + hi - 4u)) st = HDLZ_E_BAD_CHECKSUM;
            else if (((eb + 7u) >> 3) + 16u != size - TAIL) st = HDLZ_E_NO_EOF;
            else if (a.crc[b] != le32(a.in + hi - 8u)) st = HDLZ_E_BAD_CHECKSUM;
            if (st != HDLZ_OK) a.status[b] = st;
        }
        if (a.member_status) a.member_status[b] = st;
    }
    const uint64_t m = ballot64(st != HDLZ_OK);
    if (lane == 0u) s_first[wave] = m ? wave * 64u + (uint32_t)__builtin_ctzll(m) : NONE;
    __syncthreads();
    if (tid == 0u) {
        uint32_t f = NONE;
#pragma unroll
        for (uint32_t k = 0; k < JT / 64u; k++) f = min(f, s_first[k]);
        a.len[b] = f == NONE ? NONE : (uint32_t)b + f;                        // (b: the workgroup's first member; nmembers < 2^31)
    }
}

__global__ __launch_bounds__(256) void k_bgzf_finish(BgzfArgs a, uint32_t ngroups) {
    __shared__ uint32_t s_f[256];
    const uint32_t tid = threadIdx.x;
    s_f[tid] = lowest_word(a.len, ngroups, tid, 256u);
    __syncthreads();
    for (uint32_t o = 128u; o > 0u; o >>= 1) {
        if (tid < o) s_f[tid] = min(s_f[tid], s_f[tid + o]);
        __syncthreads();
    }
    if (tid != 0u) return;
    hdlz_bgzf_inflate_result res;
    res.out_len = a.nmembers ? a.out_off[a.nmembers] - a.out_off[0] : 0ull;
    res.first_bad = ~0ull; res.status = HDLZ_OK; res.reserved = 0u;
    if (s_f[0] != NONE) { res.status = a.status[s_f[0]]; res.first_bad = s_f[0]; res.out_len = 0u; }
    *a.result = res;
}

}  // namespace bgzf

hipError_t launch_crc32_batch(const uint8_t* data, const uint64_t* off, uint64_t pitch, uint32_t len, uint64_t nblocks, uint32_t* crc,
                              const uint32_t* skip, hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    const unsigned grid = (unsigned)(nblocks < (1u << 20) ? nblocks : (1u << 20));
    hipLaunchKernelGGL(bgzf::k_crc32_batch, dim3(grid), dim3(CRC_THREADS), 0, stream, data, off, pitch, len, nblocks, crc, skip);
    return hipGetLastError();
}

static inline uint64_t bgzf_windows(uint64_t file_len) { return (file_len + bgzf::WIN - 1u) >> bgzf::WIN_LOG2; }

size_t bgzf_index_work_bytes(uint64_t file_len) {
    const uint64_t W = bgzf_windows(file_len);
    return W ? round256(64u + 48u * (size_t)W) : 0u;
}

hipError_t launch_bgzf_index(const uint8_t* file, uint64_t file_len, uint64_t member_cap, uint64_t* off, uint64_t* out_off,
                             hdlz_bgzf_index_result* result, void* work, hipStream_t stream) {
    using namespace bgzf;
    const uint64_t W = bgzf_windows(file_len);
    if (W == 0) {
        hipLaunchKernelGGL(k_bgzf_index_empty, dim3(1), dim3(1), 0, stream, off, out_off, result);
        return hipGetLastError();
    }
    const IndexWork w = index_work(work, W);
    hipError_t e = launch(k_bgzf_scan, dim3((unsigned)W), dim3(256), stream, file, file_len, w);
    if (e == hipSuccess) e = launch(k_bgzf_seam, dim3(1), dim3(64), stream, file, file_len, W, member_cap, off, out_off, result, w);
    if (e == hipSuccess) e = launch(k_bgzf_emit, dim3((unsigned)((W + 255u) / 256u)), dim3(256), stream, file, W, member_cap, off, out_off, w);
    return e;
}

hipError_t launch_bgzf_check(const BgzfArgs& a, hipStream_t stream) {
    if (a.nmembers == 0) return hipSuccess;
    hipLaunchKernelGGL(bgzf::k_bgzf_check, dim3((unsigned)((a.nmembers + JT - 1u) / JT)), dim3(JT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_bgzf_judge(const BgzfArgs& a, hipStream_t stream) {
    using namespace bgzf;
    const uint32_t ngroups = (uint32_t)((a.nmembers + JT - 1u) / JT);
    if (ngroups) hipLaunchKernelGGL(k_bgzf_judge, dim3(ngroups), dim3(JT), 0, stream, a);
    hipLaunchKernelGGL(k_bgzf_finish, dim3(1), dim3(256), 0, stream, a, ngroups);
    return hipGetLastError();
}

}  // namespace hdlz
