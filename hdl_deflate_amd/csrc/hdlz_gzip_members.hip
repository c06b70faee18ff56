// hdlz_gzip_members.hip -- the kernels of include/hdlz_gzip_members.h: the member index of a plain gzip file, a guess
// by a syntactic rule, and what hdlz_gzip_members_inflate_ws runs around the member decode to verify it.
//
// k_gzm_scan     a wave per window of 32 KiB (four to a workgroup), two KiB a step: 16 bytes a lane of either, both loads in flight, and
//                the next lane's first word as the halo (lane 63: the second KiB's first word; for the second KiB a load of its own:
//                the 3 bytes over the seam of the step and of the window).  A quick test of the 32 positions (maybe: four XOR / OR
//                words and a zero-byte test per 4 positions) ends nearly every step with two ballot words of 0; only behind it the
//                exact masks are taken -> one ballot word per KiB (which lanes hold a candidate), and a KiB that holds one goes on: a
//                max-scan gives every candidate the one in front of it, the guesses between candidates of the window are summed.
//                Per window: count, first, last, that sum.
// k_gzm_seam     ONE workgroup, K consecutive windows a thread: a max-scan hands every window the last candidate in front of it, the
//                guess across the seam is taken from the file, the counts and the guesses are scanned in 64 bits; the record and the
//                two arrays' last words.
// k_gzm_emit     a wave per window that holds a candidate: only the lanes the ballot words name load their 16 bytes again, and the
//                wave writes d_off / d_out_off in order.
// k_gzm_heads    a wave per member: the index checks, then the header walk of hdlz_gzip_walk.h -> the decoder's view of the member.
// k_gzm_judge / k_gzm_finish   the verdict per member and the record; the lowest failed member travels as in hdlz_bgzf.hip.
// Plain stores only.  Loads: bytes of file[0 .. file_len), and of it in the read only the spans that passed the index checks.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_frame.h"
#include "hdlz_plan.h"
#include "hdlz_gzip_walk.h"

namespace hdlz {
namespace gzm {

constexpr uint32_t WIN_LOG2 = 15u, WIN = 1u << WIN_LOG2, KIB = 1024u, STEPS = WIN / KIB;
constexpr uint32_t SEAM_THREADS = 512u;
constexpr uint64_t NONE64 = ~0ull;
constexpr uint32_t SPAN_MIN = 18u;                       // a member is at least 10 + 2 + 8 bytes; below 18 the guess is 0
constexpr uint32_t MAGIC = 0x00088B1Fu, MAGIC_MASK = 0xE0FFFFFFu;

// ---- the scratch of the index: a head of 64 bytes, then per window 32 ballot words, five words of 64 bits and the count
struct IndexWork {
    uint64_t* flags;     // [W * STEPS]
    uint64_t *gsum, *first, *last, *cbase, *obase, *prev;      // [W] each; first / last / prev: NONE64 = none
    uint32_t* count;     // [W]
};
__host__ __device__ inline IndexWork index_work(void* work, uint64_t W) {
    IndexWork w;
    w.flags = static_cast<uint64_t*>(work) + 8;
    w.gsum = w.flags + W * STEPS; w.first = w.gsum + W; w.last = w.first + W; w.cbase = w.last + W; w.obase = w.cbase + W; w.prev = w.obase + W;
    w.count = reinterpret_cast<uint32_t*>(w.prev + W);
    return w;
}

// the guess of the member [prev, pos): pos is the next candidate, or file_len
__device__ __forceinline__ uint64_t guess(const uint8_t* __restrict__ f, uint64_t prev, uint64_t pos) {
    const uint64_t span = pos - prev;
    if (span < SPAN_MIN) return 0u;
    const uint64_t isize = le32(f + pos - 4u), bound = 1032u * span + 258u;
    return isize < bound ? isize : bound;
}

// up to 4 bytes at q as a little-endian word: nothing at or behind file_len is loaded (zeros stand for it)
__device__ __forceinline__ uint32_t load_word(const uint8_t* __restrict__ f, uint64_t file_len, uint64_t q) {
    typedef uint32_t __attribute__((aligned(1))) u32u;
    if (q + 4u <= file_len) return *reinterpret_cast<const u32u*>(f + q);
    uint32_t v = 0;
    for (uint32_t i = 0; q + i < file_len; i++) v |= (uint32_t)f[q + i] << (8u * i);
    return v;
}
// this lane's 16 bytes at q -> d[0 .. 4)
__device__ __forceinline__ void load_piece(const uint8_t* __restrict__ f, uint64_t file_len, uint64_t q, uint32_t d[5]) {
    if (q + 16u <= file_len) {
        const v4 v = *reinterpret_cast<const v4u*>(f + q);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) d[k] = load_word(f, file_len, q + 4u * k);
    }
}
// bit i: q + i is a candidate.  d[0 .. 5): the 20 bytes at q, zeros behind file_len
__device__ __forceinline__ uint32_t candidates(const uint32_t d[5], uint64_t file_len, uint64_t q) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16u; i++) {
        const uint32_t word = (i & 3u) ? __builtin_amdgcn_alignbyte(d[(i >> 2) + 1u], d[i >> 2], i & 3u) : d[i >> 2];
        m |= ((word & MAGIC_MASK) == MAGIC ? 1u : 0u) << i;
    }
    if (q + 20u > file_len) {                             // p + 4 <= file_len
        const uint64_t room = file_len > q + 3u ? file_len - 3u - q : 0u;      // positions q .. q + room - 1 may be candidates
        m &= room >= 16u ? 0xFFFFu : (1u << (uint32_t)room) - 1u;
    }
    if (q == 0u && file_len != 0u) m |= 1u;               // position 0
    return m;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
    return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, (int)src, 64) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64) << 32);
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, uint32_t d) {
    return (uint64_t)(uint32_t)__shfl_up((int)(uint32_t)v, d, 64) | ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64) << 32);
}
// the inclusive largest over the wave (the sum: wave_scan_add, hdlz_plan.h).  Positions travel as int64: -1 = none
__device__ __forceinline__ int64_t wave_scan_max(int64_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) { const int64_t t = (int64_t)shfl_up64((uint64_t)v, d); if (lane >= d && t > v) v = t; }
    return v;
}

// nonzero when one of the 16 positions at q may be a candidate, never zero when one is: byte i of y is zero iff the four bytes at
// position i match the rule, and (y - 0x01010101) & ~y & 0x80808080 is nonzero iff a byte of y is zero.  d[0 .. 5): as for candidates
__device__ __forceinline__ uint32_t maybe(const uint32_t d[5]) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t s1 = __builtin_amdgcn_alignbyte(d[k + 1u], d[k], 1u), s2 = __builtin_amdgcn_alignbyte(d[k + 1u], d[k], 2u),
                       s3 = __builtin_amdgcn_alignbyte(d[k + 1u], d[k], 3u);
        const uint32_t y = (d[k] ^ 0x1F1F1F1Fu) | (s1 ^ 0x8B8B8B8Bu) | (s2 ^ 0x08080808u) | (s3 & 0xE0E0E0E0u);
        t |= (y - 0x01010101u) & ~y & 0x80808080u;
    }
    return t;
}

// what a wave carries through its window
struct Run {
    int64_t carry;       // the last candidate in front (k_gzm_emit: of the file; k_gzm_scan: of this window); -1: none
    uint64_t idx;        // candidates in front
    uint64_t acc;        // the guesses of the members that END at a candidate in front
    uint64_t first;      // k_gzm_scan: the window's first candidate
};

// A KiB that holds a candidate (any != 0: the lanes whose mask m is not 0; q: this lane's 16 positions): a max-scan gives every
// candidate the one in front of it, the guesses are summed, and -- EMIT -- the candidates are written in order
template <bool EMIT>
__device__ __forceinline__ void kib(const uint8_t* __restrict__ f, uint64_t q, uint32_t m, uint64_t any, uint32_t lane, Run& r, uint64_t member_cap,
                                    uint64_t* __restrict__ off, uint64_t* __restrict__ out_off) {
    const int64_t mylast = m ? (int64_t)(q + (31u - (uint32_t)__builtin_clz(m))) : -1;
    const int64_t incl = wave_scan_max(mylast, lane);
    int64_t pred = (int64_t)shfl_up64((uint64_t)incl, 1u);
    if (lane == 0u || pred < r.carry) pred = r.carry;
    uint64_t gl = 0;
    {
        int64_t pv = pred;
        for (uint32_t mm = m; mm; mm &= mm - 1u) {
            const uint64_t pos = q + (uint32_t)__builtin_ctz(mm);
            if (pv >= 0) gl += guess(f, (uint64_t)pv, pos);
            pv = (int64_t)pos;
        }
    }
    const uint32_t cnt = (uint32_t)__builtin_popcount(m);
    const uint64_t icnt = wave_scan_add(cnt), igl = wave_scan_add(gl);
    if constexpr (EMIT) {
        uint64_t k = r.idx + icnt - cnt, o = r.acc + igl - gl;
        int64_t pv = pred;
        for (uint32_t mm = m; mm; mm &= mm - 1u, k++) {
            const uint64_t pos = q + (uint32_t)__builtin_ctz(mm);
            if (pv >= 0) o += guess(f, (uint64_t)pv, pos);
            pv = (int64_t)pos;
            if (k <= member_cap) { off[k] = pos; out_off[k] = o; }
        }
    } else if (r.first == NONE64) {
        r.first = shfl64(q + (m ? (uint32_t)__builtin_ctz(m) : 0u), (uint32_t)__builtin_ctzll(any));
    }
    r.carry = (int64_t)shfl64((uint64_t)incl, 63u);       // (any != 0: a position)
    r.idx += shfl64(icnt, 63u);
    r.acc += shfl64(igl, 63u);
}

// k_gzm_scan's window: two KiB a step, both loads in flight before the first test; the first KiB's halo at lane 63 is the second one's
// first word.  The quick test (maybe) decides nearly every step; the exact masks are taken only behind it.
__device__ __forceinline__ void scan_window(const uint8_t* __restrict__ f, uint64_t file_len, uint64_t win, const IndexWork& w) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lo = win << WIN_LOG2, hi = file_len - lo < WIN ? file_len : lo + WIN;
    Run r{-1, 0u, 0u, NONE64};
    static_assert(STEPS % 2u == 0u, "the second KiB of a step lies in the same window");
    for (uint32_t it = 0; it < STEPS; it += 2u) {
        const uint64_t base = lo + it * KIB;
        if (base >= hi) break;                            // (uniform)
        const bool two = base + KIB < hi;                 // (uniform; false: the file ends inside the first KiB, zeros stand behind it)
        const uint64_t qa = base + 16u * lane, qb = qa + KIB;
        uint32_t da[5] = {0u, 0u, 0u, 0u, 0u}, db[5] = {0u, 0u, 0u, 0u, 0u};
        if (qa < file_len) load_piece(f, file_len, qa, da);
        if (two && qb < file_len) load_piece(f, file_len, qb, db);
        const uint32_t halo = two && lane == 63u ? load_word(f, file_len, qb + 16u) : 0u;
        const uint32_t b0 = (uint32_t)__shfl((int)db[0], 0, 64);
        da[4] = (uint32_t)__shfl_down((int)da[0], 1u, 64);
        db[4] = (uint32_t)__shfl_down((int)db[0], 1u, 64);
        if (lane == 63u) { da[4] = b0; db[4] = halo; }
        uint32_t quick = maybe(da) | maybe(db);
        if (qa == 0u) quick = 1u;                         // position 0
        if (ballot64(quick != 0u) == 0u) {
            if (lane == 0u) { w.flags[win * STEPS + it] = 0u; w.flags[win * STEPS + it + 1u] = 0u; }
            continue;
        }
        const uint32_t ma = qa < file_len ? candidates(da, file_len, qa) : 0u, mb = two && qb < file_len ? candidates(db, file_len, qb) : 0u;
        const uint64_t anya = ballot64(ma != 0u), anyb = ballot64(mb != 0u);
        if (lane == 0u) { w.flags[win * STEPS + it] = anya; w.flags[win * STEPS + it + 1u] = anyb; }
        if (anya) kib<false>(f, qa, ma, anya, lane, r, 0u, nullptr, nullptr);
        if (anyb) kib<false>(f, qb, mb, anyb, lane, r, 0u, nullptr, nullptr);
    }
    if (lane == 0u) { w.count[win] = (uint32_t)r.idx; w.gsum[win] = r.acc; w.first[win] = r.first; w.last[win] = (uint64_t)r.carry; }
}

// k_gzm_emit's window, behind the seam pass: only the lanes the ballot words name load
__device__ __forceinline__ void emit_window(const uint8_t* __restrict__ f, uint64_t file_len, uint64_t win, const IndexWork& w, uint64_t member_cap,
                                            uint64_t* __restrict__ off, uint64_t* __restrict__ out_off) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lo = win << WIN_LOG2, hi = file_len - lo < WIN ? file_len : lo + WIN;
    Run r{(int64_t)w.prev[win], w.cbase[win], w.obase[win], NONE64};
    for (uint32_t it = 0; it < STEPS; it++) {
        const uint64_t base = lo + it * KIB;
        if (base >= hi) break;                            // (uniform)
        const uint64_t any = w.flags[win * STEPS + it];
        if (any == 0u) continue;
        const uint64_t q = base + 16u * lane;
        uint32_t m = 0;
        if ((any >> lane) & 1u) {
            uint32_t d[5];
            load_piece(f, file_len, q, d);
            d[4] = load_word(f, file_len, q + 16u);
            m = candidates(d, file_len, q);
        }
        kib<true>(f, q, m, any, lane, r, member_cap, off, out_off);
    }
}

__global__ __launch_bounds__(256) void k_gzm_scan(const uint8_t* __restrict__ f, uint64_t file_len, uint64_t W, IndexWork w) {
    const uint64_t win = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (win >= W) return;                                 // (uniform over the wave)
    scan_window(f, file_len, win, w);
}

__global__ __launch_bounds__(256) void k_gzm_emit(const uint8_t* __restrict__ f, uint64_t file_len, uint64_t W, uint64_t member_cap,
                                                  uint64_t* __restrict__ off, uint64_t* __restrict__ out_off, IndexWork w) {
    const uint64_t win = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (win >= W || w.count[win] == 0u || w.cbase[win] > member_cap) return;
    emit_window(f, file_len, win, w, member_cap, off, out_off);
}

// the exclusive largest over the seam workgroup: what the threads in front hold; *total: all of them (block_scan's barriers)
__device__ __forceinline__ int64_t block_scan_max(int64_t v, uint64_t* s, int64_t* total) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const int64_t incl = wave_scan_max(v, lane);
    __syncthreads();
    if (lane == 63u) s[wave] = (uint64_t)incl;
    __syncthreads();
    int64_t before = -1, all = -1;
    for (uint32_t k = 0; k < SEAM_THREADS / 64u; k++) { const int64_t t = (int64_t)s[k]; if (k < wave && t > before) before = t; if (t > all) all = t; }
    *total = all;
    int64_t ex = (int64_t)shfl_up64((uint64_t)incl, 1u);
    if (lane == 0u) ex = -1;
    return ex > before ? ex : before;
}

__global__ __launch_bounds__(SEAM_THREADS) void k_gzm_seam(const uint8_t* __restrict__ f, uint64_t file_len, uint64_t W, uint64_t member_cap,
                                                           uint64_t* __restrict__ off, uint64_t* __restrict__ out_off,
                                                           hdlz_gzip_members_index_result* __restrict__ result, IndexWork w) {
    __shared__ uint64_t s[2][SEAM_THREADS / 64u];
    const uint32_t tid = threadIdx.x;
    // (the strip of hdlz_plan.h, written out: tests/second_trips.py reads K from this line to place its shapes)
    const uint64_t K = (W + SEAM_THREADS - 1u) / SEAM_THREADS;
    const uint64_t w0 = tid * K < W ? tid * K : W, w1 = w0 + K < W ? w0 + K : W;
    const uint32_t* __restrict__ count = w.count;
    const uint64_t *__restrict__ gsum = w.gsum, *__restrict__ first = w.first, *__restrict__ last = w.last;
    uint64_t *__restrict__ cbase = w.cbase, *__restrict__ obase = w.obase, *__restrict__ prev = w.prev;
    int64_t lm = -1;
    for (uint64_t win = w0; win < w1; win++) { const int64_t l = (int64_t)last[win]; if (l > lm) lm = l; }
    int64_t last_all;
    const int64_t p0 = block_scan_max(lm, s[0], &last_all);  // the last candidate in front of window w0
    // this thread's windows twice: their sums for the scan, then -- with the threads' in front -- every window's words
    uint64_t mine[2] = {0u, 0u}, base[2], all[2];                // members, guessed bytes
    int64_t p = p0;
    for (uint64_t win = w0; win < w1; win++) {
        if (count[win] == 0u) continue;
        mine[0] += count[win];
        mine[1] += gsum[win] + (p >= 0 ? guess(f, (uint64_t)p, first[win]) : 0u);
        p = (int64_t)last[win];
    }
    block_scan<2, SEAM_THREADS>(mine, base, all, s);
    uint64_t c = base[0], g = base[1], total = all[1];
    const uint64_t M = all[0];
    p = p0;
    for (uint64_t win = w0; win < w1; win++) {
        cbase[win] = c; obase[win] = g; prev[win] = (uint64_t)p;
        if (count[win] == 0u) continue;
        c += count[win];
        g += gsum[win] + (p >= 0 ? guess(f, (uint64_t)p, first[win]) : 0u);
        p = (int64_t)last[win];
    }
    if (tid != 0u) return;
    if (M != 0u) total += guess(f, (uint64_t)last_all, file_len);
    if (M <= member_cap) { off[M] = file_len; out_off[M] = total; }
    hdlz_gzip_members_index_result res;
    res.nmembers = M; res.total_out = total; res.status = M > member_cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)HDLZ_OK; res.reserved = 0u;
    *result = res;
}

__global__ void k_gzm_index_empty(uint64_t* off, uint64_t* out_off, hdlz_gzip_members_index_result* result) {
    off[0] = 0u; out_off[0] = 0u;
    hdlz_gzip_members_index_result res;
    res.nmembers = 0u; res.total_out = 0u; res.status = HDLZ_OK; res.reserved = 0u;
    *result = res;
}

// ---- hdlz_gzip_members_inflate_ws: in front of the decode, a wave per member
__global__ __launch_bounds__(64) void k_gzm_heads(GzipMembersArgs a) {
    for (uint64_t b = blockIdx.x; b < a.nmembers; b += gridDim.x) {
        const uint64_t s = a.off[b], e = a.off[b + 1];
        const uint64_t o0 = a.out_off[0], o = a.out_off[b], oe = a.out_off[b + 1];
        const bool bad = e < s || e > a.in_len || e - s >= (1ull << 28) || o < o0 || oe < o || oe - o >= 0xFFFFFE00ull || oe - o0 > a.out_cap;
        uint64_t p = 0;
        const uint32_t st = bad ? (uint32_t)HDLZ_E_BAD_PARAM : gunzip::walk(a.in + s, e - s, p);      // (uniform over the wave)
        if (threadIdx.x != 0u) continue;
        a.status[b] = st; a.len[b] = 0u; a.end_bit[b] = 0u; a.p[b] = (uint32_t)p;
        a.m_off[b] = bad ? 0u : s + p; a.m_end[b] = bad ? 0u : e;
        a.m_out_off[b] = o - o0;
        if (b + 1u == a.nmembers) a.m_out_off[b + 1] = oe - o0;
    }
}

// ---- behind the decode and the CRC words: a thread per member; per workgroup the lowest failed member, in the length word of the
// workgroup's first member, which every thread has read by then (k_bgzf_judge's way)
__global__ __launch_bounds__(JT) void k_gzm_judge(GzipMembersArgs a) {
    __shared__ uint32_t s_first[JT / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t b = (uint64_t)blockIdx.x * JT + tid;
    uint32_t st = HDLZ_OK;
    if (b < a.nmembers) {
        st = a.status[b];
        if (st == HDLZ_OK) {
            const uint64_t s = a.off[b], span = a.off[b + 1] - s;             // (the index checks passed: these words are sound)
            const uint64_t slot = a.m_out_off[b + 1] - a.m_out_off[b];
            const uint64_t end = (uint64_t)a.p[b] - 2u + ((a.end_bit[b] + 7u) >> 3);     // the end bit counts from byte s + p - 2
            if (end + 8u != span) st = HDLZ_E_NO_EOF;
            else if (a.len[b] != slot) st = HDLZ_E_BAD_CHECKSUM;
            else if (le32(a.in + s + end) != a.crc[b] || le32(a.in + s + end + 4u) != (uint32_t)slot) st = HDLZ_E_BAD_CHECKSUM;
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

__global__ __launch_bounds__(256) void k_gzm_finish(GzipMembersArgs a, uint32_t ngroups) {
    __shared__ uint32_t s_f[256];
    const uint32_t tid = threadIdx.x;
    s_f[tid] = lowest_word(a.len, ngroups, tid, 256u);
    __syncthreads();
    for (uint32_t o = 128u; o > 0u; o >>= 1) {
        if (tid < o) s_f[tid] = min(s_f[tid], s_f[tid + o]);
        __syncthreads();
    }
    if (tid != 0u) return;
    hdlz_gzip_members_inflate_result res;
    res.out_len = a.nmembers ? a.out_off[a.nmembers] - a.out_off[0] : 0ull;
    res.first_bad = ~0ull; res.status = HDLZ_OK; res.reserved = 0u;
    if (s_f[0] != NONE) { res.status = a.status[s_f[0]]; res.first_bad = s_f[0]; res.out_len = 0u; }
    *a.result = res;
}

}  // namespace gzm

static inline uint64_t gzm_windows(uint64_t file_len) { return (file_len + gzm::WIN - 1u) >> gzm::WIN_LOG2; }

size_t gzip_members_index_work_bytes(uint64_t file_len) {
    const uint64_t W = gzm_windows(file_len);
    return W ? round256(64u + (8u * (gzm::STEPS + 6u) + 4u) * (size_t)W) : 0u;
}

hipError_t launch_gzip_members_index(const uint8_t* file, uint64_t file_len, uint64_t member_cap, uint64_t* off, uint64_t* out_off,
                                     hdlz_gzip_members_index_result* result, void* work, hipStream_t stream) {
    using namespace gzm;
    const uint64_t W = gzm_windows(file_len);
    if (W == 0) {
        hipLaunchKernelGGL(k_gzm_index_empty, dim3(1), dim3(1), 0, stream, off, out_off, result);
        return hipGetLastError();
    }
    const IndexWork w = index_work(work, W);
    const dim3 grid((unsigned)((W + 3u) / 4u));
    hipLaunchKernelGGL(k_gzm_scan, grid, dim3(256), 0, stream, file, file_len, W, w);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gzm_seam, dim3(1), dim3(SEAM_THREADS), 0, stream, file, file_len, W, member_cap, off, out_off, result, w);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gzm_emit, grid, dim3(256), 0, stream, file, file_len, W, member_cap, off, out_off, w);
    return hipGetLastError();
}

hipError_t launch_gzip_members_heads(const GzipMembersArgs& a, hipStream_t stream) {
    if (a.nmembers == 0) return hipSuccess;
    const uint64_t g = a.nmembers < 65536u ? a.nmembers : 65536u;
    hipLaunchKernelGGL(gzm::k_gzm_heads, dim3((unsigned)g), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_gzip_members_judge(const GzipMembersArgs& a, hipStream_t stream) {
    using namespace gzm;
    const uint32_t ngroups = (uint32_t)((a.nmembers + JT - 1u) / JT);
    if (ngroups) hipLaunchKernelGGL(k_gzm_judge, dim3(ngroups), dim3(JT), 0, stream, a);
    hipLaunchKernelGGL(k_gzm_finish, dim3(1), dim3(256), 0, stream, a, ngroups);
    return hipGetLastError();
}

}  // namespace hdlz
