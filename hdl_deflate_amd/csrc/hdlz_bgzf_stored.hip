// hdlz_bgzf_stored.hip -- the BGZF writer that can fall back to a stored member (include/hdlz_bgzf_stored.h).
//
// k_bgzf_join_stored is k_join<true>'s pattern (hdlz_join.hip; restated here in a file of its own, not shared and not a third
// instantiation: DESIGN.md 4.6b records what sharing the look-back did to k_archive's schedule, and the existing kernels' code objects
// are held to the parent's): a workgroup takes a TILE of 256 consecutive rows by a ticket, scans the 256 member lengths, publishes its
// sum as one 64-bit word {state, value} and finds its base by a decoupled look-back over the tiles in front of it; then it writes the
// 256 offsets and copies its members, a wave per row, with 16-byte stores to 16-byte aligned destinations.  Three things differ:
//   - the member's length and its SOURCE are decided per row by THE MEMBER RULE of the header: the row's fixed block (member = L + 20
//     bytes) when that is usable and not longer than the stored form (n_b + 31 bytes), else the block's input bytes;
//   - the stored form's 23 bytes in front of the payload (HEADER(16), BSIZE, 01, LEN, NLEN) replace the fixed form's 18;
//   - the tile's count of stored members travels in the second of the PARTS words, which the BGZF form of k_join leaves unused, and
//     d_kind[b] is written by the thread that owns row b.
// The scratch is hdlz_join.hip's, word for word (join_work_bytes): ticket (+ pad), one look-back word and PARTS words per tile.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"

namespace hdlz {

constexpr uint32_t JT = 256;                             // rows per tile
constexpr uint64_t J_AGG = 1ull << 62, J_PFX = 2ull << 62, J_MASK = 3ull << 62;
constexpr uint32_t PARTS = 4;                            // words a tile leaves for the finish: lowest failed row, stored members, (unused), worst status
constexpr uint32_t FIXED_HEAD = bgzf::HEAD, STORED_HEAD = bgzf::HEAD + 5u;      // bytes in front of the member's payload
constexpr uint32_t STORED_MAX = bgzf::MEMBER_MAX - STORED_HEAD - bgzf::TAIL;    // 65505: the longest block a stored member holds
constexpr uint32_t KIND_BIT = 1u << 31;                  // s_body: the payload's length (at most 65536), and this bit for the stored form
__constant__ const uint8_t HEADER16[16] = {0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0};
__constant__ const uint8_t EOF_MEMBER[28] = {0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0, 0x1B, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

struct StoredArgs {
    const uint8_t* in;
    const uint64_t* in_off;      // nullable: then block b is the in_len bytes at in + b * in_pitch
    uint64_t in_pitch;
    uint32_t in_len;
    const uint8_t* rows;
    uint64_t pitch;
    const uint32_t* len;
    const uint32_t* status;
    uint64_t nblocks;
    const uint32_t* crc;
    uint8_t* file;
    uint64_t cap;
    uint64_t* off;
    uint8_t* kind;               // nullable
    uint32_t* ticket;            // scratch: ticket (+ pad), ...
    unsigned long long* desc;    // ... one look-back word per tile, ...
    uint32_t* part;              // ... PARTS words per tile
};

static __device__ __forceinline__ uint32_t wave_add(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
static __device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}
static __device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void k_bgzf_join_stored(StoredArgs a) {
    __shared__ uint32_t s_tile;
    __shared__ uint64_t s_wsum[4], s_base;
    __shared__ uint64_t s_off[JT];
    __shared__ uint32_t s_body[JT];                      // bytes of the member that come from the row or the input, and KIND_BIT
    __shared__ uint32_t s_part[4][PARTS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0u) s_tile = atomicAdd(a.ticket, 1u);
    __syncthreads();
    const uint32_t tile = s_tile;
    const uint64_t b = (uint64_t)tile * JT + tid;

    // ---- the member rule: the row's form and its member length
    uint32_t m = 0, body = 0, st = HDLZ_OK, bad = bgzf::NONE, stored = 0;
    if (b < a.nblocks) {
        st = a.status[b];
        const uint32_t n = a.len[b];
        const uint64_t nb = a.in_off ? a.in_off[b + 1] - a.in_off[b] : (uint64_t)a.in_len;
        if (st != HDLZ_OK && st != HDLZ_E_SHORT_INPUT) {}                                          // 1. the compressor's own failure
        else if (st == HDLZ_OK && (n < 8u || (uint64_t)n > a.pitch)) st = HDLZ_E_BAD_PARAM;        // 2. what is read of the row lies inside it
        else if (nb > STORED_MAX) st = HDLZ_E_OUT_CAPACITY;                                        // 3.
        else {
            const uint32_t stored_m = (uint32_t)nb + STORED_HEAD + bgzf::TAIL;
            const bool fixed = st == HDLZ_OK && n <= bgzf::MEMBER_MAX - 20u && n + 20u <= stored_m;      // 4. and 5.: a tie goes to the fixed form
            stored = fixed ? 0u : 1u;
            body = fixed ? n - 6u : (uint32_t)nb;
            m = fixed ? n + 20u : stored_m;
            st = HDLZ_OK;
        }
        if (st != HDLZ_OK) bad = tid;
        if (a.kind) a.kind[b] = (uint8_t)stored;
    }
    s_body[tid] = body | (stored ? KIND_BIT : 0u);
    {
        const uint32_t rf = wave_min(bad), rk = wave_add(stored), rt = wave_max(st);
        if (lane == 0u) { s_part[wave][0] = rf; s_part[wave][1] = rk; s_part[wave][2] = 0u; s_part[wave][3] = rt; }
    }
    // ---- exclusive scan of the tile's member lengths
    uint64_t v = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(v, o, 64);
        if (lane >= (uint32_t)o) v += t;
    }
    if (lane == 63u) s_wsum[wave] = v;
    __syncthreads();
    const uint64_t w0 = s_wsum[0], w1 = s_wsum[1], w2 = s_wsum[2], w3 = s_wsum[3];
    const uint64_t local = v - m + (wave > 0u ? w0 : 0ull) + (wave > 1u ? w1 : 0ull) + (wave > 2u ? w2 : 0ull);
    const uint64_t tsum = w0 + w1 + w2 + w3;
    if (tid < PARTS) {
        const uint32_t x0 = s_part[0][tid], x1 = s_part[1][tid], x2 = s_part[2][tid], x3 = s_part[3][tid];
        if (tid == 0u) {
            const uint32_t f = min(min(x0, x1), min(x2, x3));
            a.part[(size_t)PARTS * tile] = f == bgzf::NONE ? bgzf::NONE : tile * JT + f;
        } else a.part[(size_t)PARTS * tile + tid] = tid == 3u ? max(max(x0, x1), max(x2, x3)) : x0 + x1 + x2 + x3;
    }
    if (wave == 0u) {
        uint64_t base = 0;
        if (tile != 0u) {
            if (lane == 0u) __hip_atomic_store(&a.desc[tile], J_AGG | tsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int64_t t = (int64_t)tile - 1 - (int64_t)lane;        // lane 0 looks at the nearest tile
            for (;;) {
                uint64_t d = J_PFX;                                // (tiles in front of tile 0: an empty prefix)
                if (t >= 0) {
                    do { d = __hip_atomic_load(&a.desc[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while ((d & J_MASK) == 0ull);
                }
                const uint64_t pm = ballot64((d & J_MASK) == J_PFX);
                const uint32_t first = pm ? (uint32_t)__builtin_ctzll(pm) : 64u;      // the nearest published prefix among these 64
                uint64_t x = lane <= first ? (d & ~J_MASK) : 0ull;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
                base += x;
                if (pm) break;
                t -= 64;
            }
        }
        if (lane == 0u) {
            __hip_atomic_store(&a.desc[tile], J_PFX | (base + tsum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_base = base;
            if ((uint64_t)(tile + 1u) * JT >= a.nblocks) a.off[a.nblocks] = base + tsum;      // the last tile: where the EOF member goes
        }
    }
    __syncthreads();
    const uint64_t mine = s_base + local;
    if (b < a.nblocks) a.off[b] = mine;
    s_off[tid] = mine;
    __syncthreads();
    // ---- the copy: a wave per row, 64 rows each
    for (uint32_t r = wave * 64u; r < wave * 64u + 64u; r++) {
        const uint64_t rb = (uint64_t)tile * JT + r;
        if (rb >= a.nblocks) break;
        const uint64_t o0 = s_off[r];
        const uint32_t rn = (uint32_t)((r + 1u < JT ? s_off[r + 1u] : s_base + tsum) - o0);      // the member's length
        if (rn == 0u || o0 + rn > a.cap) continue;            // a failed row / a member that would end beyond the capacity
        typedef uint32_t v4 __attribute__((ext_vector_type(4)));
        typedef v4 __attribute__((aligned(1))) v4u;
        const bool is_stored = (s_body[r] & KIND_BIT) != 0u;
        const uint32_t bl = s_body[r] & ~KIND_BIT;            // rn = hl + bl + 8
        const uint32_t hl = is_stored ? STORED_HEAD : FIXED_HEAD;
        // stored: the block's n_b = bl input bytes; fixed: row[2 .. 2 + bl), the block as the compressor left it
        const uint8_t* src = is_stored ? a.in + (a.in_off ? a.in_off[rb] : rb * a.in_pitch) : a.rows + rb * a.pitch + 2u;
        uint8_t* dst = a.file + o0;
        if (lane < 16u) dst[lane] = HEADER16[lane];
        else if (lane < FIXED_HEAD) dst[lane] = (uint8_t)((rn - 1u) >> (8u * (lane - 16u)));      // BSIZE
        else if (lane < hl) {                                 // stored only: 01, LEN, NLEN
            const uint32_t w = bl | (~bl << 16);
            dst[lane] = lane == FIXED_HEAD ? (uint8_t)1u : (uint8_t)(w >> (8u * (lane - FIXED_HEAD - 1u)));
        } else if (lane < hl + bgzf::TAIL) {
            const uint32_t k = lane - hl;
            const uint32_t isize = a.in_off ? (uint32_t)(a.in_off[rb + 1] - a.in_off[rb]) : a.in_len;
            dst[hl + bl + k] = (uint8_t)((k < 4u ? a.crc[rb] : isize) >> (8u * (k & 3u)));
        }
        uint8_t* d2 = dst + hl;
        const uint32_t head = min(bl, (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(d2) & 15u)) & 15u));
        if (lane < head) d2[lane] = src[lane];
        const uint32_t chunks = (bl - head) >> 4;             // whole 16-byte chunks: no load leaves src[0 .. bl)
        for (uint32_t k = lane; k < chunks; k += 64u) *reinterpret_cast<v4*>(d2 + head + 16u * k) = *reinterpret_cast<const v4u*>(src + head + 16u * k);
        const uint32_t done = head + 16u * chunks;            // at most 15 bytes are left
        if (done + lane < bl) d2[done + lane] = src[done + lane];
    }
}

// one workgroup behind k_bgzf_join_stored: the tiles' worst status, lowest failed row and stored members, the EOF member, the record
__global__ __launch_bounds__(256) void k_bgzf_join_stored_finish(StoredArgs a, uint32_t ntiles, hdlz_bgzf_stored_result* result) {
    __shared__ uint32_t s_st[256], s_f[256];
    __shared__ uint64_t s_k[256];
    const uint32_t tid = threadIdx.x;
    uint32_t st = HDLZ_OK, f = bgzf::NONE;
    uint64_t k = 0;
    for (uint32_t t = tid; t < ntiles; t += 256u) {
        const uint32_t* q = a.part + (size_t)PARTS * t;
        st = max(st, q[3]); f = min(f, q[0]); k += q[1];
    }
    s_st[tid] = st; s_f[tid] = f; s_k[tid] = k;
    __syncthreads();
    for (uint32_t o = 128u; o > 0u; o >>= 1) {
        if (tid < o) { s_st[tid] = max(s_st[tid], s_st[tid + o]); s_f[tid] = min(s_f[tid], s_f[tid + o]); s_k[tid] += s_k[tid + o]; }
        __syncthreads();
    }
    st = s_st[0];
    if (a.nblocks == 0 && tid == 0u) a.off[0] = 0u;
    const uint64_t end = a.nblocks ? a.off[a.nblocks] : 0u;      // (the last tile wrote it, in front of this launch)
    const uint64_t total = end + sizeof(EOF_MEMBER);
    if (st == HDLZ_OK && total <= a.cap && tid < sizeof(EOF_MEMBER)) a.file[end + tid] = EOF_MEMBER[tid];
    if (tid != 0u) return;
    hdlz_bgzf_stored_result res;
    res.file_len = st != HDLZ_OK ? 0u : total;
    res.nstored = st != HDLZ_OK ? 0u : s_k[0];
    res.status = st != HDLZ_OK ? st : total > a.cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)HDLZ_OK;
    res.first_bad = s_f[0];
    *result = res;
}

hipError_t launch_bgzf_join_stored(const uint8_t* in, const uint64_t* in_off, uint64_t in_pitch, uint32_t in_len, const uint8_t* rows,
                                   uint64_t pitch, const uint32_t* len, const uint32_t* status, uint64_t nblocks, const uint32_t* crc,
                                   uint8_t* file, uint64_t cap, uint64_t* off, uint8_t* kind, hdlz_bgzf_stored_result* result, void* work,
                                   hipStream_t stream) {
    const uint64_t ntiles = (nblocks + JT - 1u) / JT;
    uint32_t* ws = static_cast<uint32_t*>(work);
    StoredArgs a{in, in_off, in_pitch, in_len, rows, pitch, len, status, nblocks, crc, file, cap, off, kind, ws,
                 reinterpret_cast<unsigned long long*>(ws + 2), ws + 2u + 2u * (size_t)ntiles};
    if (ntiles) {
        const hipError_t e = zero_words(ws, (uint32_t)(2u + 2u * ntiles), stream);      // the ticket and the look-back words
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_bgzf_join_stored, dim3((unsigned)ntiles), dim3(256), 0, stream, a);
        const hipError_t e2 = hipGetLastError();
        if (e2 != hipSuccess) return e2;
    }
    hipLaunchKernelGGL(k_bgzf_join_stored_finish, dim3(1), dim3(256), 0, stream, a, (uint32_t)ntiles, result);
    return hipGetLastError();
}

}  // namespace hdlz
