// hdlz_bgzf_stored.hip -- the BGZF writer: hdlz_bgzf_join_ws (include/hdlz_bgzf.h) and hdlz_bgzf_join_stored_ws, which can
// fall back to a stored member (include/hdlz_bgzf_stored.h).
//
// k_bgzf_join<STORED> is a tile join (hdlz_frame.h): a workgroup takes a tile of 256 consecutive rows by a ticket, scans the 256 member
// lengths, finds its base by the decoupled look-back, writes the 256 offsets and copies its members, a wave per row, with 16-byte
// stores to 16-byte aligned destinations.  A member is the 16 header bytes, BSIZE, the payload, CRC-32 and ISIZE; every member is a
// gzip member of its own, so the row's block keeps BFINAL = 1 and the first member starts at 0.  The two instances differ in THE
// MEMBER RULE, which decides per row the member's length and the payload's source:
//   STORED = false   the row's fixed block, row[2 .. n - 4): member = n + 20 bytes.  A row that would not fit a member fails with
//                    HDLZ_E_OUT_CAPACITY; a.in, a.in_pitch and a.kind are not used.
//   STORED = true    the rule of include/hdlz_bgzf_stored.h: the fixed block when that is usable and not longer than the stored form
//                    (n_b + 31 bytes), else the block's input bytes behind 01, LEN, NLEN (23 bytes in front of the payload where the
//                    fixed form has 18); d_kind[b] is written by the thread that owns row b.
// Of the tile's PARTS words the first holds the lowest failed row (NONE: none), the second the tile's count of stored members, the
// last the worst status; k_bgzf_join_finish (one workgroup) reduces them and writes the EOF member and either result record.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_frame.h"

namespace hdlz {

constexpr uint32_t FIXED_HEAD = bgzf::HEAD, STORED_HEAD = bgzf::HEAD + 5u;      // bytes in front of the member's payload
constexpr uint32_t STORED_MAX = bgzf::MEMBER_MAX - STORED_HEAD - bgzf::TAIL;    // 65505: the longest block a stored member holds
constexpr uint32_t KIND_BIT = 1u << 31;                  // s_body: the payload's length (at most 65536), and this bit for the stored form

template <bool STORED>
__global__ __launch_bounds__(256) void k_bgzf_join(BgzfJoinArgs a) {
    __shared__ uint32_t s_tile;
    __shared__ uint64_t s_wsum[4], s_base;
    __shared__ uint64_t s_off[JT];
    __shared__ uint32_t s_body[JT];                      // bytes of the member that come from the row or the input, and KIND_BIT
    __shared__ uint32_t s_part[4][PARTS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0u) s_tile = atomicAdd(a.w.ticket, 1u);
    __syncthreads();
    const uint32_t tile = s_tile;
    const uint64_t b = (uint64_t)tile * JT + tid;

    // ---- the member rule: the row's form and its member length
    uint32_t m = 0, body = 0, st = HDLZ_OK, bad = NONE, stored = 0;
    if (b < a.nblocks) {
        st = a.status[b];
        const uint32_t n = a.len[b];
        const uint64_t nb = a.in_off ? a.in_off[b + 1] - a.in_off[b] : (uint64_t)a.in_len;
        if constexpr (STORED) {
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
        } else {
            if (st == HDLZ_OK && (n < 8u || (uint64_t)n > a.pitch)) st = HDLZ_E_BAD_PARAM;      // 78 9C, at least 03 00, Adler-32: what is read below lies inside the row
            else if (st == HDLZ_OK && (n > bgzf::MEMBER_MAX - 20u || nb > bgzf::MEMBER_MAX)) st = HDLZ_E_OUT_CAPACITY;
            if (st == HDLZ_OK) {
                body = n - 6u;
                m = body + FIXED_HEAD + bgzf::TAIL;
            } else bad = tid;
        }
    }
    s_body[tid] = body | (stored ? KIND_BIT : 0u);
    {
        const uint32_t rf = wave_min(bad), rk = wave_add(stored), rt = wave_max(st);
        if (lane == 0u) { s_part[wave][0] = rf; s_part[wave][1] = rk; s_part[wave][2] = 0u; s_part[wave][3] = rt; }
    }
    uint64_t tsum;
    const uint64_t local = tile_scan(m, lane, wave, s_wsum, tsum);
    if (tid < PARTS) {
        const uint32_t x0 = s_part[0][tid], x1 = s_part[1][tid], x2 = s_part[2][tid], x3 = s_part[3][tid];
        if (tid == 0u) {
            const uint32_t f = min(min(x0, x1), min(x2, x3));
            a.w.part[(size_t)PARTS * tile] = f == NONE ? NONE : tile * JT + f;
        } else a.w.part[(size_t)PARTS * tile + tid] = tid == 3u ? max(max(x0, x1), max(x2, x3)) : x0 + x1 + x2 + x3;
    }
    if (wave == 0u) {
        const uint64_t base = tile_lookback(a.w.desc, tile, tsum, lane);
        if (lane == 0u) {
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
        const bool is_stored = STORED && (s_body[r] & KIND_BIT) != 0u;
        const uint32_t bl = s_body[r] & ~KIND_BIT;            // rn = hl + bl + 8
        const uint32_t hl = is_stored ? STORED_HEAD : FIXED_HEAD;
        // stored: the block's n_b = bl input bytes; fixed: row[2 .. 2 + bl), the block as the compressor left it
        const uint8_t* src = is_stored ? a.in + (a.in_off ? a.in_off[rb] : rb * a.in_pitch) : a.rows + rb * a.pitch + 2u;
        uint8_t* dst = a.file + o0;
        if (lane < 16u) dst[lane] = bgzf::HEADER[lane];
        else if (lane < FIXED_HEAD) dst[lane] = (uint8_t)((rn - 1u) >> (8u * (lane - 16u)));      // BSIZE
        else if (lane < hl) {                                 // stored only: 01, LEN, NLEN
            const uint32_t w = bl | (~bl << 16);
            dst[lane] = lane == FIXED_HEAD ? (uint8_t)1u : (uint8_t)(w >> (8u * (lane - FIXED_HEAD - 1u)));
        } else if (lane < hl + bgzf::TAIL) {
            const uint32_t k = lane - hl;
            const uint32_t isize = a.in_off ? (uint32_t)(a.in_off[rb + 1] - a.in_off[rb]) : a.in_len;
            dst[hl + bl + k] = (uint8_t)((k < 4u ? a.crc[rb] : isize) >> (8u * (k & 3u)));
        }
        copy_to_aligned16(dst + hl, src, bl, lane, 64u);
    }
}

// one workgroup behind k_bgzf_join: the tiles' worst status, lowest failed row and stored members, the EOF member, and the record of
// the entry point: `result` or `stored_result`, the other is null
__global__ __launch_bounds__(256) void k_bgzf_join_finish(BgzfJoinArgs a, uint32_t ntiles, hdlz_bgzf_join_result* result,
                                                          hdlz_bgzf_stored_result* stored_result) {
    __shared__ uint32_t s_st[256], s_f[256];
    __shared__ uint64_t s_k[256];
    const uint32_t tid = threadIdx.x;
    uint32_t st = HDLZ_OK, f = NONE;
    uint64_t k = 0;
    for (uint32_t t = tid; t < ntiles; t += 256u) {
        const uint32_t* q = a.w.part + (size_t)PARTS * t;
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
    const uint64_t total = end + sizeof(bgzf::EOF_MEMBER);
    if (st == HDLZ_OK && total <= a.cap && tid < sizeof(bgzf::EOF_MEMBER)) a.file[end + tid] = bgzf::EOF_MEMBER[tid];
    if (tid != 0u) return;
    const uint64_t file_len = st != HDLZ_OK ? 0u : total;
    const uint32_t status = st != HDLZ_OK ? st : total > a.cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)HDLZ_OK;
    if (stored_result) *stored_result = hdlz_bgzf_stored_result{file_len, st != HDLZ_OK ? 0u : s_k[0], status, s_f[0]};
    else *result = hdlz_bgzf_join_result{file_len, status, s_f[0]};
}

template <bool STORED>
static hipError_t launch_writer(BgzfJoinArgs a, hdlz_bgzf_join_result* result, hdlz_bgzf_stored_result* stored_result, void* work, hipStream_t stream) {
    a.w = join_work(work, a.nblocks);
    return launch_tile_join(k_bgzf_join<STORED>, a, stream, [&](uint32_t ntiles) {
        return launch(k_bgzf_join_finish, dim3(1), dim3(256), stream, a, ntiles, result, stored_result);
    });
}
hipError_t launch_bgzf_join(BgzfJoinArgs a, hdlz_bgzf_join_result* result, void* work, hipStream_t stream) {
    return launch_writer<false>(a, result, nullptr, work, stream);
}
hipError_t launch_bgzf_join_stored(BgzfJoinArgs a, hdlz_bgzf_stored_result* result, void* work, hipStream_t stream) {
    return launch_writer<true>(a, nullptr, result, work, stream);
}

}  // namespace hdlz
