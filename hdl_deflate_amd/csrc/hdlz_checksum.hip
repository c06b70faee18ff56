// hdlz_checksum.hip -- the judging pass of hdlz_inflate_checked: Adler-32 of every decoded row, the zlib header and trailer of its
// stream, the verdict.  It runs behind the decode on the same stream (a kernel boundary: the rows are complete and visible) and reads
// every output byte once more.
//
// The arithmetic, its bounds and the frame test: hdlz_adler.h.
//
// Two mappings, chosen from the call's shape (judge_tiled):
//   rows   many rows of less than 64 KiB: ONE launch, 16 lanes per row (a 2 KiB row: 8 chunks per lane), the group's first lane writes the
//          verdict.  No scratch.
//   tiles  rows of 64 KiB and more: every row cut into 32 KiB tiles over the whole GPU, one workgroup each, (A, C) per tile in the
//          caller's scratch (8 bytes per 32 KiB of row capacity); a second launch, one workgroup per row, adds them and writes the verdict.
// Plain stores only.  Loads: 16 bytes at a time when d_out and out_pitch are multiples of 16 (dwords otherwise, and for a row's last
// partial chunk: only dwords that begin below out_len are loaded, so nothing beyond out_len rounded up to 4 -- inside the row, out_pitch
// is a multiple of 4 -- and bytes at or behind out_len are masked off).  Header and trailer: byte loads inside [0, end + 4) <= the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_adler.h"

namespace hdlz {
namespace chk {

constexpr uint32_t ROW_G = 16u;               // lanes per row of k_adler_rows
constexpr uint32_t SEG = 65536u;              // k_adler_rows: positions are taken relative to segments of this many bytes

struct Row {
    const uint8_t* z;           // the stream
    uint64_t len;               // its length
    uint32_t st, n, end;        // the decoder's status, out_len (0 unless the row is judged), where the final block ended
    bool judged;                // the decode succeeded and the trailer is there
};
__device__ __forceinline__ Row row_of(const JudgeArgs& a, uint64_t b) {
    Row r;
    uint64_t off;
    if (a.in_off) { off = a.in_off[b]; r.len = a.in_off[b + 1u] - off; }
    else { off = b * a.in_pitch; r.len = a.in_len; }
    r.z = a.in + off;
    r.st = a.status[b];
    r.end = a.in_used[b];
    r.judged = r.st == HDLZ_OK && (uint64_t)r.end + 4u <= r.len;
    const uint32_t cap = a.out_pitch > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)a.out_pitch;
    const uint32_t n = a.out_len[b];
    r.n = r.judged ? (n < cap ? n : cap) : 0u;
    return r;
}
// one lane: the verdict of row b from its sums (both below ADLER_MOD), in the order of precedence of include/hdlz.h
__device__ __forceinline__ void verdict(const JudgeArgs& a, uint64_t b, const Row& r, uint32_t A, uint32_t C) {
    uint32_t st = r.st, used = 0u, ad = 0u;
    if (st == HDLZ_OK && !r.judged) st = HDLZ_E_NO_EOF;                          // the trailer is cut
    else if (st == HDLZ_OK) {
        ad = adler32_from(A, C, r.n);
        used = r.end + 4u;
        const uint32_t cmf = r.z[0], flg = r.z[1], want = load_be32(r.z + r.end);
        if (HDLZ_ZLIB_HEADER_BAD(cmf, flg)) st = HDLZ_E_BAD_HEADER;
        else if (want != ad) st = HDLZ_E_BAD_CHECKSUM;
    }
    if (st != HDLZ_OK) { a.status[b] = st; a.out_len[b] = 0u; }
    a.in_used[b] = used;
    if (a.adler) a.adler[b] = ad;
}

// ---- many short rows: 16 lanes per row, one launch
template <bool A16>
__global__ __launch_bounds__(256) void k_adler_rows(JudgeArgs a) {
    const uint32_t l = threadIdx.x & (ROW_G - 1u);
    const uint64_t per = 256u / ROW_G, stride = (uint64_t)gridDim.x * per;
    for (uint64_t b = (uint64_t)blockIdx.x * per + threadIdx.x / ROW_G; b < a.nstreams; b += stride) {
        const Row r = row_of(a, b);
        const uint8_t* __restrict__ out = a.out + b * a.out_pitch;
        uint64_t A64 = 0, C64 = 0;
        for (uint64_t seg = 0; seg < r.n; seg += SEG) {
            const uint32_t segn = r.n - seg < SEG ? (uint32_t)(r.n - seg) : SEG;
            uint32_t a32 = 0;
            uint64_t c64 = 0;
#pragma unroll 4
            for (uint32_t q = 16u * l; q < segn; q += 16u * ROW_G) {
                uint32_t sx, w;
                sums16(load_chunk<A16, true>(out + seg, q, segn), sx, w);
                a32 += sx;
                c64 += (uint64_t)(__umul24(q, sx) + w);
            }
            A64 += a32;
            C64 += (uint64_t)(uint32_t)(seg % ADLER_MOD) * a32 + c64;
        }
        uint32_t Ar = (uint32_t)(A64 % ADLER_MOD), Cr = (uint32_t)(C64 % ADLER_MOD);
#pragma unroll
        for (int ofs = (int)ROW_G / 2; ofs > 0; ofs >>= 1) { Ar += (uint32_t)__shfl_xor((int)Ar, ofs, (int)ROW_G); Cr += (uint32_t)__shfl_xor((int)Cr, ofs, (int)ROW_G); }
        if (l == 0u) verdict(a, b, r, Ar % ADLER_MOD, Cr % ADLER_MOD);
    }
}

// ---- few long rows: (A, C) of every 32 KiB tile, positions relative to the tile
template <bool A16>
__global__ __launch_bounds__(64 * ADLER_TILE_WAVES) void k_adler_tiles(JudgeArgs a, uint32_t tiles_per_row) {
    __shared__ uint32_t sa[ADLER_TILE_WAVES], sc[ADLER_TILE_WAVES];
    const uint64_t b = blockIdx.x / tiles_per_row;
    const uint32_t t = blockIdx.x % tiles_per_row;
    const Row r = row_of(a, b);
    if ((uint64_t)t * ADLER_TILE >= r.n) return;                                   // (the whole workgroup: nothing of this tile is output)
    const uint32_t tn = r.n - t * ADLER_TILE < ADLER_TILE ? r.n - t * ADLER_TILE : ADLER_TILE;
    const uint8_t* __restrict__ p = a.out + b * a.out_pitch + (uint64_t)t * ADLER_TILE;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t a32 = 0, c32 = 0;
#pragma unroll
    for (uint32_t k = 0; k < ADLER_TILE_STEPS; k++) {
        // (the order is free, so it is rotated by the tile index: the tiles of one long row are all 32 KiB aligned and thousands of workgroups
        //  would walk them in the same order.  Measured 60.5 -> 58.1 us on a 256 MiB row: inside the spread, profiles/checked_inflate.txt)
        const uint32_t q = (((wave + (t >> 3)) % ADLER_TILE_WAVES) * ADLER_TILE_STEPS + ((k + t) % ADLER_TILE_STEPS)) * 1024u + 16u * lane;
        if (q < tn) {
            uint32_t sx, w;
            sums16(load_chunk<A16, true>(p, q, tn), sx, w);
            a32 += sx;
            c32 += __umul24(q, sx) + w;
        }
    }
    c32 %= ADLER_MOD;
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) { a32 += (uint32_t)__shfl_xor((int)a32, ofs, 64); c32 += (uint32_t)__shfl_xor((int)c32, ofs, 64); }
    if (lane == 0u) { sa[wave] = a32; sc[wave] = c32; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t A = 0, C = 0;
#pragma unroll
        for (uint32_t k = 0; k < ADLER_TILE_WAVES; k++) { A += sa[k]; C += sc[k]; }
        a.work[b * tiles_per_row + t] = make_uint2(A % ADLER_MOD, C % ADLER_MOD);
    }
}
// ... added per row (one workgroup: a 256 MiB row has 8192 tiles), and the verdict
constexpr uint32_t FIN_WAVES = 4u;
__global__ __launch_bounds__(64 * FIN_WAVES) void k_adler_finish(JudgeArgs a, uint32_t tiles_per_row) {
    __shared__ uint32_t sa[FIN_WAVES], sc[FIN_WAVES];
    const uint64_t b = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const Row r = row_of(a, b);
    const uint32_t nt = (uint32_t)(((uint64_t)r.n + ADLER_TILE - 1u) / ADLER_TILE);
    uint64_t A64 = 0, C64 = 0;
#pragma unroll 4
    for (uint32_t t = threadIdx.x; t < nt; t += 64u * FIN_WAVES) {
        const uint2 s = a.work[b * tiles_per_row + t];
        fold_tile(A64, C64, t, s.x, s.y);
    }
    uint32_t Ar = (uint32_t)(A64 % ADLER_MOD), Cr = (uint32_t)(C64 % ADLER_MOD);
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) { Ar += (uint32_t)__shfl_xor((int)Ar, ofs, 64); Cr += (uint32_t)__shfl_xor((int)Cr, ofs, 64); }
    if (lane == 0u) { sa[wave] = Ar; sc[wave] = Cr; }
    __syncthreads();                                                       // (also: every thread has read the row's words before the verdict overwrites them)
    if (threadIdx.x == 0u) {
        uint32_t A = 0, C = 0;
#pragma unroll
        for (uint32_t k = 0; k < FIN_WAVES; k++) { A += sa[k]; C += sc[k]; }
        verdict(a, b, r, A % ADLER_MOD, C % ADLER_MOD);
    }
}

// rows of at least two tiles go over the whole GPU (as long as the tiles of the call can be counted in a grid)
__host__ inline uint32_t tiles_of(uint64_t out_pitch) {
    const uint64_t cap = out_pitch > 0xFFFFFFFFull ? 0xFFFFFFFFull : out_pitch;
    return (uint32_t)((cap + ADLER_TILE - 1u) / ADLER_TILE);
}
__host__ inline bool judge_tiled(uint64_t nstreams, uint64_t out_pitch) {
    return out_pitch >= 2ull * ADLER_TILE && nstreams <= 0x7FFFFFFFull / tiles_of(out_pitch);
}

}  // namespace chk

size_t judge_work_bytes(uint64_t nstreams, uint64_t out_pitch) {
    if (nstreams == 0 || !chk::judge_tiled(nstreams, out_pitch)) return 0;
    return round256((size_t)nstreams * chk::tiles_of(out_pitch) * sizeof(uint2));
}

hipError_t launch_judge(const JudgeArgs& a, hipStream_t stream) {
    using namespace chk;
    if (a.nstreams == 0) return hipSuccess;
    const bool a16 = ((reinterpret_cast<uintptr_t>(a.out) | a.out_pitch) & 15u) == 0u;
    if (judge_tiled(a.nstreams, a.out_pitch)) {
        const uint32_t tpr = tiles_of(a.out_pitch);
        const dim3 grid((unsigned)(a.nstreams * tpr)), block(64 * ADLER_TILE_WAVES);
        if (a16) hipLaunchKernelGGL(k_adler_tiles<true>, grid, block, 0, stream, a, tpr);
        else hipLaunchKernelGGL(k_adler_tiles<false>, grid, block, 0, stream, a, tpr);
        hipLaunchKernelGGL(k_adler_finish, dim3((unsigned)a.nstreams), dim3(64 * FIN_WAVES), 0, stream, a, tpr);
        return hipGetLastError();
    }
    const uint64_t per = 256u / ROW_G, want = (a.nstreams + per - 1u) / per;
    const dim3 grid((unsigned)(want < (1u << 22) ? want : (1u << 22)));        // (beyond 2^26 rows a workgroup takes several)
    if (a16) hipLaunchKernelGGL(k_adler_rows<true>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_adler_rows<false>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hdlz
