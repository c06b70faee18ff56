// hdlz_checksum.hip -- the judging pass of hdlz_inflate_checked: Adler-32 of every decoded row, the zlib header and trailer of its
// stream, the verdict.  It runs behind the decode on the same stream (a kernel boundary: the rows are complete and visible) and reads
// every output byte once more.
//
// Arithmetic.  With A = sum x_p and C = sum p * x_p over the n bytes of a row (p = 0 .. n-1),
//     s1 = (1 + A) mod 65521,   s2 = (n + n * A - C) mod 65521                    (byte p is counted n - p times in s2)
// Both sums are order-free: the 16-byte chunks of a row are summed by whatever lane gets them and added, no ordered combine.  Per chunk
// at row position p0: Sx = sum of its bytes (4 x v_sad_u8), W = sum j * x_j (4 x v_dot4_u32_u8 against the weights 0 .. 15), and
// C += p0 * Sx + W with p0 taken relative to a base that is folded in mod 65521 later (base * A_part).
//
// Bounds (a row of up to 2^32 - 512 bytes, what the decoders' capacity clamp allows; the ABI's streams end below 2^28):
//   a chunk:            Sx <= 16 * 255 = 4080, W <= 255 * 120 = 30600
//   k_adler_tiles:      positions relative to the 32 KiB tile, q < 32768: a term is <= 32767 * 4080 + 30600 < 1.34e8, a lane adds 8 of
//                       them: < 1.07e9 < 2^32; Sx: 8 * 4080.  Reduced mod 65521 per lane, 64 lanes and 4 waves of values < 65521 (C) and
//                       < 2.1e6 (A) added in 32 bits.
//   k_adler_rows:       positions relative to a 64 KiB segment, q < 65536: a term is <= 65535 * 4080 + 30600 < 2^28 (q and Sx below 2^24: the
//                       24-bit multiply is exact), a lane adds 256 of them per segment into 64 bits; Sx per segment <= 256 * 4080 < 2^21.  A segment folds
//                       (base mod 65521) * A_seg + C_seg < 65521 * 2^21 + 2^36 < 2^38 into 64 bits, at most 2^16 segments per row: < 2^54.
//   k_adler_finish:     per tile (t * 32768 mod 65521) * A_t + C_t < 2^32, at most 2^17 tiles per row, 64 bits.
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

namespace hdlz {
namespace chk {

constexpr uint32_t MOD = 65521u;
constexpr uint32_t TILE = 32768u;             // bytes per workgroup of k_adler_tiles: 4 waves x 8 steps x 64 lanes x 16 bytes
constexpr uint32_t TILE_WAVES = 4u, TILE_STEPS = 8u;
static_assert(TILE == TILE_WAVES * TILE_STEPS * 1024u, "a tile is what its workgroup's waves cover");
constexpr uint32_t ROW_G = 16u;               // lanes per row of k_adler_rows
constexpr uint32_t SEG = 65536u;              // k_adler_rows: positions are taken relative to segments of this many bytes
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Sx and W of one chunk
__device__ __forceinline__ void sums16(const u32x4 v, uint32_t& sx, uint32_t& w) {
    sx = __builtin_amdgcn_sad_u8(v.x, 0u, 0u);
    sx = __builtin_amdgcn_sad_u8(v.y, 0u, sx);
    sx = __builtin_amdgcn_sad_u8(v.z, 0u, sx);
    sx = __builtin_amdgcn_sad_u8(v.w, 0u, sx);
    w = __builtin_amdgcn_udot4(v.x, 0x03020100u, 0u, false);
    w = __builtin_amdgcn_udot4(v.y, 0x07060504u, w, false);
    w = __builtin_amdgcn_udot4(v.z, 0x0B0A0908u, w, false);
    w = __builtin_amdgcn_udot4(v.w, 0x0F0E0D0Cu, w, false);
}
// the low min(cnt, 4) bytes of a dword (cnt as a signed count: <= 0 keeps nothing)
__device__ __forceinline__ uint32_t keep_bytes(uint32_t d, int32_t cnt) {
    return cnt >= 4 ? d : cnt <= 0 ? 0u : d & ((1u << (8u * (uint32_t)cnt)) - 1u);
}
// the chunk at byte q of `p` (q a multiple of 16, below n): bytes at or behind n read as zero and are not loaded beyond the dword that
// holds byte n - 1
template <bool A16>
__device__ __forceinline__ u32x4 load_chunk(const uint8_t* __restrict__ p, uint32_t q, uint32_t n) {
    u32x4 v = {0u, 0u, 0u, 0u};
    const uint32_t* d = reinterpret_cast<const uint32_t*>(p + q);
    if (q + 16u <= n) {
        if constexpr (A16) v = *reinterpret_cast<const u32x4*>(d);
        else { v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3]; }
    } else {
        const int32_t cnt = (int32_t)(n - q);                 // 1 .. 15
        v.x = keep_bytes(d[0], cnt);
        if (cnt > 4) v.y = keep_bytes(d[1], cnt - 4);
        if (cnt > 8) v.z = keep_bytes(d[2], cnt - 8);
        if (cnt > 12) v.w = keep_bytes(d[3], cnt - 12);
    }
    return v;
}

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
// one lane: the verdict of row b from its sums (both below MOD), in the order of precedence of include/hdlz.h
__device__ __forceinline__ void verdict(const JudgeArgs& a, uint64_t b, const Row& r, uint32_t A, uint32_t C) {
    uint32_t st = r.st, used = 0u, ad = 0u;
    if (st == HDLZ_OK && !r.judged) st = HDLZ_E_NO_EOF;                          // the trailer is cut
    else if (st == HDLZ_OK) {
        const uint32_t nm = r.n % MOD;
        const uint32_t s1 = (1u + A) % MOD;
        const uint32_t s2 = (uint32_t)(((uint64_t)nm + (uint64_t)nm * A + MOD - C) % MOD);
        ad = (s2 << 16) | s1;
        used = r.end + 4u;
        const uint32_t cmf = r.z[0], flg = r.z[1];
        const uint8_t* t = r.z + r.end;
        const uint32_t want = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | (uint32_t)t[3];
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (cmf * 256u + flg) % 31u != 0u || (flg & 0x20u) != 0u) st = HDLZ_E_BAD_HEADER;
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
                sums16(load_chunk<A16>(out + seg, q, segn), sx, w);
                a32 += sx;
                c64 += (uint64_t)(__umul24(q, sx) + w);
            }
            A64 += a32;
            C64 += (uint64_t)(uint32_t)(seg % MOD) * a32 + c64;
        }
        uint32_t Ar = (uint32_t)(A64 % MOD), Cr = (uint32_t)(C64 % MOD);
#pragma unroll
        for (int ofs = (int)ROW_G / 2; ofs > 0; ofs >>= 1) { Ar += (uint32_t)__shfl_xor((int)Ar, ofs, (int)ROW_G); Cr += (uint32_t)__shfl_xor((int)Cr, ofs, (int)ROW_G); }
        if (l == 0u) verdict(a, b, r, Ar % MOD, Cr % MOD);
    }
}

// ---- few long rows: (A, C) of every 32 KiB tile, positions relative to the tile
template <bool A16>
__global__ __launch_bounds__(64 * TILE_WAVES) void k_adler_tiles(JudgeArgs a, uint32_t tiles_per_row) {
    __shared__ uint32_t sa[TILE_WAVES], sc[TILE_WAVES];
    const uint64_t b = blockIdx.x / tiles_per_row;
    const uint32_t t = blockIdx.x % tiles_per_row;
    const Row r = row_of(a, b);
    if ((uint64_t)t * TILE >= r.n) return;                                   // (the whole workgroup: nothing of this tile is output)
    const uint32_t tn = r.n - t * TILE < TILE ? r.n - t * TILE : TILE;
    const uint8_t* __restrict__ p = a.out + b * a.out_pitch + (uint64_t)t * TILE;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t a32 = 0, c32 = 0;
#pragma unroll
    for (uint32_t k = 0; k < TILE_STEPS; k++) {
        // (the order is free, so it is rotated by the tile index: the tiles of one long row are all 32 KiB aligned and thousands of workgroups
        //  would walk them in the same order.  Measured 60.5 -> 58.1 us on a 256 MiB row: inside the spread, profiles/checked_inflate.txt)
        const uint32_t q = (((wave + (t >> 3)) % TILE_WAVES) * TILE_STEPS + ((k + t) % TILE_STEPS)) * 1024u + 16u * lane;
        if (q < tn) {
            uint32_t sx, w;
            sums16(load_chunk<A16>(p, q, tn), sx, w);
            a32 += sx;
            c32 += __umul24(q, sx) + w;
        }
    }
    c32 %= MOD;
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) { a32 += (uint32_t)__shfl_xor((int)a32, ofs, 64); c32 += (uint32_t)__shfl_xor((int)c32, ofs, 64); }
    if (lane == 0u) { sa[wave] = a32; sc[wave] = c32; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t A = 0, C = 0;
#pragma unroll
        for (uint32_t k = 0; k < TILE_WAVES; k++) { A += sa[k]; C += sc[k]; }
        a.work[b * tiles_per_row + t] = make_uint2(A % MOD, C % MOD);
    }
}
// ... added per row (one workgroup: a 256 MiB row has 8192 tiles), and the verdict
constexpr uint32_t FIN_WAVES = 4u;
__global__ __launch_bounds__(64 * FIN_WAVES) void k_adler_finish(JudgeArgs a, uint32_t tiles_per_row) {
    __shared__ uint32_t sa[FIN_WAVES], sc[FIN_WAVES];
    const uint64_t b = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const Row r = row_of(a, b);
    const uint32_t nt = (uint32_t)(((uint64_t)r.n + TILE - 1u) / TILE);
    uint64_t A64 = 0, C64 = 0;
#pragma unroll 4
    for (uint32_t t = threadIdx.x; t < nt; t += 64u * FIN_WAVES) {
        const uint2 s = a.work[b * tiles_per_row + t];
        const uint32_t base = ((t % MOD) * (TILE % MOD)) % MOD;           // t * TILE mod 65521 (t < 2^17: the product stays below 2^32)
        A64 += s.x;
        C64 += (uint64_t)base * s.x + s.y;
    }
    uint32_t Ar = (uint32_t)(A64 % MOD), Cr = (uint32_t)(C64 % MOD);
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) { Ar += (uint32_t)__shfl_xor((int)Ar, ofs, 64); Cr += (uint32_t)__shfl_xor((int)Cr, ofs, 64); }
    if (lane == 0u) { sa[wave] = Ar; sc[wave] = Cr; }
    __syncthreads();                                                       // (also: every thread has read the row's words before the verdict overwrites them)
    if (threadIdx.x == 0u) {
        uint32_t A = 0, C = 0;
#pragma unroll
        for (uint32_t k = 0; k < FIN_WAVES; k++) { A += sa[k]; C += sc[k]; }
        verdict(a, b, r, A % MOD, C % MOD);
    }
}

// rows of at least two tiles go over the whole GPU (as long as the tiles of the call can be counted in a grid)
__host__ inline uint32_t tiles_of(uint64_t out_pitch) {
    const uint64_t cap = out_pitch > 0xFFFFFFFFull ? 0xFFFFFFFFull : out_pitch;
    return (uint32_t)((cap + TILE - 1u) / TILE);
}
__host__ inline bool judge_tiled(uint64_t nstreams, uint64_t out_pitch) {
    return out_pitch >= 2ull * TILE && nstreams <= 0x7FFFFFFFull / tiles_of(out_pitch);
}

}  // namespace chk

size_t judge_work_bytes(uint64_t nstreams, uint64_t out_pitch) {
    if (nstreams == 0 || !chk::judge_tiled(nstreams, out_pitch)) return 0;
    return ((size_t)nstreams * chk::tiles_of(out_pitch) * sizeof(uint2) + 255u) & ~(size_t)255u;
}

hipError_t launch_judge(const JudgeArgs& a, hipStream_t stream) {
    using namespace chk;
    if (a.nstreams == 0) return hipSuccess;
    const bool a16 = ((reinterpret_cast<uintptr_t>(a.out) | a.out_pitch) & 15u) == 0u;
    if (judge_tiled(a.nstreams, a.out_pitch)) {
        const uint32_t tpr = tiles_of(a.out_pitch);
        const dim3 grid((unsigned)(a.nstreams * tpr)), block(64 * TILE_WAVES);
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
