// hdlz_unjoin.hip -- what hdlz_unjoin_ws (include/hdlz_unjoin.h) runs around the member decode: the index checks in front
// of it, the Adler-32 of the flat output and the judgement of every member and of the stream's frame behind it.
//
// The decode itself is the member view of the three batch decoders (hdlz_device.h: MemberArgs).  A decoder trusts its index words,
// so k_unjoin_index looks at them first: a member whose words are unusable, or whose first block is not a fixed one, gets its status
// here and the decoders leave it alone.  Behind the decode k_unjoin_tiles sums the CONTIGUOUS output in 32 KiB tiles over the whole GPU
// (the tile loop of k_adler_tiles, unrotated; chunk sums, tail rule and bounds: hdlz_adler.h -- out_cap may be any number, so nothing
// at or behind the total is loaded),
// k_unjoin_judge compares every member's decoded length with its slot and looks for the sync marker behind the END BIT the decoder
// left (the first bit behind the end-of-block code, counted from two bytes in front of the member), and k_unjoin_finish, one
// workgroup, reduces the tiles and the verdicts, reads the final empty block and the trailer and writes the record.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_adler.h"
#include "hdlz_crc32.h"
#include "hdlz_frame.h"

namespace hdlz {
namespace unj {

constexpr uint64_t MEMBER_MAX = 1ull << 28;   // bit positions are 32-bit in the decoders

// member b's slot of the output: [o, e) -- the caller checks what it relies on
__device__ __forceinline__ void slot_of(const UnjoinArgs& a, uint64_t b, uint64_t& o, uint64_t& e) {
    if (a.out_off) { o = a.out_off[b]; e = a.out_off[b + 1]; }
    else { o = b * (uint64_t)a.out_len; e = o + a.out_len; }
}
// the length of the output as the index states it, never beyond the capacity (a member the index checks refused may say anything)
__device__ __forceinline__ uint64_t total_of(const UnjoinArgs& a) {
    const uint64_t t = a.nmembers == 0 ? 0ull : a.out_off ? a.out_off[a.nmembers] : a.nmembers * (uint64_t)a.out_len;
    return t < a.out_cap ? t : a.out_cap;
}

// ---- in front of the decode: one thread per member, check 1 of the header and the first block's type
__global__ __launch_bounds__(JT) void k_unjoin_index(UnjoinArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * JT + threadIdx.x;
    if (b >= a.nmembers) return;
    const uint64_t lo = a.off[b], hi = a.off[b + 1];
    // (a member that ends inside the stream can be read; whether the frame's last six bytes are there is the stream's own check)
    bool bad = hi < lo || hi - lo < 5u || hi - lo >= MEMBER_MAX || hi > a.in_len;
    uint64_t o, e;
    slot_of(a, b, o, e);
    bad = bad || e < o || (o & 3u) != 0u || e > a.out_cap || (b == 0u && o != 0u);
    uint32_t st = bad ? (uint32_t)HDLZ_E_BAD_PARAM : (uint32_t)HDLZ_OK;
    if (!bad && ((a.in[lo] >> 1) & 3u) != 1u) st = HDLZ_E_BAD_BTYPE;       // (lo < hi <= in_len)
    a.status[b] = st;
    a.len[b] = 0u;
    a.end_bit[b] = 0u;
}

// ---- behind the decode: (A, C) of every 32 KiB tile of out[0 .. total), positions relative to the tile; (0, 0) for the tiles behind it
template <bool A16>
__global__ __launch_bounds__(64 * ADLER_TILE_WAVES) void k_unjoin_tiles(UnjoinArgs a, uint32_t ntiles) {
    __shared__ uint32_t sa[ADLER_TILE_WAVES], sc[ADLER_TILE_WAVES];
    const uint64_t total = total_of(a);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = (uint64_t)t * ADLER_TILE;
        uint32_t a32 = 0, c32 = 0;
        if (base < total) {
            const uint32_t tn = total - base < ADLER_TILE ? (uint32_t)(total - base) : ADLER_TILE;
            const uint8_t* __restrict__ p = a.out + base;
#pragma unroll
            for (uint32_t k = 0; k < ADLER_TILE_STEPS; k++) {
                const uint32_t q = (wave * ADLER_TILE_STEPS + k) * 1024u + 16u * lane;
                if (q < tn) {
                    uint32_t sx, w;
                    sums16(load_chunk<A16, false>(p, q, tn), sx, w);
                    a32 += sx;
                    c32 += __umul24(q, sx) + w;
                }
            }
            c32 %= ADLER_MOD;
#pragma unroll
            for (int ofs = 32; ofs > 0; ofs >>= 1) { a32 += (uint32_t)__shfl_xor((int)a32, ofs, 64); c32 += (uint32_t)__shfl_xor((int)c32, ofs, 64); }
        }
        if (lane == 0u) { sa[wave] = a32; sc[wave] = c32; }
        __syncthreads();
        if (threadIdx.x == 0u) {
            uint32_t A = 0, C = 0;
#pragma unroll
            for (uint32_t k = 0; k < ADLER_TILE_WAVES; k++) { A += sa[k]; C += sc[k]; }
            a.tiles[t] = make_uint2(A % ADLER_MOD, C % ADLER_MOD);
        }
        __syncthreads();
    }
}

// ---- one thread per member: checks 3 and 4 of the header behind the decoder's status; the member's status, and per workgroup the
// lowest member that failed -- in the length word of the workgroup's first member, which every thread has read by then
__global__ __launch_bounds__(JT) void k_unjoin_judge(UnjoinArgs a) {
    __shared__ uint32_t s_first[JT / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t b = (uint64_t)blockIdx.x * JT + tid;
    uint32_t st = HDLZ_OK;
    if (b < a.nmembers) {
        st = a.status[b];
        if (st == HDLZ_OK) {
            const uint64_t lo = a.off[b], zn = a.off[b + 1] - lo + 2u;        // (the index checks passed: these words are sound)
            uint64_t o, e;
            slot_of(a, b, o, e);
            const uint32_t eb = a.end_bit[b];
            const uint8_t* __restrict__ z = a.in + lo - 2u;                   // bit positions count from here; bytes 0 and 1 are not read
            const uint64_t q = ((uint64_t)eb + 3u + 7u) >> 3;                 // the first byte behind the stored block's header bits
            if ((uint64_t)a.len[b] < e - o) st = HDLZ_E_BAD_PARAM;            // the index contradicts the stream
            else if (eb < 16u || q + 4u != zn) st = HDLZ_E_NO_EOF;
            else {
                uint32_t hdr = 0;
                for (uint32_t k = 0; k < 3u; k++) hdr |= ((uint32_t)z[(eb + k) >> 3] >> ((eb + k) & 7u)) & 1u;
                if (hdr != 0u || z[q] != 0u || z[q + 1u] != 0u || z[q + 2u] != 0xFFu || z[q + 3u] != 0xFFu) st = HDLZ_E_NO_EOF;
            }
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

// ---- one workgroup: the tiles -> the checksum, the verdicts -> the first failure; the stream's own frame; the record
__global__ __launch_bounds__(256) void k_unjoin_finish(UnjoinArgs a, uint32_t ntiles, uint32_t ngroups) {
    __shared__ uint64_t s_a[256], s_c[256];
    __shared__ uint32_t s_f[256];
    const uint32_t tid = threadIdx.x;
    uint64_t A64 = 0, C64 = 0;
    for (uint32_t t = tid; t < ntiles; t += 256u) {
        const uint2 s = a.tiles[t];
        fold_tile(A64, C64, t, s.x, s.y);
    }
    const uint32_t f = lowest_word(a.len, ngroups, tid, 256u);
    s_a[tid] = A64 % ADLER_MOD; s_c[tid] = C64 % ADLER_MOD; s_f[tid] = f;
    __syncthreads();
    for (uint32_t o = 128u; o > 0u; o >>= 1) {
        if (tid < o) { s_a[tid] += s_a[tid + o]; s_c[tid] += s_c[tid + o]; s_f[tid] = min(s_f[tid], s_f[tid + o]); }
        __syncthreads();
    }
    if (tid != 0u) return;
    const uint64_t total = total_of(a);
    // (adler32_from, restated: called here, the kernel comes out 11 instructions shorter -- another code object, profiles/adler_shared.txt)
    const uint32_t A = (uint32_t)(s_a[0] % ADLER_MOD), C = (uint32_t)(s_c[0] % ADLER_MOD), nm = (uint32_t)(total % ADLER_MOD);
    const uint32_t s1 = (1u + A) % ADLER_MOD, s2 = (uint32_t)(((uint64_t)nm + (uint64_t)nm * A + ADLER_MOD - C) % ADLER_MOD);
    hdlz_unjoin_result res;
    res.out_len = total; res.first_bad = ~0ull; res.status = HDLZ_OK; res.adler = (s2 << 16) | s1;
    if (s_f[0] != NONE) {
        res.status = a.status[s_f[0]]; res.first_bad = s_f[0]; res.adler = 0u;
    } else {
        const uint64_t end = a.off[a.nmembers];
        bool head = a.off[0] == 2u && a.in_len >= 2u;
        if (head) {
            const uint32_t cmf = a.in[0], flg = a.in[1];
            head = !HDLZ_ZLIB_HEADER_BAD(cmf, flg);
        }
        if (!head) res.status = HDLZ_E_BAD_HEADER;
        else if (a.in_len < 6u || end > a.in_len - 6u || a.in[end] != 3u || a.in[end + 1u] != 0u) res.status = HDLZ_E_NO_EOF;
        else {
            const uint32_t want = load_be32(a.in + end + 2u);
            if (want != res.adler) res.status = HDLZ_E_BAD_CHECKSUM;
        }
        if (res.status != HDLZ_OK) res.first_bad = a.nmembers;
    }
    if (res.status != HDLZ_OK) res.out_len = 0u;
    *a.result = res;
}

// ---- the gzip form (include/hdlz_gzip.h): the index checks, the decode and k_unjoin_judge are the zlib form's; the
// checksum tiles and the finishing workgroup are these two.  a.tiles holds ONE raw CRC word per 32 KiB tile of out[0 .. total) (tile
// loop, tree and bounds: hdlz_crc32.h -- nothing at or behind the total is loaded), a.result is a hdlz_unjoin_gzip_result.
static_assert(sizeof(hdlz_unjoin_gzip_result) == sizeof(hdlz_unjoin_result) && sizeof(hdlz_unjoin_gzip_result) == 24u, "one record layout");

__global__ __launch_bounds__(CRC_THREADS) void k_unjoin_gzip_tiles(UnjoinArgs a) {
    __shared__ CrcTileLds s;
    crc_tiles(a.out, total_of(a), reinterpret_cast<uint32_t*>(a.tiles), s);
}

// one workgroup of CRC_FIN_THREADS: the tile words -> the CRC-32, the verdicts -> the first failure; the gzip frame; the record
__global__ __launch_bounds__(CRC_FIN_THREADS) void k_unjoin_gzip_finish(UnjoinArgs a, uint32_t ngroups) {
    __shared__ uint32_t s_fin[CRC_FIN_THREADS], s_f[CRC_FIN_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint64_t total = total_of(a);
    s_f[tid] = lowest_word(a.len, ngroups, tid, CRC_FIN_THREADS);
    const uint32_t crc = crc_finish(reinterpret_cast<const uint32_t*>(a.tiles), total, s_fin);      // (synchronises: s_f is written)
    for (uint32_t o = CRC_FIN_THREADS / 2u; o > 0u; o >>= 1) {
        if (tid < o) s_f[tid] = min(s_f[tid], s_f[tid + o]);
        __syncthreads();
    }
    if (tid != 0u) return;
    hdlz_unjoin_gzip_result res;
    res.out_len = total; res.first_bad = ~0ull; res.status = HDLZ_OK; res.crc = crc;
    if (s_f[0] != NONE) {
        res.status = a.status[s_f[0]]; res.first_bad = s_f[0]; res.crc = 0u;
    } else {
        const uint64_t end = a.off[a.nmembers];
        const bool head = a.off[0] == 10u && a.in_len >= 10u && a.in[0] == 0x1Fu && a.in[1] == 0x8Bu && a.in[2] == 8u && a.in[3] == 0u;
        if (!head) res.status = HDLZ_E_BAD_HEADER;
        else if (end > a.in_len - 10u || a.in[end] != 3u || a.in[end + 1u] != 0u) res.status = HDLZ_E_NO_EOF;
        else if (le32(a.in + end + 2u) != crc || le32(a.in + end + 6u) != (uint32_t)total) res.status = HDLZ_E_BAD_CHECKSUM;
        if (res.status != HDLZ_OK) res.first_bad = a.nmembers;
    }
    if (res.status != HDLZ_OK) res.out_len = 0u;
    *reinterpret_cast<hdlz_unjoin_gzip_result*>(a.result) = res;
}

}  // namespace unj

size_t unjoin_tiles(uint64_t total_out) { return (size_t)((total_out + ADLER_TILE - 1u) / ADLER_TILE); }

hipError_t launch_unjoin_index(const UnjoinArgs& a, hipStream_t stream) {
    if (a.nmembers == 0) return hipSuccess;
    hipLaunchKernelGGL(unj::k_unjoin_index, dim3((unsigned)((a.nmembers + JT - 1u) / JT)), dim3(JT), 0, stream, a);
    return hipGetLastError();
}

// the tiles, the judge and the finishing workgroup, behind the decode on the same stream
hipError_t launch_unjoin_judge(const UnjoinArgs& a, hipStream_t stream) {
    using namespace unj;
    const uint64_t nt64 = a.nmembers ? unjoin_tiles(a.out_cap) : 0u;
    const uint32_t ntiles = (uint32_t)(nt64 < 0x80000000ull ? nt64 : 0x80000000ull);      // (2^46 bytes: the ABI's bound)
    const uint32_t ngroups = (uint32_t)((a.nmembers + JT - 1u) / JT);
    if (ntiles) {
        const dim3 grid(ntiles < (1u << 22) ? ntiles : (1u << 22)), block(64 * ADLER_TILE_WAVES);
        if ((reinterpret_cast<uintptr_t>(a.out) & 15u) == 0u) hipLaunchKernelGGL(k_unjoin_tiles<true>, grid, block, 0, stream, a, ntiles);
        else hipLaunchKernelGGL(k_unjoin_tiles<false>, grid, block, 0, stream, a, ntiles);
    }
    if (ngroups) hipLaunchKernelGGL(k_unjoin_judge, dim3(ngroups), dim3(JT), 0, stream, a);
    hipLaunchKernelGGL(k_unjoin_finish, dim3(1), dim3(256), 0, stream, a, ntiles, ngroups);
    return hipGetLastError();
}

// the gzip form's tiles, the judge (the zlib form's kernel) and the finishing workgroup
hipError_t launch_unjoin_gzip_judge(const UnjoinArgs& a, hipStream_t stream) {
    using namespace unj;
    const size_t ntiles = a.nmembers ? crc32_tiles(a.out_cap) : 0u;
    const uint32_t ngroups = (uint32_t)((a.nmembers + JT - 1u) / JT);
    if (ntiles) hipLaunchKernelGGL(k_unjoin_gzip_tiles, dim3((unsigned)(ntiles < CRC_GRID_MAX ? ntiles : CRC_GRID_MAX)), dim3(CRC_THREADS), 0, stream, a);
    if (ngroups) hipLaunchKernelGGL(k_unjoin_judge, dim3(ngroups), dim3(JT), 0, stream, a);
    hipLaunchKernelGGL(k_unjoin_gzip_finish, dim3(1), dim3(CRC_FIN_THREADS), 0, stream, a, ngroups);
    return hipGetLastError();
}

}  // namespace hdlz
