// hdlz_frame.h -- what the join, unjoin and BGZF kernels share, each once: the reductions of a wave,
// little-endian loads, the finishing workgroup's share of the judges' words, the copy to a 16-byte aligned destination, the BGZF
// format's constants and bytes with the header test, and the tile join -- scan, look-back, scratch and launch.  What a kernel could not
// take from here without another instruction sequence stands in that kernel and is listed in profiles/framing_shared.txt, section 3.
#pragma once
#include "hdlz_device.h"
#include "hdlz_plan.h"                                   // wave_scan_add

namespace hdlz {

// ---- a wave's sum, largest and smallest word
__device__ __forceinline__ uint32_t wave_add(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

// ---- JT threads a workgroup, a thread per member (the judges) or per row (the tile joins); NONE: no member failed
constexpr uint32_t JT = 256u;
constexpr uint32_t NONE = 0xFFFFFFFFu;

// a judge (k_unjoin_judge, k_bgzf_judge) leaves workgroup g's lowest failed member in word JT g of its length words; behind it, in
// one workgroup of `threads`: this thread's share of those words
__device__ __forceinline__ uint32_t lowest_word(const uint32_t* words, uint32_t ngroups, uint32_t tid, uint32_t threads) {
    uint32_t f = NONE;
    for (uint32_t g = tid; g < ngroups; g += threads) f = min(f, words[(size_t)g * JT]);
    return f;
}

// ---- n bytes src -> dst by `nlanes` lanes: up to 15 bytes to dst's next 16-byte boundary, whole chunks with 16-byte stores (no load
// leaves src[0 .. n)), at most 15 bytes behind them
__device__ __forceinline__ void copy_to_aligned16(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane, uint32_t nlanes) {
    const uint32_t head = min(n, (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u));
    if (lane < head) dst[lane] = src[lane];
    const uint32_t chunks = (n - head) >> 4;
    for (uint32_t k = lane; k < chunks; k += nlanes) *reinterpret_cast<v4*>(dst + head + 16u * k) = *reinterpret_cast<const v4u*>(src + head + 16u * k);
    const uint32_t done = head + 16u * chunks;
    if (done + lane < n) dst[done + lane] = src[done + lane];
}

// ---- the BGZF format (include/hdlz_bgzf.h): a member is HEADER(16), BSIZE(2), the deflate data, CRC-32(4), ISIZE(4)
namespace bgzf {
constexpr uint32_t HEAD = 18u, TAIL = 8u, MEMBER_MIN = HEAD + 2u + TAIL, MEMBER_MAX = 65536u, ISIZE_MAX = 65536u;
#define HDLZ_BGZF_HEADER_BYTES 0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0
constexpr uint32_t HEADER_FREE = 0x03F0u;      // bit i: byte i of a HEADER may be anything (MTIME, XFL, OS)
static __constant__ const uint8_t HEADER[16] = {HDLZ_BGZF_HEADER_BYTES};
static __constant__ const uint8_t EOF_MEMBER[MEMBER_MIN] = {HDLZ_BGZF_HEADER_BYTES, 0x1B, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// the fixed bytes of a HEADER; the caller has checked that p[0 .. 18) lies inside the file
__device__ __forceinline__ bool is_header(const uint8_t* p) {
    constexpr uint8_t want[16] = {HDLZ_BGZF_HEADER_BYTES};
    bool ok = true;
    static_for<0, 16>([&](auto i) {
        if constexpr (((HEADER_FREE >> i) & 1u) == 0u) ok = ok && p[i] == want[i];
    });
    return ok;
}
#undef HDLZ_BGZF_HEADER_BYTES

}  // namespace bgzf

// ---- a tile join (k_join, hdlz_join.hip; k_bgzf_join, hdlz_bgzf_stored.hip): a workgroup takes a tile of JT consecutive rows by a
// ticket, scans their member lengths, publishes the sum as one 64-bit word {state, value} and finds its base by a decoupled look-back
// over the tiles in front of it.  The scratch, in words of 32 bits: ticket (+ pad), one look-back word and PARTS words per tile.
constexpr uint64_t J_AGG = 1ull << 62, J_PFX = 2ull << 62, J_MASK = 3ull << 62;
constexpr uint32_t PARTS = 4;                            // words a tile leaves for the finishing workgroup; the last is its worst status

// the exclusive scan of the tile's 256 lengths m: this thread's prefix, and the tile's sum in tsum (one __syncthreads inside)
__device__ __forceinline__ uint64_t tile_scan(uint32_t m, uint32_t lane, uint32_t wave, uint64_t (&s_wsum)[4], uint64_t& tsum) {
    const uint64_t v = wave_scan_add(m);
    if (lane == 63u) s_wsum[wave] = v;
    __syncthreads();
    const uint64_t w0 = s_wsum[0], w1 = s_wsum[1], w2 = s_wsum[2], w3 = s_wsum[3];
    tsum = w0 + w1 + w2 + w3;
    return v - m + (wave > 0u ? w0 : 0ull) + (wave > 1u ? w1 : 0ull) + (wave > 2u ? w2 : 0ull);
}
// wave 0 of a tile: the sum of the tiles in front of it; publishes the tile's own sum first and its inclusive prefix last
__device__ __forceinline__ uint64_t tile_lookback(unsigned long long* desc, uint32_t tile, uint64_t tsum, uint32_t lane) {
    uint64_t base = 0;
    if (tile != 0u) {
        if (lane == 0u) __hip_atomic_store(&desc[tile], J_AGG | tsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int64_t t = (int64_t)tile - 1 - (int64_t)lane;        // lane 0 looks at the nearest tile
        for (;;) {
            uint64_t d = J_PFX;                                // (tiles in front of tile 0: an empty prefix)
            if (t >= 0) {
                do { d = __hip_atomic_load(&desc[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while ((d & J_MASK) == 0ull);
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
    if (lane == 0u) __hip_atomic_store(&desc[tile], J_PFX | (base + tsum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return base;
}

inline uint64_t join_tiles(uint64_t nblocks) { return (nblocks + JT - 1u) / JT; }
inline size_t join_zeroed_words(uint64_t ntiles) { return 2u + 2u * (size_t)ntiles; }      // the ticket and the look-back words
inline JoinWork join_work(void* work, uint64_t nblocks) {
    uint32_t* ws = static_cast<uint32_t*>(work);
    return JoinWork{ws, reinterpret_cast<unsigned long long*>(ws + 2), ws + join_zeroed_words(join_tiles(nblocks))};
}

template <class... P, class... A>
hipError_t launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t stream, const A&... a) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, a...);
    return hipGetLastError();
}
// zero the ticket and the look-back words, a workgroup per tile of `kernel`, then finish()
template <class Args, class Finish>
hipError_t launch_tile_join(void (*kernel)(Args), const Args& a, hipStream_t stream, Finish finish) {
    const uint64_t ntiles = join_tiles(a.nblocks);
    if (ntiles) {
        hipError_t e = zero_words(a.w.ticket, (uint32_t)join_zeroed_words(ntiles), stream);
        if (e == hipSuccess) e = launch(kernel, dim3((unsigned)ntiles), dim3(JT), stream, a);
        if (e != hipSuccess) return e;
    }
    return finish((uint32_t)ntiles);
}

}  // namespace hdlz
