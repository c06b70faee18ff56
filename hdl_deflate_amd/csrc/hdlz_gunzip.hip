// hdlz_gunzip.hip -- what hdlz_gunzip_ws (include/hdlz_gunzip.h) runs around the decode: the header walk of every
// stream's gzip member in front of it, the CRC-32 of every decoded row and the verdict behind it.  The decode itself is an existing
// kernel either way (hdlz_api.hip): the member view of the wave-per-stream decoder, or -- one stream -- the batch call's own path.
//
// k_gunzip_heads      a wave per stream: the RFC 1952 header in the order of the member rule (walk and wave_crc32 of hdlz_gzip_walk.h,
//                     which hdlz_gzip_members.hip shares).  The zero bytes that end FNAME and
//                     FCOMMENT are found 64 bytes a step (bounds-checked byte loads, one ballot); FHCRC, when its flag is set, is the
//                     CRC-32 of the header bytes in front of it, a strip per lane and a tree over the wave (crc_byte, crc_mul and
//                     crc_xpow of hdlz_crc32.h: no table).  Writes p, the header's verdict and the decoder's view of the stream.
// k_gunzip_crc_rows   rows below 64 KiB: a workgroup per row, crc_block over d_out_len[b] bytes.
// k_gunzip_crc_tiles / k_gunzip_crc_finish   longer rows: crc_tiles over every row (blockIdx.y: the row; the grid is sized from the
//                     capacity, n is the row's d_out_len: tiles behind it leave at once), then crc_finish, a workgroup per row.
// k_gunzip_judge      a thread per stream: steps 3 to 5 of the rule, the five result words.
// Plain stores only.  Loads: bytes of the streams inside [start, start + len); of row b only bytes below d_out_len[b].
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_crc32.h"
#include "hdlz_gzip_walk.h"

namespace hdlz {
namespace gunzip {

constexpr uint32_t ROWS_MAX = 65536u;          // rows of at least this capacity take the tiles mapping (two tiles and more)

__device__ __forceinline__ void stream_of(const GunzipArgs& a, uint64_t b, uint64_t& start, uint64_t& len) {
    if (a.in_off) { start = a.in_off[b]; len = a.in_off[b + 1u] - start; }
    else { start = b * a.in_pitch; len = a.in_len; }
}
__device__ __forceinline__ uint32_t row_len(const GunzipArgs& a, uint64_t b) {
    const uint32_t cap = a.out_pitch > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)a.out_pitch, n = a.out_len[b];
    return n < cap ? n : cap;
}

__global__ __launch_bounds__(64) void k_gunzip_heads(GunzipArgs a) {
    for (uint64_t b = blockIdx.x; b < a.nstreams; b += gridDim.x) {
        uint64_t start, len, p = 0;
        stream_of(a, b, start, len);
        const uint32_t v = walk(a.in + start, len, p);
        if (threadIdx.x != 0u) continue;
        a.p[b] = (uint32_t)p;
        a.verdict[b] = v;
        if (a.single) {                                   // the batch call's ragged index of ONE stream: it skips two bytes unread
            a.idx[0] = v == HDLZ_OK ? start + p - 2u : start;
            a.idx[1] = v == HDLZ_OK ? start + len : start;      // a failed header: an empty range
        } else {                                          // the member view: what it reads first is the status word
            a.idx[b] = start + p;
            a.idx[a.nstreams + b] = start + len;
            a.status[b] = v;
            if (v != HDLZ_OK) { a.out_len[b] = 0u; a.in_used[b] = 0u; }
        }
    }
}

__global__ __launch_bounds__(CRC_THREADS) void k_gunzip_crc_rows(GunzipArgs a) {
    __shared__ CrcTileLds s;
    crc_build_tables(s);
    __syncthreads();
    for (uint64_t b = blockIdx.x; b < a.nstreams; b += gridDim.x) {
        if (a.status[b] != HDLZ_OK) continue;             // (uniform over the workgroup)
        const uint32_t c = crc_block(a.out + b * a.out_pitch, row_len(a, b), s);
        if (threadIdx.x == 0u) a.crcw[b] = c;
    }
}

__global__ __launch_bounds__(CRC_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_gunzip_crc_tiles(GunzipArgs a, uint32_t tiles_per_row) {
    __shared__ CrcTileLds s;
    for (uint64_t b = blockIdx.y; b < a.nstreams; b += gridDim.y) {
        if (a.status[b] != HDLZ_OK) continue;
        crc_tiles(a.out + b * a.out_pitch, row_len(a, b), a.tiles + b * tiles_per_row, s);
        __syncthreads();                                  // (the next row builds the tables again: every read of this row's is over)
    }
}

__global__ __launch_bounds__(CRC_FIN_THREADS) void k_gunzip_crc_finish(GunzipArgs a, uint32_t tiles_per_row) {
    __shared__ uint32_t s_fin[CRC_FIN_THREADS];
    for (uint64_t b = blockIdx.x; b < a.nstreams; b += gridDim.x) {
        if (a.status[b] != HDLZ_OK) continue;
        const uint32_t c = crc_finish(a.tiles + b * tiles_per_row, row_len(a, b), s_fin);
        if (threadIdx.x == 0u) a.crcw[b] = c;
        __syncthreads();                                  // (s_fin[0] has been read)
    }
}

__device__ __forceinline__ uint32_t load_le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__global__ __launch_bounds__(256) void k_gunzip_judge(GunzipArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= a.nstreams) return;
    uint64_t start, len;
    stream_of(a, b, start, len);
    const uint32_t head = a.verdict[b];
    uint32_t st = head != HDLZ_OK ? head : a.status[b], n = 0u, used = 0u, crc = 0u;      // the header's verdict comes first
    if (st == HDLZ_OK) {
        // where the final block ended, from the stream's first byte: the decoder counted from byte p - 2 -- bytes (the batch call's
        // path) or bits (the member view's END BIT)
        const uint32_t e = a.in_used[b];
        const uint64_t end = (uint64_t)a.p[b] - 2u + (a.single ? e : (e + 7u) >> 3);
        if (end + 8u > len) st = HDLZ_E_NO_EOF;           // the trailer is cut
        else {
            const uint8_t* t = a.in + start + end;
            n = row_len(a, b);
            crc = a.crcw[b];
            used = (uint32_t)end + 8u;
            if (load_le32(t) != crc || load_le32(t + 4) != n) { st = HDLZ_E_BAD_CHECKSUM; n = 0u; }
        }
    }
    a.status[b] = st;
    a.out_len[b] = n;
    a.in_used[b] = used;
    if (a.crc) a.crc[b] = crc;
}

}  // namespace gunzip

// rows of at least two tiles go over the whole GPU (as long as the call's tile words can be counted in 32 bits): judge_tiled's shape
static uint32_t gunzip_tiles_of(uint64_t out_pitch) {
    const uint64_t cap = out_pitch > 0xFFFFFFFFull ? 0xFFFFFFFFull : out_pitch;
    return (uint32_t)((cap + CRC_TILE - 1u) / CRC_TILE);
}
static bool gunzip_tiled(uint64_t nstreams, uint64_t out_pitch) {
    return out_pitch >= gunzip::ROWS_MAX && nstreams <= 0x7FFFFFFFull / gunzip_tiles_of(out_pitch);
}
size_t gunzip_tile_words(uint64_t nstreams, uint64_t out_pitch) {
    return gunzip_tiled(nstreams, out_pitch) ? (size_t)nstreams * gunzip_tiles_of(out_pitch) : 0u;
}

hipError_t launch_gunzip_heads(const GunzipArgs& a, hipStream_t stream) {
    if (a.nstreams == 0) return hipSuccess;
    const uint64_t g = a.nstreams < 65536u ? a.nstreams : 65536u;
    hipLaunchKernelGGL(gunzip::k_gunzip_heads, dim3((unsigned)g), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_gunzip_crc(const GunzipArgs& a, hipStream_t stream) {
    using namespace gunzip;
    if (a.nstreams == 0) return hipSuccess;
    if (!gunzip_tiled(a.nstreams, a.out_pitch)) {
        const unsigned grid = (unsigned)(a.nstreams < (1u << 20) ? a.nstreams : (1u << 20));
        hipLaunchKernelGGL(k_gunzip_crc_rows, dim3(grid), dim3(CRC_THREADS), 0, stream, a);
        return hipGetLastError();
    }
    const uint32_t tpr = gunzip_tiles_of(a.out_pitch);
    const dim3 grid(tpr < CRC_GRID_MAX ? tpr : CRC_GRID_MAX, (unsigned)(a.nstreams < 65535u ? a.nstreams : 65535u));
    hipLaunchKernelGGL(k_gunzip_crc_tiles, grid, dim3(CRC_THREADS), 0, stream, a, tpr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gunzip_crc_finish, dim3((unsigned)(a.nstreams < 65536u ? a.nstreams : 65536u)), dim3(CRC_FIN_THREADS), 0, stream, a, tpr);
    return hipGetLastError();
}

hipError_t launch_gunzip_judge(const GunzipArgs& a, hipStream_t stream) {
    if (a.nstreams == 0) return hipSuccess;
    hipLaunchKernelGGL(gunzip::k_gunzip_judge, dim3((unsigned)((a.nstreams + 255u) / 256u)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hdlz

#ifdef HDLZ_DEBUG_EXPORTS      // (lib/libhdlz_dbg.so, tools/probe_gunzip.py: the CRC pass alone, over rows whose lengths and statuses the caller wrote)
extern "C" int hdlz_debug_gunzip_crc(const uint8_t* d_out, uint64_t out_pitch, uint64_t nstreams, uint32_t* d_out_len, uint32_t* d_status,
                                     uint32_t* d_crcw, uint32_t* d_tiles, void* stream) {
    hdlz::GunzipArgs a{};
    a.nstreams = nstreams; a.out = d_out; a.out_pitch = out_pitch; a.out_len = d_out_len; a.status = d_status; a.crcw = d_crcw; a.tiles = d_tiles;
    return (int)hdlz::launch_gunzip_crc(a, static_cast<hipStream_t>(stream));
}
#endif
