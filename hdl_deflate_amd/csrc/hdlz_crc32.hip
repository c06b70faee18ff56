// hdlz_crc32.hip -- hdlz_crc32_ws (include/hdlz_gzip.h): the CRC-32 of a flat device buffer in two launches.
//
// k_crc32_tiles: workgroups of four waves take 32 KiB tiles, grid-stride, and leave one raw 32-bit word per tile in the scratch;
// k_crc32_finish: one workgroup of 1024 threads reduces the words, numbered from the end, and writes the checksum.  The arithmetic,
// the tile loop and the tree are hdlz_crc32.h's (the gzip judgement of hdlz_unjoin.hip runs the same two functions over its output).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_crc32.h"

namespace hdlz {

__global__ __launch_bounds__(CRC_THREADS) void k_crc32_tiles(const uint8_t* __restrict__ data, uint64_t n, uint32_t* __restrict__ words) {
    __shared__ CrcTileLds s;
    crc_tiles(data, n, words, s);
}

__global__ __launch_bounds__(CRC_FIN_THREADS) void k_crc32_finish(const uint32_t* __restrict__ words, uint64_t n, uint32_t* __restrict__ crc) {
    __shared__ uint32_t s_fin[CRC_FIN_THREADS];
    const uint32_t c = crc_finish(words, n, s_fin);
    if (threadIdx.x == 0u) crc[0] = c;
}

size_t crc32_tiles(uint64_t n) { return (size_t)((n + CRC_TILE - 1u) / CRC_TILE); }

static unsigned crc32_grid(uint64_t n) {
    const size_t nt = crc32_tiles(n);
    return (unsigned)(nt < CRC_GRID_MAX ? nt : CRC_GRID_MAX);
}

hipError_t launch_crc32(const uint8_t* data, uint64_t n, uint32_t* crc, uint32_t* words, hipStream_t stream) {
    if (n) {
        hipLaunchKernelGGL(k_crc32_tiles, dim3(crc32_grid(n)), dim3(CRC_THREADS), 0, stream, data, n, words);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_crc32_finish, dim3(1), dim3(CRC_FIN_THREADS), 0, stream, words, n, crc);
    return hipGetLastError();
}

}  // namespace hdlz
