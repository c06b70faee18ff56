// hdlz_png_rules.h -- the facts of the PNG format and of include/hdlz_png.h that the reader (hdlz_png.hip) and the writer
// (hdlz_png_write.hip) both state, each once: the signature, the chunk frame and tags, the legal (colour, depth) pairs, the decoders'
// limits, and what an indexed image takes of the three buffers of a decode.  The statuses a refusal gets differ between the two
// sides: sizes_of and check_spec stay in their files, built from these -- with the row's bytes and the stream's length written out
// in each, as the kernels that are launched per image or per band need them (profiles/planner_shared.txt, section 3).
#pragma once
#include <stdint.h>
#include "hdlz_device.h"

namespace hdlz {
namespace png {

// ---- a file: the 8 signature bytes, then chunks of length (4, big-endian), type (4), data, CRC-32 over type and data (4); the first
// chunk is an IHDR of 13 bytes, so the chunk behind it starts at SIG_IHDR_END
constexpr uint32_t SIG_HI = 0x89504E47u, SIG_LO = 0x0D0A1A0Au;
constexpr uint32_t T_IHDR = 0x49484452u, T_PLTE = 0x504C5445u, T_IDAT = 0x49444154u, T_IEND = 0x49454E44u, T_TRNS = 0x74524E53u;
constexpr uint32_t CHUNK = 12u, IHDR_LEN = 13u, SIG_IHDR_END = 8u + CHUNK + IHDR_LEN;
#define HDLZ_BE32_BYTES(x) (uint8_t)((x) >> 24), (uint8_t)((x) >> 16), (uint8_t)((x) >> 8), (uint8_t)(x)      // a word as a writer lists its bytes

// ---- the decoders' limits (hdlz_zip.h): an image's scanlines with their filter bytes, and its zlib stream
constexpr uint64_t RAW_MAX = 0xFFFFFE00ull, Z_MAX = 0x10000000ull - 7u;

__host__ __device__ inline uint64_t r16(uint64_t x) { return (x + 15u) & ~15ull; }

// ---- the pairs the format allows; channels a pixel.  (The writer takes those of depth 8 and 16 without the palette: its check_spec.)
__device__ __forceinline__ bool pair_ok(uint32_t colour, uint32_t depth) {
    const bool d8 = depth == 8u || depth == 16u, low = depth == 1u || depth == 2u || depth == 4u;
    return colour == 0u ? (d8 || low) : colour == 3u ? (low || depth == 8u) : (colour == 2u || colour == 4u || colour == 6u) && d8;
}
__device__ __forceinline__ uint32_t channels_of(uint32_t colour) { return colour == 2u ? 3u : colour == 4u ? 2u : colour == 6u ? 4u : 1u; }

// ---- step 5: what an indexed image takes of z, raw and out -- its stream and the 8 bytes the decoders may load behind it (z8 =
// zlen + 8) and its scanlines, each to a multiple of 16, its output to a multiple of out_align (align_mask = out_align - 1).  An
// image that failed takes nothing: all three lengths are 0
struct Slots { uint64_t z, raw, out; };
__host__ __device__ inline Slots slots_of(uint64_t z8, uint64_t raw_len, uint64_t out_len, uint64_t align_mask) {
    return Slots{r16(z8), r16(raw_len), (out_len + align_mask) & ~align_mask};
}

}  // namespace png
}  // namespace hdlz
