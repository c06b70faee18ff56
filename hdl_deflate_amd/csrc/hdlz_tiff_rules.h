// hdlz_tiff_rules.h -- the facts of the TIFF format and of include/hdlz_tiff.h that the index (k_tiff_parse) and the decode's checks
// (k_tiff_plan) both state, each once: the tags read, the acceptance table of steps 4 and 5 of THE RULE, and the geometry of step 6 --
// what an image takes of the chunk list, the decoded chunks and the output.  The statuses differ between the two sides (the index
// answers with the rule's, the decode refuses a record that does not hold with HDLZ_E_BAD_PARAM), so both build theirs from these.
#pragma once
#include <stdint.h>
#include "hdlz_device.h"

namespace hdlz {
namespace tiff {

// ---- the tags read, in the order of the slots the parser keeps them in
constexpr uint32_t NTAGS = 16u;
enum Slot : uint32_t { S_WIDTH, S_HEIGHT, S_BITS, S_COMP, S_PHOTO, S_SOFF, S_SPP, S_RPS, S_SCNT, S_PLANAR, S_PRED, S_TW, S_TH, S_TOFF, S_TCNT, S_FORMAT };
__host__ __device__ inline uint32_t slot_of(uint32_t tag) {
    switch (tag) {
        case 256u: return S_WIDTH; case 257u: return S_HEIGHT; case 258u: return S_BITS; case 259u: return S_COMP; case 262u: return S_PHOTO;
        case 273u: return S_SOFF; case 277u: return S_SPP; case 278u: return S_RPS; case 279u: return S_SCNT; case 284u: return S_PLANAR;
        case 317u: return S_PRED; case 322u: return S_TW; case 323u: return S_TH; case 324u: return S_TOFF; case 325u: return S_TCNT;
        case 339u: return S_FORMAT; default: return 0xFFFFFFFFu;
    }
}
constexpr uint32_t T_SHORT = 3u, T_LONG = 4u;
constexpr uint32_t PAGE_MAX = 65535u;                            // the hops of one record
constexpr uint32_t PHOTO_NONE = 0xFFFFFFFFu;                     // no tag 262 in the IFD

// ---- the decoders' limits (hdlz_zip.h): a chunk's decoded bytes and its zlib stream; and the bound on out_len (no product leaves 64 bits)
constexpr uint64_t RAW_MAX = 0xFFFFFE00ull, Z_MAX = 0x10000000ull - 7u, OUT_MAX = 1ull << 62;
constexpr uint32_t C_NONE = 1u, C_DEFLATE = 8u, C_DEFLATE_OLD = 32946u;

__host__ __device__ inline uint64_t r16(uint64_t x) { return (x + 15u) & ~15ull; }

// ---- steps 4 and 5: 0 = accepted; 1 = a value another reader would read (HDLZ_E_BAD_BTYPE); 2 = one the format does not know (HDLZ_E_BAD_HEADER).
// The first line that applies, in the header's order.  unequal: the values of BitsPerSample or of SampleFormat differ between samples
__host__ __device__ inline uint32_t accept(uint32_t samples, uint32_t bits, uint32_t format, uint32_t comp, uint32_t photo, uint32_t planar,
                                           uint32_t pred, bool unequal) {
    if (samples == 0u) return 2u;
    if (samples > 8u) return 1u;
    if (bits == 0u || bits > 64u) return 2u;
    if (unequal || (bits != 8u && bits != 16u && bits != 32u && bits != 64u)) return 1u;
    if (format == 0u || format > 6u) return 2u;
    if (format > 3u || (format == 3u && bits < 32u)) return 1u;
    if (comp != C_NONE && comp != C_DEFLATE && comp != C_DEFLATE_OLD) {
        const bool known = (comp >= 2u && comp <= 7u) || comp == 32773u || comp == 34712u || comp == 34925u || comp == 50000u || comp == 50001u;
        return known ? 1u : 2u;
    }
    if (photo == 6u) return 1u;
    if (planar != 1u) return planar == 2u ? 1u : 2u;
    if (pred != 1u && pred != 2u) {
        if (pred != 3u) return 2u;
        if (format != 3u) return 1u;
    }
    return 0u;
}

// ---- step 6, for 0 < width, height < 2^31, 0 < tile_w, tile_h < 2^31 and an accepted (samples, bits): chunks of tile_w x tile_h pixels,
// `across` a row of them (strips: tile_w = width, tile_h = min(RowsPerStrip, height), across = 1); full / last: the decoded bytes of
// every chunk but the last / of the last one (tiles: equal).  0 = it holds; else the limit it is past (the header's order)
struct Geometry { uint64_t across, nchunks, full, last, raw_len, raw16, out_len; uint32_t px; };
__host__ __device__ inline uint32_t geometry(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, bool tiled, uint32_t samples, uint32_t bits, Geometry& g) {
    g.px = samples * (bits >> 3);                                 // bytes a pixel: at most 64
    g.across = ((uint64_t)width + tile_w - 1u) / tile_w;
    const uint64_t down = ((uint64_t)height + tile_h - 1u) / tile_h;
    g.nchunks = g.across * down;                                  // (below 2^62)
    if (g.nchunks > 0x7FFFFFFFull) return 1u;
    const uint64_t cpx = (uint64_t)tile_w * tile_h;               // (below 2^62)
    if (cpx > RAW_MAX / g.px) return 2u;
    g.full = cpx * g.px;
    g.last = tiled ? g.full : ((uint64_t)height - (down - 1u) * tile_h) * tile_w * g.px;
    const uint64_t pixels = (uint64_t)width * height;
    if (pixels > OUT_MAX / g.px) return 3u;
    g.out_len = pixels * g.px;
    g.raw_len = (g.nchunks - 1u) * g.full + g.last;               // (nchunks < 2^31, full < 2^32)
    g.raw16 = (g.nchunks - 1u) * r16(g.full) + r16(g.last);
    return 0u;
}

}  // namespace tiff
}  // namespace hdlz
