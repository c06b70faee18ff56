// hdlz_png.hip -- the kernels of include/hdlz_png.h: the chunk walk of a batch of PNG files, and what hdlz_png_decode_ws runs around the
// decode.  The decode itself is an existing kernel either way (hdlz_api.hip): the task view of the wave-per-member decoder, or -- one
// image -- the batch call's own path; the CRC-32 is crc_block of hdlz_crc32.h, the Adler-32 the tile sums of hdlz_adler.h.
//
// k_png_parse        a thread per image: THE RULE's steps 0 to 4 -> the record (but the offsets) and the three sizes it counts.
// k_png_offsets      ONE workgroup: the three scans -> z_off, raw_off, out_off, the totals, the result record.
// k_png_plan         ONE workgroup: the checks of every record in front of the decode, and the exclusive scans of what an image takes of
//                    the call's lists: chunks, Adler tiles, gather tiles, bands of 64 rows.  A list that would not fit refuses the image.
// k_png_list         a thread per image: its chunks from idat_off on -> the chunk list (the IDATs first, ascending; then IHDR, PLTE, tRNS,
//                    IEND for the CRC); the decoder's view of the image.
// k_png_gather       a workgroup per 16 KiB of an image's zlib stream: the chunks that lie there (a binary search in the list), copied
//                    with 16-byte stores.
// k_png_crc          a workgroup per listed chunk: crc_block over type and data against the word behind them.
// k_png_adler        a workgroup per 32 KiB tile of a decoded stream: (A, C) of the tile (the loop of k_adler_tiles).
// k_png_unfilter     a WAVE per segment (see below): rows are lanes, skewed by one pixel; LDS-staged tiles of 64 rows x 128 bytes.
// k_png_expand       the types whose samples are not the scanline's bytes: byte swap, unpack and scale, palette look-up.
// k_png_deinterlace  (HDLZ_PNG_ADAM7 only) the interlaced images: the seven unfiltered passes scattered into the slot, expanded on the way.
// k_png_judge / k_png_finish   the verdict per image; the lowest failed image and the record.
// Plain stores only; no workgroup waits for another.  Loads: inside the files of the range; of the scratch only what the call wrote.
// The planners' strip and scan and the owner search are hdlz_plan.h's; the format's facts shared with the writer: hdlz_png_rules.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "hdlz_device.h"
#include "hdlz_crc32.h"
#include "hdlz_frame.h"
#include "hdlz_adler.h"
#include "hdlz_plan.h"
#include "hdlz_png_rules.h"

namespace hdlz {
namespace png {

constexpr uint32_t SCAN_THREADS = 1024u;
constexpr uint32_t GATHER_TILE = 16384u;
constexpr uint32_t BAND = 64u;                                   // rows a wave unfilters together
constexpr uint32_t CB = 128u, LPITCH = 132u;                     // bytes of a row a tile holds; its pitch in LDS (33 words: a column of 64 rows spreads over all banks)
constexpr uint64_t NONE64 = ~0ull;


// Adam7 (step 4 of THE RULE for an interlaced image): pass p = 0 .. 6 takes the pixels (x0 + i dx, y0 + j dy) of the image.  The four
// tables are nibbles of a word, pass 0 the lowest: x0 = 0 4 0 2 0 1 0, y0 = 0 0 4 0 2 0 1, log2 dx = 3 3 2 2 1 1 0, log2 dy = 3 3 3 2 2 1 1
struct Pass { uint32_t x0, y0, ldx, ldy, pw, ph; uint64_t prb; };      // pw x ph pixels, prb bytes a row; absent: pw or ph is 0
__host__ __device__ inline Pass adam7_pass(uint32_t p, uint32_t width, uint32_t height, uint32_t bits) {
    Pass q;
    q.x0 = (0x0102040u >> (4u * p)) & 15u; q.y0 = (0x1020400u >> (4u * p)) & 15u;
    q.ldx = (0x0112233u >> (4u * p)) & 15u; q.ldy = (0x1122333u >> (4u * p)) & 15u;
    q.pw = width > q.x0 ? (uint32_t)(((uint64_t)width - q.x0 + (1u << q.ldx) - 1u) >> q.ldx) : 0u;
    q.ph = height > q.y0 ? (uint32_t)(((uint64_t)height - q.y0 + (1u << q.ldy) - 1u) >> q.ldy) : 0u;
    q.prb = ((uint64_t)q.pw * bits + 7u) >> 3;
    return q;
}
// the pass of pixel (x, y) by (y & 7, x & 7): a word per row, x = 0 the lowest nibble
__constant__ uint32_t ADAM7_OF[8] = {0x53515350u, 0x66666666u, 0x54545454u, 0x66666666u, 0x53525352u, 0x66666666u, 0x54545454u, 0x66666666u};
// the sum over the present passes of ph (prb + 1); false: past the decoders' limit (no product or sum here leaves 64 bits)
__host__ __device__ inline bool adam7_raw_len(uint32_t width, uint32_t height, uint32_t bits, uint64_t& raw_len) {
    uint64_t sum = 0;
    for (uint32_t p = 0; p < 7u; p++) {
        const Pass q = adam7_pass(p, width, height, bits);
        if (q.pw == 0u || q.ph == 0u) continue;
        if (q.prb + 1u > RAW_MAX / q.ph) return false;
        sum += (uint64_t)q.ph * (q.prb + 1u);
    }
    if (sum > RAW_MAX) return false;
    raw_len = sum;
    return true;
}
// the bands of 64 rows that the present passes of an interlaced image take: a slot of k_png_unfilter each
__device__ __forceinline__ uint64_t adam7_bands(uint32_t width, uint32_t height) {
    uint64_t nb = 0;
    for (uint32_t p = 0; p < 7u; p++) {
        const Pass q = adam7_pass(p, width, height, 8u);
        if (q.pw != 0u) nb += ((uint64_t)q.ph + BAND - 1u) / BAND;
    }
    return nb;
}

// step 4 of THE RULE for a (colour, depth) pair that pair_ok accepts and 0 < width, height < 2^31; false: raw_len is past the limit
struct Sizes { uint64_t row_bytes, raw_len, out_len; uint32_t channels_out, sample_bytes; };
__device__ __forceinline__ bool sizes_of(uint32_t width, uint32_t height, uint32_t depth, uint32_t colour, bool trns, uint32_t flags, bool lace, Sizes& s) {
    const uint32_t ch = channels_of(colour);
    s.row_bytes = ((uint64_t)width * depth * ch + 7u) >> 3;
    s.sample_bytes = depth == 16u ? 2u : 1u;
    s.channels_out = (flags & HDLZ_PNG_EXPAND) && colour == 3u ? (trns ? 4u : 3u) : ch;
    s.raw_len = 0u; s.out_len = 0u;
    if (lace) {
        if (!adam7_raw_len(width, height, depth * ch, s.raw_len)) return false;
    } else {
        if (s.row_bytes + 1u > RAW_MAX / height) return false;
        s.raw_len = (uint64_t)height * (s.row_bytes + 1u);
    }
    s.out_len = (flags & HDLZ_PNG_EXPAND) ? (uint64_t)height * width * s.channels_out * s.sample_bytes : (uint64_t)height * s.row_bytes;
    return true;
}

// the scratch of the index: a summary, then three sizes per image
struct IndexWork { uint64_t *wz, *wr, *wo; };
__host__ __device__ inline IndexWork index_work(void* work, uint64_t n) {
    IndexWork w;
    w.wz = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(work) + 256u);
    w.wr = w.wz + n; w.wo = w.wr + n;
    return w;
}

// ---- hdlz_png_index_ws, steps 0 to 4
__global__ __launch_bounds__(256) void k_png_parse(const uint8_t* __restrict__ files, uint64_t files_len, const uint64_t* __restrict__ file_off,
                                                   const uint64_t* __restrict__ file_len, uint64_t n, uint32_t flags, uint64_t image_cap,
                                                   hdlz_png_image* __restrict__ images, IndexWork w) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t off = file_off[i], len = file_len[i];
    hdlz_png_image rec;
    memset(&rec, 0, sizeof(rec));
    rec.file_off = off; rec.file_len = len;
    uint32_t st = HDLZ_OK;
    uint64_t idat_off = 0, zlen = 0, plte_off = 0, trns_off = 0, used = 0;
    uint32_t nidat = 0, plte_n = 0, trns_n = 0;
    Sizes s{};
    const uint8_t* f = files + off;
    if (off > files_len || len > files_len - off) st = HDLZ_E_BAD_PARAM;
    else if (len < 8u || load_be32(f) != SIG_HI || load_be32(f + 4) != SIG_LO) st = HDLZ_E_BAD_HEADER;
    else if (len >= 16u && (load_be32(f + 8) != IHDR_LEN || load_be32(f + 12) != T_IHDR)) st = HDLZ_E_BAD_HEADER;
    else {
        uint64_t p = 8;
        bool seen = false, gap = false, plte = false, trns = false;
        for (;;) {
            if (p + CHUNK > len) { st = HDLZ_E_NO_EOF; break; }
            const uint64_t L = load_be32(f + p);
            if (L >= 0x80000000ull) { st = HDLZ_E_BAD_HEADER; break; }
            if (p + CHUNK + L > len) { st = HDLZ_E_NO_EOF; break; }
            const uint32_t type = load_be32(f + p + 4);
            if (type == T_IEND) { used = p + CHUNK + L; break; }
            if (type == T_IHDR) {
                if (p != 8u) { st = HDLZ_E_BAD_HEADER; break; }
            } else if (type == T_IDAT) {
                if (gap) { st = HDLZ_E_BAD_HEADER; break; }
                if (!seen) idat_off = p;
                nidat += 1u; zlen += L; seen = true;
            } else {
                if (seen) gap = true;
                if (!(type & 0x20000000u) && type != T_PLTE) { st = HDLZ_E_BAD_BTYPE; break; }
                if (type == T_PLTE && !seen && !plte) {
                    if (L == 0u || L > 768u || L % 3u != 0u) { st = HDLZ_E_BAD_HEADER; break; }
                    plte = true; plte_off = p + 8u; plte_n = (uint32_t)L / 3u;
                } else if (type == T_TRNS && !seen && !trns && f[25] == 3u) {
                    if (L > 256u) { st = HDLZ_E_BAD_HEADER; break; }
                    trns = true; trns_off = p + 8u; trns_n = (uint32_t)L;
                }
            }
            p += CHUNK + L;
        }
        if (st == HDLZ_OK && (!seen || (f[25] == 3u && !plte))) st = HDLZ_E_BAD_HEADER;
        if (st == HDLZ_OK) {
            const uint32_t width = load_be32(f + 16), height = load_be32(f + 20), depth = f[24], colour = f[25], comp = f[26], filt = f[27], lace = f[28];
            if (width == 0u || height == 0u || width >= 0x80000000u || height >= 0x80000000u) st = HDLZ_E_BAD_HEADER;
            else if (!pair_ok(colour, depth) || comp != 0u || filt != 0u) st = HDLZ_E_BAD_HEADER;
            else if (lace == 1u && !(flags & HDLZ_PNG_ADAM7)) st = HDLZ_E_BAD_BTYPE;
            else if (lace > 1u) st = HDLZ_E_BAD_HEADER;
            else if (!sizes_of(width, height, depth, colour, trns, flags, lace == 1u, s) || zlen > Z_MAX) st = HDLZ_E_OUT_CAPACITY;
            else {
                rec.idat_off = idat_off; rec.zlen = zlen; rec.plte_off = plte_off; rec.trns_off = trns_off; rec.used = used;
                rec.row_bytes = s.row_bytes; rec.raw_len = s.raw_len; rec.out_len = s.out_len;
                rec.width = width; rec.height = height; rec.nidat = nidat; rec.plte_n = plte_n; rec.trns_n = trns_n;
                rec.depth = (uint8_t)depth; rec.colour = (uint8_t)colour; rec.interlace = (uint8_t)lace;
                rec.channels_out = (uint8_t)s.channels_out; rec.sample_bytes = (uint8_t)s.sample_bytes;
            }
        }
    }
    rec.status = st;
    const bool ok = st == HDLZ_OK;
    w.wz[i] = ok ? zlen + 8u : 0u; w.wr[i] = ok ? s.raw_len : 0u; w.wo[i] = ok ? s.out_len : 0u;
    if (i < image_cap) images[i] = rec;
}

// ---- step 5 and the record: a strip of the images a thread (hdlz_plan.h)
__global__ __launch_bounds__(SCAN_THREADS) void k_png_offsets(uint64_t n, uint64_t image_cap, uint32_t out_align, hdlz_png_image* __restrict__ images,
                                                              hdlz_png_index_result* __restrict__ result, IndexWork w) {
    __shared__ uint64_t s_wave[3][SCAN_THREADS / 64u];
    __shared__ uint64_t s_end;
    const uint32_t tid = threadIdx.x;
    const uint64_t mask = (uint64_t)out_align - 1u;
    uint64_t lo, hi;
    strip(n, SCAN_THREADS, tid, lo, hi);
    uint64_t mine[3] = {0u, 0u, 0u}, base[3], tot[3];
    for (uint64_t e = lo; e < hi; e++) {
        const Slots s = slots_of(w.wz[e], w.wr[e], w.wo[e], mask);
        mine[0] += s.z; mine[1] += s.raw; mine[2] += s.out;
    }
    if (tid == 0u) s_end = 0u;
    block_scan<3, SCAN_THREADS>(mine, base, tot, s_wave);
    for (uint64_t e = lo; e < hi; e++) {
        if (e < image_cap) { images[e].z_off = base[0]; images[e].raw_off = base[1]; images[e].out_off = base[2]; }
        if (e + 1u == n) s_end = base[2] + w.wo[e];               // the end of the last slot
        const Slots s = slots_of(w.wz[e], w.wr[e], w.wo[e], mask);
        base[0] += s.z; base[1] += s.raw; base[2] += s.out;
    }
    __syncthreads();
    if (tid != 0u) return;
    hdlz_png_index_result res;
    res.nimages = n; res.total_z = tot[0]; res.total_raw = tot[1]; res.total_out = s_end;
    res.status = n > image_cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)HDLZ_OK;
    res.reserved = 0u;
    *result = res;
}

// ---- hdlz_png_decode_ws: the checks of a record (all but the chunk list)
__device__ __forceinline__ uint32_t check_record(const PngArgs& a, const hdlz_png_image& r, const hdlz_png_image& r0) {
    if (r.status != HDLZ_OK) return r.status;
    if (r.file_off > a.in_len || r.file_len > a.in_len - r.file_off || r.used > r.file_len) return HDLZ_E_BAD_PARAM;
    if (r.width == 0u || r.height == 0u || r.width >= 0x80000000u || r.height >= 0x80000000u || !pair_ok(r.colour, r.depth) ||
        r.interlace > ((a.flags & HDLZ_PNG_ADAM7) ? 1u : 0u)) return HDLZ_E_BAD_PARAM;
    Sizes s;
    if (!sizes_of(r.width, r.height, r.depth, r.colour, r.trns_off != 0u, a.flags, r.interlace != 0u, s)) return HDLZ_E_BAD_PARAM;
    if (s.row_bytes != r.row_bytes || s.raw_len != r.raw_len || s.out_len != r.out_len || s.channels_out != r.channels_out || s.sample_bytes != r.sample_bytes) return HDLZ_E_BAD_PARAM;
    if (r.zlen > Z_MAX) return HDLZ_E_BAD_PARAM;
    if (r.nidat == 0u || r.idat_off < 8u || r.idat_off > r.used || r.used - r.idat_off < CHUNK) return HDLZ_E_BAD_PARAM;
    if (r.colour == 3u && (r.plte_n == 0u || r.plte_n > 256u || r.plte_off < 16u || r.plte_off > r.used || r.used - r.plte_off < 3u * r.plte_n + 4u)) return HDLZ_E_BAD_PARAM;
    if (r.trns_off != 0u && (r.trns_n > 256u || r.trns_off < 16u || r.trns_off > r.used || r.used - r.trns_off < r.trns_n + 4u)) return HDLZ_E_BAD_PARAM;
    if (r.plte_off != 0u && (r.plte_n == 0u || r.plte_n > 256u || r.plte_off < 16u || r.plte_off > r.used || r.used - r.plte_off < 3u * r.plte_n + 4u)) return HDLZ_E_BAD_PARAM;
    if (r.z_off < r0.z_off || r.raw_off < r0.raw_off || r.out_off < r0.out_off || ((r.raw_off - r0.raw_off) & 15u)) return HDLZ_E_BAD_PARAM;
    const uint64_t zo = r.z_off - r0.z_off, ro = r.raw_off - r0.raw_off, oo = r.out_off - r0.out_off;
    if (zo > a.z_bytes || r16(r.zlen + 8u) > a.z_bytes - zo || ro > a.raw_bytes || r16(r.raw_len) > a.raw_bytes - ro ||
        oo > a.out_cap || r.out_len > a.out_cap - oo) return HDLZ_E_BAD_PARAM;
    if (r.zlen < 6u) return HDLZ_E_NO_EOF;
    return HDLZ_OK;
}
// does the image's output differ from its unfiltered scanlines?
__device__ __forceinline__ bool expands(const PngArgs& a, const hdlz_png_image& r) { return (a.flags & HDLZ_PNG_EXPAND) && (r.depth != 8u || r.colour == 3u); }

// ---- the checks and the four scans.  head: [0] chunks, [1] Adler tiles, [2] gather tiles, [3] bands
__global__ __launch_bounds__(SCAN_THREADS) void k_png_plan(PngArgs a) {
    __shared__ uint64_t s_wave[4][SCAN_THREADS / 64u];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = a.count;
    uint64_t lo, hi;
    strip(n, SCAN_THREADS, tid, lo, hi);
    const hdlz_png_image r0 = a.images[0];
    uint64_t mine[4] = {0u, 0u, 0u, 0u}, base[4], tot[4];
    for (uint64_t b = lo; b < hi; b++) {
        const hdlz_png_image r = a.images[b];
        const uint32_t st = check_record(a, r, r0);
        a.verdict[b] = st;
        const bool ok = st == HDLZ_OK;
        const uint64_t nc = ok ? (uint64_t)r.nidat + 4u : 0u, nt = ok ? (r.raw_len + ADLER_TILE - 1u) / ADLER_TILE : 0u,
                       nz = ok ? (r.zlen + GATHER_TILE - 1u) / GATHER_TILE : 0u,
                       nb = !ok ? 0u : r.interlace ? adam7_bands(r.width, r.height) : ((uint64_t)r.height + BAND - 1u) / BAND;
        a.cbase[b] = nc; a.tb[b] = nt; a.zb[b] = nz; a.sb[b] = nb;
        mine[0] += nc; mine[1] += nt; mine[2] += nz; mine[3] += nb;
    }
    block_scan<4, SCAN_THREADS>(mine, base, tot, s_wave);
    for (uint64_t b = lo; b < hi; b++) {
        const uint64_t nc = a.cbase[b], nt = a.tb[b], nz = a.zb[b], nb = a.sb[b];
        a.cbase[b] = base[0]; a.tb[b] = base[1]; a.zb[b] = base[2]; a.sb[b] = base[3];
        // (an image whose share does not fit the lists the query sized -- records of overlapping slots, an idat_cap too small -- is refused:
        //  no kernel behind this one writes a list entry or a tile word of a refused image)
        if (a.verdict[b] == HDLZ_OK && (base[0] + nc > a.list_cap || base[1] + nt > a.tile_cap)) a.verdict[b] = HDLZ_E_BAD_PARAM;
        base[0] += nc; base[1] += nt; base[2] += nz; base[3] += nb;
    }
    if (tid == 0u) {
        a.cbase[n] = tot[0]; a.tb[n] = tot[1]; a.zb[n] = tot[2]; a.sb[n] = tot[3];
        a.head[0] = tot[0] < a.list_cap ? tot[0] : a.list_cap; a.head[1] = tot[1]; a.head[2] = tot[2]; a.head[3] = tot[3];
    }
}

// ---- the chunk list and the decoder's view: a thread per image
__global__ __launch_bounds__(JT) void k_png_list(PngArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * JT + threadIdx.x;
    if (b >= a.count) return;
    const hdlz_png_image r = a.images[b], r0 = a.images[0];
    uint32_t st = a.verdict[b];
    if (st == HDLZ_OK) {
        const uint8_t* f = a.in + r.file_off;
        const uint64_t c0 = a.cbase[b], abs0 = r.file_off;
        uint64_t p = r.idat_off, z = 0;
        bool good = true;
        uint32_t k = 0;
        for (; k < r.nidat; k++) {
            if (p > r.used || r.used - p < CHUNK) { good = false; break; }
            const uint64_t L = load_be32(f + p);
            if (L > r.used - p - CHUNK || load_be32(f + p + 4) != T_IDAT || L > r.zlen - z) { good = false; break; }
            a.c_src[c0 + k] = abs0 + p + 4u; a.c_dst[c0 + k] = z; a.c_len[c0 + k] = (uint32_t)L; a.c_img[c0 + k] = (uint32_t)b;
            z += L; p += CHUNK + L;
        }
        if (good && z != r.zlen) good = false;
        uint64_t iend = 0;
        while (good) {                                            // the chunks behind the IDATs, up to the IEND that ends at `used`
            if (p > r.used || r.used - p < CHUNK) { good = false; break; }
            const uint64_t L = load_be32(f + p);
            if (L > r.used - p - CHUNK) { good = false; break; }
            if (load_be32(f + p + 4) == T_IEND) { if (p + CHUNK + L != r.used) good = false; iend = p; break; }
            p += CHUNK + L;
        }
        // IHDR (the rule's step 1 is checked again: the chunk at 8), PLTE, tRNS: type and length in front of the data
        if (good && (r.used < SIG_IHDR_END || load_be32(f + 8) != IHDR_LEN || load_be32(f + 12) != T_IHDR)) good = false;
        if (good && r.plte_off && (load_be32(f + r.plte_off - 8u) != 3u * r.plte_n || load_be32(f + r.plte_off - 4u) != T_PLTE)) good = false;
        if (good && r.trns_off && (load_be32(f + r.trns_off - 8u) != r.trns_n || load_be32(f + r.trns_off - 4u) != T_TRNS)) good = false;
        const uint64_t x = c0 + r.nidat;
        if (good) {
            a.c_src[x] = abs0 + 12u; a.c_len[x] = IHDR_LEN; a.c_img[x] = (uint32_t)b;
            a.c_src[x + 1u] = abs0 + r.plte_off - 4u; a.c_len[x + 1u] = 3u * r.plte_n; a.c_img[x + 1u] = r.plte_off ? (uint32_t)b : NONE;
            a.c_src[x + 2u] = abs0 + r.trns_off - 4u; a.c_len[x + 2u] = r.trns_n; a.c_img[x + 2u] = r.trns_off ? (uint32_t)b : NONE;
            a.c_src[x + 3u] = abs0 + iend + 4u; a.c_len[x + 3u] = (uint32_t)(r.used - iend - CHUNK); a.c_img[x + 3u] = (uint32_t)b;
            for (uint32_t j = 0; j < 4u; j++) a.c_dst[x + j] = NONE64;
        } else {
            st = HDLZ_E_BAD_PARAM;
            a.verdict[b] = st;                                    // (no kernel reads the list of a refused image)
        }
    }
    const bool decode = st == HDLZ_OK;
    const uint64_t zo = r.z_off - r0.z_off, ro = r.raw_off - r0.raw_off;
    a.len[b] = 0u; a.end_bit[b] = 0u; a.crcbad[b] = 0u; a.fltbad[b] = 0u;
    a.status[b] = st;
    if (a.single) {                                               // the batch call's ragged index of ONE stream: it skips two bytes unread
        a.m_off[0] = decode ? zo : 0u;
        a.m_end[0] = decode ? zo + r.zlen : 0u;                   // (count == 1: m_end[0] is the word behind m_off[0])
        return;
    }
    a.m_off[b] = decode ? zo + 2u : 2u;
    a.m_end[b] = decode ? zo + r.zlen : 2u;                       // (the Adler-32 supplies the four bytes the end-of-input rules want)
    a.m_dst[b] = a.raw + (decode ? ro : 0u);
    a.cap[b] = decode ? (uint32_t)r.raw_len : 0u;
}

// ---- (a) the gather: gather tile g is 16 KiB of one image's zlib stream
__global__ __launch_bounds__(256) void k_png_gather(PngArgs a) {
    const uint64_t total = a.head[2];
    for (uint64_t g = blockIdx.x; g < total; g += gridDim.x) {
        const uint64_t b = owner(a.zb, a.count, g);
        if (a.verdict[b] != HDLZ_OK) continue;                    // (uniform)
        const hdlz_png_image r = a.images[b];
        const uint64_t t0 = (g - a.zb[b]) * GATHER_TILE, t1 = t0 + GATHER_TILE < r.zlen ? t0 + GATHER_TILE : r.zlen;
        const uint64_t c0 = a.cbase[b];
        uint64_t k = owner(a.c_dst + c0, r.nidat, t0);            // the chunk that holds byte t0 (empty chunks in front of it are passed)
        uint8_t* const z = a.z + (r.z_off - a.images[0].z_off);
        for (; k < r.nidat; k++) {
            const uint64_t d0 = a.c_dst[c0 + k], d1 = d0 + a.c_len[c0 + k];
            if (d0 >= t1) break;
            const uint64_t lo = d0 > t0 ? d0 : t0, hi = d1 < t1 ? d1 : t1;
            if (hi > lo) copy_to_aligned16(z + lo, a.in + a.c_src[c0 + k] + 4u + (lo - d0), (uint32_t)(hi - lo), threadIdx.x, 256u);
        }
    }
}

// ---- (b) the CRC-32 of every listed chunk
__global__ __launch_bounds__(CRC_THREADS) void k_png_crc(PngArgs a) {
    __shared__ CrcTileLds s;
    crc_build_tables(s);
    __syncthreads();
    const uint64_t total = a.head[0];
    for (uint64_t e = blockIdx.x; e < total; e += gridDim.x) {
        const uint64_t img = owner(a.cbase, a.count, e);          // (the entries of a refused image were never written: its verdict comes first)
        if (a.verdict[img] != HDLZ_OK || a.c_img[e] == NONE) continue;      // (uniform)
        const uint8_t* p = a.in + a.c_src[e];
        const uint32_t L = a.c_len[e] + 4u;
        const uint32_t c = crc_block(p, L, s);
        if (threadIdx.x == 0u && c != load_be32(p + L)) a.crcbad[img] = 1u;
    }
}

// what of an image's decoded stream counts: nothing unless the decoder finished; never more than raw_len
__device__ __forceinline__ uint32_t decoded(const PngArgs& a, uint64_t b, const hdlz_png_image& r) {
    if (a.verdict[b] != HDLZ_OK || a.status[b] != HDLZ_OK) return 0u;
    const uint32_t n = a.len[b];
    return n < r.raw_len ? n : (uint32_t)r.raw_len;
}

// ---- the Adler-32 tiles of the decoded streams (the loop of k_adler_tiles; an image's stream starts at a multiple of 16)
__global__ __launch_bounds__(64 * ADLER_TILE_WAVES) void k_png_adler(PngArgs a) {
    __shared__ uint32_t sa[ADLER_TILE_WAVES], sc[ADLER_TILE_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t total = a.head[1];
    for (uint64_t g = blockIdx.x; g < total; g += gridDim.x) {
        const uint64_t b = owner(a.tb, a.count, g);
        if (a.verdict[b] != HDLZ_OK) continue;                    // (uniform)
        const hdlz_png_image r = a.images[b];
        const uint32_t n = decoded(a, b, r), t = (uint32_t)(g - a.tb[b]);
        if ((uint64_t)t * ADLER_TILE >= n) continue;
        const uint32_t tn = n - t * ADLER_TILE < ADLER_TILE ? n - t * ADLER_TILE : ADLER_TILE;
        const uint8_t* __restrict__ p = a.raw + (r.raw_off - a.images[0].raw_off) + (uint64_t)t * ADLER_TILE;
        uint32_t a32 = 0, c32 = 0;
#pragma unroll
        for (uint32_t k = 0; k < ADLER_TILE_STEPS; k++) {
            const uint32_t q = (wave * ADLER_TILE_STEPS + k) * 1024u + 16u * lane;
            if (q < tn) {
                uint32_t sx, w;
                sums16(load_chunk<true, true>(p, q, tn), sx, w);
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
            a.tiles[g] = make_uint2(A % ADLER_MOD, C % ADLER_MOD);
        }
        __syncthreads();
    }
}

// ---- (d) the unfilter.  A pixel of BPP bytes travels in one register (two for 6 and 8 bytes); its bytes lie in LDS at a multiple of
// what BPP is a multiple of, so it is read and written in the widest pieces that holds for
template <uint32_t BPP> using Px = std::conditional_t<(BPP <= 4u), uint32_t, uint64_t>;
template <uint32_t BPP> __device__ __forceinline__ Px<BPP> px_read(const uint8_t* p) {
    if constexpr (BPP == 4u) return *reinterpret_cast<const uint32_t*>(p);
    else if constexpr (BPP == 8u) return (uint64_t)reinterpret_cast<const uint32_t*>(p)[0] | ((uint64_t)reinterpret_cast<const uint32_t*>(p)[1] << 32);
    else if constexpr (BPP == 2u) return *reinterpret_cast<const uint16_t*>(p);
    else if constexpr (BPP == 6u) {
        const uint16_t* h = reinterpret_cast<const uint16_t*>(p);
        return (uint64_t)h[0] | ((uint64_t)h[1] << 16) | ((uint64_t)h[2] << 32);
    } else {
        Px<BPP> v = 0;
#pragma unroll
        for (uint32_t k = 0; k < BPP; k++) v |= (Px<BPP>)p[k] << (8u * k);
        return v;
    }
}
template <uint32_t BPP> __device__ __forceinline__ void px_write(uint8_t* p, Px<BPP> v) {
    if constexpr (BPP == 4u) *reinterpret_cast<uint32_t*>(p) = v;
    else if constexpr (BPP == 8u) { reinterpret_cast<uint32_t*>(p)[0] = (uint32_t)v; reinterpret_cast<uint32_t*>(p)[1] = (uint32_t)(v >> 32); }
    else if constexpr (BPP == 2u) *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
    else if constexpr (BPP == 6u) {
        uint16_t* h = reinterpret_cast<uint16_t*>(p);
        h[0] = (uint16_t)v; h[1] = (uint16_t)(v >> 16); h[2] = (uint16_t)(v >> 32);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < BPP; k++) p[k] = (uint8_t)(v >> (8u * k));
    }
}
__device__ __forceinline__ uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int32_t pa = abs((int32_t)b - (int32_t)c), pb = abs((int32_t)a - (int32_t)c), pc = abs((int32_t)a + (int32_t)b - 2 * (int32_t)c);
    return (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;        // ties: a, then b, then c
}

// Rows [r0, r1) of one image: r0's filter is 0 or 1, or r0 is the image's first row, so nothing above r0 is looked at.  Row r is the
// rb + 1 bytes at src + r (rb + 1); its unfiltered bytes go to dst + r dpitch (in place: dst = src + 1, dpitch = rb + 1).
// A band is 64 rows, lane l the row base + l.  At step t lane l holds pixel x = t - l: the pixel above it is what lane l - 1 put out
// one step earlier (one wave shuffle), the one above-left what it received the step before, the one to the left its own last output.
// Lane 0 takes the row above from the band in front, which this wave has written to dst (and which is staged like the band's rows).
// A tile is S = 128 / BPP steps: for row q the bytes of pixels [t0 - q, t0 - q + S), a parallelogram in the image and a rectangle in
// LDS -- every lane reads byte s BPP of its own LDS row at step s, rows 33 words apart: no bank conflict.
template <uint32_t BPP>
__device__ void unfilter_rows(const uint8_t* src, uint8_t* dst, uint64_t dpitch, uint32_t rb, uint32_t r0, uint32_t r1, uint8_t* lds, uint32_t* bad) {
    using P = Px<BPP>;
    constexpr uint32_t S = CB / BPP, SB = S * BPP;
    const uint32_t lane = threadIdx.x;
    const uint32_t npx = rb / BPP;
    const uint64_t spitch = (uint64_t)rb + 1u;
    for (uint32_t base = r0; base < r1; base += BAND) {
        const uint32_t rows = r1 - base < BAND ? r1 - base : BAND;
        const bool active = lane < rows;
        uint32_t f = active ? src[(uint64_t)(base + lane) * spitch] : 0u;
        if (f > 4u) { *bad = 1u; f = 0u; }
        const bool any4 = ballot64(f == 4u) != 0ull;
        const bool above = base != r0;                            // (the band's first row has a row of this segment above it)
        if (above) __threadfence();                               // the band in front is in dst: its stores have landed and no stale line answers for them
        P prev_out = 0, prev_b = 0;
        const uint32_t steps = npx + rows - 1u, ntiles = (steps + S - 1u) / S;
        for (uint32_t T = 0; T < ntiles; T++) {
            const int64_t t0 = (int64_t)T * S;
            // stage: 8 lanes a row, 16 bytes each; LDS row 64 is the row above the band
#pragma unroll 1
            for (uint32_t it = 0; it < 9u; it++) {
                const uint32_t q = it * 8u + (lane >> 3), i0 = (lane & 7u) * 16u;
                const bool up = q == BAND;
                if (q > BAND || (up ? !above : q >= rows)) continue;
                const int64_t g0 = (up ? t0 : t0 - (int64_t)q) * BPP + i0;       // the piece's first byte in its row
                if (g0 + 16 <= 0 || g0 >= (int64_t)rb) continue;
                const uint8_t* row = up ? dst + (uint64_t)(base - 1u) * dpitch : src + (uint64_t)(base + q) * spitch + 1u;
                uint8_t* l = lds + q * LPITCH + i0;
                if (g0 >= 0 && g0 + 16 <= (int64_t)rb) {
                    const v4 v = *reinterpret_cast<const v4u*>(row + g0);
                    uint32_t* lw = reinterpret_cast<uint32_t*>(l);
                    lw[0] = v.x; lw[1] = v.y; lw[2] = v.z; lw[3] = v.w;
                } else {
                    for (int32_t i = 0; i < 16; i++)
                        if (g0 + i >= 0 && g0 + i < (int64_t)rb) l[i] = row[g0 + i];
                }
            }
            __syncthreads();
            uint8_t* mine = lds + lane * LPITCH;
            const uint8_t* top = lds + BAND * LPITCH;
            const uint32_t smax = steps - (uint32_t)t0 < S ? steps - (uint32_t)t0 : S;
            // (the bytes of a pixel are worked on together where the arithmetic allows: x + pred and the Average as SWAR words, the
            //  filter's choice as one select a word; only Paeth goes byte by byte, and only in a band that has a Paeth row.  The next
            //  step's filtered pixel is read in front of this step's store: the LDS wait falls into the next iteration.)
            constexpr P M7 = (P)0x7F7F7F7F7F7F7F7Full, M8 = (P)0x8080808080808080ull, ME = (P)0xFEFEFEFEFEFEFEFEull;
            const int64_t x0 = t0 - (int64_t)lane;
            P xr = px_read<BPP>(mine);
            for (uint32_t s = 0; s < smax; s++) {
                const P xn = px_read<BPP>(mine + (s + 1u) * BPP);      // (behind the tile's last pixel: inside the LDS array, not used)
                const int64_t x = x0 + s;
                const bool valid = active && x >= 0 && x < (int64_t)npx;
                P b = (P)__shfl_up(prev_out, 1, 64);
                if (lane == 0u) b = above && valid ? px_read<BPP>(top + s * BPP) : (P)0;
                P av = prev_out, c = prev_b;
                if (x <= 0) { av = 0; c = 0; }
                P pred = f == 1u ? av : f == 2u ? b : f == 3u ? (P)((av & b) + (((av ^ b) & ME) >> 1)) : (P)0;
                if (any4) {
                    P pp = 0;
#pragma unroll
                    for (uint32_t k = 0; k < BPP; k++) {
                        const uint32_t xa = (uint32_t)(av >> (8u * k)) & 255u, xb = (uint32_t)(b >> (8u * k)) & 255u, xc = (uint32_t)(c >> (8u * k)) & 255u;
                        pp |= (P)paeth(xa, xb, xc) << (8u * k);
                    }
                    pred = f == 4u ? pp : pred;
                }
                const P o = ((xr & M7) + (pred & M7)) ^ ((xr ^ pred) & M8);
                if (valid) { px_write<BPP>(mine + s * BPP, o); prev_out = o; }
                prev_b = b;
                xr = xn;
            }
            __syncthreads();
            // write back what the tile's steps covered: row q, bytes [0, SB) of its LDS row
#pragma unroll 1
            for (uint32_t it = 0; it < 8u; it++) {
                const uint32_t q = it * 8u + (lane >> 3), i0 = (lane & 7u) * 16u;
                if (q >= rows || i0 >= SB) continue;
                const int64_t g0 = (t0 - (int64_t)q) * BPP + i0;
                if (g0 + 16 <= 0 || g0 >= (int64_t)rb) continue;
                uint8_t* row = dst + (uint64_t)(base + q) * dpitch;
                const uint8_t* l = lds + q * LPITCH + i0;
                if (g0 >= 0 && g0 + 16 <= (int64_t)rb && i0 + 16u <= SB) {
                    const uint32_t* lw = reinterpret_cast<const uint32_t*>(l);
                    v4 v; v.x = lw[0]; v.y = lw[1]; v.z = lw[2]; v.w = lw[3];
                    *reinterpret_cast<v4u*>(row + g0) = v;
                } else {
                    for (int32_t i = 0; i < 16 && i0 + (uint32_t)i < SB; i++)
                        if (g0 + i >= 0 && g0 + i < (int64_t)rb) row[g0 + i] = l[i];
                }
            }
            __syncthreads();
        }
    }
}

// A SEGMENT starts at row 0 and at the first row of every band of 64 rows (counted from row 0) whose filter is 0 or 1 -- such a row
// does not look up --, and ends where the next one starts.  Slot k of an image is the segment that starts in its band k, if one does.
__global__ __launch_bounds__(64) void k_png_unfilter(PngArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[(BAND + 1u) * LPITCH];
    const uint32_t lane = threadIdx.x;
    const uint64_t total = a.head[3];
    for (uint64_t g = blockIdx.x; g < total; g += gridDim.x) {
        const uint64_t b = owner(a.sb, a.count, g);
        if (a.verdict[b] != HDLZ_OK) continue;                    // (uniform)
        const hdlz_png_image r = a.images[b];
        if (decoded(a, b, r) != r.raw_len || a.len[b] != r.raw_len) continue;      // only a stream of exactly raw_len bytes has rows
        const uint32_t bits = (uint32_t)r.depth * channels_of(r.colour), bpp = bits < 8u ? 1u : bits >> 3;
        uint32_t rb = (uint32_t)r.row_bytes, h = r.height, k = (uint32_t)(g - a.sb[b]);
        uint8_t* raw = a.raw + (r.raw_off - a.images[0].raw_off);
        if (r.interlace) {                                        // slot k is band k of the passes' bands, counted through the present passes:
            bool found = false;                                   // the pass is an image of pw x ph of its own, where its rows start
            for (uint32_t p = 0; p < 7u && !found; p++) {
                const Pass q = adam7_pass(p, r.width, r.height, bits);
                if (q.pw == 0u || q.ph == 0u) continue;
                const uint32_t nbp = (q.ph + BAND - 1u) / BAND;
                if (k < nbp) { rb = (uint32_t)q.prb; h = q.ph; found = true; }
                else { k -= nbp; raw += (uint64_t)q.ph * (q.prb + 1u); }
            }
            if (!found) continue;                                 // (k_png_plan counted the same bands: every slot has its pass)
        }
        const uint32_t nb = (h + BAND - 1u) / BAND;
        const uint64_t spitch = (uint64_t)rb + 1u;
        // the first row of band kk that does not look up (a filter byte above 4 is read as 0), or h
        auto start_in = [&](uint32_t kk) -> uint32_t {
            const uint32_t row = kk * BAND + lane;
            const uint32_t f = row < h ? raw[(uint64_t)row * spitch] : 2u;
            const uint64_t m = ballot64(f <= 1u || f > 4u);
            return m ? kk * BAND + (uint32_t)__builtin_ctzll(m) : h;
        };
        uint32_t r0 = 0;
        if (k != 0u) { r0 = start_in(k); if (r0 == h) continue; }
        uint32_t r1 = h;
        for (uint32_t kk = k + 1u; kk < nb; kk++) { r1 = start_in(kk); if (r1 != h) break; }
        const bool inplace = r.interlace || expands(a, r);        // (a pass's rows are not the slot's: k_png_deinterlace writes it)
        uint8_t* dst = inplace ? raw + 1u : a.out + (r.out_off - a.images[0].out_off);
        const uint64_t dpitch = inplace ? spitch : rb;
        uint32_t* bad = a.fltbad + b;
        switch (bpp) {
            case 1u: unfilter_rows<1u>(raw, dst, dpitch, rb, r0, r1, s_tile, bad); break;
            case 2u: unfilter_rows<2u>(raw, dst, dpitch, rb, r0, r1, s_tile, bad); break;
            case 3u: unfilter_rows<3u>(raw, dst, dpitch, rb, r0, r1, s_tile, bad); break;
            case 4u: unfilter_rows<4u>(raw, dst, dpitch, rb, r0, r1, s_tile, bad); break;
            case 6u: unfilter_rows<6u>(raw, dst, dpitch, rb, r0, r1, s_tile, bad); break;
            default: unfilter_rows<8u>(raw, dst, dpitch, rb, r0, r1, s_tile, bad); break;
        }
    }
}

// ---- the types whose output is not the scanline: a thread per pixel, blockIdx.y strides over the images
__global__ __launch_bounds__(256) void k_png_expand(PngArgs a) {
    for (uint64_t b = blockIdx.y; b < a.count; b += gridDim.y) {
        if (a.verdict[b] != HDLZ_OK) continue;                    // (uniform)
        const hdlz_png_image r = a.images[b];
        if (r.interlace || !expands(a, r) || decoded(a, b, r) != r.raw_len || a.len[b] != r.raw_len) continue;
        const uint8_t* raw = a.raw + (r.raw_off - a.images[0].raw_off);
        uint8_t* out = a.out + (r.out_off - a.images[0].out_off);
        const uint8_t* f = a.in + r.file_off;
        const uint64_t spitch = r.row_bytes + 1u, npix = (uint64_t)r.width * r.height;
        const uint32_t d = r.depth, co = r.channels_out;
        for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < npix; p += (uint64_t)gridDim.x * 256u) {
            const uint64_t row = p / r.width, x = p % r.width;
            const uint8_t* line = raw + row * spitch + 1u;
            if (d == 16u) {
                const uint8_t* s = line + x * co * 2u;
                uint8_t* o = out + p * co * 2u;
                for (uint32_t c = 0; c < co; c++) { o[2u * c] = s[2u * c + 1u]; o[2u * c + 1u] = s[2u * c]; }
                continue;
            }
            const uint64_t bit = x * d;
            const uint32_t v = (line[bit >> 3] >> (8u - d - (uint32_t)(bit & 7u))) & ((1u << d) - 1u);
            if (r.colour != 3u) { out[p] = (uint8_t)(v * (255u / ((1u << d) - 1u))); continue; }
            uint8_t* o = out + p * co;
            const bool in = v < r.plte_n;
            const uint8_t* e = f + r.plte_off + 3u * v;
            o[0] = in ? e[0] : 0u; o[1] = in ? e[1] : 0u; o[2] = in ? e[2] : 0u;
            if (co == 4u) o[3] = v < r.trns_n ? f[r.trns_off + v] : 255u;
        }
    }
}

// ---- the interlaced images: the seven unfiltered sub-images -> the slot, expanded on the way (what k_png_expand does for the others).
// Threads are OUTPUT elements -- a pixel, or in RAW mode below 8 bits a byte of a packed row --, W2 = 256 of one row a workgroup, or, where
// a row has fewer, its elements rounded up to a power of two and 256 / W2 rows: a wave's stores are consecutive bytes of the slot.  A
// row takes its pixels from at most four passes, by (x & 7, y & 7) (ADAM7_OF), and the lanes that read one pass read consecutive pixels
// of one of its rows: every fetched line is used whole.  The pieces of a pixel are moved at any address: 1, 2, 4 or 8 bytes at once.
typedef uint16_t u16u __attribute__((aligned(1), may_alias));
typedef uint32_t u32u __attribute__((aligned(1), may_alias));
typedef uint64_t u64u __attribute__((aligned(1), may_alias));
template <uint32_t N> __device__ __forceinline__ void lace_move(uint8_t* o, const uint8_t* s, bool swap) {
    uint64_t v;
    if constexpr (N == 1u) v = s[0];
    else if constexpr (N == 2u) v = *reinterpret_cast<const u16u*>(s);
    else if constexpr (N == 3u) v = (uint64_t)*reinterpret_cast<const u16u*>(s) | ((uint64_t)s[2] << 16);
    else if constexpr (N == 4u) v = *reinterpret_cast<const u32u*>(s);
    else if constexpr (N == 6u) v = (uint64_t)*reinterpret_cast<const u32u*>(s) | ((uint64_t)*reinterpret_cast<const u16u*>(s + 4) << 32);
    else v = *reinterpret_cast<const u64u*>(s);
    if (swap) v = ((v & 0x00FF00FF00FF00FFull) << 8) | ((v >> 8) & 0x00FF00FF00FF00FFull);       // 16-bit samples: big-endian -> little-endian
    if constexpr (N == 1u) o[0] = (uint8_t)v;
    else if constexpr (N == 2u) *reinterpret_cast<u16u*>(o) = (uint16_t)v;
    else if constexpr (N == 3u) { *reinterpret_cast<u16u*>(o) = (uint16_t)v; o[2] = (uint8_t)(v >> 16); }
    else if constexpr (N == 4u) *reinterpret_cast<u32u*>(o) = (uint32_t)v;
    else if constexpr (N == 6u) { *reinterpret_cast<u32u*>(o) = (uint32_t)v; *reinterpret_cast<u16u*>(o + 4) = (uint16_t)(v >> 32); }
    else *reinterpret_cast<u64u*>(o) = v;
}
// sample i of d <= 8 bits in a packed row
__device__ __forceinline__ uint32_t lace_sample(const uint8_t* line, uint32_t i, uint32_t d) {
    const uint64_t bit = (uint64_t)i * d;
    return (line[bit >> 3] >> (8u - d - (uint32_t)(bit & 7u))) & ((1u << d) - 1u);
}

__global__ __launch_bounds__(256) void k_png_deinterlace(PngArgs a) {
    __shared__ uint32_t s_off[7], s_pitch[7];                     // where a pass's rows start in the image's stream; prb + 1
    const uint32_t tid = threadIdx.x;
    for (uint64_t b = blockIdx.y; b < a.count; b += gridDim.y) {
        if (a.verdict[b] != HDLZ_OK) continue;                    // (uniform, as every `continue` of this loop)
        const hdlz_png_image r = a.images[b];
        if (!r.interlace || decoded(a, b, r) != r.raw_len || a.len[b] != r.raw_len) continue;
        const uint32_t d = r.depth, bits = d * channels_of(r.colour), co = r.channels_out;
        __syncthreads();                                          // (nobody reads the table of the image before any more)
        if (tid == 0u) {
            uint64_t off = 0;
            for (uint32_t p = 0; p < 7u; p++) {
                const Pass q = adam7_pass(p, r.width, r.height, bits);
                s_off[p] = (uint32_t)off; s_pitch[p] = (uint32_t)(q.prb + 1u);
                if (q.pw != 0u && q.ph != 0u) off += (uint64_t)q.ph * (q.prb + 1u);
            }
        }
        __syncthreads();
        const uint8_t* raw = a.raw + (r.raw_off - a.images[0].raw_off);
        uint8_t* out = a.out + (r.out_off - a.images[0].out_off);
        const uint8_t* f = a.in + r.file_off;
        // the unfiltered row of its pass that holds pixel (x, y), and which pixel of that row it is
        auto row_of = [&](uint32_t x, uint32_t y, uint32_t& px) -> const uint8_t* {
            const uint32_t p4 = 4u * ((ADAM7_OF[y & 7u] >> (4u * (x & 7u))) & 15u);
            px = (x - ((0x0102040u >> p4) & 15u)) >> ((0x0112233u >> p4) & 15u);
            const uint32_t py = (y - ((0x1020400u >> p4) & 15u)) >> ((0x1122333u >> p4) & 15u);
            return raw + s_off[p4 >> 2] + (uint64_t)py * s_pitch[p4 >> 2] + 1u;
        };
        const bool ex = (a.flags & HDLZ_PNG_EXPAND) != 0u;
        const bool packed = !ex && d < 8u;                        // the elements are the bytes of a packed row, 8 / d pixels each
        const bool looked = ex && (d < 8u || r.colour == 3u);     // unpacked and scaled, or looked up in the palette
        const uint64_t epr = packed ? r.row_bytes : r.width;      // elements a row
        const uint32_t eb = looked ? co : packed ? 1u : bits >> 3;      // bytes an element
        uint32_t lg = 0;
        while (lg < 8u && (1ull << lg) < epr) lg++;
        const uint32_t W2 = 1u << lg, R = 256u >> lg;
        const uint64_t chunks = (epr + W2 - 1u) >> lg, groups = ((uint64_t)r.height + R - 1u) / R;
        for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
            const uint64_t y64 = g * R + (tid >> lg);
            if (y64 >= r.height) continue;
            const uint32_t y = (uint32_t)y64;
            for (uint64_t c = 0; c < chunks; c++) {
                const uint64_t e = c * W2 + (tid & (W2 - 1u));
                if (e >= epr) break;
                uint8_t* o = out + (y64 * epr + e) * eb;
                uint32_t px;
                if (packed) {
                    uint32_t v = 0;
                    for (uint32_t j = 0; j < 8u / d; j++) {       // (pixels past the row's last: pad bits, 0)
                        const uint64_t x = e * (8u / d) + j;
                        if (x >= r.width) break;
                        const uint8_t* line = row_of((uint32_t)x, y, px);
                        v |= lace_sample(line, px, d) << (8u - d * (j + 1u));
                    }
                    o[0] = (uint8_t)v;
                    continue;
                }
                const uint8_t* line = row_of((uint32_t)e, y, px);
                if (looked) {
                    const uint32_t v = lace_sample(line, px, d);
                    if (r.colour != 3u) { o[0] = (uint8_t)(v * (255u / ((1u << d) - 1u))); continue; }
                    const bool in = v < r.plte_n;
                    const uint8_t* t = f + r.plte_off + 3u * v;
                    const uint32_t rgb = in ? (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) : 0u;
                    if (co == 4u) *reinterpret_cast<u32u*>(o) = rgb | ((v < r.trns_n ? (uint32_t)f[r.trns_off + v] : 255u) << 24);
                    else { *reinterpret_cast<u16u*>(o) = (uint16_t)rgb; o[2] = (uint8_t)(rgb >> 16); }
                    continue;
                }
                const bool swap = ex && d == 16u;
                switch (eb) {
                    case 1u: lace_move<1u>(o, line + px, swap); break;
                    case 2u: lace_move<2u>(o, line + 2ull * px, swap); break;
                    case 3u: lace_move<3u>(o, line + 3ull * px, swap); break;
                    case 4u: lace_move<4u>(o, line + 4ull * px, swap); break;
                    case 6u: lace_move<6u>(o, line + 6ull * px, swap); break;
                    default: lace_move<8u>(o, line + 8ull * px, swap); break;
                }
            }
        }
    }
}

// ---- (e) the judgement: a wave per image folds its Adler tiles
__global__ __launch_bounds__(64) void k_png_judge(PngArgs a) {
    const uint32_t lane = threadIdx.x;
    for (uint64_t b = blockIdx.x; b < a.count; b += gridDim.x) {
        const hdlz_png_image r = a.images[b];
        uint32_t st = a.verdict[b];
        if (st == HDLZ_OK && a.crcbad[b]) st = HDLZ_E_BAD_CHECKSUM;
        if (st == HDLZ_OK) st = a.status[b];
        if (st == HDLZ_OK) {
            const uint8_t* z = a.z + (r.z_off - a.images[0].z_off);
            const uint32_t len = a.len[b], eb = a.end_bit[b];
            const uint64_t end = a.single ? eb : (eb + 7u) >> 3;     // bytes from the stream's first to the end of the final block
            const uint32_t cmf = z[0], flg = z[1];
            if (HDLZ_ZLIB_HEADER_BAD(cmf, flg)) st = HDLZ_E_BAD_HEADER;
            else if (len > r.raw_len) st = HDLZ_E_OUT_CAPACITY;
            else if (len < r.raw_len) st = HDLZ_E_BAD_CHECKSUM;
            else if (end + 4u != r.zlen) st = HDLZ_E_NO_EOF;
            else {
                const uint32_t nt = (uint32_t)((r.raw_len + ADLER_TILE - 1u) / ADLER_TILE);
                const uint2* tiles = a.tiles + a.tb[b];
                uint64_t A64 = 0, C64 = 0;
                for (uint32_t t = lane; t < nt; t += 64u) { const uint2 s = tiles[t]; fold_tile(A64, C64, t, s.x, s.y); }
                uint32_t Ar = (uint32_t)(A64 % ADLER_MOD), Cr = (uint32_t)(C64 % ADLER_MOD);
#pragma unroll
                for (int ofs = 32; ofs > 0; ofs >>= 1) { Ar += (uint32_t)__shfl_xor((int)Ar, ofs, 64); Cr += (uint32_t)__shfl_xor((int)Cr, ofs, 64); }
                if (adler32_from(Ar % ADLER_MOD, Cr % ADLER_MOD, r.raw_len) != load_be32(z + r.zlen - 4u)) st = HDLZ_E_BAD_CHECKSUM;
                else if (a.fltbad[b]) st = HDLZ_E_BAD_SYMBOL;
            }
        }
        if (lane == 0u) {
            a.fin[b] = st;
            if (a.image_status) a.image_status[b] = st;
        }
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_png_finish(PngArgs a) {
    __shared__ uint64_t s_f[SCAN_THREADS];
    const uint32_t tid = threadIdx.x;
    uint64_t f = NONE64;
    for (uint64_t b = tid; b < a.count; b += SCAN_THREADS)
        if (a.fin[b] != HDLZ_OK) { f = b; break; }
    s_f[tid] = f;
    __syncthreads();
    for (uint32_t o = SCAN_THREADS / 2u; o > 0u; o >>= 1) {
        if (tid < o) s_f[tid] = s_f[tid] < s_f[tid + o] ? s_f[tid] : s_f[tid + o];
        __syncthreads();
    }
    if (tid != 0u) return;
    hdlz_png_decode_result res;
    res.out_len = 0u; res.first_bad = NONE64; res.status = HDLZ_OK; res.reserved = 0u;
    if (s_f[0] != NONE64) { res.status = a.fin[s_f[0]]; res.first_bad = s_f[0]; }
    else if (a.count) {
        const hdlz_png_image last = a.images[a.count - 1u];
        res.out_len = last.out_off - a.images[0].out_off + last.out_len;
    }
    *a.result = res;
}

static unsigned grid_of(uint64_t want, uint64_t most) { return (unsigned)(want < 1u ? 1u : want < most ? want : most); }

}  // namespace png

size_t png_index_work_bytes(uint64_t n) { return 256u + round256(3u * sizeof(uint64_t) * (size_t)n); }

hipError_t launch_png_index(const uint8_t* files, uint64_t files_len, const uint64_t* file_off, const uint64_t* file_len, uint64_t n, uint32_t flags,
                            uint32_t out_align, uint64_t image_cap, hdlz_png_image* images, hdlz_png_index_result* result, void* work, hipStream_t stream) {
    using namespace png;
    const IndexWork w = index_work(work, n);
    hipError_t e = hipSuccess;
    if (n) e = launch(k_png_parse, dim3((unsigned)((n + 255u) / 256u)), dim3(256), stream, files, files_len, file_off, file_len, n, flags, image_cap, images, w);
    if (e == hipSuccess) e = launch(k_png_offsets, dim3(1), dim3(SCAN_THREADS), stream, n, image_cap, out_align, images, result, w);
    return e;
}

// in front of the decode: the checks, the chunk list, the gather, the chunk CRCs
hipError_t launch_png_front(const PngArgs& a, hipStream_t stream) {
    using namespace png;
    if (a.count == 0) return hipSuccess;
    hipError_t e = launch(k_png_plan, dim3(1), dim3(SCAN_THREADS), stream, a);
    if (e == hipSuccess) e = launch(k_png_list, dim3((unsigned)((a.count + JT - 1u) / JT)), dim3(JT), stream, a);
    if (e == hipSuccess) e = launch(k_png_gather, dim3(grid_of(a.z_bytes / GATHER_TILE + a.count, 8192u)), dim3(256), stream, a);
    if (e == hipSuccess) e = launch(k_png_crc, dim3(grid_of(a.list_cap, 4096u)), dim3(CRC_THREADS), stream, a);
    return e;
}

// behind the decode: the Adler tiles, the unfilter, the expansion, (under HDLZ_PNG_ADAM7) the deinterlace, the verdicts and the record
hipError_t launch_png_back(const PngArgs& a, hipStream_t stream) {
    using namespace png;
    hipError_t e = hipSuccess;
    if (a.count) {
        e = launch(k_png_adler, dim3(grid_of(a.tile_cap, 8192u)), dim3(64 * ADLER_TILE_WAVES), stream, a);
        if (e == hipSuccess) e = launch(k_png_unfilter, dim3(grid_of(a.raw_bytes / (2u * BAND) + a.count, 8192u)), dim3(64), stream, a);
        if ((a.flags & HDLZ_PNG_EXPAND) && e == hipSuccess)
            e = launch(k_png_expand, dim3(grid_of(a.out_cap / a.count / 4096u, 512u), grid_of(a.count, 4096u)), dim3(256), stream, a);
        if ((a.flags & HDLZ_PNG_ADAM7) && e == hipSuccess)
            e = launch(k_png_deinterlace, dim3(grid_of(a.out_cap / a.count / 4096u, 512u), grid_of(a.count, 4096u)), dim3(256), stream, a);
        if (e == hipSuccess) e = launch(k_png_judge, dim3(grid_of(a.count, 65536u)), dim3(64), stream, a);
    }
    if (e == hipSuccess) e = launch(k_png_finish, dim3(1), dim3(SCAN_THREADS), stream, a);
    return e;
}

}  // namespace hdlz
