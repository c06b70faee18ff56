// hdlz_tiff.hip -- the kernels of include/hdlz_tiff.h: the directory walk of a batch of TIFF images, and what hdlz_tiff_decode_ws runs
// around the decode.  The decode itself is an existing kernel either way (hdlz_api.hip): the task view of the wave-per-member decoder
// over ALL chunks of the range, or -- one image of one chunk -- the batch call's own path; the Adler-32 is the tile sums of hdlz_adler.h.
//
// k_tiff_parse       a thread per image: THE RULE's steps 0 to 6 -> the record (but the offsets) and the three sizes it counts.
// k_tiff_offsets     ONE workgroup: the three scans -> chunk_off, raw_off, out_off, the totals, the result record.
// k_tiff_plan        ONE workgroup: the checks of every record in front of the decode, and the exclusive scans of what an image takes
//                    of the call's lists: chunks and Adler tiles.  A list that would not fit refuses the image.
// k_tiff_chunks      a thread per chunk: its offset and byte count from the file, its checks, the decoder's view of it.
// k_tiff_adler       a workgroup per 32 KiB tile of a decoded chunk: (A, C) of the tile (the loop of k_png_adler).
// k_tiff_unpredict   a WAVE per chunk row (or several short rows): predictor, byte order, crop, the slot -- see there.
// k_tiff_judge / k_tiff_finish   the verdict per chunk and image; the lowest failed image and the record.
// Plain stores only; no workgroup waits for another.  Loads: inside the files of the range; of the scratch only what the call wrote.
// The planners' strip and scan and the owner search are hdlz_plan.h's; the format's facts: hdlz_tiff_rules.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "hdlz_device.h"
#include "hdlz_frame.h"
#include "hdlz_adler.h"
#include "hdlz_plan.h"
#include "hdlz_tiff_rules.h"

namespace hdlz {
namespace tiff {

constexpr uint32_t SCAN_THREADS = 1024u;
constexpr uint64_t NONE64 = ~0ull;
constexpr uint32_t SKIP = 0xFFFFFFFFu;                           // the decoder's status word of a chunk it is not to touch
constexpr uint32_t UNP_WAVES = 4u;                               // waves a workgroup of k_tiff_unpredict

// ---- words in the file's byte order; value k of an array of SHORTs or LONGs
__device__ __forceinline__ uint32_t rd16(const uint8_t* p, bool be) { return be ? ((uint32_t)p[0] << 8) | p[1] : ((uint32_t)p[1] << 8) | p[0]; }
__device__ __forceinline__ uint32_t rd32(const uint8_t* p, bool be) {
    return be ? load_be32(p) : ((uint32_t)p[3] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | (uint32_t)p[0];
}
__device__ __forceinline__ uint32_t value(const uint8_t* p, uint32_t type, uint64_t k, bool be) { return type == T_SHORT ? rd16(p + 2u * k, be) : rd32(p + 4u * k, be); }

// the scratch of the index: a summary, then three sizes per image
struct IndexWork { uint64_t *wc, *wr, *wo; };
__host__ __device__ inline IndexWork index_work(void* work, uint64_t n) {
    IndexWork w;
    w.wc = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(work) + 256u);
    w.wr = w.wc + n; w.wo = w.wr + n;
    return w;
}

// ---- hdlz_tiff_index_ws, steps 0 to 6
struct Tag { uint64_t at; uint32_t type, count; };               // where its values stand; count 0: not taken
__global__ __launch_bounds__(256) void k_tiff_parse(const uint8_t* __restrict__ files, uint64_t files_len, const uint64_t* __restrict__ file_off,
                                                    const uint64_t* __restrict__ file_len, const uint32_t* __restrict__ pages, uint64_t n,
                                                    uint64_t image_cap, hdlz_tiff_image* __restrict__ images, IndexWork w) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t off = file_off[i], len = file_len[i];
    const uint32_t page = pages ? pages[i] : 0u;
    hdlz_tiff_image rec;
    memset(&rec, 0, sizeof(rec));
    rec.file_off = off; rec.file_len = len;
    uint32_t st = HDLZ_OK;
    const uint8_t* f = files + off;
    bool be = false;
    if (off > files_len || len > files_len - off || page > PAGE_MAX) st = HDLZ_E_BAD_PARAM;
    else if (len < 4u) st = HDLZ_E_BAD_HEADER;
    else {
        const uint32_t m = load_be32(f);
        if (m == 0x49492A00u) be = false;
        else if (m == 0x4D4D002Au) be = true;
        else st = (m == 0x49492B00u || m == 0x4D4D002Bu) ? HDLZ_E_BAD_BTYPE : HDLZ_E_BAD_HEADER;
        if (st == HDLZ_OK && len < 8u) st = HDLZ_E_BAD_HEADER;
    }
    uint64_t o = 0, next = 0;
    uint32_t nent = 0;
    if (st == HDLZ_OK) {                                          // step 2: at most page + 1 hops
        o = rd32(f + 4, be);
        for (uint32_t k = 0;; k++) {
            if (o == 0u) { st = HDLZ_E_NO_EOF; break; }
            if ((o & 1u) || o < 8u) { st = HDLZ_E_BAD_HEADER; break; }
            if (o + 2u > len) { st = HDLZ_E_NO_EOF; break; }
            nent = rd16(f + o, be);
            if (nent == 0u) { st = HDLZ_E_BAD_HEADER; break; }
            if (o + 2u + 12u * (uint64_t)nent + 4u > len) { st = HDLZ_E_NO_EOF; break; }
            next = rd32(f + o + 2u + 12u * (uint64_t)nent, be);
            if (k == page) break;
            o = next;
        }
    }
    Tag t[NTAGS];
    for (uint32_t s = 0; s < NTAGS; s++) t[s] = Tag{0u, 0u, 0u};
    if (st == HDLZ_OK) {                                          // step 3: the first entry of every tag of the table
        for (uint32_t e = 0; e < nent; e++) {
            const uint64_t at = o + 2u + 12u * (uint64_t)e;
            const uint32_t s = slot_of(rd16(f + at, be));
            if (s >= NTAGS || t[s].count) continue;
            const uint32_t type = rd16(f + at + 2u, be), cnt = rd32(f + at + 4u, be);
            if ((type != T_SHORT && type != T_LONG) || cnt == 0u) { st = HDLZ_E_BAD_HEADER; break; }
            const uint64_t bytes = (uint64_t)cnt * (type == T_SHORT ? 2u : 4u);
            uint64_t where = at + 8u;
            if (bytes > 4u) {
                where = rd32(f + at + 8u, be);
                if (where > len || bytes > len - where) { st = HDLZ_E_NO_EOF; break; }
            }
            const bool array = s == S_BITS || s == S_FORMAT || s == S_SOFF || s == S_SCNT || s == S_TOFF || s == S_TCNT;
            if (!array && cnt != 1u) { st = HDLZ_E_BAD_HEADER; break; }
            t[s] = Tag{where, type, cnt};
        }
    }
    Geometry g{};
    if (st == HDLZ_OK) {                                          // steps 4 to 6
        auto scalar = [&](uint32_t s, uint32_t dflt) -> uint32_t { return t[s].count ? value(f + t[s].at, t[s].type, 0u, be) : dflt; };
        // the first of the values of 258 / 339 (`samples` of them: at most 8); do they differ?
        auto same = [&](uint32_t s, uint32_t dflt, uint32_t samples, bool& unequal) -> uint32_t {
            if (!t[s].count) return dflt;
            const uint32_t v0 = value(f + t[s].at, t[s].type, 0u, be);
            for (uint32_t k = 1; k < samples; k++) unequal |= value(f + t[s].at, t[s].type, k, be) != v0;
            return v0;
        };
        const uint32_t width = scalar(S_WIDTH, 0u), height = scalar(S_HEIGHT, 0u), samples = scalar(S_SPP, 1u);
        const bool tiled = t[S_TW].count != 0u;
        uint32_t tile_w = 0, tile_h = 0, bits = 1, format = 1;
        if (width == 0u || height == 0u || width >= 0x80000000u || height >= 0x80000000u) st = HDLZ_E_BAD_HEADER;
        else if (samples == 0u) st = HDLZ_E_BAD_HEADER;
        else if (samples > 8u) st = HDLZ_E_BAD_BTYPE;
        else if ((t[S_BITS].count && t[S_BITS].count != samples) || (t[S_FORMAT].count && t[S_FORMAT].count != samples)) st = HDLZ_E_BAD_HEADER;
        else {
            bool unequal = false;
            bits = same(S_BITS, 1u, samples, unequal); format = same(S_FORMAT, 1u, samples, unequal);
            const uint32_t a = accept(samples, bits, format, scalar(S_COMP, 1u), scalar(S_PHOTO, PHOTO_NONE), scalar(S_PLANAR, 1u), scalar(S_PRED, 1u), unequal);
            if (a) st = a == 1u ? HDLZ_E_BAD_BTYPE : HDLZ_E_BAD_HEADER;
        }
        if (st == HDLZ_OK) {                                      // step 5
            const bool any_tile = t[S_TH].count || t[S_TOFF].count || t[S_TCNT].count;
            if (tiled) {
                tile_w = scalar(S_TW, 0u); tile_h = scalar(S_TH, 0u);
                if (!t[S_TH].count || !t[S_TOFF].count || !t[S_TCNT].count || t[S_SOFF].count || t[S_SCNT].count) st = HDLZ_E_BAD_HEADER;
                else if (tile_w == 0u || tile_h == 0u || tile_w >= 0x80000000u || tile_h >= 0x80000000u) st = HDLZ_E_BAD_HEADER;
            } else {
                const uint32_t rps = scalar(S_RPS, height);
                if (!t[S_SOFF].count || !t[S_SCNT].count || any_tile) st = HDLZ_E_BAD_HEADER;
                else if (rps == 0u) st = HDLZ_E_BAD_HEADER;
                tile_w = width; tile_h = rps < height ? rps : height;
            }
        }
        if (st == HDLZ_OK) {                                      // step 6
            const Tag &ao = t[tiled ? S_TOFF : S_SOFF], &ac = t[tiled ? S_TCNT : S_SCNT];
            if (geometry(width, height, tile_w, tile_h, tiled, samples, bits, g)) st = HDLZ_E_OUT_CAPACITY;
            else if (ao.count != g.nchunks || ac.count != g.nchunks) st = HDLZ_E_BAD_HEADER;
            else {
                rec.ifd_off = o; rec.next_ifd = next; rec.off_arr = ao.at; rec.cnt_arr = ac.at; rec.raw_len = g.raw_len; rec.out_len = g.out_len;
                rec.width = width; rec.height = height; rec.tile_w = tile_w; rec.tile_h = tile_h; rec.nchunks = (uint32_t)g.nchunks;
                rec.compression = scalar(S_COMP, 1u); rec.photometric = scalar(S_PHOTO, PHOTO_NONE);
                rec.off_type = (uint8_t)ao.type; rec.cnt_type = (uint8_t)ac.type; rec.bits = (uint8_t)bits; rec.samples = (uint8_t)samples;
                rec.format = (uint8_t)format; rec.predictor = (uint8_t)scalar(S_PRED, 1u); rec.big_endian = be ? 1u : 0u; rec.tiled = tiled ? 1u : 0u;
            }
        }
    }
    rec.status = st;
    const bool ok = st == HDLZ_OK;
    w.wc[i] = ok ? g.nchunks : 0u; w.wr[i] = ok ? g.raw16 : 0u; w.wo[i] = ok ? g.out_len : 0u;
    if (i < image_cap) images[i] = rec;
}

// ---- step 7 and the record: a strip of the images a thread (hdlz_plan.h)
__global__ __launch_bounds__(SCAN_THREADS) void k_tiff_offsets(uint64_t n, uint64_t image_cap, uint32_t out_align, hdlz_tiff_image* __restrict__ images,
                                                               hdlz_tiff_index_result* __restrict__ result, IndexWork w) {
    __shared__ uint64_t s_wave[3][SCAN_THREADS / 64u];
    __shared__ uint64_t s_end;
    const uint32_t tid = threadIdx.x;
    const uint64_t mask = (uint64_t)out_align - 1u;
    uint64_t lo, hi;
    strip(n, SCAN_THREADS, tid, lo, hi);
    uint64_t mine[3] = {0u, 0u, 0u}, base[3], tot[3];
    for (uint64_t e = lo; e < hi; e++) { mine[0] += w.wc[e]; mine[1] += w.wr[e]; mine[2] += (w.wo[e] + mask) & ~mask; }
    if (tid == 0u) s_end = 0u;
    block_scan<3, SCAN_THREADS>(mine, base, tot, s_wave);
    for (uint64_t e = lo; e < hi; e++) {
        if (e < image_cap) { images[e].chunk_off = base[0]; images[e].raw_off = base[1]; images[e].out_off = base[2]; }
        if (e + 1u == n) s_end = base[2] + w.wo[e];               // the end of the last slot
        base[0] += w.wc[e]; base[1] += w.wr[e]; base[2] += (w.wo[e] + mask) & ~mask;
    }
    __syncthreads();
    if (tid != 0u) return;
    hdlz_tiff_index_result res;
    res.nimages = n; res.total_chunks = tot[0]; res.total_raw = tot[1]; res.total_out = s_end;
    res.status = n > image_cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)HDLZ_OK;
    res.reserved = 0u;
    *result = res;
}

// ---- hdlz_tiff_decode_ws: the checks of a record
__device__ __forceinline__ bool deflated(const hdlz_tiff_image& r) { return r.compression != C_NONE; }
__device__ __forceinline__ uint32_t check_record(const TiffArgs& a, const hdlz_tiff_image& r, const hdlz_tiff_image& r0, Geometry& g) {
    if (r.status != HDLZ_OK) return r.status;
    if (r.file_off > a.in_len || r.file_len > a.in_len - r.file_off) return HDLZ_E_BAD_PARAM;
    if (r.width == 0u || r.height == 0u || r.tile_w == 0u || r.tile_h == 0u || r.width >= 0x80000000u || r.height >= 0x80000000u ||
        r.tile_w >= 0x80000000u || r.tile_h >= 0x80000000u || r.tiled > 1u || r.big_endian > 1u) return HDLZ_E_BAD_PARAM;
    if (!r.tiled && (r.tile_w != r.width || r.tile_h > r.height)) return HDLZ_E_BAD_PARAM;
    if (accept(r.samples, r.bits, r.format, r.compression, r.photometric, 1u, r.predictor, false)) return HDLZ_E_BAD_PARAM;
    if (geometry(r.width, r.height, r.tile_w, r.tile_h, r.tiled != 0u, r.samples, r.bits, g)) return HDLZ_E_BAD_PARAM;
    if (g.nchunks != r.nchunks || g.raw_len != r.raw_len || g.out_len != r.out_len) return HDLZ_E_BAD_PARAM;
    if ((r.off_type != T_SHORT && r.off_type != T_LONG) || (r.cnt_type != T_SHORT && r.cnt_type != T_LONG)) return HDLZ_E_BAD_PARAM;
    const uint64_t ob = g.nchunks * (r.off_type == T_SHORT ? 2u : 4u), cb = g.nchunks * (r.cnt_type == T_SHORT ? 2u : 4u);
    if (r.off_arr > r.file_len || ob > r.file_len - r.off_arr || r.cnt_arr > r.file_len || cb > r.file_len - r.cnt_arr) return HDLZ_E_BAD_PARAM;
    if (r.chunk_off < r0.chunk_off || r.raw_off < r0.raw_off || r.out_off < r0.out_off || ((r.raw_off - r0.raw_off) & 15u)) return HDLZ_E_BAD_PARAM;
    const uint64_t ro = r.raw_off - r0.raw_off, oo = r.out_off - r0.out_off;
    if (ro > a.raw_bytes || g.raw16 > a.raw_bytes - ro || oo > a.out_cap || r.out_len > a.out_cap - oo) return HDLZ_E_BAD_PARAM;
    return HDLZ_OK;
}
// the Adler tiles of an image: every chunk but the last takes ceil(full / 32768), the last ceil(last / 32768); a stored image none
__device__ __forceinline__ uint64_t tiles_of(uint64_t bytes) { return (bytes + ADLER_TILE - 1u) / ADLER_TILE; }

// ---- the checks and the two scans.  head: [0] chunks, [1] Adler tiles
__global__ __launch_bounds__(SCAN_THREADS) void k_tiff_plan(TiffArgs a) {
    __shared__ uint64_t s_wave[2][SCAN_THREADS / 64u];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = a.count;
    uint64_t lo, hi;
    strip(n, SCAN_THREADS, tid, lo, hi);
    const hdlz_tiff_image r0 = a.images[0];
    uint64_t mine[2] = {0u, 0u}, base[2], tot[2];
    for (uint64_t b = lo; b < hi; b++) {
        const hdlz_tiff_image r = a.images[b];
        Geometry g{};
        const uint32_t st = check_record(a, r, r0, g);
        a.verdict[b] = st;
        const bool ok = st == HDLZ_OK;
        const uint64_t nc = ok ? g.nchunks : 0u, nt = ok && deflated(r) ? (g.nchunks - 1u) * tiles_of(g.full) + tiles_of(g.last) : 0u;
        a.cb[b] = nc; a.tb[b] = nt;
        mine[0] += nc; mine[1] += nt;
    }
    block_scan<2, SCAN_THREADS>(mine, base, tot, s_wave);
    for (uint64_t b = lo; b < hi; b++) {
        const uint64_t nc = a.cb[b], nt = a.tb[b];
        a.cb[b] = base[0]; a.tb[b] = base[1];
        // (an image whose share does not fit the lists the query sized -- records of overlapping slots, a chunk_cap too small -- is
        //  refused: no kernel behind this one writes a list entry or a tile word of a refused image)
        if (a.verdict[b] == HDLZ_OK && (base[0] + nc > a.chunk_cap || base[1] + nt > a.tile_cap)) a.verdict[b] = HDLZ_E_BAD_PARAM;
        base[0] += nc; base[1] += nt;
    }
    if (tid == 0u) {
        a.cb[n] = tot[0]; a.tb[n] = tot[1];
        a.head[0] = tot[0] < a.chunk_cap ? tot[0] : a.chunk_cap; a.head[1] = tot[1] < a.tile_cap ? tot[1] : a.tile_cap;
    }
}

// ---- (a) a thread per slot of the chunk list: the chunk's two words, its checks, the decoder's view
__global__ __launch_bounds__(JT) void k_tiff_chunks(TiffArgs a) {
    const uint64_t c = (uint64_t)blockIdx.x * JT + threadIdx.x;
    if (c >= a.chunk_cap) return;
    uint32_t st = SKIP;                                           // a slot behind the range's chunks, or of a refused image: nobody's
    uint64_t src = 0, cnt = 0, raw_c = 0;
    uint8_t* dst = a.raw;
    bool decode = false;
    if (c < a.head[0]) {
        const uint64_t b = owner(a.cb, a.count, c);
        if (a.verdict[b] == HDLZ_OK && c - a.cb[b] < a.images[b].nchunks) {
            const hdlz_tiff_image r = a.images[b];
            const uint64_t k = c - a.cb[b];
            Geometry g{};
            geometry(r.width, r.height, r.tile_w, r.tile_h, r.tiled != 0u, r.samples, r.bits, g);
            const uint8_t* f = a.in + r.file_off;
            const uint64_t o = value(f + r.off_arr, r.off_type, k, r.big_endian != 0u);
            cnt = value(f + r.cnt_arr, r.cnt_type, k, r.big_endian != 0u);
            raw_c = k + 1u == g.nchunks ? g.last : g.full;
            st = HDLZ_OK;
            if (o > r.file_len || cnt > r.file_len - o) st = HDLZ_E_NO_EOF;
            else if (deflated(r)) {
                if (cnt < 6u) st = HDLZ_E_NO_EOF;
                else if (cnt > Z_MAX) st = HDLZ_E_OUT_CAPACITY;
                else if (a.single && cnt > a.bound) st = HDLZ_E_BAD_PARAM;
            } else if (cnt < raw_c) st = HDLZ_E_NO_EOF;
            src = r.file_off + o;
            dst = a.raw + (r.raw_off - a.images[0].raw_off) + k * r16(g.full);
            decode = st == HDLZ_OK && deflated(r);
        }
    }
    a.cst[c] = st; a.len[c] = 0u; a.end_bit[c] = 0u;
    a.status[c] = decode ? (uint32_t)HDLZ_OK : SKIP;              // (the member decoder leaves a chunk alone whose word is not HDLZ_OK)
    a.m_dst[c] = dst;
    a.cap[c] = decode ? (uint32_t)raw_c : 0u;
    if (a.single) {                                               // the batch call's ragged index of ONE stream: it skips two bytes unread
        a.m_off[0] = decode ? src : 0u;                           // (a stored or refused chunk: an empty range; m_end[0] is the word behind m_off[0])
        a.m_end[0] = decode ? src + cnt : 0u;
        return;
    }
    // the stream behind its two header bytes, the Adler-32 supplying the four bytes the end-of-input rules want
    a.m_off[c] = decode ? src + 2u : 2u;
    a.m_end[c] = decode ? src + cnt : 2u;
}

// the image and chunk of slot c of the chunk list, for the kernels behind the decode.  false: the slot is nobody's
struct Chunk { uint64_t b, k, raw_c; hdlz_tiff_image r; Geometry g; };
__device__ __forceinline__ bool chunk_of(const TiffArgs& a, uint64_t c, Chunk& q) {
    q.b = owner(a.cb, a.count, c);
    if (a.verdict[q.b] != HDLZ_OK) return false;
    q.r = a.images[q.b];
    q.k = c - a.cb[q.b];
    if (q.k >= q.r.nchunks) return false;
    geometry(q.r.width, q.r.height, q.r.tile_w, q.r.tile_h, q.r.tiled != 0u, q.r.samples, q.r.bits, q.g);
    q.raw_c = q.k + 1u == q.g.nchunks ? q.g.last : q.g.full;
    return true;
}
// where the bytes of a stored chunk stand in d_files: its word of the offsets array, which k_tiff_chunks held against the file's length
__device__ __forceinline__ uint64_t stored_at(const TiffArgs& a, const Chunk& q) {
    return q.r.file_off + value(a.in + q.r.file_off + q.r.off_arr, q.r.off_type, q.k, q.r.big_endian != 0u);
}
// what of a chunk's decoded stream counts: nothing unless the decoder finished; never more than the chunk's bytes
__device__ __forceinline__ uint32_t decoded(const TiffArgs& a, uint64_t c, uint64_t raw_c) {
    if (a.cst[c] != HDLZ_OK || a.status[c] != HDLZ_OK) return 0u;
    const uint32_t n = a.len[c];
    return n < raw_c ? n : (uint32_t)raw_c;
}

// ---- (c) the Adler-32 tiles of the decoded chunks (the loop of k_png_adler; a chunk's bytes start at a multiple of 16)
__global__ __launch_bounds__(64 * ADLER_TILE_WAVES) void k_tiff_adler(TiffArgs a) {
    __shared__ uint32_t sa[ADLER_TILE_WAVES], sc[ADLER_TILE_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t total = a.head[1];
    for (uint64_t g = blockIdx.x; g < total; g += gridDim.x) {
        const uint64_t b = owner(a.tb, a.count, g);
        if (a.verdict[b] != HDLZ_OK) continue;                    // (uniform, as every `continue` of this loop)
        const hdlz_tiff_image r = a.images[b];
        Geometry gm{};
        geometry(r.width, r.height, r.tile_w, r.tile_h, r.tiled != 0u, r.samples, r.bits, gm);
        const uint64_t tf = tiles_of(gm.full), gi = g - a.tb[b];
        const uint64_t k = gi / tf < gm.nchunks - 1u ? gi / tf : gm.nchunks - 1u, c = a.cb[b] + k;
        const uint32_t t = (uint32_t)(gi - k * tf);
        const uint32_t n = decoded(a, c, k + 1u == gm.nchunks ? gm.last : gm.full);
        if ((uint64_t)t * ADLER_TILE >= n) continue;
        const uint32_t tn = n - t * ADLER_TILE < ADLER_TILE ? n - t * ADLER_TILE : ADLER_TILE;
        const uint8_t* __restrict__ p = a.m_dst[c] + (uint64_t)t * ADLER_TILE;
        uint32_t a32 = 0, c32 = 0;
#pragma unroll
        for (uint32_t s = 0; s < ADLER_TILE_STEPS; s++) {
            const uint32_t q = (wave * ADLER_TILE_STEPS + s) * 1024u + 16u * lane;
            if (q < tn) {
                uint32_t sx, wgt;
                sums16(load_chunk<true, true>(p, q, tn), sx, wgt);
                a32 += sx;
                c32 += __umul24(q, sx) + wgt;
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
            for (uint32_t s = 0; s < ADLER_TILE_WAVES; s++) { A += sa[s]; C += sc[s]; }
            a.tiles[g] = make_uint2(A % ADLER_MOD, C % ADLER_MOD);
        }
        __syncthreads();
    }
}

// ---- (d) the unpredict.  16 bytes at any address, of which only the first n (0 .. 16) may be touched
typedef uint16_t u16u __attribute__((aligned(1), may_alias));
typedef uint32_t u32u __attribute__((aligned(1), may_alias));
__device__ __forceinline__ v4 load16(const uint8_t* p, uint32_t n) {
    if (n >= 16u) return *reinterpret_cast<const v4u*>(p);
    auto part = [&](uint32_t k) -> uint32_t {
        const int32_t c = (int32_t)n - 4 * (int32_t)k;
        return c >= 4 ? *reinterpret_cast<const u32u*>(p + 4u * k) : c > 0 ? load_tail(p + 4u * k, c) : 0u;
    };
    v4 v;
    v.x = part(0u); v.y = part(1u); v.z = part(2u); v.w = part(3u);
    return v;
}
__device__ __forceinline__ void store16(uint8_t* p, const v4 v, uint32_t n) {
    if (n >= 16u) { *reinterpret_cast<v4u*>(p) = v; return; }
    auto part = [&](uint32_t k, uint32_t d) {
        const int32_t c = (int32_t)n - 4 * (int32_t)k;
        if (c >= 4) { *reinterpret_cast<u32u*>(p + 4u * k) = d; return; }
        for (int32_t i = 0; i < c; i++) p[4u * k + i] = (uint8_t)(d >> (8 * i));
    };
    part(0u, v.x); part(1u, v.y); part(2u, v.z); part(3u, v.w);
}

// One step of a chunk row for predictors 1 and 2: the lane's 16 bytes v stand at byte q of the row (bytes past the row are 0), as
// E = 16 / B words of B bytes; the row's words cycle through S channels.  The words are swapped to little-endian; under predictor 2
// every word becomes the sum of the words of its channel up to and with it, mod 2^(8 B):
//   the lane sums its own words per channel -- word j looks back S words --; the last S words then hold the lane's totals, by PHASE
//   (U[p]: the channel of the lane's word p; a lane's first word has channel e0 mod S, e0 = q / B, which for S = 3 does not align to
//   the lanes) -- rotated into channel order where the phase can differ between lanes (S * B does not divide 16);
//   the lanes' totals are scanned over the lpr lanes of the row, per channel (wave_scan_add's loop, mod 2^32 or 2^64);
//   `carry` holds the sums of the row's steps in front (per channel) and takes this step's on.
// All lanes of the wave call it (the scan shuffles); lir: the lane's index among the lpr lanes (a power of two) of its row.
template <uint32_t B> using Acc = std::conditional_t<(B == 8u), uint64_t, uint32_t>;
template <uint32_t B, uint32_t S>
__device__ __forceinline__ void step_words(v4& v, bool be, bool pred2, uint64_t q, uint32_t lir, uint32_t lpr, Acc<B> (&carry)[S]) {
    using A = Acc<B>;
    constexpr uint32_t E = 16u / B;
    uint32_t d[4] = {v.x, v.y, v.z, v.w};
    if (be) {
        if constexpr (B == 2u) {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) d[k] = ((d[k] & 0x00FF00FFu) << 8) | ((d[k] >> 8) & 0x00FF00FFu);
        } else if constexpr (B >= 4u) {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) d[k] = __builtin_bswap32(d[k]);
            if constexpr (B == 8u) { uint32_t s = d[0]; d[0] = d[1]; d[1] = s; s = d[2]; d[2] = d[3]; d[3] = s; }
        }
    }
    if (pred2) {
        A x[E];
#pragma unroll
        for (uint32_t j = 0; j < E; j++) {
            if constexpr (B == 8u) x[j] = (uint64_t)d[2u * j] | ((uint64_t)d[2u * j + 1u] << 32);
            else if constexpr (B == 4u) x[j] = d[j];
            else x[j] = (d[j * B / 4u] >> (8u * ((j * B) & 3u))) & (B == 1u ? 0xFFu : 0xFFFFu);
        }
#pragma unroll
        for (uint32_t j = S; j < E; j++) x[j] += x[j - S];
        A U[S], T[S];
#pragma unroll
        for (uint32_t p = 0; p < S; p++) {                        // the last word of phase p, if the lane has one
            constexpr uint32_t none = 0xFFFFFFFFu;
            const uint32_t jl = p < E ? p + (E - 1u - p) / S * S : none;
            U[p] = jl != none ? x[jl < E ? jl : 0u] : (A)0;
        }
        constexpr bool ALIGNED = 16u % (S * B) == 0u;
        const uint32_t phase = ALIGNED ? 0u : (uint32_t)((q / B) % S);
        if constexpr (ALIGNED) {
#pragma unroll
            for (uint32_t c = 0; c < S; c++) T[c] = U[c];
        } else {
#pragma unroll
            for (uint32_t c = 0; c < S; c++) {                    // channel c is the lane's phase (c - phase) mod S
                const uint32_t s = c + S - phase, idx = s >= S ? s - S : s;
                T[c] = 0;
#pragma unroll
                for (uint32_t p = 0; p < S; p++) T[c] = idx == p ? U[p] : T[c];
            }
        }
        A ex[S];
#pragma unroll
        for (uint32_t c = 0; c < S; c++) {
            A s = T[c];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const A t = __shfl_up(s, o, 64);
                if (lir >= (uint32_t)o) s += t;
            }
            const A tot = __shfl(s, (int)((threadIdx.x & 63u) | (lpr - 1u)), 64);
            ex[c] = s - T[c] + carry[c];
            carry[c] += tot;
        }
        A basep[S];
        if constexpr (ALIGNED) {
#pragma unroll
            for (uint32_t p = 0; p < S; p++) basep[p] = ex[p];
        } else {
#pragma unroll
            for (uint32_t p = 0; p < S; p++) {                    // phase p is channel (phase + p) mod S
                const uint32_t s = phase + p, idx = s >= S ? s - S : s;
                basep[p] = 0;
#pragma unroll
                for (uint32_t c = 0; c < S; c++) basep[p] = idx == c ? ex[c] : basep[p];
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < E; j++) x[j] += basep[j % S];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) d[k] = 0u;
#pragma unroll
        for (uint32_t j = 0; j < E; j++) {
            if constexpr (B == 8u) { d[2u * j] = (uint32_t)x[j]; d[2u * j + 1u] = (uint32_t)(x[j] >> 32); }
            else if constexpr (B == 4u) d[j] = x[j];
            else d[j * B / 4u] |= (x[j] & (B == 1u ? 0xFFu : 0xFFFFu)) << (8u * ((j * B) & 3u));
        }
    }
    v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3];
}

// what a wave needs of one chunk: its rows at src (rb bytes each), the rows' place in the slot, what of them lies inside the image
struct RowsOf {
    const uint8_t* src; uint8_t* tmp; uint8_t* dst;
    uint64_t rb, dpitch, vb;      // bytes of a chunk row, of a slot row, of a chunk row inside the image
    uint32_t vh;                  // rows inside the image
    bool be, pred2;
};

// predictors 1 and 2: row groups [w0, ...) in steps of nw -- a group is 64 / lpr rows, lpr the lanes a row's vb bytes need (64: a row a
// wave, 1 KiB a step, the carry going from step to step)
template <uint32_t B, uint32_t S>
__device__ void rows_words(const RowsOf& c, uint32_t w0, uint32_t nw) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lg = 6u;
    if (c.vb <= 512u) { lg = 0u; while ((16ull << lg) < c.vb) lg++; }
    const uint32_t lpr = 1u << lg, R = 64u >> lg, lir = lane & (lpr - 1u);
    const uint64_t groups = ((uint64_t)c.vh + R - 1u) / R;
    for (uint64_t rg = w0; rg < groups; rg += nw) {
        const uint64_t row = rg * R + (lane >> lg);
        const bool active = row < c.vh;
        Acc<B> carry[S];
#pragma unroll
        for (uint32_t k = 0; k < S; k++) carry[k] = 0;
        for (uint64_t q0 = 0; q0 < c.vb; q0 += 1024u) {
            const uint64_t q = q0 + 16u * lir;
            const uint32_t n = !active || q >= c.vb ? 0u : c.vb - q < 16u ? (uint32_t)(c.vb - q) : 16u;
            v4 v = load16(c.src + row * c.rb + q, n);
            step_words<B, S>(v, c.be, c.pred2, q, lir, lpr, carry);
            store16(c.dst + row * c.dpitch + q, v, n);
        }
    }
}

// predictor 3: a row a wave.  First the byte sums over the WHOLE chunk row (the planes follow each other: a running sum crosses their
// borders) into the chunk's place in the scratch -- in place for a deflate chunk, out of the file for a stored one --, then the B
// planes of N = rb / B bytes are read back, 16 / B floats a lane, the most significant plane first, and stored as little-endian words.
// The planes of a row lie N bytes apart, N being anything up to 2^29: they go through memory the wave has just written (the L2 holds
// it), not through LDS, which would bound the row.
template <uint32_t B, uint32_t S>
__device__ void rows_planes(const RowsOf& c, uint32_t w0, uint32_t nw) {
    const uint32_t lane = threadIdx.x & 63u;
    constexpr uint32_t V = 16u / B;                               // floats a lane
    const uint64_t N = c.rb / B, ve = c.vb / B;
    for (uint64_t row = w0; row < c.vh; row += nw) {
        const uint8_t* s = c.src + row * c.rb;
        uint8_t* t = c.tmp + row * c.rb;
        uint32_t carry[S];
#pragma unroll
        for (uint32_t k = 0; k < S; k++) carry[k] = 0u;
        for (uint64_t q0 = 0; q0 < c.rb; q0 += 1024u) {
            const uint64_t q = q0 + 16u * lane;
            const uint32_t n = q >= c.rb ? 0u : c.rb - q < 16u ? (uint32_t)(c.rb - q) : 16u;
            v4 v = load16(s + q, n);
            step_words<1u, S>(v, false, true, q, lane, 64u, carry);
            store16(t + q, v, n);
        }
        __threadfence();                                          // the sums are in memory, and no stale line answers for them
        for (uint64_t e0 = 0; e0 < ve; e0 += 64u * V) {
            const uint64_t e = e0 + (uint64_t)lane * V;
            if (e >= ve) continue;
            const uint32_t m = ve - e < V ? (uint32_t)(ve - e) : V;
            uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t p = 0; p < B; p++) {                    // plane p holds byte B - 1 - p of every word
                const uint8_t* pl = t + p * N + e;
                uint32_t bytes;
                if (m == V) bytes = B == 4u ? *reinterpret_cast<const u32u*>(pl) : (uint32_t)*reinterpret_cast<const u16u*>(pl);
                else bytes = load_tail(pl, (int32_t)m);
#pragma unroll
                for (uint32_t j = 0; j < V; j++) {
                    const uint32_t at = j * B + (B - 1u - p);     // the byte's place among the lane's 16
                    d[at >> 2] |= ((bytes >> (8u * j)) & 0xFFu) << (8u * (at & 3u));
                }
            }
            v4 v;
            v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3];
            store16(c.dst + row * c.dpitch + e * B, v, m * B);
        }
    }
}

// A workgroup is UNP_WAVES waves; blockIdx.y strides over the slots of the chunk list, blockIdx.x and the wave over the rows of a chunk.
__global__ __launch_bounds__(64 * UNP_WAVES) void k_tiff_unpredict(TiffArgs a) {
    const uint32_t w0 = blockIdx.x * UNP_WAVES + (threadIdx.x >> 6), nw = gridDim.x * UNP_WAVES;
    const uint64_t total = a.head[0];
    for (uint64_t c = blockIdx.y; c < total; c += gridDim.y) {
        Chunk q;
        if (!chunk_of(a, c, q) || a.cst[c] != HDLZ_OK) continue;  // (uniform, as every `continue` of this loop)
        const hdlz_tiff_image& r = q.r;
        const bool stored = !deflated(r);
        if (!stored && (a.status[c] != HDLZ_OK || a.len[c] != q.raw_c)) continue;      // only a stream of exactly the chunk's bytes has rows
        const uint64_t tx = q.k % q.g.across, ty = q.k / q.g.across;
        const uint64_t x0 = tx * r.tile_w, y0 = ty * r.tile_h;
        const uint32_t px = q.g.px, B = r.bits >> 3;
        RowsOf rows;
        rows.tmp = a.m_dst[c];
        rows.src = stored ? a.in + stored_at(a, q) : rows.tmp;
        rows.rb = (uint64_t)r.tile_w * px; rows.dpitch = (uint64_t)r.width * px;
        rows.vb = (r.width - x0 < r.tile_w ? r.width - x0 : r.tile_w) * px;
        rows.vh = (uint32_t)(r.height - y0 < r.tile_h ? r.height - y0 : r.tile_h);
        rows.dst = a.out + (r.out_off - a.images[0].out_off) + (y0 * r.width + x0) * px;
        rows.be = r.big_endian != 0u; rows.pred2 = r.predictor == 2u;
#define HDLZ_TIFF_S(F, BB) \
        switch (r.samples) { \
            case 1u: F<BB, 1u>(rows, w0, nw); break; case 2u: F<BB, 2u>(rows, w0, nw); break; case 3u: F<BB, 3u>(rows, w0, nw); break; \
            case 4u: F<BB, 4u>(rows, w0, nw); break; case 5u: F<BB, 5u>(rows, w0, nw); break; case 6u: F<BB, 6u>(rows, w0, nw); break; \
            case 7u: F<BB, 7u>(rows, w0, nw); break; default: F<BB, 8u>(rows, w0, nw); break; \
        }
        if (r.predictor == 3u) {
            if (B == 4u) { HDLZ_TIFF_S(rows_planes, 4u) } else { HDLZ_TIFF_S(rows_planes, 8u) }
        } else if (B == 1u) { HDLZ_TIFF_S(rows_words, 1u) }
        else if (B == 2u) { HDLZ_TIFF_S(rows_words, 2u) }
        else if (B == 4u) { HDLZ_TIFF_S(rows_words, 4u) }
        else { HDLZ_TIFF_S(rows_words, 8u) }
#undef HDLZ_TIFF_S
    }
}

// ---- (e) the judgement: a wave per image, a lane per chunk; the image's status is that of its lowest failed chunk
__global__ __launch_bounds__(64) void k_tiff_judge(TiffArgs a) {
    const uint32_t lane = threadIdx.x;
    for (uint64_t b = blockIdx.x; b < a.count; b += gridDim.x) {
        uint32_t st = a.verdict[b];
        if (st == HDLZ_OK) {
            const hdlz_tiff_image r = a.images[b];
            Geometry g{};
            geometry(r.width, r.height, r.tile_w, r.tile_h, r.tiled != 0u, r.samples, r.bits, g);
            const uint64_t tf = tiles_of(g.full);
            uint64_t bad = NONE64;
            uint32_t bad_st = HDLZ_OK;
            for (uint64_t k = lane; k < g.nchunks && bad == NONE64; k += 64u) {
                const uint64_t c = a.cb[b] + k, raw_c = k + 1u == g.nchunks ? g.last : g.full;
                uint32_t s = a.cst[c];
                if (s == HDLZ_OK && deflated(r)) s = a.status[c];
                if (s == HDLZ_OK && deflated(r)) {
                    const uint64_t at = a.single ? a.m_off[0] : a.m_off[c] - 2u, cnt = (a.single ? a.m_end[0] : a.m_end[c]) - at;
                    const uint8_t* z = a.in + at;
                    const uint32_t len = a.len[c], eb = a.end_bit[c];
                    const uint64_t end = a.single ? eb : (eb + 7u) >> 3;      // bytes from the stream's first to the end of the final block
                    const uint32_t cmf = z[0], flg = z[1];
                    if (HDLZ_ZLIB_HEADER_BAD(cmf, flg)) s = HDLZ_E_BAD_HEADER;
                    else if (len > raw_c) s = HDLZ_E_OUT_CAPACITY;
                    else if (len < raw_c) s = HDLZ_E_BAD_CHECKSUM;
                    else if (end + 4u > cnt) s = HDLZ_E_NO_EOF;
                    else {
                        const uint32_t nt = (uint32_t)tiles_of(raw_c);
                        const uint2* tiles = a.tiles + a.tb[b] + k * tf;
                        uint64_t A64 = 0, C64 = 0;
                        for (uint32_t t = 0; t < nt; t++) { const uint2 w = tiles[t]; fold_tile(A64, C64, t, w.x, w.y); }
                        if (adler32_from((uint32_t)(A64 % ADLER_MOD), (uint32_t)(C64 % ADLER_MOD), raw_c) != load_be32(z + end)) s = HDLZ_E_BAD_CHECKSUM;
                    }
                }
                if (s != HDLZ_OK) { bad = k; bad_st = s; }
            }
            uint64_t low = bad;
#pragma unroll
            for (int ofs = 32; ofs > 0; ofs >>= 1) { const uint64_t o = __shfl_xor(low, ofs, 64); low = o < low ? o : low; }
            if (low != NONE64) st = (uint32_t)__shfl((int)bad_st, (int)(low & 63u), 64);      // (chunk k is lane k mod 64's)
        }
        if (lane == 0u) {
            a.fin[b] = st;
            if (a.image_status) a.image_status[b] = st;
        }
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_tiff_finish(TiffArgs a) {
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
    hdlz_tiff_decode_result res;
    res.out_len = 0u; res.first_bad = NONE64; res.status = HDLZ_OK; res.reserved = 0u;
    if (s_f[0] != NONE64) { res.status = a.fin[s_f[0]]; res.first_bad = s_f[0]; }
    else if (a.count) {
        const hdlz_tiff_image last = a.images[a.count - 1u];
        res.out_len = last.out_off - a.images[0].out_off + last.out_len;
    }
    *a.result = res;
}

static unsigned grid_of(uint64_t want, uint64_t most) { return (unsigned)(want < 1u ? 1u : want < most ? want : most); }

}  // namespace tiff

size_t tiff_index_work_bytes(uint64_t n) { return 256u + round256(3u * sizeof(uint64_t) * (size_t)n); }

hipError_t launch_tiff_index(const uint8_t* files, uint64_t files_len, const uint64_t* file_off, const uint64_t* file_len, const uint32_t* pages, uint64_t n,
                             uint32_t out_align, uint64_t image_cap, hdlz_tiff_image* images, hdlz_tiff_index_result* result, void* work, hipStream_t stream) {
    using namespace tiff;
    const IndexWork w = index_work(work, n);
    hipError_t e = hipSuccess;
    if (n) e = launch(k_tiff_parse, dim3((unsigned)((n + 255u) / 256u)), dim3(256), stream, files, files_len, file_off, file_len, pages, n, image_cap, images, w);
    if (e == hipSuccess) e = launch(k_tiff_offsets, dim3(1), dim3(SCAN_THREADS), stream, n, image_cap, out_align, images, result, w);
    return e;
}

// in front of the decode: the checks of the records, the chunk list
hipError_t launch_tiff_front(const TiffArgs& a, hipStream_t stream) {
    using namespace tiff;
    if (a.count == 0) return hipSuccess;
    hipError_t e = launch(k_tiff_plan, dim3(1), dim3(SCAN_THREADS), stream, a);
    if (e == hipSuccess && a.chunk_cap) e = launch(k_tiff_chunks, dim3((unsigned)((a.chunk_cap + JT - 1u) / JT)), dim3(JT), stream, a);
    return e;
}

// behind the decode: the Adler tiles, the unpredict, the verdicts and the record
hipError_t launch_tiff_back(const TiffArgs& a, hipStream_t stream) {
    using namespace tiff;
    hipError_t e = hipSuccess;
    if (a.count) {
        if (a.chunk_cap) {
            e = launch(k_tiff_adler, dim3(grid_of(a.tile_cap, 8192u)), dim3(64 * ADLER_TILE_WAVES), stream, a);
            // a workgroup's waves take a row (or a group of short rows) each: about 16 KiB of an average chunk a workgroup
            if (e == hipSuccess) e = launch(k_tiff_unpredict, dim3(grid_of(a.raw_bytes / a.chunk_cap / 16384u, 1024u), grid_of(a.chunk_cap, 16384u)),
                                            dim3(64 * UNP_WAVES), stream, a);
        }
        if (e == hipSuccess) e = launch(k_tiff_judge, dim3(grid_of(a.count, 65536u)), dim3(64), stream, a);
    }
    if (e == hipSuccess) e = launch(k_tiff_finish, dim3(1), dim3(SCAN_THREADS), stream, a);
    return e;
}

}  // namespace hdlz
