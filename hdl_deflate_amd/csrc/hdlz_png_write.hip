// hdlz_png_write.hip -- the kernels of include/hdlz_png_write.h: PNG files written on the device.
//
// hdlz_png_filter_ws:
// k_pngw_plan     ONE workgroup over the images: the checks of a spec, the exclusive scans of raw_len (raw_off), of the rows and of the
//                 bands of HDLZ_PNGW_BAND rows -> d_status, d_raw_off and the plan in the scratch.
// k_pngw_filter   the hot path, a WAVE per band of one image (a search in the plan's band prefix; the grid comes from the host's
//                 total_rows and strides).  A wave step is 1 KiB of a row: lane l loads the 16 bytes at 16 l of the row and of the
//                 row above (unaligned 16-byte loads; the last, partial piece of a row by bytes, so no load leaves the row), swaps
//                 16-bit samples in registers, takes the 8 bytes to its left from lane l - 1 (lane 0: from lane 63 of the step
//                 before, carried) and so has a, b, c of all its 16 bytes in registers.  Sub, Up, Average and the cost of a byte are
//                 SWAR words; Paeth goes byte by byte.  Adaptive mode: the five sums per lane, reduced across the wave (64 bits for
//                 rows of several steps).  A row of at most one step takes only the lanes it needs and the wave several rows at a
//                 time (filter_narrow), all five filters' words kept for the choice; a row of up to ROW_REG_MAX = 4 steps keeps its
//                 pieces in registers and the chosen filter's bytes come from them; a wider row is loaded once more (the wave
//                 read it a moment ago, but the rows in flight exceed the L2: profiles/png_write.txt).  The output
//                 row starts at any alignment (pitch row_bytes + 1): a step's 1 KiB is staged in the wave's LDS and leaves as single
//                 bytes up to the next 16-byte boundary of d_raw, whole aligned 16-byte pieces, single bytes behind them -- every
//                 byte is stored by the wave that owns it, none is read back.
// hdlz_png_write_ws:
// k_pngw_scan     ONE workgroup over the blocks, a run a thread: the exclusive prefixes of |M_b|, of the counts of failed and of
//                 contradictory rows (one word, as k_zipw_scan), and of the three sums the Adler-32 combination of hdlz_join.hip adds up.
// k_pngw_layout   ONE workgroup over the images: the checks, zlen, the Adler-32, file_len; the scans -> d_file_off, d_file_len, the
//                 records, the CRC list's chunk prefix, the result record.
// k_pngw_gather   a wave per block: M_b to its place, cut at the chunk seams (stream byte s lies at 41 + s + 12 (s / idat_len) of the
//                 file), k_join's loop per piece; and a wave per image: signature, IHDR, every chunk's length and type, 78 9C, the
//                 stream's tail (or the whole stored stream), IEND.
// k_pngw_crc      a workgroup per IHDR / IDAT chunk: crc_block over type and data, the word stored behind them.
// Plain stores only; no workgroup waits for another.
// The planners' strip and scan, the searches and the rows' verdict are hdlz_plan.h's; the format's facts shared with the reader:
// hdlz_png_rules.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_compress_common.h"                        // member_len
#include "hdlz_crc32.h"
#include "hdlz_frame.h"
#include "hdlz_adler.h"
#include "hdlz_plan.h"
#include "hdlz_png_rules.h"

namespace hdlz {
namespace pngw {

constexpr uint32_t BAND = HDLZ_PNGW_BAND, STEP = HDLZ_PNGW_STEP, KREG = HDLZ_PNGW_ROW_REG_MAX / HDLZ_PNGW_STEP;
using namespace png;                                     // hdlz_png_rules.h
constexpr uint32_t PLAN_THREADS = 1024u, PLAN_WAVES = PLAN_THREADS / 64u;
constexpr uint64_t NONE64 = ~0ull;
constexpr uint32_t FIRST_DATA = SIG_IHDR_END + 8u;      // the first IDAT's data
constexpr uint32_t STORED_HEAD = 7u, Z_TAIL = 6u;        // 78 9C 01 LEN NLEN; 03 00 + Adler-32
constexpr uint32_t CRC_GROUPS_MAX = 4096u, FILTER_GRID_MAX = 1u << 20;


// the first three lines of the per-image refusals; rb = row_bytes, bpp as the header states them.  The pairs that are written are
// those of pair_ok (hdlz_png_rules.h) with whole bytes a sample and without a palette, spelled out here: the filter kernel calls this
// for rb and bpp, and the test's text is part of its instruction sequence (profiles/planner_shared.txt, section 3)
__device__ __forceinline__ uint32_t check_spec(const hdlz_png_spec& s, uint64_t& rb, uint64_t& raw_len, uint32_t& bpp) {
    rb = 0u; raw_len = 0u; bpp = 1u;
    if (s.width == 0u || s.height == 0u || s.width >= 0x80000000u || s.height >= 0x80000000u) return HDLZ_E_BAD_HEADER;
    const bool pair = (s.colour == 0u || s.colour == 2u || s.colour == 4u || s.colour == 6u) && (s.depth == 8u || s.depth == 16u);
    bool res = false;
    for (int k = 0; k < 6; k++) res = res || s.reserved[k] != 0u;
    if (!pair || res) return HDLZ_E_BAD_HEADER;
    bpp = channels_of(s.colour) * (s.depth >> 3);
    rb = (uint64_t)s.width * bpp;
    if (rb + 1u > RAW_MAX / s.height) return HDLZ_E_OUT_CAPACITY;
    raw_len = (uint64_t)s.height * (rb + 1u);
    return HDLZ_OK;
}

// ---- hdlz_png_filter_ws: the plan.  A strip of the images a thread (hdlz_plan.h)
__global__ __launch_bounds__(PLAN_THREADS) void k_pngw_plan(PngFilterArgs a) {
    __shared__ uint64_t s_wave[3][PLAN_WAVES];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = a.n;
    uint64_t lo, hi;
    strip(n, PLAN_THREADS, tid, lo, hi);
    uint64_t mine[3] = {0u, 0u, 0u}, base[3], total[3];           // raw_len, rows, bands
    for (uint64_t i = lo; i < hi; i++) {
        const hdlz_png_spec s = a.specs[i];
        uint64_t rb, raw_len;
        uint32_t bpp;
        uint32_t st = check_spec(s, rb, raw_len, bpp);
        if (st == HDLZ_OK && (s.pix_off > a.pix_len || (uint64_t)s.height * rb > a.pix_len - s.pix_off)) st = HDLZ_E_BAD_PARAM;
        a.status[i] = st;
        if (st == HDLZ_OK) { mine[0] += raw_len; mine[1] += s.height; mine[2] += ((uint64_t)s.height + BAND - 1u) / BAND; }
    }
    block_scan<3, PLAN_THREADS>(mine, base, total, s_wave);
    for (uint64_t i = lo; i < hi; i++) {
        a.raw_off[i] = base[0]; a.row_base[i] = base[1]; a.band_base[i] = base[2];
        if (a.status[i] != HDLZ_OK) continue;
        const hdlz_png_spec s = a.specs[i];
        uint64_t rb, raw_len;
        uint32_t bpp;
        (void)check_spec(s, rb, raw_len, bpp);
        if (base[0] + raw_len > a.raw_cap) a.status[i] = HDLZ_E_OUT_CAPACITY;      // (it keeps its bands: the waves that find it pass on)
        base[0] += raw_len; base[1] += s.height; base[2] += ((uint64_t)s.height + BAND - 1u) / BAND;
    }
    if (tid == 0u) { a.raw_off[n] = total[0]; a.row_base[n] = total[1]; a.band_base[n] = total[2]; }
}

// ---- the filter.  A piece: the 16 bytes of a lane of the row (x) and of the row above (b), and the 8 bytes in front of each
struct Piece { v4 x, b; uint32_t px0, px1, pb0, pb1; };

template <bool D16> __device__ __forceinline__ uint32_t swap16(uint32_t v) {
    if constexpr (D16) return ((v & 0x00FF00FFu) << 8) | ((v >> 8) & 0x00FF00FFu);
    else return v;
}
// the 16 bytes at q of a row of rb bytes (q a multiple of 16); bytes at or behind rb read as zero and are not loaded
template <bool D16>
__device__ __forceinline__ v4 load16(const uint8_t* __restrict__ row, uint64_t q, uint64_t rb) {
    v4 v = {0u, 0u, 0u, 0u};
    if (q + 16u <= rb) v = *reinterpret_cast<const v4u*>(row + q);
    else if (q < rb) {
        const uint32_t cnt = (uint32_t)(rb - q);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < 16u; j++)
            if (j < cnt) w[j >> 2] |= (uint32_t)row[q + j] << (8u * (j & 3u));
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    }
    v.x = swap16<D16>(v.x); v.y = swap16<D16>(v.y); v.z = swap16<D16>(v.z); v.w = swap16<D16>(v.w);
    return v;
}
// step s of a row; carry: the last 8 bytes of the step before (x, then b), zero in front of the row -- updated for the next step
template <bool D16>
__device__ __forceinline__ Piece load_piece(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ up, uint64_t s, uint32_t lane, uint64_t rb, uint32_t (&carry)[4]) {
    Piece p;
    const uint64_t q = s * STEP + 16u * lane;
    p.x = load16<D16>(cur, q, rb);
    if (up) p.b = load16<D16>(up, q, rb);
    else p.b = v4{0u, 0u, 0u, 0u};
    p.px0 = __shfl_up(p.x.z, 1, 64); p.px1 = __shfl_up(p.x.w, 1, 64);
    p.pb0 = __shfl_up(p.b.z, 1, 64); p.pb1 = __shfl_up(p.b.w, 1, 64);
    if (lane == 0u) { p.px0 = carry[0]; p.px1 = carry[1]; p.pb0 = carry[2]; p.pb1 = carry[3]; }
    carry[0] = __shfl(p.x.z, 63, 64); carry[1] = __shfl(p.x.w, 63, 64); carry[2] = __shfl(p.b.z, 63, 64); carry[3] = __shfl(p.b.w, 63, 64);
    return p;
}
// ---- the arithmetic: four bytes a word (SWAR) wherever the bytes do not talk to each other -- x - a, x - b and the Average's
// (a + b) >> 1 --, as is the cost |int8(y)| of a filtered byte; only Paeth goes byte by byte (its p = a + b - c takes ten bits).
constexpr uint32_t H8 = 0x80808080u;
__device__ __forceinline__ uint32_t sub4(uint32_t x, uint32_t p) { return ((x | H8) - (p & ~H8)) ^ ((x ^ ~p) & H8); }      // x - p, every byte mod 256
__device__ __forceinline__ uint32_t avg4(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) & 0xFEFEFEFEu) >> 1); }
__device__ __forceinline__ uint32_t paeth4(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t aj = (a >> (8u * j)) & 255u, bj = (b >> (8u * j)) & 255u, cj = (c >> (8u * j)) & 255u;
        const uint32_t pa = __builtin_amdgcn_sad_u8(bj, cj, 0u), pb = __builtin_amdgcn_sad_u8(aj, cj, 0u);
        const int32_t t = (int32_t)(aj + bj) - (int32_t)(2u * cj);
        const uint32_t pc = (uint32_t)(t < 0 ? -t : t);
        r |= ((pa <= pb && pa <= pc) ? aj : pb <= pc ? bj : cj) << (8u * j);      // ties: a, then b, then c
    }
    return r;
}
// acc + the sum over the word's bytes of (y < 128 ? y : 256 - y)
__device__ __forceinline__ uint32_t cost4(uint32_t y, uint32_t acc) {
    const uint32_t sb = y & H8, s = (sb << 1) - (sb >> 7);       // FF in every byte at or above 128: there 256 - y = (y ^ FF) + 1
    return __builtin_amdgcn_sad_u8(y ^ s, 0u, acc) + (uint32_t)__builtin_popcount(sb);
}
// the words of a piece: x and b as they are; a and c, the same bytes BPP to the left, from the 8 bytes in front
struct Words { uint32_t x[4], a[4], b[4], c[4]; };
template <uint32_t BPP>
__device__ __forceinline__ Words words_of(const Piece& p) {
    const uint32_t wx[6] = {p.px0, p.px1, p.x.x, p.x.y, p.x.z, p.x.w}, wb[6] = {p.pb0, p.pb1, p.b.x, p.b.y, p.b.z, p.b.w};
    Words w;
    static_for<0, 4>([&](auto k) {
        constexpr uint32_t K = (uint32_t)decltype(k)::value, t = 8u + 4u * K - BPP, lo = t >> 2, sh = t & 3u;
        w.x[K] = wx[2u + K]; w.b[K] = wb[2u + K];
        if constexpr (sh == 0u) { w.a[K] = wx[lo]; w.c[K] = wb[lo]; }
        else { w.a[K] = __builtin_amdgcn_alignbyte(wx[lo + 1u], wx[lo], sh); w.c[K] = __builtin_amdgcn_alignbyte(wb[lo + 1u], wb[lo], sh); }
    });
    return w;
}
template <uint32_t F> __device__ __forceinline__ uint32_t filter4(uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    if constexpr (F == 0u) return x;
    else if constexpr (F == 1u) return sub4(x, a);
    else if constexpr (F == 2u) return sub4(x, b);
    else if constexpr (F == 3u) return sub4(x, avg4(a, b));
    else return sub4(x, paeth4(a, b, c));
}
// FF in the bytes of word k that lie among a piece's first `valid` bytes
__device__ __forceinline__ uint32_t valid_mask(uint32_t valid, uint32_t k) {
    return valid >= 4u * k + 4u ? 0xFFFFFFFFu : valid <= 4u * k ? 0u : (1u << (8u * (valid - 4u * k))) - 1u;
}
// all five filters of a piece: the filtered words Y[f] and the five sums of its first `valid` bytes
template <uint32_t BPP>
__device__ __forceinline__ void piece_all(const Piece& p, uint32_t valid, uint32_t (&Y)[5][4], uint32_t (&S)[5]) {
    const Words w = words_of<BPP>(p);
#pragma unroll
    for (int f = 0; f < 5; f++) S[f] = 0u;
    static_for<0, 4>([&](auto k) {
        constexpr uint32_t K = (uint32_t)decltype(k)::value;
        const uint32_t vm = valid_mask(valid, K);
        static_for<0, 5>([&](auto f) {
            constexpr uint32_t F = (uint32_t)decltype(f)::value;
            Y[F][K] = filter4<F>(w.x[K], w.a[K], w.b[K], w.c[K]);
            S[F] = cost4(Y[F][K] & vm, S[F]);
        });
    });
}
template <uint32_t BPP, uint32_t F>
__device__ __forceinline__ v4 piece_filter(const Piece& p) {
    if constexpr (F == 0u) return p.x;
    const Words w = words_of<BPP>(p);
    return v4{filter4<F>(w.x[0], w.a[0], w.b[0], w.c[0]), filter4<F>(w.x[1], w.a[1], w.b[1], w.c[1]), filter4<F>(w.x[2], w.a[2], w.b[2], w.c[2]),
              filter4<F>(w.x[3], w.a[3], w.b[3], w.c[3])};
}
template <uint32_t BPP>
__device__ __forceinline__ v4 piece_filter_any(const Piece& p, uint32_t f) {      // (f is uniform over the wave)
    switch (f) {
        case 0u: return piece_filter<BPP, 0u>(p);
        case 1u: return piece_filter<BPP, 1u>(p);
        case 2u: return piece_filter<BPP, 2u>(p);
        case 3u: return piece_filter<BPP, 3u>(p);
        default: return piece_filter<BPP, 4u>(p);
    }
}
// the filtered bytes y of a GROUP of `lanes` lanes (sl: this lane's place in it; it holds bytes [16 sl, 16 sl + 16)) -> dst[0 .. len),
// len <= 16 lanes, dst at any alignment.  stage: the wave's STEP / 4 + 8 words of LDS, a group's bytes at `gbase` (a multiple of 16).
__device__ __forceinline__ void store_group(uint8_t* __restrict__ dst, v4 y, uint32_t len, uint32_t* stage, uint32_t lane, uint32_t sl, uint32_t lanes, uint32_t gbase) {
    *reinterpret_cast<v4*>(stage + 4u * lane) = y;
    wave_lds_order();
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(stage) + gbase;
    const uint32_t head = min(len, (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u));
    for (uint32_t j = sl; j < head; j += lanes) dst[j] = sb[j];  // (a group of fewer than 15 lanes takes more than one turn)
    const uint32_t nvec = (len - head) >> 4;                      // at most the group's lanes
    if (sl < nvec) {
        const uint32_t o = head + 16u * sl, w0 = (gbase + o) >> 2, sh = o & 3u;
        const uint32_t a0 = stage[w0], a1 = stage[w0 + 1u], a2 = stage[w0 + 2u], a3 = stage[w0 + 3u], a4 = stage[w0 + 4u];      // (a4: the next group's or the padding when sh == 0, and then not used)
        v4 v;
        v.x = __builtin_amdgcn_alignbyte(a1, a0, sh); v.y = __builtin_amdgcn_alignbyte(a2, a1, sh);
        v.z = __builtin_amdgcn_alignbyte(a3, a2, sh); v.w = __builtin_amdgcn_alignbyte(a4, a3, sh);
        *reinterpret_cast<v4*>(dst + o) = v;
    }
    const uint32_t done = head + 16u * nvec;                      // at most 15 bytes are left
    for (uint32_t j = done + sl; j < len; j += lanes) dst[j] = sb[j];
    wave_lds_order();                                             // (the next step overwrites the stage)
}
__device__ __forceinline__ void store_step(uint8_t* __restrict__ dst, v4 y, uint32_t len, uint32_t* stage, uint32_t lane) { store_group(dst, y, len, stage, lane, lane, 64u, 0u); }
__device__ __forceinline__ uint64_t wave_add64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one row of more than one step: cur / up (null above the first row) -> dst[0 .. rb + 1); returns the row's filter
template <uint32_t BPP, bool D16>
__device__ __forceinline__ uint32_t filter_row(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ up, uint64_t rb, uint32_t mode,
                                               uint8_t* __restrict__ dst, uint32_t* stage, uint32_t lane) {
    const uint64_t nsteps = (rb + STEP - 1u) / STEP;
    auto valid_of = [&](uint64_t s) -> uint32_t {
        const uint64_t q = s * STEP + 16u * lane;
        return q >= rb ? 0u : rb - q < 16u ? (uint32_t)(rb - q) : 16u;
    };
    auto len_of = [&](uint64_t s) -> uint32_t { return rb - s * STEP < STEP ? (uint32_t)(rb - s * STEP) : STEP; };
    auto choose = [&](const uint64_t (&S)[5]) -> uint32_t {
        uint32_t f = 0u;
        uint64_t best = wave_add64(S[0]);
#pragma unroll
        for (uint32_t k = 1; k < 5u; k++) { const uint64_t t = wave_add64(S[k]); if (t < best) { best = t; f = k; } }
        return f;
    };
    uint32_t f = mode;
    if (mode == HDLZ_PNG_FILTER_ADAPTIVE && nsteps <= KREG) {
        // the row stays in registers between the sums and the chosen filter's bytes
        Piece P[KREG];
        uint32_t carry[4] = {0u, 0u, 0u, 0u};
        uint64_t S[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t k = 0; k < KREG; k++)
            if (k < nsteps) {
                uint32_t Y[5][4], T[5];
                P[k] = load_piece<D16>(cur, up, k, lane, rb, carry);
                piece_all<BPP>(P[k], valid_of(k), Y, T);
#pragma unroll
                for (int q = 0; q < 5; q++) S[q] += T[q];
            }
        f = choose(S);
        if (lane == 0u) dst[0] = (uint8_t)f;
#pragma unroll
        for (uint32_t k = 0; k < KREG; k++)
            if (k < nsteps) store_step(dst + 1u + (uint64_t)k * STEP, piece_filter_any<BPP>(P[k], f), len_of(k), stage, lane);
        return f;
    }
    if (mode == HDLZ_PNG_FILTER_ADAPTIVE) {
        uint32_t carry[4] = {0u, 0u, 0u, 0u};
        uint64_t S[5] = {0u, 0u, 0u, 0u, 0u};
        for (uint64_t s = 0; s < nsteps; s++) {
            uint32_t Y[5][4], T[5];
            const Piece p = load_piece<D16>(cur, up, s, lane, rb, carry);
            piece_all<BPP>(p, valid_of(s), Y, T);
#pragma unroll
            for (int q = 0; q < 5; q++) S[q] += T[q];
        }
        f = choose(S);
    }
    if (lane == 0u) dst[0] = (uint8_t)f;
    uint32_t carry[4] = {0u, 0u, 0u, 0u};
    for (uint64_t s = 0; s < nsteps; s++) {
        const Piece p = load_piece<D16>(cur, up, s, lane, rb, carry);
        store_step(dst + 1u + s * STEP, piece_filter_any<BPP>(p, f), len_of(s), stage, lane);
    }
    return f;
}

// Rows of at most one step, SEVERAL A WAVE: a row takes the `lpr` lanes its bytes need (a power of two), the wave 64 / lpr rows at a
// time, so the rows of a small image fill the wave as the steps of a wide one do.  All five filters' words are kept between the sums
// and the choice, which is a group's own: no byte is computed twice and none is loaded twice.
template <uint32_t BPP, bool D16>
__device__ __forceinline__ void filter_narrow(const PngFilterArgs& a, const uint8_t* __restrict__ pix, uint8_t* __restrict__ raw, uint32_t rb, uint32_t r0, uint32_t r1,
                                              uint64_t row0, uint32_t* stage, uint32_t lane) {
    uint32_t lpr = 1u;
    while (16u * lpr < rb) lpr <<= 1;
    const uint32_t G = 64u / lpr, sl = lane & (lpr - 1u), grp = lane / lpr, gbase = 16u * lpr * grp;
    for (uint32_t rr = r0; rr < r1; rr += G) {
        const uint32_t r = rr + grp;
        const bool active = r < r1;
        const uint32_t n = active ? rb : 0u;                      // (a group without a row loads and stores nothing)
        const uint8_t* cur = pix + (uint64_t)r * rb;
        Piece p;
        p.x = load16<D16>(cur, 16u * sl, n);
        p.b = load16<D16>(cur - rb, 16u * sl, r ? n : 0u);       // (above the first row: not loaded)
        p.px0 = __shfl_up(p.x.z, 1, 64); p.px1 = __shfl_up(p.x.w, 1, 64);
        p.pb0 = __shfl_up(p.b.z, 1, 64); p.pb1 = __shfl_up(p.b.w, 1, 64);
        if (sl == 0u) { p.px0 = 0u; p.px1 = 0u; p.pb0 = 0u; p.pb1 = 0u; }
        uint32_t f = a.mode;
        v4 y;
        if (a.mode == HDLZ_PNG_FILTER_ADAPTIVE) {
            const uint32_t q = 16u * sl, valid = q >= n ? 0u : n - q < 16u ? n - q : 16u;
            uint32_t Y[5][4], S[5];
            piece_all<BPP>(p, valid, Y, S);
#pragma unroll
            for (int k = 0; k < 5; k++)
                for (uint32_t o = lpr >> 1; o > 0u; o >>= 1) S[k] += __shfl_xor(S[k], o, 64);      // (a row of 1 KiB: below 2^17)
            f = 0u;
            uint32_t best = S[0];
#pragma unroll
            for (uint32_t k = 1; k < 5u; k++) if (S[k] < best) { best = S[k]; f = k; }
            y = v4{Y[0][0], Y[0][1], Y[0][2], Y[0][3]};
#pragma unroll
            for (uint32_t k = 1; k < 5u; k++)
                if (f == k) y = v4{Y[k][0], Y[k][1], Y[k][2], Y[k][3]};
        } else y = piece_filter_any<BPP>(p, f);
        uint8_t* dst = raw + (uint64_t)r * (rb + 1u);
        if (active && sl == 0u) {
            dst[0] = (uint8_t)f;
            if (a.row_filter && row0 + r < a.total_rows) a.row_filter[row0 + r] = (uint8_t)f;
        }
        store_group(dst + 1u, y, n, stage, lane, sl, lpr, gbase);
    }
}

template <uint32_t BPP, bool D16>
__device__ void filter_band(const PngFilterArgs& a, const uint8_t* __restrict__ pix, uint8_t* __restrict__ raw, uint64_t rb, uint32_t r0, uint32_t r1,
                            uint64_t row0, uint32_t* stage, uint32_t lane) {
    if (rb <= STEP) return filter_narrow<BPP, D16>(a, pix, raw, (uint32_t)rb, r0, r1, row0, stage, lane);
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t f = filter_row<BPP, D16>(pix + (uint64_t)r * rb, r ? pix + (uint64_t)(r - 1u) * rb : nullptr, rb, a.mode, raw + (uint64_t)r * (rb + 1u), stage, lane);
        if (a.row_filter && lane == 0u && row0 + r < a.total_rows) a.row_filter[row0 + r] = (uint8_t)f;
    }
}

__global__ __launch_bounds__(256) void k_pngw_filter(PngFilterArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[4][STEP / 4u + 8u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t* stage = s_stage[wave];
    const uint64_t nbands = a.band_base[a.n];
    for (uint64_t g = (uint64_t)blockIdx.x * 4u + wave; g < nbands; g += (uint64_t)gridDim.x * 4u) {
        const uint64_t i = owner(a.band_base, a.n, g);
        if (a.status[i] != HDLZ_OK) continue;                    // (uniform over the wave)
        const hdlz_png_spec s = a.specs[i];
        uint64_t rb, raw_len;
        uint32_t bpp;
        (void)check_spec(s, rb, raw_len, bpp);
        const uint32_t r0 = (uint32_t)(g - a.band_base[i]) * BAND, r1 = s.height - r0 < BAND ? s.height : r0 + BAND;
        const uint8_t* pix = a.pix + s.pix_off;
        uint8_t* raw = a.raw + a.raw_off[i];
        const uint64_t row0 = a.row_base[i];
        const bool d16 = s.depth == 16u;
        switch (bpp) {
            case 1u: filter_band<1u, false>(a, pix, raw, rb, r0, r1, row0, stage, lane); break;
            case 2u: if (d16) filter_band<2u, true>(a, pix, raw, rb, r0, r1, row0, stage, lane); else filter_band<2u, false>(a, pix, raw, rb, r0, r1, row0, stage, lane); break;
            case 3u: filter_band<3u, false>(a, pix, raw, rb, r0, r1, row0, stage, lane); break;
            case 4u: if (d16) filter_band<4u, true>(a, pix, raw, rb, r0, r1, row0, stage, lane); else filter_band<4u, false>(a, pix, raw, rb, r0, r1, row0, stage, lane); break;
            case 6u: filter_band<6u, true>(a, pix, raw, rb, r0, r1, row0, stage, lane); break;
            default: filter_band<8u, true>(a, pix, raw, rb, r0, r1, row0, stage, lane); break;
        }
    }
}

// ---- hdlz_png_write_ws.  The prefixes over the rows: a strip of the blocks a thread
__global__ __launch_bounds__(PLAN_THREADS) void k_pngw_scan(PngWriteArgs a) {
    __shared__ uint64_t s_wave[5][PLAN_WAVES];
    const uint32_t tid = threadIdx.x;
    const uint64_t B = a.nblocks;
    uint64_t lo, hi;
    strip(B, PLAN_THREADS, tid, lo, hi);
    uint64_t mine[5] = {0u, 0u, 0u, 0u, 0u}, base[5], total[5];
    const uint64_t in0 = a.in_off[0];
    for (uint64_t b = lo; b < hi; b++) {
        uint64_t m = 0u, k = 0u, pa = 0u, pe = 0u, ps = 0u;
        if (a.status[b] != HDLZ_OK) k = 1u;
        else {
            uint32_t body;
            m = member_len(a.len[b], a.end_bits[b], a.pitch, body);
            const uint64_t i0 = a.in_off[b], i1 = a.in_off[b + 1u];
            if (i1 < i0 || i0 < in0) m = 0u;
            if (m == 0u) k = 1ull << COUNT_BITS;
            else {
                const uint8_t* t = a.rows + b * a.pitch + (a.len[b] - 4u);        // the row's trailer: s2 then s1, big-endian
                const uint32_t s2 = ((uint32_t)t[0] << 8) | t[1], s1 = ((uint32_t)t[2] << 8) | t[3];
                pa = (s1 % ADLER_MOD + ADLER_MOD - 1u) % ADLER_MOD;
                pe = ((i1 - in0) % ADLER_MOD) * pa % ADLER_MOD;
                ps = (s2 % ADLER_MOD + ADLER_MOD - (uint32_t)((i1 - i0) % ADLER_MOD)) % ADLER_MOD;
            }
        }
        a.pre[b] = m; a.cnt[b] = k; a.pa[b] = pa; a.pe[b] = pe; a.ps[b] = ps;
        mine[0] += m; mine[1] += k; mine[2] += pa; mine[3] += pe; mine[4] += ps;
    }
    block_scan<5, PLAN_THREADS>(mine, base, total, s_wave);
    for (uint64_t b = lo; b < hi; b++) {
        const uint64_t m = a.pre[b], k = a.cnt[b], pa = a.pa[b], pe = a.pe[b], ps = a.ps[b];
        a.pre[b] = base[0]; a.cnt[b] = base[1]; a.pa[b] = base[2]; a.pe[b] = base[3]; a.ps[b] = base[4];
        base[0] += m; base[1] += k; base[2] += pa; base[3] += pe; base[4] += ps;
    }
    if (tid == 0u) { a.pre[B] = total[0]; a.cnt[B] = total[1]; a.pa[B] = total[2]; a.pe[B] = total[3]; a.ps[B] = total[4]; }
}

// the writer's view of image i: its status (all lines of the header's list) and, when that is HDLZ_OK, zlen and the Adler-32
__device__ __forceinline__ uint32_t check_image(const PngWriteArgs& a, uint64_t i, const hdlz_png_spec& s, uint64_t& rb, uint64_t& raw_len, uint64_t& zlen, uint32_t& adler) {
    uint32_t bpp;
    zlen = 0u; adler = 0u;
    uint32_t st = check_spec(s, rb, raw_len, bpp);
    if (st != HDLZ_OK) return st;
    if (a.fstatus && a.fstatus[i] != HDLZ_OK) return a.fstatus[i];
    const uint64_t F0 = a.blk_first[i], F1 = a.blk_first[i + 1u];
    if (F0 > F1 || F1 > a.nblocks) return HDLZ_E_BAD_PARAM;
    if (F1 > F0) {
        st = rows_verdict(a.cnt, a.status, F0, F1);
        if (st != HDLZ_OK) return st;
        if (a.in_off[F1] - a.in_off[F0] != raw_len) return HDLZ_E_BAD_PARAM;
    } else if (raw_len >= 5u || !a.raw) return HDLZ_E_BAD_PARAM;
    if (a.raw_off[i + 1u] - a.raw_off[i] != raw_len) return HDLZ_E_BAD_PARAM;
    if (F1 > F0) {
        zlen = 2u + (a.pre[F1] - a.pre[F0]) + Z_TAIL;
        // the combination of hdlz_join.hip, the blocks' ends counted from the image's first byte
        const uint64_t A = (a.pa[F1] - a.pa[F0]) % ADLER_MOD, S = (a.ps[F1] - a.ps[F0]) % ADLER_MOD;
        const uint64_t start = (a.in_off[F0] - a.in_off[0]) % ADLER_MOD;
        const uint64_t EA = ((a.pe[F1] - a.pe[F0]) % ADLER_MOD + ADLER_MOD - start * A % ADLER_MOD) % ADLER_MOD;
        const uint64_t Nm = raw_len % ADLER_MOD;
        const uint32_t s1 = (uint32_t)((1u + A) % ADLER_MOD);
        const uint32_t s2 = (uint32_t)((Nm + Nm * A % ADLER_MOD + (ADLER_MOD - EA) + S) % ADLER_MOD);
        adler = (s2 << 16) | s1;
    } else {
        zlen = STORED_HEAD + raw_len + 4u;
        uint32_t s1 = 1u, s2 = 0u;
        const uint8_t* p = a.raw + a.raw_off[i];
        for (uint32_t j = 0; j < (uint32_t)raw_len; j++) { s1 += p[j]; s2 += s1; }      // (under 5 bytes: no reduction needed)
        adler = (s2 << 16) | s1;
    }
    return HDLZ_OK;
}

__global__ __launch_bounds__(PLAN_THREADS) void k_pngw_layout(PngWriteArgs a) {
    __shared__ uint64_t s_wave[5][PLAN_WAVES];
    __shared__ uint32_t s_worst[PLAN_WAVES];
    __shared__ uint64_t s_first[PLAN_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t n = a.n, amask = (uint64_t)a.out_align - 1u;
    uint64_t lo, hi;
    strip(n, PLAN_THREADS, tid, lo, hi);
    uint64_t mine[5] = {0u, 0u, 0u, 0u, 0u}, base[5], total[5];  // file_len, the index's z / raw / out slots, chunks of the CRC list
    uint32_t worst = HDLZ_OK;
    uint64_t first = NONE64;
    // (none of the 8 pairs is expanded: the samples HDLZ_PNG_EXPAND delivers take the scanlines' bytes, under either flag)
    auto out_len_of = [&](const hdlz_png_spec& s, uint64_t rb) { return (uint64_t)s.height * rb; };
    for (uint64_t i = lo; i < hi; i++) {
        const hdlz_png_spec s = a.specs[i];
        uint64_t rb, raw_len, zlen;
        uint32_t adler;
        const uint32_t st = check_image(a, i, s, rb, raw_len, zlen, adler);
        a.ist[i] = st; a.zlen[i] = zlen; a.adler[i] = adler;
        if (st == HDLZ_OK) {
            const uint64_t nidat = (zlen + a.idat - 1u) / a.idat;
            mine[0] += SIG_IHDR_END + zlen + CHUNK * nidat + CHUNK;
            if (zlen <= Z_MAX) { const Slots t = slots_of(zlen + 8u, raw_len, out_len_of(s, rb), amask); mine[1] += t.z; mine[2] += t.raw; mine[3] += t.out; }
            mine[4] += 1u + nidat;
        } else {
            worst = max(worst, st);
            first = first < i ? first : i;
        }
    }
    {
        const uint32_t rw = wave_max(worst);
        uint64_t rf = first;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint64_t t = __shfl_xor(rf, o, 64); rf = rf < t ? rf : t; }
        if (lane == 0u) { s_worst[wave] = rw; s_first[wave] = rf; }
    }
    block_scan<5, PLAN_THREADS>(mine, base, total, s_wave);      // (its barriers stand behind the stores of s_worst and s_first, too)
    worst = HDLZ_OK; first = NONE64;
    for (uint32_t k = 0; k < PLAN_WAVES; k++) { worst = max(worst, s_worst[k]); first = first < s_first[k] ? first : s_first[k]; }
    const bool write = total[0] <= a.cap;
    for (uint64_t i = lo; i < hi; i++) {
        const hdlz_png_spec s = a.specs[i];
        const uint32_t st = a.ist[i];
        const uint64_t zlen = a.zlen[i];
        uint64_t rb, raw_len;
        uint32_t bpp;
        (void)check_spec(s, rb, raw_len, bpp);
        const uint64_t nidat = st == HDLZ_OK ? (zlen + a.idat - 1u) / a.idat : 0u;
        const uint64_t flen = st == HDLZ_OK ? SIG_IHDR_END + zlen + CHUNK * nidat + CHUNK : 0u;
        a.file_off[i] = base[0]; a.file_len[i] = flen; a.cbase[i] = base[4];
        if (a.image_status) a.image_status[i] = st;
        const bool indexed = st == HDLZ_OK && zlen <= Z_MAX;      // (else: what hdlz_png_index_ws answers for a stream past its limit)
        if (a.images) {
            hdlz_png_image rec;
            memset(&rec, 0, sizeof(rec));
            rec.file_off = base[0]; rec.file_len = flen; rec.z_off = base[1]; rec.raw_off = base[2]; rec.out_off = base[3];
            rec.status = st != HDLZ_OK ? st : indexed ? (uint32_t)HDLZ_OK : (uint32_t)HDLZ_E_OUT_CAPACITY;
            if (indexed) {
                rec.idat_off = SIG_IHDR_END; rec.zlen = zlen; rec.used = flen; rec.row_bytes = rb; rec.raw_len = raw_len; rec.out_len = out_len_of(s, rb);
                rec.width = s.width; rec.height = s.height; rec.nidat = (uint32_t)nidat; rec.depth = s.depth; rec.colour = s.colour;
                rec.channels_out = (uint8_t)(bpp / (s.depth >> 3)); rec.sample_bytes = (uint8_t)(s.depth >> 3);
            }
            a.images[i] = rec;
        }
        if (st == HDLZ_OK) {
            base[0] += flen; base[4] += 1u + nidat;
            if (indexed) { const Slots t = slots_of(zlen + 8u, raw_len, out_len_of(s, rb), amask); base[1] += t.z; base[2] += t.raw; base[3] += t.out; }
        }
    }
    if (tid != 0u) return;
    a.cbase[n] = total[4];
    a.head[0] = write ? 1u : 0u; a.head[1] = write ? total[4] : 0u;
    hdlz_png_write_result res;
    res.total_len = total[0]; res.first_bad = first;
    res.status = worst != HDLZ_OK ? worst : !write ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)HDLZ_OK;
    res.reserved = 0u;
    *a.result = res;
}

// where stream byte s of an image lies in its file
__device__ __forceinline__ uint64_t file_pos(uint64_t s, uint32_t idat) { return FIRST_DATA + s + (uint64_t)CHUNK * (s / idat); }

// byte i of M_b: [0, bl) from the row (src = row + 2; byte 0: BFINAL cleared), zeros, FF FF at [m - 2, m)
__device__ __forceinline__ uint8_t member_byte(const uint8_t* src, uint32_t i, uint32_t bl, uint32_t m) {
    if (i < bl) return i == 0u ? (uint8_t)(src[0] & 0xFEu) : src[i];
    return i < m - 2u ? (uint8_t)0u : (uint8_t)0xFFu;
}

__global__ __launch_bounds__(256) void k_pngw_gather(PngWriteArgs a, uint32_t row_groups) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (a.head[0] == 0u) return;                                  // (uniform over the grid: the files do not fit)
    if (blockIdx.x < row_groups) {
        // ---- a wave per block
        const uint64_t b = (uint64_t)blockIdx.x * 4u + wave;
        if (b >= a.nblocks) return;
        const uint64_t ub = upper(a.blk_first, a.n + 1u, b);
        if (ub == 0u || ub > a.n) return;                         // (a row that no image owns)
        const uint64_t i = ub - 1u;
        if (a.ist[i] != HDLZ_OK) return;
        uint32_t bl;
        const uint32_t m = member_len(a.len[b], a.end_bits[b], a.pitch, bl);
        const uint8_t* __restrict__ src = a.rows + b * a.pitch + 2u;
        uint8_t* const file = a.file + a.file_off[i];
        const uint64_t o = 2u + (a.pre[b] - a.pre[a.blk_first[i]]);      // where M_b starts in the image's stream
        for (uint64_t s0 = o; s0 < o + m;) {
            const uint64_t k = s0 / a.idat, seam = (k + 1u) * a.idat, s1 = seam < o + m ? seam : o + m;
            const uint32_t i0 = (uint32_t)(s0 - o), i1 = (uint32_t)(s1 - o), rn = i1 - i0;      // the piece: bytes [i0, i1) of the member
            uint8_t* __restrict__ dst = file + FIRST_DATA + s0 + (uint64_t)CHUNK * k;
            const uint32_t head = min(rn, (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u));
            if (lane < head) dst[lane] = member_byte(src, i0 + lane, bl, m);
            const uint32_t top = i1 < bl ? i1 : bl;               // whole 16-byte chunks of the row's bytes: no load leaves row[2 .. nbytes)
            const uint32_t body = top > i0 + head ? (top - i0 - head) >> 4 : 0u;
            for (uint32_t c = lane; c < body; c += 64u) {
                v4 x = *reinterpret_cast<const v4u*>(src + i0 + head + 16u * c);
                if (i0 + head == 0u && c == 0u) x.x &= ~1u;       // (the member starts at a 16-byte boundary: BFINAL sits in the body)
                *reinterpret_cast<v4*>(dst + head + 16u * c) = x;
            }
            for (uint32_t j = head + 16u * body + lane; j < rn; j += 64u) dst[j] = member_byte(src, i0 + j, bl, m);
            s0 = s1;
        }
        return;
    }
    // ---- a wave per image: everything that is not a member or a CRC-32
    const uint64_t i = (uint64_t)(blockIdx.x - row_groups) * 4u + wave;
    if (i >= a.n || a.ist[i] != HDLZ_OK) return;
    const hdlz_png_spec s = a.specs[i];
    uint8_t* const file = a.file + a.file_off[i];
    const uint64_t zlen = a.zlen[i], nidat = (zlen + a.idat - 1u) / a.idat;
    const uint32_t adler = a.adler[i];
    if (lane < SIG_IHDR_END - 4u) {                               // the signature and IHDR up to its CRC-32
        const uint8_t fixed[16] = {HDLZ_BE32_BYTES(SIG_HI), HDLZ_BE32_BYTES(SIG_LO), HDLZ_BE32_BYTES(IHDR_LEN), HDLZ_BE32_BYTES(T_IHDR)};
        uint8_t v = 0u;
        if (lane < 16u) { for (uint32_t k = 0; k < 16u; k++) if (k == lane) v = fixed[k]; }
        else if (lane < 20u) v = (uint8_t)(s.width >> (8u * (19u - lane)));
        else if (lane < 24u) v = (uint8_t)(s.height >> (8u * (23u - lane)));
        else if (lane == 24u) v = s.depth;
        else if (lane == 25u) v = s.colour;
        file[lane] = v;
    }
    for (uint64_t k = lane; k < nidat; k += 64u) {                // every IDAT's length and type
        uint8_t* h = file + SIG_IHDR_END + k * ((uint64_t)a.idat + CHUNK);
        const uint64_t left = zlen - k * a.idat;
        put_be32(h, (uint32_t)(left < a.idat ? left : a.idat));
        put_be32(h + 4, T_IDAT);
    }
    const bool stored = a.blk_first[i] == a.blk_first[i + 1u];
    const uint32_t raw_len = stored ? (uint32_t)(zlen - STORED_HEAD - 4u) : 0u;
    // the stream's bytes that are not members: 78 9C (01 LEN NLEN and the stream) in front, (03 00 and) the Adler-32 behind
    const uint32_t front = stored ? STORED_HEAD + raw_len : 2u, back = stored ? 4u : Z_TAIL;
    if (lane < front + back) {
        const bool tail = lane >= front;
        const uint64_t sp = tail ? zlen - back + (lane - front) : lane;
        uint8_t v;
        if (tail) {
            const uint32_t t = lane - front + (stored ? 2u : 0u); // 0, 1: 03 00
            v = t == 0u ? (uint8_t)0x03u : t == 1u ? (uint8_t)0u : (uint8_t)(adler >> (8u * (5u - t)));
        } else if (lane == 0u) v = 0x78u;
        else if (lane == 1u) v = 0x9Cu;
        else if (lane == 2u) v = 0x01u;
        else if (lane == 3u) v = (uint8_t)raw_len;
        else if (lane == 4u) v = 0u;
        else if (lane == 5u) v = (uint8_t)~raw_len;
        else if (lane == 6u) v = 0xFFu;
        else v = a.raw[a.raw_off[i] + (lane - STORED_HEAD)];
        file[file_pos(sp, a.idat)] = v;
    }
    if (lane < CHUNK) {                                           // IEND, its CRC-32 a constant
        const uint8_t iend[CHUNK] = {0, 0, 0, 0, HDLZ_BE32_BYTES(T_IEND), 0xAE, 0x42, 0x60, 0x82};
        uint8_t v = 0u;
        for (uint32_t k = 0; k < CHUNK; k++) if (k == lane) v = iend[k];
        file[SIG_IHDR_END + zlen + CHUNK * nidat + lane] = v;
    }
}

// ---- the CRC-32 of IHDR and of every IDAT: entry e of the list is chunk e - cbase[i] of image i (0: IHDR)
__global__ __launch_bounds__(CRC_THREADS) void k_pngw_crc(PngWriteArgs a) {
    __shared__ CrcTileLds s;
    crc_build_tables(s);
    __syncthreads();
    const uint64_t total = a.head[1];                             // (0 unless the files are written)
    for (uint64_t e = blockIdx.x; e < total; e += gridDim.x) {
        const uint64_t i = owner(a.cbase, a.n, e), k = e - a.cbase[i];
        uint8_t* const file = a.file + a.file_off[i];
        uint8_t* p;
        uint32_t L;
        if (k == 0u) { p = file + 12u; L = 4u + IHDR_LEN; }
        else {
            const uint64_t left = a.zlen[i] - (k - 1u) * a.idat;
            p = file + SIG_IHDR_END + (k - 1u) * ((uint64_t)a.idat + CHUNK) + 4u;
            L = 4u + (uint32_t)(left < a.idat ? left : a.idat);
        }
        const uint32_t c = crc_block(p, L, s);
        if (threadIdx.x == 0u) put_be32(p + L, c);
    }
}

__global__ void k_pngw_empty(hdlz_png_write_result* result) {
    hdlz_png_write_result res;
    res.total_len = 0u; res.first_bad = NONE64; res.status = HDLZ_OK; res.reserved = 0u;
    *result = res;
}

static unsigned grid_of(uint64_t want, uint64_t most) { return (unsigned)(want < 1u ? 1u : want < most ? want : most); }

}  // namespace pngw

size_t png_filter_work_bytes(uint64_t n) { return 2u * round256(8u * ((size_t)n + 1u)); }

hipError_t launch_png_filter(PngFilterArgs a, void* work, hipStream_t stream) {
    using namespace pngw;
    if (a.n == 0) return hipSuccess;
    uint8_t* w = static_cast<uint8_t*>(work);
    a.row_base = reinterpret_cast<uint64_t*>(w);
    a.band_base = reinterpret_cast<uint64_t*>(w + round256(8u * ((size_t)a.n + 1u)));
    hipError_t e = launch(k_pngw_plan, dim3(1), dim3(PLAN_THREADS), stream, a);
    // a wave per band, four a workgroup; the bands from what the host knows: an image ends in at most one partial band
    const uint64_t bands = a.total_rows / BAND + a.n;
    if (e == hipSuccess) e = launch(k_pngw_filter, dim3(grid_of((bands + 3u) / 4u, FILTER_GRID_MAX)), dim3(256), stream, a);
    return e;
}

// the scratch, in this order, every piece a multiple of 256 bytes (include/hdlz_png_write.h states the sum)
static size_t png_write_work(PngWriteArgs& a, void* work) {
    const uintptr_t base = reinterpret_cast<uintptr_t>(work);
    size_t at = 0;
    auto piece = [&](size_t n) { const uintptr_t p = base + at; at += round256(n); return p; };
    const size_t B1 = (size_t)a.nblocks + 1u, n = (size_t)a.n;
    a.pre = reinterpret_cast<uint64_t*>(piece(8u * B1)); a.cnt = reinterpret_cast<uint64_t*>(piece(8u * B1));
    a.pa = reinterpret_cast<uint64_t*>(piece(8u * B1)); a.pe = reinterpret_cast<uint64_t*>(piece(8u * B1)); a.ps = reinterpret_cast<uint64_t*>(piece(8u * B1));
    a.zlen = reinterpret_cast<uint64_t*>(piece(8u * (n + 1u))); a.cbase = reinterpret_cast<uint64_t*>(piece(8u * (n + 1u)));
    a.adler = reinterpret_cast<uint32_t*>(piece(4u * n)); a.ist = reinterpret_cast<uint32_t*>(piece(4u * n));
    a.head = reinterpret_cast<uint64_t*>(piece(256u));
    return at;
}

size_t png_write_work_bytes(uint64_t n, uint64_t nblocks) {
    PngWriteArgs a{};
    a.n = n; a.nblocks = nblocks;
    return png_write_work(a, nullptr);
}

hipError_t launch_png_write(PngWriteArgs a, void* work, hipStream_t stream) {
    using namespace pngw;
    if (a.n == 0) return launch(k_pngw_empty, dim3(1), dim3(1), stream, a.result);      // no image: the record alone
    (void)png_write_work(a, work);
    hipError_t e = hipSuccess;
    if (a.nblocks) e = launch(k_pngw_scan, dim3(1), dim3(PLAN_THREADS), stream, a);
    if (e == hipSuccess) e = launch(k_pngw_layout, dim3(1), dim3(PLAN_THREADS), stream, a);
    const uint64_t row_groups = (a.nblocks + 3u) / 4u, image_groups = (a.n + 3u) / 4u;
    if (e == hipSuccess) e = launch(k_pngw_gather, dim3((unsigned)(row_groups + image_groups)), dim3(256), stream, a, (uint32_t)row_groups);
    // the chunks from what the host knows: files that are written fit file_cap, an IDAT but an image's last takes idat_len + 12 bytes
    const uint64_t chunks = 2u * a.n + a.cap / ((uint64_t)a.idat + CHUNK);
    if (e == hipSuccess) e = launch(k_pngw_crc, dim3(grid_of(chunks, CRC_GROUPS_MAX)), dim3(CRC_THREADS), stream, a);
    return e;
}

}  // namespace hdlz
