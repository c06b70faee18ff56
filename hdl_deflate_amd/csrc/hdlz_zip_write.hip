// hdlz_zip_write.hip -- the kernels of include/hdlz_zip_write.h: a ZIP archive written from the rows of ONE compress
// batch.  A ZIP is ragged twice -- entries, and blocks inside entries --, a header with a name of any length stands in front of every
// payload and a directory behind them, and whether an entry is deflated at all depends on the sum of ALL its members: so, unlike k_join,
// the scan cannot copy on its way.  Three kernels behind the zeroing of the look-back words:
//
// k_zipw_scan    a tile join's first half (hdlz_frame.h: tile_scan, tile_lookback): a workgroup takes a TILE of 256 consecutive rows by a
//                ticket and leaves, per row, the exclusive prefix of the member lengths |M_b| and of two counts in one word -- rows
//                whose status is not HDLZ_OK (bits 0 .. 30) and rows whose length, end bit and pitch contradict each other (bits
//                31 .. 61; a block of negative length counts among them) --, so that an entry's payload length and "does a block of
//                mine fail" are each two loads.  The two look-backs run side by side, a wave each.
// k_zipw_plan    ONE workgroup of 1024 threads, 64 entries each at most (strip, block_scan: hdlz_plan.h): the checks of step 1
//                (entry_check, shared with k_zipw64_plan), c_e and the form, the scans of the record
//                sizes (local offsets, directory offsets, out_off, the tiles of the stored copy) -> the plan in the scratch; thread 0
//                writes the end record and the result record.  An entry with a failed row walks its rows for the largest status:
//                the one serial loop, on the failing path only.
// k_zipw_gather  the hot path, three kinds of workgroup in one grid (a kind per range of blockIdx.x, uniform over a workgroup):
//                  rows     16 consecutive rows a workgroup (256 from 65536 rows on), a quarter of them a wave.  Every wave finds its
//                           first row's entry by a 64-way search in d_blk_first (three rounds of dependent loads, not sixteen), its
//                           other rows' entries among the next 64 (one round), and leaves every row's source, destination and
//                           lengths in LDS: what depends on the plan is loaded once a wave, all its rows at a time, not row after
//                           row, and no wave waits for another's loads.  A deflated entry's row: M_b to its place with BFINAL
//                           cleared and the marker appended -- k_join's loop, four 16-byte loads in flight a lane --, 03 00 behind
//                           the entry's last member.  A stored entry's row: the block's input bytes (copy_to_aligned16).
//                  tiles    the stored entries WITHOUT rows, cut into tiles of 64 KiB: a workgroup finds its tile's entry by a search
//                           in the plan's tile prefix and copies with copy_to_aligned16; the number of these workgroups comes from
//                           total_in and nentries, and they stride when that understated the bytes.
//                  entries  a wave per entry: the 30 and the 46 header bytes (a lane a byte, picked from the words of the record), the
//                           name behind both (copy_to_aligned16), d_entries[e].
// Plain stores only; all bulk stores are 16 bytes to 16-byte aligned addresses.  Loads: the index arrays; names exactly; of a row only
// [2, d_len - 4) and only for a deflated entry; of an entry only its bytes and only when it is stored.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_compress_common.h"                        // member_len
#include "hdlz_frame.h"                                  // the tile's scan and look-back, the wave reductions, copy_to_aligned16
#include "hdlz_plan.h"                                   // strip, block_scan, upper, rows_verdict

namespace hdlz {
namespace zipw {

constexpr uint32_t LOCREC = 30u, CDREC = 46u, EOCD = 22u;
constexpr uint32_t SIG_LOCAL = 0x04034B50u, SIG_CD = 0x02014B50u, SIG_EOCD = 0x06054B50u;
constexpr uint32_t VERSION = 20u;                                // needed to extract, and made by (host 0): 2.0
constexpr uint32_t METHOD_DEFLATED = 8u, NAME_LEN_MAX = 65535u;
constexpr uint64_t NO_ZIP64 = 0xFFFFFFFFull;                     // a size or offset of FFFFFFFF means "see the ZIP64 field"
constexpr uint32_t PLAN_THREADS = 1024u, PLAN_WAVES = PLAN_THREADS / 64u;      // 65535 entries: 64 a thread
constexpr uint32_t STORE_TILE = 65536u;                          // 16 stores of 16 bytes a thread
constexpr uint32_t ROWS_MAX = 256u, ROWS_FEW = 16u, ROWS_MANY_MIN = 1u << 16;      // rows a workgroup of the gather takes: 16, or 256 from 65536 rows on (not measured: between the profile's two shapes)
// the summary at w.head
enum { H_WRITE = 0, H_TILES = 1, H_FAILED = 2 };


// ---- (a) the prefixes over the rows
__global__ __launch_bounds__(JT) void k_zipw_scan(ZipWriteArgs a) {
    __shared__ uint32_t s_tile;
    __shared__ uint64_t s_wsum[4], s_wsum2[4], s_base, s_base2;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0u) s_tile = atomicAdd(a.w.ticket, 1u);
    __syncthreads();
    const uint32_t tile = s_tile;
    const uint64_t b = (uint64_t)tile * JT + tid;
    uint32_t m = 0u, k = 0u;                                      // k: failed in the low half, contradictory in the high half
    if (b < a.nblocks) {
        if (a.status[b] != HDLZ_OK) k = 1u;
        else {
            uint32_t body;
            m = member_len(a.len[b], a.end_bits[b], a.pitch, body);
            if (a.in_off[b + 1u] < a.in_off[b]) m = 0u;           // (a block of negative length: the copy of a stored entry's rows trusts these)
            if (m == 0u) k = 1u << 16;
        }
    }
    // (a tile's counts are at most 256: they are scanned as halves of one word and widened to COUNT_BITS for the look-back)
    auto wide = [](uint64_t v) { return (v & 0xFFFFu) | ((v >> 16) << COUNT_BITS); };
    uint64_t tsum, tsum2;
    const uint64_t local = tile_scan(m, lane, wave, s_wsum, tsum);
    const uint64_t local2 = wide(tile_scan(k, lane, wave, s_wsum2, tsum2));
    tsum2 = wide(tsum2);
    // the two look-backs side by side, a wave each: neither chain waits for the other's
    const bool last_tile = (uint64_t)(tile + 1u) * JT >= a.nblocks;
    if (wave == 0u) {
        const uint64_t base = tile_lookback(a.w.desc, tile, tsum, lane);
        if (lane == 0u) {
            s_base = base;
            if (last_tile) a.w.pre[a.nblocks] = base + tsum;
        }
    } else if (wave == 1u) {
        const uint64_t base2 = tile_lookback(a.w.desc2, tile, tsum2, lane);
        if (lane == 0u) {
            s_base2 = base2;
            if (last_tile) a.w.cnt[a.nblocks] = base2 + tsum2;
        }
    }
    __syncthreads();
    if (b < a.nblocks) { a.w.pre[b] = s_base + local; a.w.cnt[b] = s_base2 + local2; }
}

// byte i of the record whose little-endian words are w[0 .. N)
template <int N>
__device__ __forceinline__ uint8_t record_byte(const uint32_t (&w)[N], uint32_t i) {
    uint32_t x = 0u;
    static_for<0, N>([&](auto k) {
        if ((i >> 2) == (uint32_t)k) x = w[k];
    });
    return (uint8_t)(x >> (8u * (i & 3u)));
}

// the checks of step 1 for entry e of u bytes with a name of n bytes (but the classic format's size limit), and its form: stored with
// c = u, or deflated -- the members and 03 00 -- where that is shorter
__device__ __forceinline__ uint32_t entry_check(const ZipWriteArgs& a, uint64_t e, uint64_t u, uint64_t n, uint32_t& method, uint64_t& c) {
    const uint64_t F0 = a.blk_first[e], F1 = a.blk_first[e + 1u];
    uint32_t st = HDLZ_OK;
    method = 0u; c = u;
    if (F0 > F1 || F1 > a.nblocks) st = HDLZ_E_BAD_PARAM;
    else if (F1 > F0) {
        st = rows_verdict(a.w.cnt, a.status, F0, F1);
        if (st == HDLZ_OK && a.in_off[F1] - a.in_off[F0] != u) st = HDLZ_E_BAD_PARAM;
    }
    if (st == HDLZ_OK && n > NAME_LEN_MAX) st = HDLZ_E_BAD_PARAM;
    if (st == HDLZ_OK && F1 > F0) {
        const uint64_t cd = a.w.pre[F1] - a.w.pre[F0] + 2u;
        if (cd < u) { method = METHOD_DEFLATED; c = cd; }
    }
    return st;
}

// ---- (b) the plan: a strip of the entries a thread (hdlz_plan.h)
__global__ __launch_bounds__(PLAN_THREADS) void k_zipw_plan(ZipWriteArgs a) {
    __shared__ uint64_t s_wave[4][PLAN_WAVES];
    __shared__ uint32_t s_worst[PLAN_WAVES], s_first[PLAN_WAVES], s_nst[PLAN_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t E = (uint32_t)a.nentries;
    const uint64_t amask = (uint64_t)a.out_align - 1u;
    uint64_t lo, hi;
    strip(E, PLAN_THREADS, tid, lo, hi);                          // at most 64 entries
    uint64_t mine[4] = {0u, 0u, 0u, 0u}, base[4], total[4];      // local records, central records, output slots, tiles of the stored copy
    uint32_t worst = HDLZ_OK, first = NONE, nst = 0u;
    for (uint64_t e = lo; e < hi; e++) {
        const uint64_t u = a.ent_off[e + 1u] - a.ent_off[e], n = a.name_off[e + 1u] - a.name_off[e];
        uint32_t method;
        uint64_t c;
        uint32_t st = entry_check(a, e, u, n, method, c);
        if (st == HDLZ_OK && u >= NO_ZIP64) { st = HDLZ_E_OUT_CAPACITY; method = 0u; c = u; }
        a.w.csize[e] = (uint32_t)c;
        a.w.form[e] = method | (st << 8);
        if (st == HDLZ_OK) {
            mine[0] += LOCREC + n + c; mine[1] += CDREC + n; mine[2] += (u + amask) & ~amask;
            if (a.blk_first[e] == a.blk_first[e + 1u]) mine[3] += (u + STORE_TILE - 1u) / STORE_TILE;
            nst += method == 0u ? 1u : 0u;
        } else {
            worst = max(worst, st);
            first = min(first, (uint32_t)e);
        }
    }
    {
        const uint32_t rw = wave_max(worst), rf = wave_min(first), rn = wave_add(nst);
        if (lane == 0u) { s_worst[wave] = rw; s_first[wave] = rf; s_nst[wave] = rn; }
    }
    block_scan<4, PLAN_THREADS>(mine, base, total, s_wave);      // (its barriers stand behind the stores of s_worst, s_first and s_nst, too)
    worst = HDLZ_OK; first = NONE; nst = 0u;
    for (uint32_t k = 0; k < PLAN_WAVES; k++) { worst = max(worst, s_worst[k]); first = min(first, s_first[k]); nst += s_nst[k]; }
    const bool failed = worst != HDLZ_OK;
    const uint64_t cd_off = total[0], cd_size = total[1], file_len = cd_off + cd_size + EOCD;
    const bool limit = cd_off >= NO_ZIP64 || file_len > NO_ZIP64;       // (the local offsets ascend to cd_off)
    const bool write = !failed && !limit && file_len <= a.cap;
    for (uint64_t e = lo; e < hi; e++) {
        const uint64_t u = a.ent_off[e + 1u] - a.ent_off[e], n = a.name_off[e + 1u] - a.name_off[e];
        const bool none = a.blk_first[e] == a.blk_first[e + 1u];
        a.w.pay[e] = base[0] + LOCREC + n; a.w.cdrec[e] = cd_off + base[1]; a.w.out_off[e] = base[2]; a.w.tile0[e] = (uint32_t)base[3];
        if ((a.w.form[e] >> 8) == HDLZ_OK) {
            base[0] += LOCREC + n + a.w.csize[e]; base[1] += CDREC + n; base[2] += (u + amask) & ~amask;
            if (none) base[3] += (u + STORE_TILE - 1u) / STORE_TILE;
        }
    }
    if (tid != 0u) return;
    a.w.tile0[E] = write ? (uint32_t)total[3] : 0u;
    a.w.head[H_WRITE] = write ? 1u : 0u; a.w.head[H_TILES] = write ? total[3] : 0u; a.w.head[H_FAILED] = failed ? 1u : 0u;
    hdlz_zip_write_result res;
    res.file_len = failed ? 0u : file_len; res.cd_off = failed ? 0u : cd_off; res.cd_size = failed ? 0u : cd_size; res.nstored = failed ? 0u : nst;
    res.status = failed ? worst : (limit || file_len > a.cap) ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)HDLZ_OK;
    res.first_bad = first;
    *a.result = res;
    if (!write) return;
    uint8_t* t = a.file + cd_off + cd_size;
    const uint32_t w[6] = {SIG_EOCD, 0u, E | (E << 16), (uint32_t)cd_size, (uint32_t)cd_off, 0u};
    for (uint32_t i = 0; i < EOCD; i++) t[i] = record_byte(w, i);
}

// ---- hdlz_zip64_write_ws (include/hdlz_zip64.h): the plan for any E and the entries' headers with their ZIP64 fields
constexpr uint32_t SIG_EOCD64 = 0x06064B50u, SIG_LOCATOR = 0x07064B50u, EOCD64 = 56u, LOCATOR = 20u;
constexpr uint32_t VERSION64 = 45u, LOCAL_EXTRA64 = 20u;

// the bytes of an entry's local ZIP64 extra, and how many values its central one holds (from = zip64_from)
__device__ __forceinline__ uint32_t local_extra(uint64_t u, uint64_t c, uint64_t from) { return u >= from || c >= from ? LOCAL_EXTRA64 : 0u; }
__device__ __forceinline__ uint32_t central_extra(uint64_t u, uint64_t c, uint64_t L, uint64_t from) {
    const uint32_t k = (u >= from ? 1u : 0u) + (c >= from ? 1u : 0u) + (L >= from ? 1u : 0u);
    return k ? 4u + 8u * k : 0u;
}

// ONE workgroup, a strip of the entries a thread, E without a limit.  A local record's size hangs on u_e and
// c_e alone, a central record's on the local offset L_e too: so two scans one behind the other -- the local records (with the slots and
// the tiles), then, L_e known, the central records -- and a coalesced sweep that makes the central offsets, run-relative until then, absolute.
__global__ __launch_bounds__(PLAN_THREADS) void k_zipw64_plan(ZipWriteArgs a) {
    __shared__ uint64_t s_wave[4][PLAN_WAVES];
    __shared__ uint32_t s_worst[PLAN_WAVES], s_first[PLAN_WAVES];
    __shared__ uint64_t s_cbase[PLAN_THREADS];                    // where each thread's run of central records starts
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t E = a.nentries, from = a.zip64_from;
    const uint64_t amask = (uint64_t)a.out_align - 1u;
    uint64_t lo, hi;
    const uint64_t per = strip(E, PLAN_THREADS, tid, lo, hi);
    uint64_t mine[4] = {0u, 0u, 0u, 0u};                          // local records, entries stored, output slots, tiles of the stored copy
    uint32_t worst = HDLZ_OK, first = NONE;
    for (uint64_t e = lo; e < hi; e++) {
        const uint64_t u = a.ent_off[e + 1u] - a.ent_off[e], n = a.name_off[e + 1u] - a.name_off[e];
        uint32_t method;
        uint64_t c;
        const uint32_t st = entry_check(a, e, u, n, method, c);
        a.w.csize64[e] = c;
        a.w.form[e] = method | (st << 8);
        if (st == HDLZ_OK) {
            mine[0] += LOCREC + n + local_extra(u, c, from) + c; mine[1] += method == 0u ? 1u : 0u; mine[2] += (u + amask) & ~amask;
            if (a.blk_first[e] == a.blk_first[e + 1u]) mine[3] += (u + STORE_TILE - 1u) / STORE_TILE;
        } else {
            worst = max(worst, st);
            first = min(first, (uint32_t)e);
        }
    }
    {
        const uint32_t rw = wave_max(worst), rf = wave_min(first);
        if (lane == 0u) { s_worst[wave] = rw; s_first[wave] = rf; }
    }
    uint64_t base[4], total[4];
    block_scan<4, PLAN_THREADS>(mine, base, total, s_wave);      // (its barriers stand behind the stores of s_worst and s_first, too)
    worst = HDLZ_OK; first = NONE;
    for (uint32_t k = 0; k < PLAN_WAVES; k++) { worst = max(worst, s_worst[k]); first = min(first, s_first[k]); }
    const bool failed = worst != HDLZ_OK;
    const uint64_t cd_off = total[0];
    // the second scan: the central records, every local offset known
    uint64_t cmine[1] = {0u}, cbase[1], ctotal[1];
    for (uint64_t e = lo; e < hi; e++) {
        const uint64_t u = a.ent_off[e + 1u] - a.ent_off[e], n = a.name_off[e + 1u] - a.name_off[e], c = a.w.csize64[e];
        const bool none = a.blk_first[e] == a.blk_first[e + 1u];
        const uint64_t L = base[0];
        a.w.pay[e] = L + LOCREC + n + local_extra(u, c, from); a.w.out_off[e] = base[2]; a.w.tile0[e] = (uint32_t)base[3];
        a.w.cdrec[e] = cmine[0];                                  // relative to the run's first central record, until the sweep below
        if ((a.w.form[e] >> 8) == HDLZ_OK) {
            cmine[0] += CDREC + n + central_extra(u, c, L, from);
            base[0] += LOCREC + n + local_extra(u, c, from) + c; base[2] += (u + amask) & ~amask;
            if (none) base[3] += (u + STORE_TILE - 1u) / STORE_TILE;
        }
    }
    block_scan<1, PLAN_THREADS>(cmine, cbase, ctotal, s_wave);
    const uint64_t cd_size = ctotal[0];
    // pass 2 left every central offset relative to its thread's run: the runs' starts go through LDS and the third pass is one
    // coalesced sweep -- a load, an add and a store an entry, independent of each other, where a third walk of the runs would cost
    // as much as the second (a run is latency-bound: profiles/zip64.txt section 5)
    s_cbase[tid] = cd_off + cbase[0];
    __syncthreads();
    for (uint64_t e = tid; e < E; e += PLAN_THREADS) a.w.cdrec[e] += s_cbase[(uint32_t)e / (uint32_t)per];
    if (tid != 0u) return;
    const bool big = E > 65535u || cd_off >= from || cd_size >= from;      // the ZIP64 end record and its locator
    const uint64_t r = cd_off + cd_size, file_len = r + (big ? EOCD64 + LOCATOR : 0u) + EOCD;
    const bool write = !failed && file_len <= a.cap;
    a.w.tile0[E] = write ? (uint32_t)total[3] : 0u;
    a.w.head[H_WRITE] = write ? 1u : 0u; a.w.head[H_TILES] = write ? total[3] : 0u; a.w.head[H_FAILED] = failed ? 1u : 0u;
    hdlz_zip_write_result res;
    res.file_len = failed ? 0u : file_len; res.cd_off = failed ? 0u : cd_off; res.cd_size = failed ? 0u : cd_size; res.nstored = failed ? 0u : total[1];
    res.status = failed ? worst : file_len > a.cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)HDLZ_OK;
    res.first_bad = first;
    *a.result = res;
    if (!write) return;
    uint8_t* t = a.file + r;
    if (big) {
        const uint32_t w64[19] = {SIG_EOCD64, 44u, 0u, VERSION64 | (VERSION64 << 16), 0u, 0u, (uint32_t)E, (uint32_t)(E >> 32), (uint32_t)E, (uint32_t)(E >> 32),
                                  (uint32_t)cd_size, (uint32_t)(cd_size >> 32), (uint32_t)cd_off, (uint32_t)(cd_off >> 32),
                                  SIG_LOCATOR, 0u, (uint32_t)r, (uint32_t)(r >> 32), 1u};
        for (uint32_t i = 0; i < EOCD64 + LOCATOR; i++) t[i] = record_byte(w64, i);
        t += EOCD64 + LOCATOR;
    }
    const uint32_t n16 = E > 0xFFFFu ? 0xFFFFu : (uint32_t)E;
    const uint32_t w[6] = {SIG_EOCD, 0u, n16 | (n16 << 16), cd_size >= from ? 0xFFFFFFFFu : (uint32_t)cd_size, cd_off >= from ? 0xFFFFFFFFu : (uint32_t)cd_off, 0u};
    for (uint32_t i = 0; i < EOCD; i++) t[i] = record_byte(w, i);
}

// the entries' part of the gather for hdlz_zip64_write_ws, a wave per entry: both headers, the name and the ZIP64 extra behind each, the record
__device__ __forceinline__ void entry_headers64(const ZipWriteArgs& a, uint32_t e, uint32_t lane, bool write) {
    const uint64_t from = a.zip64_from;
    const uint32_t form = a.w.form[e], method = form & 0xFFu, crc = a.crc[e];
    const uint64_t c = a.w.csize64[e], u = a.ent_off[e + 1u] - a.ent_off[e];
    const uint32_t n = (uint32_t)(a.name_off[e + 1u] - a.name_off[e]);
    const uint32_t lx = local_extra(u, c, from);
    const uint64_t pay = a.w.pay[e], L = pay - LOCREC - n - lx, cd = a.w.cdrec[e];
    const bool zu = u >= from, zc = c >= from, zl = L >= from;
    const uint32_t cx = central_extra(u, c, L, from);
    if (a.entries64 && lane == 0u) {
        hdlz_zip64_entry rec;
        const bool sound = a.w.head[H_FAILED] == 0u;
        rec.cd_off = sound ? cd : 0u; rec.payload_off = sound ? pay : 0u; rec.out_off = sound ? a.w.out_off[e] : 0u;
        rec.csize = sound ? c : 0u; rec.usize = sound ? u : 0u; rec.crc = sound ? crc : 0u;
        rec.method = (uint16_t)(sound ? method : 0u); rec.flags = (uint16_t)(sound ? a.flags : 0u); rec.name_len = (uint16_t)(sound ? n : 0u);
        rec.reserved = 0u; rec.reserved2 = 0u;
        rec.status = form >> 8;
        a.entries64[e] = rec;
    }
    if (!write) return;
    const uint32_t time = a.datetime & 0xFFFFu, date = a.datetime >> 16;
    const uint32_t ver = cx ? VERSION64 : VERSION;                // (a local extra never stands without a central one)
    const uint32_t lc = lx ? 0xFFFFFFFFu : (uint32_t)c, lu = lx ? 0xFFFFFFFFu : (uint32_t)u;
    const uint32_t cc = zc ? 0xFFFFFFFFu : (uint32_t)c, cu = zu ? 0xFFFFFFFFu : (uint32_t)u, cl = zl ? 0xFFFFFFFFu : (uint32_t)L;
    const uint32_t lw[8] = {SIG_LOCAL, ver | (a.flags << 16), method | (time << 16), date | (crc << 16), (crc >> 16) | (lc << 16),
                            (lc >> 16) | (lu << 16), (lu >> 16) | (n << 16), lx};
    const uint32_t cw[12] = {SIG_CD, ver | (ver << 16), a.flags | (method << 16), time | (date << 16), crc, cc, cu, n | (cx << 16), 0u, 0u,
                             cl << 16, cl >> 16};
    if (lane < LOCREC) a.file[L + lane] = record_byte(lw, lane);
    if (lane < CDREC) a.file[cd + lane] = record_byte(cw, lane);
    const uint8_t* name = a.names + a.name_off[e];
    copy_to_aligned16(a.file + L + LOCREC, name, n, lane, 64u);
    copy_to_aligned16(a.file + cd + CDREC, name, n, lane, 64u);
    // the extras: 01 00 10 00 | u | c behind the local name; 01 00 | 8k | the k values that moved, in the order u, c, L, behind the central one
    const uint32_t xl[5] = {0x00100001u, (uint32_t)u, (uint32_t)(u >> 32), (uint32_t)c, (uint32_t)(c >> 32)};
    if (lane < lx) a.file[L + LOCREC + n + lane] = record_byte(xl, lane);
    const uint64_t v0 = zu ? u : zc ? c : L, v1 = zu && zc ? c : L;
    const uint32_t xc[7] = {1u | ((cx - 4u) << 16), (uint32_t)v0, (uint32_t)(v0 >> 32), (uint32_t)v1, (uint32_t)(v1 >> 32), (uint32_t)L, (uint32_t)(L >> 32)};
    if (lane < cx) a.file[cd + CDREC + n + lane] = record_byte(xc, lane);
}

// the number of elements of the ascending v[0 .. n) that are <= x (the first index with v[i] > x), by a whole wave: 64 probes a round,
// so three rounds of dependent loads for the 65536 words of a ZIP's entries where a lane alone takes sixteen
__device__ __forceinline__ uint32_t wave_upper_bound(const uint64_t* __restrict__ v, uint32_t n, uint64_t x, uint32_t lane) {
    uint32_t base = 0u, width = n;
    while (width > 64u) {
        const uint32_t chunk = (width + 63u) / 64u, p = (lane + 1u) * chunk - 1u;      // lane i probes the last word of chunk i
        const uint32_t c = (uint32_t)__builtin_popcountll(ballot64(p < width && v[base + p] <= x));
        base += c * chunk;                                        // (the chunks in front hold only words <= x)
        width = width - c * chunk < chunk ? width - c * chunk : chunk;
    }
    return base + (uint32_t)__builtin_popcountll(ballot64(lane < width && v[base + lane] <= x));
}

// byte i of M_b followed by 03 00: [0, bl) from the row (src = row + 2; byte 0: BFINAL cleared), zeros, FF FF at [m - 2, m), then 03 00
__device__ __forceinline__ uint8_t member_byte(const uint8_t* src, uint32_t i, uint32_t bl, uint32_t m) {
    if (i < bl) return i == 0u ? (uint8_t)(src[0] & 0xFEu) : src[i];
    if (i < m - 2u) return (uint8_t)0u;
    return i < m ? (uint8_t)0xFFu : i == m ? (uint8_t)0x03u : (uint8_t)0u;
}

// ---- (c) the gather.  A row of the rows' part, as a wave leaves it in LDS for its own copy loop
enum { ROW_SKIP = 0, ROW_STORED = 1, ROW_MEMBER = 2, ROW_LAST_MEMBER = 3 };

// (W: the call is hdlz_zip64_write_ws -- the rows and the tiles are the same code; the entries' part writes the ZIP64 forms)
template <bool W>
__global__ __launch_bounds__(256) void k_zipw_gather(ZipWriteArgs a, uint32_t row_groups, uint32_t tile_groups, uint32_t rows_per_group) {
    __shared__ uint64_t s_dst[ROWS_MAX], s_src[ROWS_MAX];         // where the row's bytes go in the file; where they come from (rows / in)
    __shared__ uint32_t s_len[ROWS_MAX], s_m[ROWS_MAX], s_kind[ROWS_MAX];      // the bytes taken from there; |M_b|
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t E = (uint32_t)a.nentries;
    const bool write = a.w.head[H_WRITE] != 0u;                   // (uniform over the grid)
    if (blockIdx.x < row_groups) {
        // ---- rows
        if (!write) return;
        // every wave looks up and copies its own quarter of the group's rows: no wave waits for another's loads
        const uint32_t per = rows_per_group / 4u, w0 = wave * per;          // 4 or 64 rows a wave
        const uint64_t b0 = (uint64_t)blockIdx.x * rows_per_group + w0;      // the wave's first row
        {
            // the entry of the wave's first row by the whole wave; the rows behind it lie in that entry or in one of the next 64,
            // which one round of loads shows (a lane whose row lies further on -- many entries without rows -- searches alone)
            const uint32_t ub0 = wave_upper_bound(a.blk_first, E + 1u, b0, lane);       // F_{ub0 - 1} <= b0 < F_{ub0}
            const uint64_t next = ub0 + lane <= E ? a.blk_first[ub0 + lane] : ~0ull;
            uint32_t ub = ub0;
            for (uint32_t r = 0; r < per; r++) {
                const uint32_t c = (uint32_t)__builtin_popcountll(ballot64(next <= b0 + r));
                if (lane == r) ub = ub0 + c;
            }
            const uint64_t b = b0 + lane;
            uint32_t kind = ROW_SKIP;
            if (lane < per && b < a.nblocks) {
                if (ub == ub0 + 64u) ub = upper(a.blk_first, E + 1u, b);
                if (ub >= 1u && ub <= E) {                        // (else: a row that no entry owns)
                    const uint32_t e = ub - 1u;
                    const uint64_t F0 = a.blk_first[e], skip = a.in_off[b] - a.in_off[F0];      // skip: the entry's bytes in front of this block
                    if ((a.w.form[e] & 0xFFu) != METHOD_DEFLATED) {
                        kind = ROW_STORED;                        // a stored entry that has rows: the block's input bytes
                        s_dst[w0 + lane] = a.w.pay[e] + skip; s_src[w0 + lane] = a.ent_off[e] + skip;
                        s_len[w0 + lane] = (uint32_t)(a.in_off[b + 1u] - a.in_off[b]); s_m[w0 + lane] = 0u;
                    } else {
                        uint32_t bl;
                        const uint32_t m = member_len(a.len[b], a.end_bits[b], a.pitch, bl);
                        kind = b + 1u == a.blk_first[ub] ? ROW_LAST_MEMBER : ROW_MEMBER;
                        s_dst[w0 + lane] = a.w.pay[e] + (a.w.pre[b] - a.w.pre[F0]); s_src[w0 + lane] = b * a.pitch + 2u;
                        s_len[w0 + lane] = bl; s_m[w0 + lane] = m;
                    }
                }
            }
            if (lane < per) s_kind[w0 + lane] = kind;
        }
        wave_lds_order();                                         // (the wave reads only what it wrote itself)
        {
            for (uint32_t r = w0; r < w0 + per; r++) {
                const uint32_t kind = s_kind[r];
                if (kind == ROW_SKIP) continue;
                if (kind == ROW_STORED) {
                    copy_to_aligned16(a.file + s_dst[r], a.in + s_src[r], s_len[r], lane, 64u);
                    continue;
                }
                const uint32_t bl = s_len[r], m = s_m[r];
                const uint32_t rn = m + (kind == ROW_LAST_MEMBER ? 2u : 0u);
                const uint8_t* __restrict__ src = a.rows + s_src[r];
                uint8_t* __restrict__ dst = a.file + s_dst[r];
                const uint32_t head = min(rn, (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u));
                if (lane < head) dst[lane] = member_byte(src, lane, bl, m);
                const uint32_t body = bl > head ? (bl - head) >> 4 : 0u;      // whole 16-byte chunks of the row's bytes: no load leaves row[2 .. nbytes)
                const uint8_t* s16 = src + head;
                uint8_t* d16 = dst + head;
                uint32_t k = lane;
                for (; k + 192u < body; k += 256u) {              // four loads in flight a lane
                    v4 x0 = *reinterpret_cast<const v4u*>(s16 + 16u * k), x1 = *reinterpret_cast<const v4u*>(s16 + 16u * (k + 64u));
                    v4 x2 = *reinterpret_cast<const v4u*>(s16 + 16u * (k + 128u)), x3 = *reinterpret_cast<const v4u*>(s16 + 16u * (k + 192u));
                    if (head == 0u && k == 0u) x0.x &= ~1u;       // (the member starts at a 16-byte boundary: BFINAL sits in the body)
                    *reinterpret_cast<v4*>(d16 + 16u * k) = x0; *reinterpret_cast<v4*>(d16 + 16u * (k + 64u)) = x1;
                    *reinterpret_cast<v4*>(d16 + 16u * (k + 128u)) = x2; *reinterpret_cast<v4*>(d16 + 16u * (k + 192u)) = x3;
                }
                for (; k < body; k += 64u) {
                    v4 x = *reinterpret_cast<const v4u*>(s16 + 16u * k);
                    if (head == 0u && k == 0u) x.x &= ~1u;
                    *reinterpret_cast<v4*>(d16 + 16u * k) = x;
                }
                const uint32_t done = head + 16u * body;          // at most 15 bytes of the row, the marker and 03 00 are left
                if (done + lane < rn) dst[done + lane] = member_byte(src, done + lane, bl, m);
            }
        }
        return;
    }
    if (blockIdx.x < row_groups + tile_groups) {
        // ---- tiles of the stored entries without rows
        __shared__ uint32_t s_e;
        const uint64_t ntiles = a.w.head[H_TILES];                // (0 unless the file is written)
        for (uint64_t t = blockIdx.x - row_groups; t < ntiles; t += tile_groups) {
            if (tid == 0u) s_e = upper(a.w.tile0, E + 1u, t) - 1u;            // tile0[e] <= t < tile0[e + 1]
            __syncthreads();
            const uint32_t e = s_e;
            const uint64_t u = a.ent_off[e + 1u] - a.ent_off[e], at = (t - a.w.tile0[e]) * STORE_TILE;
            const uint32_t n = u - at < STORE_TILE ? (uint32_t)(u - at) : STORE_TILE;
            copy_to_aligned16(a.file + a.w.pay[e] + at, a.in + a.ent_off[e] + at, n, tid, 256u);
            __syncthreads();                                      // (s_e has been read)
        }
        return;
    }
    // ---- entries: the two headers, the name behind both, the record
    const uint32_t e = (blockIdx.x - row_groups - tile_groups) * 4u + wave;
    if (e >= E) return;
    if constexpr (W) {
        entry_headers64(a, e, lane, write);
        return;
    }
    const uint32_t form = a.w.form[e], method = form & 0xFFu, csize = a.w.csize[e], crc = a.crc[e];
    const uint32_t usize = (uint32_t)(a.ent_off[e + 1u] - a.ent_off[e]), n = (uint32_t)(a.name_off[e + 1u] - a.name_off[e]);
    const uint64_t pay = a.w.pay[e], L = pay - LOCREC - n, cd = a.w.cdrec[e];
    if (a.entries && lane == 0u) {
        hdlz_zip_entry rec;
        const bool sound = a.w.head[H_FAILED] == 0u;
        rec.cd_off = sound ? cd : 0u; rec.payload_off = sound ? pay : 0u; rec.out_off = sound ? a.w.out_off[e] : 0u;
        rec.csize = sound ? csize : 0u; rec.usize = sound ? usize : 0u; rec.crc = sound ? crc : 0u;
        rec.method = (uint16_t)(sound ? method : 0u); rec.flags = (uint16_t)(sound ? a.flags : 0u); rec.name_len = (uint16_t)(sound ? n : 0u);
        rec.reserved = 0u;
        rec.status = form >> 8;
        a.entries[e] = rec;
    }
    if (!write) return;
    const uint32_t time = a.datetime & 0xFFFFu, date = a.datetime >> 16;
    const uint32_t lw[8] = {SIG_LOCAL, VERSION | (a.flags << 16), method | (time << 16), date | (crc << 16), (crc >> 16) | (csize << 16),
                            (csize >> 16) | (usize << 16), (usize >> 16) | (n << 16), 0u};
    const uint32_t cw[12] = {SIG_CD, VERSION | (VERSION << 16), a.flags | (method << 16), time | (date << 16), crc, csize, usize, n, 0u, 0u,
                             (uint32_t)L << 16, (uint32_t)L >> 16};
    if (lane < LOCREC) a.file[L + lane] = record_byte(lw, lane);
    if (lane < CDREC) a.file[cd + lane] = record_byte(cw, lane);
    const uint8_t* name = a.names + a.name_off[e];
    copy_to_aligned16(a.file + L + LOCREC, name, n, lane, 64u);
    copy_to_aligned16(a.file + cd + CDREC, name, n, lane, 64u);
}

}  // namespace zipw

// the scratch, in this order, every piece a multiple of 256 bytes (include/hdlz_zip_write.h states the sum)
// (wide: hdlz_zip64_write_ws -- c_e is a 64-bit word; include/hdlz_zip64.h states that sum)
static ZipWriteWork zip_write_work(void* work, uint64_t nentries, uint64_t nblocks, bool wide, size_t* bytes) {
    const uintptr_t base = reinterpret_cast<uintptr_t>(work);
    const uint64_t ntiles = join_tiles(nblocks);
    size_t at = 0;
    auto piece = [&](size_t n) { const uintptr_t p = base + at; at += round256(n); return p; };
    ZipWriteWork w;
    w.ticket = reinterpret_cast<uint32_t*>(piece(8u + 16u * (size_t)ntiles));
    w.desc = reinterpret_cast<unsigned long long*>(w.ticket + 2);
    w.desc2 = w.desc + ntiles;
    w.pre = reinterpret_cast<uint64_t*>(piece(8u * ((size_t)nblocks + 1u)));
    w.cnt = reinterpret_cast<uint64_t*>(piece(8u * ((size_t)nblocks + 1u)));
    w.head = reinterpret_cast<uint64_t*>(piece(256u));
    w.pay = reinterpret_cast<uint64_t*>(piece(8u * ((size_t)nentries + 1u)));
    w.cdrec = reinterpret_cast<uint64_t*>(piece(8u * ((size_t)nentries + 1u)));
    w.out_off = reinterpret_cast<uint64_t*>(piece(8u * ((size_t)nentries + 1u)));
    w.csize = reinterpret_cast<uint32_t*>(piece((wide ? 8u : 4u) * ((size_t)nentries + 1u)));
    w.csize64 = reinterpret_cast<uint64_t*>(w.csize);
    w.form = reinterpret_cast<uint32_t*>(piece(4u * ((size_t)nentries + 1u)));
    w.tile0 = reinterpret_cast<uint32_t*>(piece(4u * ((size_t)nentries + 1u)));
    *bytes = at;
    return w;
}

size_t zip_write_work_bytes(uint64_t nentries, uint64_t nblocks, bool wide) {
    size_t bytes;
    (void)zip_write_work(nullptr, nentries, nblocks, wide, &bytes);
    return bytes;
}

hipError_t launch_zip_write(ZipWriteArgs a, void* work, hipStream_t stream, bool wide) {
    using namespace zipw;
    size_t bytes;
    a.w = zip_write_work(work, a.nentries, a.nblocks, wide, &bytes);
    const uint64_t ntiles = join_tiles(a.nblocks);
    hipError_t e = hipSuccess;
    if (ntiles) {
        e = zero_words(a.w.ticket, (uint32_t)(2u + 4u * ntiles), stream);      // the ticket and both look-back words of every tile
        if (e == hipSuccess) e = launch(k_zipw_scan, dim3((unsigned)ntiles), dim3(JT), stream, a);
    }
    if (e == hipSuccess) e = launch(wide ? k_zipw64_plan : k_zipw_plan, dim3(1), dim3(PLAN_THREADS), stream, a);
    if (e != hipSuccess) return e;
    // the gather's three kinds of workgroup, every count from what the host knows
    // rows a workgroup: 16 keep every CU busy with a few thousand large rows; with many small ones 64 spread the search over more rows
    const uint32_t rows_per_group = a.nblocks >= ROWS_MANY_MIN ? ROWS_MAX : ROWS_FEW;
    const uint64_t row_groups = (a.nblocks + rows_per_group - 1u) / rows_per_group;
    uint64_t tile_groups = a.nentries ? a.total_in / STORE_TILE + a.nentries : 0u;      // (an entry ends in at most one partial tile)
    if (tile_groups > (1u << 17)) tile_groups = 1u << 17;
    const uint64_t entry_groups = (a.nentries + 3u) / 4u;
    if (row_groups + tile_groups + entry_groups == 0u) return hipSuccess;
    return launch(wide ? k_zipw_gather<true> : k_zipw_gather<false>, dim3((unsigned)(row_groups + tile_groups + entry_groups)), dim3(256), stream, a, (uint32_t)row_groups, (uint32_t)tile_groups, rows_per_group);
}

}  // namespace hdlz
