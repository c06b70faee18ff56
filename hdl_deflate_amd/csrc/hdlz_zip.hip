// hdlz_zip.hip -- the kernels of include/hdlz_zip.h: the index of a ZIP file's directory, and what hdlz_zip_inflate_ws
// runs around the decode.  The decode itself is an existing kernel either way (hdlz_api.hip): the task view of the wave-per-member
// decoder, or -- one entry -- the batch call's own path; the CRC-32 is crc_block / crc_tiles / crc_finish of hdlz_crc32.h.
//
// k_zip_end          ONE workgroup: the end record.  Each thread tests one position a step, 256 positions from the file's end down; the
//                    largest position of a step whose signature and comment length fit wins and ends the search (positions of later
//                    steps are smaller).  Thread 0 makes the checks of step 1 and writes the summary.
// k_zip_walk         ONE workgroup: the directory staged through LDS in pieces of PIECE bytes, coalesced 16-byte loads; one lane
//                    follows the hops in LDS (scalar code: aligned words and funnel shifts, one LDS round trip a hop) and the
//                    workgroup writes the offsets of the piece's central records out together.  A piece starts AT the record the last
//                    one could not hold whole (its 46 fixed bytes), so a record may straddle any boundary or be longer than a piece.
// k_zip_entries      a thread per entry: the 46 bytes, the local header's two lengths, the checks of step 3 -> the record (but out_off)
//                    and the size the entry counts in the output.
// k_zip_offsets      ONE workgroup: the scan of the rounded sizes -> out_off, total_out, the result record.
// k_zip_check        a thread per entry of hdlz_zip_inflate_ws: the checks in front of the decode, the decoder's view of the entry.
// k_zip_copy         stored entries: blockIdx.y strides over the entries, blockIdx.x over the pieces of one (count >= 2: one workgroup
//                    an entry; count == 1: the grid sized from out_cap).  16-byte loads and stores at any alignment, bytes at the end.
// k_zip_crc_slots    count >= 2: a workgroup per entry, crc_block over its slot.
// k_zip_crc_tiles / k_zip_crc_finish   count == 1: crc_tiles over the slot (the grid sized from out_cap), then crc_finish.
// k_zip_judge / k_zip_finish   the verdict per entry; the lowest failed entry and the record.
// Plain stores only.  Loads: d_file[0 .. file_len) only; of a slot only its usize bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_crc32.h"
#include "hdlz_frame.h"
#include "hdlz_plan.h"

namespace hdlz {
namespace zip {

constexpr uint32_t EOCD = 22u, CDREC = 46u, LOCREC = 30u, COMMENT_MAX = 65535u, ENTRIES_MAX = 65536u;      // (a directory holds at most 65535)
constexpr uint32_t SIG_EOCD = 0x06054B50u, SIG_CD = 0x02014B50u, SIG_LOCAL = 0x04034B50u, SIG_LOCATOR = 0x07064B50u;
constexpr uint32_t PIECE = 16384u, WALK_THREADS = 256u;          // a staging piece: four 16-byte loads a thread
constexpr uint32_t SCAN_THREADS = 1024u;
constexpr uint32_t SKIP = 0xFFFFFFFFu;                           // the decoder's status word of a stored entry: it is left alone
constexpr uint32_t DST_CAP_MAX = 0xFFFFFE00u;                    // the task view's room (member_view: o + 258 never wraps)


// the summary at the front of the index scratch (64-bit words), then cdoff[65536] and size[65536] (32-bit words)
struct IndexWork {
    uint64_t* head;      // [0] p, [1] cd_off, [2] cd_size, [3] total entries, [4] step 1's status, [5] entries passed, [6] the walk's status
    uint32_t *cdoff, *size;
};
__host__ __device__ inline IndexWork index_work(void* work) {
    IndexWork w;
    w.head = static_cast<uint64_t*>(work);
    w.cdoff = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(work) + 256u);
    w.size = w.cdoff + ENTRIES_MAX;
    return w;
}

// ---- hdlz_zip_index_ws, step 1
__global__ __launch_bounds__(256) void k_zip_end(const uint8_t* __restrict__ f, uint64_t file_len, IndexWork w) {
    __shared__ uint32_t s_best;                                   // p + 1 of the step's largest fitting position; 0: none
    const uint32_t tid = threadIdx.x;
    uint32_t status = HDLZ_OK;
    uint64_t p = 0;
    if (file_len < EOCD) status = HDLZ_E_NO_EOF;
    else {
        const uint64_t hi = file_len - EOCD, lo = hi > COMMENT_MAX ? hi - COMMENT_MAX : 0u;
        if (tid == 0u) s_best = 0u;
        __syncthreads();
        bool found = false;
        for (uint64_t top = hi;; top -= 256u) {                   // this step: positions top, top - 1, .. top - 255
            const bool mine = top >= lo + tid && le32(f + (top - tid)) == SIG_EOCD &&
                              (top - tid) + EOCD + le16(f + (top - tid) + 20u) == file_len;
            if (__syncthreads_or(mine)) {
                if (mine) atomicMax(&s_best, (uint32_t)(top - tid) + 1u);      // (file_len < 2^32)
                __syncthreads();
                found = true;
                break;
            }
            if (top < lo + 256u) break;                           // (uniform)
        }
        if (!found) status = HDLZ_E_BAD_HEADER;
        else p = s_best - 1u;
    }
    if (tid != 0u) return;
    uint64_t cd_off = 0, cd_size = 0, total = 0;
    if (status == HDLZ_OK) {
        const uint8_t* r = f + p;
        cd_size = le32(r + 12u); cd_off = le32(r + 16u); total = le16(r + 10u);
        if (p >= 20u && le32(r - 20u) == SIG_LOCATOR) status = HDLZ_E_BAD_HEADER;
        else if (le16(r + 4u) != 0u || le16(r + 6u) != 0u || le16(r + 8u) != total || cd_off + cd_size != p) status = HDLZ_E_BAD_HEADER;
    }
    if (status != HDLZ_OK) { p = 0; cd_off = 0; cd_size = 0; total = 0; }
    w.head[0] = p; w.head[1] = cd_off; w.head[2] = cd_size; w.head[3] = total; w.head[4] = status;
}

// ---- step 2
__global__ __launch_bounds__(WALK_THREADS) void k_zip_walk(const uint8_t* __restrict__ f, IndexWork w) {
    __shared__ __attribute__((aligned(16))) uint32_t s_words[PIECE / 4u];
    __shared__ uint32_t s_cd[PIECE / CDREC + 4u];                 // the records that start in the piece (at most PIECE / 46 + 1)
    __shared__ uint64_t s_q;
    __shared__ uint32_t s_done, s_e0, s_e1;
    uint8_t* const s_piece = reinterpret_cast<uint8_t*>(s_words);
    const uint32_t tid = threadIdx.x;
    const uint64_t p = w.head[0];
    const uint32_t total = (uint32_t)w.head[3];
    if (w.head[4] != HDLZ_OK) {                                   // (uniform)
        if (tid == 0u) { w.head[5] = 0u; w.head[6] = HDLZ_OK; }
        return;
    }
    // the four bytes at byte x of the piece, any alignment: two aligned LDS words and a funnel shift (x + 8 <= the piece's bytes)
    auto word_at = [&](uint32_t x) { return __funnelshift_r(s_words[x >> 2], s_words[(x >> 2) + 1u], (x & 3u) * 8u); };
    uint64_t q = w.head[1];
    uint32_t e = 0, status = HDLZ_OK;                             // (thread 0's)
    for (;;) {
        // the piece [q, q + PIECE) of the directory, as far as it lies in front of p: nothing at or behind p is loaded
        const uint32_t room = (uint32_t)(p - q);                  // (q <= p < 2^32: cd_off + cd_size == p, and a hop beyond p stops the walk)
        const uint32_t have = room < PIECE ? room : PIECE;
#pragma unroll
        for (uint32_t k = 0; k < PIECE / (16u * WALK_THREADS); k++) {
            const uint32_t at = (k * WALK_THREADS + tid) * 16u;
            if (at + 16u <= have) *reinterpret_cast<v4*>(s_piece + at) = *reinterpret_cast<const v4u*>(f + q + at);
            else for (uint32_t i = at; i < have; i++) s_piece[i] = f[q + i];
        }
        __syncthreads();
        if (tid == 0u) {
            uint32_t at = 0;                                      // q = the piece's start + at
            bool done = false;
            const uint32_t e0 = __builtin_amdgcn_readfirstlane(e);      // the piece's first entry
            // (one lane: every value of the walk is the wave's, which keeps the hops' branches out of the execution mask)
            e = e0;
            for (;;) {
                if (e == total) { if (at != room) status = HDLZ_E_BAD_HEADER; done = true; break; }      // q != p
                if (at + CDREC > have) {
                    if (room - at < CDREC) { status = HDLZ_E_BAD_HEADER; done = true; }      // q + 46 > p
                    break;                                        // else: the record starts the next piece
                }
                // the signature and the three lengths: bytes at .. at + 3 and at + 28 .. at + 33 (the words read end in front of at + 46)
                const uint32_t sig = __builtin_amdgcn_readfirstlane(word_at(at)), nm = __builtin_amdgcn_readfirstlane(word_at(at + 28u)),
                               k = __builtin_amdgcn_readfirstlane(word_at(at + 32u)) & 0xFFFFu;
                const uint32_t hop = CDREC + (nm & 0xFFFFu) + (nm >> 16) + k;
                // one test for both stops (no signature; q' > p), so that the three reads fly together: one LDS round trip a hop
                if ((uint32_t)(sig != SIG_CD) | (uint32_t)(hop > room - at)) { status = HDLZ_E_BAD_HEADER; done = true; break; }
                s_cd[e - e0] = (uint32_t)q + at;                  // (the workgroup writes them out together)
                e += 1u;
                if (hop > have - at) { at += hop; break; }        // q' lies behind the piece (at > have; q' <= p)
                at += hop;
            }
            s_q = q + at;
            s_done = done ? 1u : 0u;
            s_e0 = e0; s_e1 = e;
        }
        __syncthreads();
        for (uint32_t i = s_e0 + tid; i < s_e1; i += WALK_THREADS) w.cdoff[i] = s_cd[i - s_e0];
        if (s_done) break;
        q = s_q;
        __syncthreads();                                          // (s_q and s_done have been read; the piece may be staged again)
    }
    if (tid == 0u) { w.head[5] = e; w.head[6] = status; }
}

// ---- step 3: a thread per passed entry
__global__ __launch_bounds__(256) void k_zip_entries(const uint8_t* __restrict__ f, uint64_t entry_cap, hdlz_zip_entry* __restrict__ entries,
                                                     IndexWork w) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= w.head[5]) return;
    const uint64_t cd_off = w.head[1];
    const uint64_t q = w.cdoff[e];
    const uint8_t* r = f + q;
    const uint32_t flags = le16(r + 8u), method = le16(r + 10u), crc = le32(r + 16u), csize = le32(r + 20u), usize = le32(r + 24u);
    const uint32_t name_len = le16(r + 28u), disk = le16(r + 34u);
    const uint64_t L = le32(r + 42u);
    uint32_t st = HDLZ_OK;
    uint64_t payload = 0;
    if (flags & 0x41u) st = HDLZ_E_BAD_BTYPE;
    else if (method != 0u && method != 8u) st = HDLZ_E_BAD_BTYPE;
    else if (csize == 0xFFFFFFFFu || usize == 0xFFFFFFFFu || L == 0xFFFFFFFFull || disk != 0u) st = HDLZ_E_BAD_HEADER;
    else if (method == 0u && csize != usize) st = HDLZ_E_BAD_HEADER;
    else if (L + LOCREC > cd_off || le32(f + L) != SIG_LOCAL) st = HDLZ_E_BAD_HEADER;
    else {
        payload = L + LOCREC + le16(f + L + 26u) + le16(f + L + 28u);
        if (payload + csize > cd_off) { st = HDLZ_E_BAD_HEADER; payload = 0; }
    }
    w.size[e] = st == HDLZ_OK ? usize : 0u;
    if (e >= entry_cap) return;
    hdlz_zip_entry rec;
    rec.cd_off = q; rec.payload_off = payload; rec.out_off = 0u;          // (k_zip_offsets writes out_off)
    rec.csize = csize; rec.usize = usize; rec.crc = crc;
    rec.method = (uint16_t)method; rec.flags = (uint16_t)flags; rec.name_len = (uint16_t)name_len; rec.reserved = 0u;
    rec.status = st;
    entries[e] = rec;
}

// ---- step 4 and the record: a strip of the entries a thread (hdlz_plan.h)
__global__ __launch_bounds__(SCAN_THREADS) void k_zip_offsets(uint64_t entry_cap, uint32_t out_align, hdlz_zip_entry* __restrict__ entries,
                                                              hdlz_zip_index_result* __restrict__ result, IndexWork w) {
    __shared__ uint64_t s_wave[1][SCAN_THREADS / 64u];
    __shared__ uint64_t s_total;
    const uint32_t tid = threadIdx.x;
    const uint64_t n = (uint32_t)w.head[5];                       // (at most ENTRIES_MAX)
    const uint64_t mask = (uint64_t)out_align - 1u;
    uint64_t lo, hi;
    strip(n, SCAN_THREADS, tid, lo, hi);
    uint64_t mine[1] = {0u}, base[1], total[1];
    for (uint64_t e = lo; e < hi; e++) mine[0] += ((uint64_t)w.size[e] + mask) & ~mask;
    if (tid == 0u) s_total = 0u;                                  // (no entries)
    block_scan<1, SCAN_THREADS>(mine, base, total, s_wave);
    for (uint64_t e = lo; e < hi; e++) {
        const uint64_t s = w.size[e];
        if (e < entry_cap) entries[e].out_off = base[0];
        if (e + 1u == n) s_total = base[0] + s;                   // the end of the last slot
        base[0] += (s + mask) & ~mask;
    }
    __syncthreads();
    if (tid != 0u) return;
    hdlz_zip_index_result res;
    res.nentries = n; res.total_out = s_total; res.cd_off = w.head[1]; res.cd_size = w.head[2];
    const uint32_t s1 = (uint32_t)w.head[4];
    res.status = s1 != HDLZ_OK ? s1 : n > entry_cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)w.head[6];
    res.reserved = 0u;
    *result = res;
}

// ---- hdlz_zip64_index_ws (include/hdlz_zip64.h): the four kernels above, generalised -- a locator and the ZIP64 end record, offsets and
// counts in 64 bits, the ZIP64 extra field, a scratch and a scan sized from entry_cap.  The classic call keeps its own four.
constexpr uint32_t SIG_END64 = 0x06064B50u, END64 = 56u, LOCATOR = 20u, EXTRA_ZIP64 = 0x0001u;

__device__ __forceinline__ uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

// the summary (64-bit words), then for each of the entry_cap entries that get a record the offset of its central record and its size
struct Index64Work {
    uint64_t* head;      // [0] D, [1] cd_off, [2] cd_size, [3] total entries, [4] step 1's status, [5] entries passed, [6] the walk's status
    uint64_t *cdoff, *size;
};
__host__ __device__ inline Index64Work index64_work(void* work, uint64_t entry_cap) {
    Index64Work w;
    w.head = static_cast<uint64_t*>(work);
    w.cdoff = w.head + 32;
    w.size = w.cdoff + entry_cap;
    return w;
}

// step 1: the search of k_zip_end -- the lowest lane of the first step with a fit holds the largest position, so the offset in the
// step is what the workgroup agrees on (p itself may pass 2^32) --, then thread 0 reads the locator and the ZIP64 end record
__global__ __launch_bounds__(256) void k_zip64_end(const uint8_t* __restrict__ f, uint64_t file_len, Index64Work w) {
    __shared__ uint32_t s_best;                                   // the lowest lane whose position fits
    const uint32_t tid = threadIdx.x;
    uint32_t status = HDLZ_OK;
    uint64_t p = 0;
    if (file_len < EOCD) status = HDLZ_E_NO_EOF;
    else {
        const uint64_t hi = file_len - EOCD, lo = hi > COMMENT_MAX ? hi - COMMENT_MAX : 0u;
        if (tid == 0u) s_best = 256u;
        __syncthreads();
        bool found = false;
        for (uint64_t top = hi;; top -= 256u) {                   // this step: positions top, top - 1, .. top - 255
            const bool mine = top >= lo + tid && le32(f + (top - tid)) == SIG_EOCD &&
                              (top - tid) + EOCD + le16(f + (top - tid) + 20u) == file_len;
            if (__syncthreads_or(mine)) {
                if (mine) atomicMin(&s_best, tid);
                __syncthreads();
                p = top - s_best;
                found = true;
                break;
            }
            if (top < lo + 256u) break;                           // (uniform)
        }
        if (!found) status = HDLZ_E_BAD_HEADER;
    }
    if (tid != 0u) return;
    uint64_t D = 0, cd_off = 0, cd_size = 0, total = 0;
    if (status == HDLZ_OK) {
        const uint8_t* c = f + p;                                 // the classic record
        const uint32_t c_disk = le16(c + 4u), c_cddisk = le16(c + 6u), c_here = le16(c + 8u), c_total = le16(c + 10u), c_size = le32(c + 12u),
                       c_off = le32(c + 16u);
        if (p >= LOCATOR && le32(c - 20u) == SIG_LOCATOR) {
            const uint64_t lim = p - LOCATOR, r = le64(c - 12u);  // the ZIP64 end record must end at the locator
            bool ok = le32(c - 16u) == 0u && le32(c - 4u) <= 1u && r <= lim && lim - r >= END64 && le32(f + r) == SIG_END64;
            if (ok) {
                const uint8_t* z = f + r;
                const uint64_t s = le64(z + 4u), here = le64(z + 24u);
                total = le64(z + 32u); cd_size = le64(z + 40u); cd_off = le64(z + 48u);
                ok = s >= 44u && s == lim - r - 12u && le32(z + 16u) == 0u && le32(z + 20u) == 0u && here == total &&
                     cd_off <= r && cd_size == r - cd_off && total <= cd_size / CDREC &&
                     // each classic value: the ZIP64 one, or all ones
                     (c_disk == 0u || c_disk == 0xFFFFu) && (c_cddisk == 0u || c_cddisk == 0xFFFFu) &&
                     (c_here == total || c_here == 0xFFFFu) && (c_total == total || c_total == 0xFFFFu) &&
                     (c_size == cd_size || c_size == 0xFFFFFFFFu) && (c_off == cd_off || c_off == 0xFFFFFFFFu);
            }
            if (!ok) status = HDLZ_E_BAD_HEADER;
            D = r;
        } else {
            cd_size = c_size; cd_off = c_off; total = c_total; D = p;
            if (c_disk != 0u || c_cddisk != 0u || c_here != total || cd_off + cd_size != p) status = HDLZ_E_BAD_HEADER;
        }
    }
    if (status != HDLZ_OK) { D = 0; cd_off = 0; cd_size = 0; total = 0; }
    w.head[0] = D; w.head[1] = cd_off; w.head[2] = cd_size; w.head[3] = total; w.head[4] = status;
}

// step 2: k_zip_walk with the piece's start q in 64 bits.  Inside a piece every value of the hop loop stays 32-bit: the room in front
// of D and the entries left are clipped to 2^32 - 1, which no offset in a piece (at most PIECE + 46 + 3 * 65535) and no count of a
// piece's records reaches.  The offsets of the first entry_cap records are stored; the entries behind them are counted.
__global__ __launch_bounds__(WALK_THREADS) void k_zip64_walk(const uint8_t* __restrict__ f, uint64_t entry_cap, Index64Work w) {
    __shared__ __attribute__((aligned(16))) uint32_t s_words[PIECE / 4u];
    __shared__ uint32_t s_cd[PIECE / CDREC + 4u];                 // where in the piece its records start
    __shared__ uint32_t s_at, s_done, s_n;
    uint8_t* const s_piece = reinterpret_cast<uint8_t*>(s_words);
    const uint32_t tid = threadIdx.x;
    const uint64_t D = w.head[0], total = w.head[3];
    if (w.head[4] != HDLZ_OK) {                                   // (uniform)
        if (tid == 0u) { w.head[5] = 0u; w.head[6] = HDLZ_OK; }
        return;
    }
    auto word_at = [&](uint32_t x) { return __funnelshift_r(s_words[x >> 2], s_words[(x >> 2) + 1u], (x & 3u) * 8u); };
    uint64_t q = w.head[1], e = 0;                                // the piece's start and its first entry (uniform)
    uint32_t status = HDLZ_OK;                                    // (thread 0's)
    for (;;) {
        const uint64_t room64 = D - q, left64 = total - e;        // (q <= D: cd_off + cd_size == D, and a hop beyond D stops the walk)
        const uint32_t room = room64 < 0xFFFFFFFFull ? (uint32_t)room64 : 0xFFFFFFFFu, left = left64 < 0xFFFFFFFFull ? (uint32_t)left64 : 0xFFFFFFFFu;
        const uint32_t have = room < PIECE ? room : PIECE;
#pragma unroll
        for (uint32_t k = 0; k < PIECE / (16u * WALK_THREADS); k++) {
            const uint32_t at = (k * WALK_THREADS + tid) * 16u;
            if (at + 16u <= have) *reinterpret_cast<v4*>(s_piece + at) = *reinterpret_cast<const v4u*>(f + q + at);
            else for (uint32_t i = at; i < have; i++) s_piece[i] = f[q + i];
        }
        __syncthreads();
        if (tid == 0u) {
            uint32_t at = 0, n = 0;                               // q' = the piece's start + at; n records start in the piece
            bool done = false;
            for (;;) {
                if (n == left) { if (at != room) status = HDLZ_E_BAD_HEADER; done = true; break; }      // q != D
                if (at + CDREC > have) {
                    if (room - at < CDREC) { status = HDLZ_E_BAD_HEADER; done = true; }      // q + 46 > D
                    break;                                        // else: the record starts the next piece
                }
                const uint32_t sig = __builtin_amdgcn_readfirstlane(word_at(at)), nm = __builtin_amdgcn_readfirstlane(word_at(at + 28u)),
                               k = __builtin_amdgcn_readfirstlane(word_at(at + 32u)) & 0xFFFFu;
                const uint32_t hop = CDREC + (nm & 0xFFFFu) + (nm >> 16) + k;
                if ((uint32_t)(sig != SIG_CD) | (uint32_t)(hop > room - at)) { status = HDLZ_E_BAD_HEADER; done = true; break; }
                s_cd[n] = at;
                n += 1u;
                if (hop > have - at) { at += hop; break; }        // q' lies behind the piece (at > have; q' <= D)
                at += hop;
            }
            s_at = at; s_n = n;
            s_done = done ? 1u : 0u;
        }
        __syncthreads();
        for (uint32_t i = tid; i < s_n; i += WALK_THREADS)
            if (e + i < entry_cap) w.cdoff[e + i] = q + s_cd[i];
        e += s_n;
        if (s_done) break;
        q += s_at;
        __syncthreads();                                          // (s_at, s_n and s_done have been read; the piece may be staged again)
    }
    if (tid == 0u) { w.head[5] = e; w.head[6] = status; }
}

// step 3: a thread per entry that gets a record
__global__ __launch_bounds__(256) void k_zip64_entries(const uint8_t* __restrict__ f, uint64_t entry_cap, hdlz_zip64_entry* __restrict__ entries,
                                                       Index64Work w) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= w.head[5] || e >= entry_cap) return;
    const uint64_t cd_off = w.head[1];
    const uint64_t q = w.cdoff[e];
    const uint8_t* r = f + q;
    const uint32_t flags = le16(r + 8u), method = le16(r + 10u), crc = le32(r + 16u), name_len = le16(r + 28u), m = le16(r + 30u);
    uint64_t csize = le32(r + 20u), usize = le32(r + 24u), L = le32(r + 42u);
    uint32_t disk = le16(r + 34u);
    uint32_t st = HDLZ_OK;
    uint64_t payload = 0;
    if (flags & 0x41u) st = HDLZ_E_BAD_BTYPE;
    else if (method != 0u && method != 8u) st = HDLZ_E_BAD_BTYPE;
    else {
        if (csize == 0xFFFFFFFFull || usize == 0xFFFFFFFFull || L == 0xFFFFFFFFull || disk == 0xFFFFu) {
            // the ZIP64 field: the first extra field with id 0001 (all of the walk lies inside the record, which ends at or in front of D)
            const uint8_t* x = r + CDREC + name_len;
            uint32_t at = 0, have = 0;                            // the field's data: x[at .. at + have)
            while (m - at >= 4u) {
                const uint32_t id = le16(x + at), len = le16(x + at + 2u);
                if (len > m - at - 4u) break;                     // the field overruns m
                if (id == EXTRA_ZIP64) { at += 4u; have = len; break; }
                at += 4u + len;
            }
            bool ok = true;                                       // a value X cannot supply: it keeps its word and no later one is taken
            auto take8 = [&](uint64_t& v) {
                if (!ok || v != 0xFFFFFFFFull) return;
                if (have < 8u) { ok = false; return; }
                v = le64(x + at); at += 8u; have -= 8u;
            };
            take8(usize); take8(csize); take8(L);
            if (ok && disk == 0xFFFFu) {
                if (have < 4u) ok = false;
                else disk = le32(x + at);
            }
            if (!ok) st = HDLZ_E_BAD_HEADER;
        }
        if (st != HDLZ_OK) {}
        else if (disk != 0u) st = HDLZ_E_BAD_HEADER;
        else if (method == 0u && csize != usize) st = HDLZ_E_BAD_HEADER;
        else if (L > cd_off || cd_off - L < LOCREC || le32(f + L) != SIG_LOCAL) st = HDLZ_E_BAD_HEADER;
        else {
            payload = L + LOCREC + le16(f + L + 26u) + le16(f + L + 28u);
            if (payload > cd_off || csize > cd_off - payload) { st = HDLZ_E_BAD_HEADER; payload = 0; }
        }
    }
    w.size[e] = st == HDLZ_OK ? usize : 0u;
    hdlz_zip64_entry rec;
    rec.cd_off = q; rec.payload_off = payload; rec.out_off = 0u;          // (k_zip64_offsets writes out_off)
    rec.csize = csize; rec.usize = usize; rec.crc = crc; rec.status = st;
    rec.method = (uint16_t)method; rec.flags = (uint16_t)flags; rec.name_len = (uint16_t)name_len; rec.reserved = 0u; rec.reserved2 = 0u;
    entries[e] = rec;
}

// step 4 and the record: k_zip_offsets over the n = min(entries passed, entry_cap) entries that have a record
__global__ __launch_bounds__(SCAN_THREADS) void k_zip64_offsets(uint64_t entry_cap, uint32_t out_align, hdlz_zip64_entry* __restrict__ entries,
                                                                hdlz_zip_index_result* __restrict__ result, Index64Work w) {
    __shared__ uint64_t s_wave[1][SCAN_THREADS / 64u];
    __shared__ uint64_t s_total;
    const uint32_t tid = threadIdx.x;
    const uint64_t passed = w.head[5], n = passed < entry_cap ? passed : entry_cap;
    const uint64_t mask = (uint64_t)out_align - 1u;
    uint64_t lo, hi;
    strip(n, SCAN_THREADS, tid, lo, hi);
    uint64_t mine[1] = {0u}, base[1], total[1];
    for (uint64_t e = lo; e < hi; e++) mine[0] += (w.size[e] + mask) & ~mask;
    if (tid == 0u) s_total = 0u;                                  // (no entries)
    block_scan<1, SCAN_THREADS>(mine, base, total, s_wave);
    for (uint64_t e = lo; e < hi; e++) {
        const uint64_t s = w.size[e];
        entries[e].out_off = base[0];
        if (e + 1u == n) s_total = base[0] + s;                   // the end of the last slot
        base[0] += (s + mask) & ~mask;
    }
    __syncthreads();
    if (tid != 0u) return;
    hdlz_zip_index_result res;
    res.nentries = passed; res.total_out = s_total; res.cd_off = w.head[1]; res.cd_size = w.head[2];
    const uint32_t s1 = (uint32_t)w.head[4];
    res.status = s1 != HDLZ_OK ? s1 : passed > entry_cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)w.head[6];
    res.reserved = 0u;
    *result = res;
}

// ---- hdlz_zip_inflate_ws and hdlz_zip64_inflate_ws: in front of the decode.  The kernels from here on are instantiated for either
// record; `wide` marks the lines that only the 64-bit one has (include/hdlz_zip64.h)
template <class Rec> constexpr bool wide = sizeof(Rec::usize) == 8u;

template <class Rec> __global__ __launch_bounds__(JT) void k_zip_check(ZipArgsT<Rec> a) {
    const uint64_t b = (uint64_t)blockIdx.x * JT + threadIdx.x;
    if (b >= a.count) return;
    const Rec en = a.entries[b];
    const uint64_t o0 = a.entries[0].out_off;
    const bool deflated = en.method == 8u;
    const uint64_t room = a.single ? a.out_cap & ~3ull : a.out_cap;
    uint32_t st = HDLZ_OK;
    if (en.status != HDLZ_OK) st = en.status;
    else if ((en.method != 0u && en.method != 8u) || (en.method == 0u && en.csize != en.usize)) st = HDLZ_E_BAD_PARAM;
    else if (en.payload_off < LOCREC || en.payload_off > a.in_len || en.csize > a.in_len - en.payload_off || a.in_len - en.payload_off - en.csize < 4u) st = HDLZ_E_BAD_PARAM;
    else if (en.out_off < o0 || en.out_off - o0 > room || en.usize > room - (en.out_off - o0)) st = HDLZ_E_BAD_PARAM;
    else if (wide<Rec> && deflated && en.usize > DST_CAP_MAX) st = HDLZ_E_OUT_CAPACITY;
    else if (deflated && en.csize > 0x10000000u - 7u) st = HDLZ_E_BAD_PARAM;
    else if (wide<Rec> && !a.single && en.usize > 0xFFFFFFFFull) st = HDLZ_E_BAD_PARAM;      // (crc_block's length is 32-bit)
    else if (a.bound != 0u && (a.count > 1u ? en.csize > a.bound : deflated && (uint64_t)en.csize + 6u > a.bound)) st = HDLZ_E_BAD_PARAM;
    const bool decode = st == HDLZ_OK && deflated;
    a.verdict[b] = st;
    a.len[b] = 0u; a.end_bit[b] = 0u;
    a.status[b] = decode ? (uint32_t)HDLZ_OK : st == HDLZ_OK ? SKIP : st;
    if (a.single) {                                               // the batch call's ragged index of ONE stream: it skips two bytes unread
        a.m_off[0] = decode ? en.payload_off - 2u : 0u;           // (a stored or refused entry: an empty range)
        a.m_end[0] = decode ? en.payload_off + en.csize + 4u : 0u;      // (count == 1: m_end[0] is the word behind m_off[0])
        return;
    }
    a.m_off[b] = decode ? en.payload_off : 2u;
    a.m_end[b] = decode ? en.payload_off + en.csize + 4u : 2u;
    a.m_dst[b] = a.out + (st == HDLZ_OK ? en.out_off - o0 : 0u);
    a.cap[b] = en.usize > DST_CAP_MAX ? DST_CAP_MAX : (uint32_t)en.usize;
}

// ---- stored entries
template <class Rec> __global__ __launch_bounds__(256) void k_zip_copy(ZipArgsT<Rec> a) {
    for (uint64_t b = blockIdx.y; b < a.count; b += gridDim.y) {
        const Rec en = a.entries[b];
        if (a.verdict[b] != HDLZ_OK || en.method != 0u) continue; // (uniform)
        const uint8_t* __restrict__ src = a.in + en.payload_off;
        uint8_t* __restrict__ dst = a.out + (en.out_off - a.entries[0].out_off);
        // up to 15 bytes to dst's next 16-byte boundary, whole pieces with 16-byte stores, at most 15 bytes behind them
        const uint64_t n = en.usize;
        const uint32_t head16 = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
        const uint32_t head = n < head16 ? (uint32_t)n : head16;
        const uint64_t pieces = (n - head) >> 4, done = head + 16u * pieces;
        if (blockIdx.x == 0u && threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
        for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < pieces; k += (uint64_t)gridDim.x * 256u)
            *reinterpret_cast<v4*>(dst + head + 16u * k) = *reinterpret_cast<const v4u*>(src + head + 16u * k);
        if (blockIdx.x == 0u && done + threadIdx.x < n) dst[done + threadIdx.x] = src[done + threadIdx.x];
    }
}

// the slot of entry b and the bytes in it that count: the decoded length, never more than usize (a stored entry: usize)
template <class Rec> using size_of = decltype(Rec::usize);
template <class Rec> __device__ __forceinline__ const uint8_t* slot_of(const ZipArgsT<Rec>& a, uint64_t b, size_of<Rec>& n) {
    const Rec en = a.entries[b];
    const size_of<Rec> len = en.method == 0u ? en.usize : a.len[b];
    n = len < en.usize ? len : en.usize;
    return a.out + (en.out_off - a.entries[0].out_off);
}
// does entry b have bytes to sum?  (a stored entry the checks passed, or a deflated one the decoder finished)
template <class Rec> __device__ __forceinline__ bool summed(const ZipArgsT<Rec>& a, uint64_t b) {
    return a.verdict[b] == HDLZ_OK && (a.entries[b].method == 0u || a.status[b] == HDLZ_OK);
}

template <class Rec> __global__ __launch_bounds__(CRC_THREADS) void k_zip_crc_slots(ZipArgsT<Rec> a) {
    __shared__ CrcTileLds s;
    crc_build_tables(s);
    __syncthreads();
    for (uint64_t b = blockIdx.x; b < a.count; b += gridDim.x) {
        if (!summed(a, b)) continue;                              // (uniform over the workgroup)
        size_of<Rec> n;
        const uint8_t* p = slot_of(a, b, n);
        const uint32_t c = crc_block(p, (uint32_t)n, s);            // (the 64-bit record: the checks refused a longer one)
        if (threadIdx.x == 0u) a.crc[b] = c;
    }
}

template <class Rec> __global__ __launch_bounds__(CRC_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_zip_crc_tiles(ZipArgsT<Rec> a) {
    __shared__ CrcTileLds s;
    if (!summed(a, 0)) return;
    size_of<Rec> n;
    const uint8_t* p = slot_of(a, 0, n);
    crc_tiles(p, n, a.tiles, s);
}

template <class Rec> __global__ __launch_bounds__(CRC_FIN_THREADS) void k_zip_crc_finish(ZipArgsT<Rec> a) {
    __shared__ uint32_t s_fin[CRC_FIN_THREADS];
    if (!summed(a, 0)) return;
    size_of<Rec> n;
    (void)slot_of(a, 0, n);
    const uint32_t c = crc_finish(a.tiles, n, s_fin);
    if (threadIdx.x == 0u) a.crc[0] = c;
}

// ---- behind the decode and the CRC words: a thread per entry; per workgroup the lowest failed entry, in the length word of the
// workgroup's first entry, which every thread has read by then (as k_bgzf_judge does)
template <class Rec> __global__ __launch_bounds__(JT) void k_zip_judge(ZipArgsT<Rec> a) {
    __shared__ uint32_t s_first[JT / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t b = (uint64_t)blockIdx.x * JT + tid;
    uint32_t st = HDLZ_OK;
    if (b < a.count) {
        const Rec en = a.entries[b];
        st = a.verdict[b];
        if (st == HDLZ_OK && en.method != 0u) {
            st = a.status[b];
            if (st == HDLZ_OK) {
                // where the final block ended: the decoder counted from byte payload_off - 2 -- bytes (the batch call's path) or bits
                // (the task view's END BIT)
                const uint32_t eb = a.end_bit[b], len = a.len[b];
                const uint64_t end = en.payload_off - 2u + (a.single ? eb : (eb + 7u) >> 3);
                if (len > en.usize) st = HDLZ_E_OUT_CAPACITY;
                else if (len != en.usize) st = HDLZ_E_BAD_CHECKSUM;
                else if (end != en.payload_off + en.csize) st = HDLZ_E_NO_EOF;
            }
        }
        if (st == HDLZ_OK && a.crc[b] != en.crc) st = HDLZ_E_BAD_CHECKSUM;
        a.status[b] = st;
        if (a.entry_status) a.entry_status[b] = st;
    }
    const uint64_t m = ballot64(st != HDLZ_OK);
    if (lane == 0u) s_first[wave] = m ? wave * 64u + (uint32_t)__builtin_ctzll(m) : NONE;
    __syncthreads();
    if (tid == 0u) {
        uint32_t f = NONE;
#pragma unroll
        for (uint32_t k = 0; k < JT / 64u; k++) f = min(f, s_first[k]);
        a.len[b] = f == NONE ? NONE : (uint32_t)b + f;            // (b: the workgroup's first entry; count < 2^31)
    }
}

template <class Rec> __global__ __launch_bounds__(256) void k_zip_finish(ZipArgsT<Rec> a, uint32_t ngroups) {
    __shared__ uint32_t s_f[256];
    const uint32_t tid = threadIdx.x;
    s_f[tid] = lowest_word(a.len, ngroups, tid, 256u);
    __syncthreads();
    for (uint32_t o = 128u; o > 0u; o >>= 1) {
        if (tid < o) s_f[tid] = min(s_f[tid], s_f[tid + o]);
        __syncthreads();
    }
    if (tid != 0u) return;
    hdlz_zip_inflate_result res;
    res.out_len = 0u; res.first_bad = ~0ull; res.status = HDLZ_OK; res.reserved = 0u;
    if (s_f[0] != NONE) { res.status = a.status[s_f[0]]; res.first_bad = s_f[0]; }
    else if (a.count) {
        const Rec last = a.entries[a.count - 1u];
        res.out_len = last.out_off - a.entries[0].out_off + last.usize;
    }
    *a.result = res;
}

}  // namespace zip

size_t zip_index_work_bytes() { return 256u + 2u * sizeof(uint32_t) * zip::ENTRIES_MAX; }

hipError_t launch_zip_index(const uint8_t* file, uint64_t file_len, uint64_t entry_cap, uint32_t out_align, hdlz_zip_entry* entries,
                            hdlz_zip_index_result* result, void* work, hipStream_t stream) {
    using namespace zip;
    const IndexWork w = index_work(work);
    hipError_t e = launch(k_zip_end, dim3(1), dim3(256), stream, file, file_len, w);
    if (e == hipSuccess) e = launch(k_zip_walk, dim3(1), dim3(WALK_THREADS), stream, file, w);
    if (e == hipSuccess) e = launch(k_zip_entries, dim3(ENTRIES_MAX / 256u), dim3(256), stream, file, entry_cap, entries, w);
    if (e == hipSuccess) e = launch(k_zip_offsets, dim3(1), dim3(SCAN_THREADS), stream, entry_cap, out_align, entries, result, w);
    return e;
}

size_t zip64_index_work_bytes(uint64_t entry_cap) { return 256u + round256(2u * sizeof(uint64_t) * (size_t)entry_cap); }

hipError_t launch_zip64_index(const uint8_t* file, uint64_t file_len, uint64_t entry_cap, uint32_t out_align, hdlz_zip64_entry* entries,
                              hdlz_zip_index_result* result, void* work, hipStream_t stream) {
    using namespace zip;
    const Index64Work w = index64_work(work, entry_cap);
    hipError_t e = launch(k_zip64_end, dim3(1), dim3(256), stream, file, file_len, w);
    if (e == hipSuccess) e = launch(k_zip64_walk, dim3(1), dim3(WALK_THREADS), stream, file, entry_cap, w);
    if (e == hipSuccess && entry_cap) e = launch(k_zip64_entries, dim3((unsigned)((entry_cap + 255u) / 256u)), dim3(256), stream, file, entry_cap, entries, w);
    if (e == hipSuccess) e = launch(k_zip64_offsets, dim3(1), dim3(SCAN_THREADS), stream, entry_cap, out_align, entries, result, w);
    return e;
}

template <class Rec> static hipError_t zip_check(const ZipArgsT<Rec>& a, hipStream_t stream) {
    if (a.count == 0) return hipSuccess;
    return launch(zip::k_zip_check<Rec>, dim3((unsigned)((a.count + JT - 1u) / JT)), dim3(JT), stream, a);
}

// stored entries, then (behind the decode, which the caller launched in front of this) the CRC-32 of every slot
template <class Rec> static hipError_t zip_copy(const ZipArgsT<Rec>& a, hipStream_t stream) {
    if (a.count == 0) return hipSuccess;
    const uint64_t pieces = (a.out_cap >> 4) / 256u + 1u;         // count == 1: a workgroup per 4 KiB of capacity, the rest is the stride
    const dim3 grid(a.single ? (unsigned)(pieces < 4096u ? pieces : 4096u) : 1u, (unsigned)(a.count < 65535u ? a.count : 65535u));
    return launch(zip::k_zip_copy<Rec>, grid, dim3(256), stream, a);
}

template <class Rec> static hipError_t zip_crc(const ZipArgsT<Rec>& a, hipStream_t stream) {
    using namespace zip;
    if (a.count == 0) return hipSuccess;
    if (!a.single) return launch(k_zip_crc_slots<Rec>, dim3((unsigned)(a.count < (1u << 20) ? a.count : (1u << 20))), dim3(CRC_THREADS), stream, a);
    const uint64_t tiles = crc32_tiles(a.out_cap);                  // (at least one: out_cap >= 4)
    hipError_t e = launch(k_zip_crc_tiles<Rec>, dim3((unsigned)(tiles < CRC_GRID_MAX ? tiles : CRC_GRID_MAX)), dim3(CRC_THREADS), stream, a);
    if (e == hipSuccess) e = launch(k_zip_crc_finish<Rec>, dim3(1), dim3(CRC_FIN_THREADS), stream, a);
    return e;
}

template <class Rec> static hipError_t zip_judge(const ZipArgsT<Rec>& a, hipStream_t stream) {
    using namespace zip;
    const uint32_t ngroups = (uint32_t)((a.count + JT - 1u) / JT);
    if (ngroups) {
        const hipError_t e = launch(k_zip_judge<Rec>, dim3(ngroups), dim3(JT), stream, a);
        if (e != hipSuccess) return e;
    }
    return launch(k_zip_finish<Rec>, dim3(1), dim3(256), stream, a, ngroups);
}


hipError_t launch_zip_check(const ZipArgs& a, hipStream_t stream) { return zip_check(a, stream); }
hipError_t launch_zip_copy(const ZipArgs& a, hipStream_t stream) { return zip_copy(a, stream); }
hipError_t launch_zip_crc(const ZipArgs& a, hipStream_t stream) { return zip_crc(a, stream); }
hipError_t launch_zip_judge(const ZipArgs& a, hipStream_t stream) { return zip_judge(a, stream); }
hipError_t launch_zip_check(const ZipArgs64& a, hipStream_t stream) { return zip_check(a, stream); }
hipError_t launch_zip_copy(const ZipArgs64& a, hipStream_t stream) { return zip_copy(a, stream); }
hipError_t launch_zip_crc(const ZipArgs64& a, hipStream_t stream) { return zip_crc(a, stream); }
hipError_t launch_zip_judge(const ZipArgs64& a, hipStream_t stream) { return zip_judge(a, stream); }

}  // namespace hdlz
