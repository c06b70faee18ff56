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

namespace hdlz {
namespace zip {

constexpr uint32_t EOCD = 22u, CDREC = 46u, LOCREC = 30u, COMMENT_MAX = 65535u, ENTRIES_MAX = 65536u;      // (a directory holds at most 65535)
constexpr uint32_t SIG_EOCD = 0x06054B50u, SIG_CD = 0x02014B50u, SIG_LOCAL = 0x04034B50u, SIG_LOCATOR = 0x07064B50u;
constexpr uint32_t PIECE = 16384u, WALK_THREADS = 256u;          // a staging piece: four 16-byte loads a thread
constexpr uint32_t SCAN_THREADS = 1024u, SCAN_PER = ENTRIES_MAX / SCAN_THREADS;
constexpr uint32_t SKIP = 0xFFFFFFFFu;                           // the decoder's status word of a stored entry: it is left alone
constexpr uint32_t DST_CAP_MAX = 0xFFFFFE00u;                    // the task view's room (member_view: o + 258 never wraps)

typedef uint32_t v4 __attribute__((ext_vector_type(4)));
typedef v4 __attribute__((aligned(1))) v4u;

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

// ---- step 4 and the record: thread t takes the entries [SCAN_PER t, SCAN_PER (t + 1))
__global__ __launch_bounds__(SCAN_THREADS) void k_zip_offsets(uint64_t entry_cap, uint32_t out_align, hdlz_zip_entry* __restrict__ entries,
                                                              hdlz_zip_index_result* __restrict__ result, IndexWork w) {
    __shared__ uint64_t s_wave[SCAN_THREADS / 64u];
    __shared__ uint64_t s_total;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = (uint32_t)w.head[5];
    const uint64_t mask = (uint64_t)out_align - 1u;
    const uint32_t lo = tid * SCAN_PER, hi = lo + SCAN_PER < n ? lo + SCAN_PER : n;
    uint64_t mine = 0;
    for (uint32_t e = lo; e < hi; e++) mine += ((uint64_t)w.size[e] + mask) & ~mask;
    uint64_t v = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(v, o, 64);
        if (lane >= (uint32_t)o) v += t;
    }
    if (lane == 63u) s_wave[wave] = v;
    if (tid == 0u) s_total = 0u;                                  // (no entries)
    __syncthreads();
    uint64_t base = v - mine;
    for (uint32_t k = 0; k < wave; k++) base += s_wave[k];
    for (uint32_t e = lo; e < hi; e++) {
        const uint64_t s = w.size[e];
        if (e < entry_cap) entries[e].out_off = base;
        if (e + 1u == n) s_total = base + s;                      // the end of the last slot
        base += (s + mask) & ~mask;
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

// ---- hdlz_zip_inflate_ws: in front of the decode
__global__ __launch_bounds__(JT) void k_zip_check(ZipArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * JT + threadIdx.x;
    if (b >= a.count) return;
    const hdlz_zip_entry en = a.entries[b];
    const uint64_t o0 = a.entries[0].out_off;
    const bool deflated = en.method == 8u;
    const uint64_t room = a.single ? a.out_cap & ~3ull : a.out_cap;
    uint32_t st = HDLZ_OK;
    if (en.status != HDLZ_OK) st = en.status;
    else if ((en.method != 0u && en.method != 8u) || (en.method == 0u && en.csize != en.usize)) st = HDLZ_E_BAD_PARAM;
    else if (en.payload_off < LOCREC || en.payload_off > a.in_len || (uint64_t)en.csize + 4u > a.in_len - en.payload_off) st = HDLZ_E_BAD_PARAM;
    else if (en.out_off < o0 || en.out_off - o0 > room || en.usize > room - (en.out_off - o0)) st = HDLZ_E_BAD_PARAM;
    else if (deflated && en.csize > 0x10000000u - 7u) st = HDLZ_E_BAD_PARAM;
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
    a.cap[b] = en.usize > DST_CAP_MAX ? DST_CAP_MAX : en.usize;
}

// ---- stored entries
__global__ __launch_bounds__(256) void k_zip_copy(ZipArgs a) {
    for (uint64_t b = blockIdx.y; b < a.count; b += gridDim.y) {
        const hdlz_zip_entry en = a.entries[b];
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
__device__ __forceinline__ const uint8_t* slot_of(const ZipArgs& a, uint64_t b, uint32_t& n) {
    const hdlz_zip_entry en = a.entries[b];
    const uint32_t len = en.method == 0u ? en.usize : a.len[b];
    n = len < en.usize ? len : en.usize;
    return a.out + (en.out_off - a.entries[0].out_off);
}
// does entry b have bytes to sum?  (a stored entry the checks passed, or a deflated one the decoder finished)
__device__ __forceinline__ bool summed(const ZipArgs& a, uint64_t b) {
    return a.verdict[b] == HDLZ_OK && (a.entries[b].method == 0u || a.status[b] == HDLZ_OK);
}

__global__ __launch_bounds__(CRC_THREADS) void k_zip_crc_slots(ZipArgs a) {
    __shared__ CrcTileLds s;
    crc_build_tables(s);
    __syncthreads();
    for (uint64_t b = blockIdx.x; b < a.count; b += gridDim.x) {
        if (!summed(a, b)) continue;                              // (uniform over the workgroup)
        uint32_t n;
        const uint8_t* p = slot_of(a, b, n);
        const uint32_t c = crc_block(p, n, s);
        if (threadIdx.x == 0u) a.crc[b] = c;
    }
}

__global__ __launch_bounds__(CRC_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_zip_crc_tiles(ZipArgs a) {
    __shared__ CrcTileLds s;
    if (!summed(a, 0)) return;
    uint32_t n;
    const uint8_t* p = slot_of(a, 0, n);
    crc_tiles(p, n, a.tiles, s);
}

__global__ __launch_bounds__(CRC_FIN_THREADS) void k_zip_crc_finish(ZipArgs a) {
    __shared__ uint32_t s_fin[CRC_FIN_THREADS];
    if (!summed(a, 0)) return;
    uint32_t n;
    (void)slot_of(a, 0, n);
    const uint32_t c = crc_finish(a.tiles, n, s_fin);
    if (threadIdx.x == 0u) a.crc[0] = c;
}

// ---- behind the decode and the CRC words: a thread per entry; per workgroup the lowest failed entry, in the length word of the
// workgroup's first entry, which every thread has read by then (as k_bgzf_judge does)
__global__ __launch_bounds__(JT) void k_zip_judge(ZipArgs a) {
    __shared__ uint32_t s_first[JT / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t b = (uint64_t)blockIdx.x * JT + tid;
    uint32_t st = HDLZ_OK;
    if (b < a.count) {
        const hdlz_zip_entry en = a.entries[b];
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

__global__ __launch_bounds__(256) void k_zip_finish(ZipArgs a, uint32_t ngroups) {
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
        const hdlz_zip_entry last = a.entries[a.count - 1u];
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

hipError_t launch_zip_check(const ZipArgs& a, hipStream_t stream) {
    if (a.count == 0) return hipSuccess;
    return launch(zip::k_zip_check, dim3((unsigned)((a.count + JT - 1u) / JT)), dim3(JT), stream, a);
}

// stored entries, then (behind the decode, which the caller launched in front of this) the CRC-32 of every slot
hipError_t launch_zip_copy(const ZipArgs& a, hipStream_t stream) {
    if (a.count == 0) return hipSuccess;
    const uint64_t pieces = (a.out_cap >> 4) / 256u + 1u;         // count == 1: a workgroup per 4 KiB of capacity, the rest is the stride
    const dim3 grid(a.single ? (unsigned)(pieces < 4096u ? pieces : 4096u) : 1u, (unsigned)(a.count < 65535u ? a.count : 65535u));
    return launch(zip::k_zip_copy, grid, dim3(256), stream, a);
}

hipError_t launch_zip_crc(const ZipArgs& a, hipStream_t stream) {
    using namespace zip;
    if (a.count == 0) return hipSuccess;
    if (!a.single) return launch(k_zip_crc_slots, dim3((unsigned)(a.count < (1u << 20) ? a.count : (1u << 20))), dim3(CRC_THREADS), stream, a);
    const uint64_t tiles = crc32_tiles(a.out_cap);                  // (at least one: out_cap >= 4)
    hipError_t e = launch(k_zip_crc_tiles, dim3((unsigned)(tiles < CRC_GRID_MAX ? tiles : CRC_GRID_MAX)), dim3(CRC_THREADS), stream, a);
    if (e == hipSuccess) e = launch(k_zip_crc_finish, dim3(1), dim3(CRC_FIN_THREADS), stream, a);
    return e;
}

hipError_t launch_zip_judge(const ZipArgs& a, hipStream_t stream) {
    using namespace zip;
    const uint32_t ngroups = (uint32_t)((a.count + JT - 1u) / JT);
    if (ngroups) {
        const hipError_t e = launch(k_zip_judge, dim3(ngroups), dim3(JT), stream, a);
        if (e != hipSuccess) return e;
    }
    return launch(k_zip_finish, dim3(1), dim3(256), stream, a, ngroups);
}

}  // namespace hdlz
