// hdlz_join.hip -- join the rows of a compressed batch into ONE standard zlib stream (include/hdlz_join.h).
//
// Row b of hdlz_compress_batch_bits is a complete zlib stream: 78 9C, one FINAL fixed block, Adler-32.  Its member of the joined stream
// is the block alone with BFINAL cleared, followed by the sync marker of an empty stored block, which brings the stream back to a byte
// boundary: with E = the bit the end-of-block code starts at (counted from the row's first bit: only the compress kernel knows it,
// the pad bits behind the code cannot be told from the zero bits a literal may end in), nbytes = (E + 14) >> 3 and p = 8 nbytes - E - 7
// pad bits (0 .. 7),
//     member = row[2 .. nbytes) with bit 0 of its first byte cleared, then 00 00 FF FF when p >= 3 (the stored block's three header
//              bits fall inside the padding), else 00 00 00 FF FF
//     stream = 78 9C, the members, 03 00 (a final empty fixed block), Adler-32 of the whole input, big-endian.
// k_join is k_archive's pattern (hdlz_compact.hip; restated here, not shared: as a shared inline function the look-back changed
// k_archive's instruction schedule): a workgroup takes a TILE of 256 consecutive rows by a ticket, scans the 256 member lengths,
// publishes its sum as one 64-bit word {state, value} and finds its base by a decoupled look-back over the tiles in front of it; then
// it writes the 256 offsets and copies its members, a wave per row, with 16-byte stores to 16-byte aligned destinations.  The same
// pass reads every row's trailer and leaves the tile's three Adler sums and its worst status in the scratch; k_join_finish (one
// workgroup) reduces them and writes the header, the final block, the checksum and the result record.
//
// The Adler-32 of the concatenation X (N bytes) from the blocks' own: with A_b = s1_b - 1 (the block's byte sum), n_b its length and e_b
// its END offset in X, s2(X) = N + sum_p (N - p) x_p and N - p = (N - e_b) + (n_b - q) for byte q of block b, so (all mod 65521)
//     s1 = 1 + sum A_b          s2 = N + N sum A_b - sum e_b A_b + sum (s2_b - n_b)
// -- three sums over the blocks in any order: a reduction, not a scan.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_device.h"
#include "hdlz_compress_common.h"                        // the framing constants: HEADER_WORD, HEADER_BITS, block_nbytes; hdlz_adler.h: ADLER_MOD

namespace hdlz {

constexpr uint32_t JT = 256;                             // rows per tile
constexpr uint64_t J_AGG = 1ull << 62, J_PFX = 2ull << 62, J_MASK = 3ull << 62;
constexpr uint32_t PARTS = 4;                            // words a tile leaves for k_join_finish: sum A, sum e A, sum (s2 - n), worst status
constexpr uint64_t STREAM_HEAD = 2;                      // 78 9C: the first member starts here
constexpr uint32_t HEAD0 = HEADER_WORD & 0xFFu, HEAD1 = (HEADER_WORD >> 8) & 0xFFu;      // 78 9C
constexpr uint32_t FINAL_EMPTY = HEADER_WORD >> 16;      // 03 (+ 00): BFINAL = 1, BTYPE = 01 and the seven zero bits of the end-of-block code
constexpr uint32_t STREAM_TAIL = 6;                      // 03 00 + Adler-32

struct JoinArgs {
    const uint8_t* rows;
    uint64_t pitch;
    const uint32_t* len;
    const uint64_t* end_bits;
    const uint32_t* status;
    const uint64_t* in_off;      // nullable: then every block has in_len bytes
    uint32_t in_len;
    uint64_t nblocks;
    uint8_t* stream;
    uint64_t cap;
    uint64_t* off;
    hdlz_join_result* result;
    uint32_t* ticket;            // scratch: ticket (+ pad), ...
    unsigned long long* desc;    // ... one look-back word per tile, ...
    uint32_t* part;              // ... PARTS words per tile
    const uint32_t* crc = nullptr;      // BGZF only: the CRC-32 of every input block
};

__device__ __forceinline__ uint32_t wave_add(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}

// BGZF = true (hdlz_bgzf_join_ws; include/hdlz_bgzf.h) is the same scan and gather for another member: the row's block
// as it is (BFINAL stays 1: every member is a gzip member of its own) between an 18-byte header that carries the member's size and
// the trailer CRC-32, ISIZE.  The first member starts at 0, a.end_bits is not read, and of the tile's PARTS words the first holds
// the lowest failed row (NONE_BAD: none) in place of an Adler sum; the others but the status are not used.
constexpr uint32_t BGZF_HEAD = 18, BGZF_TAIL = 8, BGZF_MAX = 65536, NONE_BAD = 0xFFFFFFFFu;
__constant__ const uint8_t BGZF_HEADER[16] = {0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0};
__constant__ const uint8_t BGZF_EOF[28] = {0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0, 0x1B, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

template <bool BGZF>
__global__ __launch_bounds__(256) void k_join(JoinArgs a) {
    constexpr uint64_t HEAD = BGZF ? 0u : STREAM_HEAD;   // where the first member starts
    __shared__ uint32_t s_tile;
    __shared__ uint64_t s_wsum[4], s_base;
    __shared__ uint64_t s_off[JT];
    __shared__ uint32_t s_body[JT];                      // bytes of the member that come from the row (0: no member)
    __shared__ uint32_t s_part[4][PARTS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0u) s_tile = atomicAdd(a.ticket, 1u);
    __syncthreads();
    const uint32_t tile = s_tile;
    const uint64_t b = (uint64_t)tile * JT + tid;

    // ---- the row's member length, and its share of the three Adler sums
    uint32_t m = 0, body_len = 0, st = HDLZ_OK, pa = 0, pe = 0, ps = 0;
    if constexpr (BGZF) {
        pa = NONE_BAD;
        if (b < a.nblocks) {
            st = a.status[b];
            const uint32_t n = a.len[b];
            const uint64_t nb = a.in_off ? a.in_off[b + 1] - a.in_off[b] : (uint64_t)a.in_len;
            if (st == HDLZ_OK && (n < 8u || (uint64_t)n > a.pitch)) st = HDLZ_E_BAD_PARAM;      // 78 9C, at least 03 00, Adler-32: what is read below lies inside the row
            else if (st == HDLZ_OK && (n > BGZF_MAX - 20u || nb > BGZF_MAX)) st = HDLZ_E_OUT_CAPACITY;
            if (st == HDLZ_OK) {
                body_len = n - 6u;
                m = body_len + BGZF_HEAD + BGZF_TAIL;
            } else pa = tid;
        }
    } else if (b < a.nblocks) {
        st = a.status[b];
        const uint32_t n = a.len[b];
        const uint64_t E = a.end_bits[b];
        // (the three arrays must describe the same row, and the row must lie inside the pitch: what is read below follows from them)
        if (st == HDLZ_OK && (E < HEADER_BITS || block_nbytes(E) + 4u != (uint64_t)n || (uint64_t)n > a.pitch)) st = HDLZ_E_BAD_PARAM;
        if (st == HDLZ_OK) {
            const uint32_t nbytes = n - 4u;
            const uint32_t p = (uint32_t)(8ull * nbytes - E) - 7u;            // pad bits behind the end-of-block code
            body_len = nbytes - (uint32_t)STREAM_HEAD;
            m = body_len + (p >= 3u ? 4u : 5u);
            uint64_t e, nb;
            if (a.in_off) {
                const uint64_t hi = a.in_off[b + 1];
                e = hi - a.in_off[0];
                nb = hi - a.in_off[b];
            } else {
                nb = a.in_len;
                e = (b + 1u) * (uint64_t)a.in_len;
            }
            const uint8_t* t = a.rows + b * a.pitch + nbytes;                 // the row's trailer: s2 then s1, big-endian
            const uint32_t s2 = ((uint32_t)t[0] << 8) | t[1], s1 = ((uint32_t)t[2] << 8) | t[3];
            pa = (s1 % ADLER_MOD + ADLER_MOD - 1u) % ADLER_MOD;
            pe = (uint32_t)((e % ADLER_MOD) * pa % ADLER_MOD);
            ps = (s2 % ADLER_MOD + ADLER_MOD - (uint32_t)(nb % ADLER_MOD)) % ADLER_MOD;
        }
    }
    s_body[tid] = body_len;
    {   // (256 residues below 65521: the sums stay below 2^24)
        const uint32_t ra = BGZF ? wave_min(pa) : wave_add(pa), re = wave_add(pe), rs = wave_add(ps), rt = wave_max(st);
        if (lane == 0u) { s_part[wave][0] = ra; s_part[wave][1] = re; s_part[wave][2] = rs; s_part[wave][3] = rt; }
    }
    // ---- exclusive scan of the tile's member lengths
    uint64_t v = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(v, o, 64);
        if (lane >= (uint32_t)o) v += t;
    }
    if (lane == 63u) s_wsum[wave] = v;
    __syncthreads();
    const uint64_t w0 = s_wsum[0], w1 = s_wsum[1], w2 = s_wsum[2], w3 = s_wsum[3];
    const uint64_t local = v - m + (wave > 0u ? w0 : 0ull) + (wave > 1u ? w1 : 0ull) + (wave > 2u ? w2 : 0ull);
    const uint64_t tsum = w0 + w1 + w2 + w3;
    if (tid < PARTS) {
        const uint32_t x0 = s_part[0][tid], x1 = s_part[1][tid], x2 = s_part[2][tid], x3 = s_part[3][tid];
        if (BGZF && tid == 0u) {
            const uint32_t f = min(min(x0, x1), min(x2, x3));
            a.part[(size_t)PARTS * tile] = f == NONE_BAD ? NONE_BAD : tile * JT + f;
        } else a.part[(size_t)PARTS * tile + tid] = tid == 3u ? max(max(x0, x1), max(x2, x3)) : x0 + x1 + x2 + x3;
    }
    if (wave == 0u) {
        uint64_t base = 0;
        if (tile != 0u) {
            if (lane == 0u) __hip_atomic_store(&a.desc[tile], J_AGG | tsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int64_t t = (int64_t)tile - 1 - (int64_t)lane;        // lane 0 looks at the nearest tile
            for (;;) {
                uint64_t d = J_PFX;                                // (tiles in front of tile 0: an empty prefix)
                if (t >= 0) {
                    do { d = __hip_atomic_load(&a.desc[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while ((d & J_MASK) == 0ull);
                }
                const uint64_t pm = ballot64((d & J_MASK) == J_PFX);
                const uint32_t first = pm ? (uint32_t)__builtin_ctzll(pm) : 64u;      // the nearest published prefix among these 64
                uint64_t x = lane <= first ? (d & ~J_MASK) : 0ull;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
                base += x;
                if (pm) break;
                t -= 64;
            }
        }
        if (lane == 0u) {
            __hip_atomic_store(&a.desc[tile], J_PFX | (base + tsum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_base = base;
            if ((uint64_t)(tile + 1u) * JT >= a.nblocks) a.off[a.nblocks] = HEAD + base + tsum;      // the last tile: where 03 00 (BGZF: the EOF member) goes
        }
    }
    __syncthreads();
    const uint64_t mine = HEAD + s_base + local;
    if (b < a.nblocks) a.off[b] = mine;
    s_off[tid] = mine;
    __syncthreads();
    // ---- the copy: a wave per row, 64 rows each
    for (uint32_t r = wave * 64u; r < wave * 64u + 64u; r++) {
        const uint64_t rb = (uint64_t)tile * JT + r;
        if (rb >= a.nblocks) break;
        const uint64_t o0 = s_off[r];
        const uint32_t rn = (uint32_t)((r + 1u < JT ? s_off[r + 1u] : HEAD + s_base + tsum) - o0);      // the member's length
        if (rn == 0u || o0 + rn > a.cap) continue;            // a failed row / a member that would end beyond the capacity
        typedef uint32_t v4 __attribute__((ext_vector_type(4)));
        typedef v4 __attribute__((aligned(1))) v4u;
        if constexpr (BGZF) {
            const uint32_t bl = s_body[r];                    // rn = 18 + bl + 8
            const uint8_t* src = a.rows + rb * a.pitch + 2u;  // row[2 .. 2 + bl): the block
            uint8_t* dst = a.stream + o0;
            if (lane < 16u) dst[lane] = BGZF_HEADER[lane];
            else if (lane < BGZF_HEAD) dst[lane] = (uint8_t)((rn - 1u) >> (8u * (lane - 16u)));      // BSIZE
            else if (lane < BGZF_HEAD + BGZF_TAIL) {
                const uint32_t k = lane - BGZF_HEAD;
                const uint32_t isize = a.in_off ? (uint32_t)(a.in_off[rb + 1] - a.in_off[rb]) : a.in_len;
                dst[BGZF_HEAD + bl + k] = (uint8_t)((k < 4u ? a.crc[rb] : isize) >> (8u * (k & 3u)));
            }
            uint8_t* d2 = dst + BGZF_HEAD;
            const uint32_t head = min(bl, (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(d2) & 15u)) & 15u));
            if (lane < head) d2[lane] = src[lane];
            const uint32_t body = (bl - head) >> 4;           // whole 16-byte chunks: no load leaves row[2 .. 2 + bl)
            for (uint32_t k = lane; k < body; k += 64u) *reinterpret_cast<v4*>(d2 + head + 16u * k) = *reinterpret_cast<const v4u*>(src + head + 16u * k);
            const uint32_t done = head + 16u * body;          // at most 15 bytes are left
            if (done + lane < bl) d2[done + lane] = src[done + lane];
            continue;
        }
        const uint32_t bl = s_body[r], mark0 = rn - 2u;      // [0, bl): from the row; [bl, mark0): 00; [mark0, rn): FF
        const uint8_t* src = a.rows + rb * a.pitch + STREAM_HEAD;
        uint8_t* dst = a.stream + o0;
        auto member_byte = [&](uint32_t i) -> uint8_t {
            if (i < bl) return i == 0u ? (uint8_t)(src[0] & 0xFEu) : src[i];      // byte 0: BFINAL cleared
            return i >= mark0 ? (uint8_t)0xFFu : (uint8_t)0u;
        };
        const uint32_t head = min(rn, (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u));
        if (lane < head) dst[lane] = member_byte(lane);
        const uint32_t body = bl > head ? (bl - head) >> 4 : 0u;      // whole 16-byte chunks of the row's bytes: no load leaves row[2 .. nbytes)
        for (uint32_t k = lane; k < body; k += 64u) {
            v4 x = *reinterpret_cast<const v4u*>(src + head + 16u * k);
            if (head == 0u && k == 0u) x.x &= ~1u;            // (the member starts at a 16-byte boundary: BFINAL sits in the body)
            *reinterpret_cast<v4*>(dst + head + 16u * k) = x;
        }
        const uint32_t done = head + 16u * body;              // at most 15 bytes of the row and the marker are left
        if (done + lane < rn) dst[done + lane] = member_byte(done + lane);
    }
}

// one workgroup: the tiles' sums -> the checksum, the worst status; the header, the final block, the trailer, the result record
__global__ __launch_bounds__(256) void k_join_finish(JoinArgs a, uint32_t ntiles) {
    __shared__ uint64_t s_sum[256][3];
    __shared__ uint32_t s_st[256];
    const uint32_t tid = threadIdx.x;
    uint64_t sa = 0, se = 0, ss = 0;
    uint32_t st = HDLZ_OK;
    for (uint32_t t = tid; t < ntiles; t += 256u) {          // (up to 2^23 tiles of sums below 2^24)
        const uint32_t* q = a.part + (size_t)PARTS * t;
        sa += q[0]; se += q[1]; ss += q[2]; st = max(st, q[3]);
    }
    s_sum[tid][0] = sa; s_sum[tid][1] = se; s_sum[tid][2] = ss; s_st[tid] = st;
    __syncthreads();
    for (uint32_t o = 128u; o > 0u; o >>= 1) {
        if (tid < o) {
            s_sum[tid][0] += s_sum[tid + o][0]; s_sum[tid][1] += s_sum[tid + o][1]; s_sum[tid][2] += s_sum[tid + o][2];
            s_st[tid] = max(s_st[tid], s_st[tid + o]);
        }
        __syncthreads();
    }
    if (tid != 0u) return;
    const uint64_t A = s_sum[0][0] % ADLER_MOD, EA = s_sum[0][1] % ADLER_MOD, S = s_sum[0][2] % ADLER_MOD;
    uint64_t N = 0;
    if (a.nblocks) N = a.in_off ? a.in_off[a.nblocks] - a.in_off[0] : a.nblocks * (uint64_t)a.in_len;
    const uint64_t Nm = N % ADLER_MOD;
    const uint32_t s1 = (uint32_t)((1u + A) % ADLER_MOD);
    const uint32_t s2 = (uint32_t)((Nm + Nm * A % ADLER_MOD + (ADLER_MOD - EA) + S) % ADLER_MOD);
    if (a.nblocks == 0) a.off[0] = STREAM_HEAD;
    const uint64_t end = a.off[a.nblocks];                   // (k_join's last tile wrote it, in front of this launch)
    const uint64_t total = end + STREAM_TAIL;
    hdlz_join_result res;
    res.stream_len = s_st[0] != HDLZ_OK ? 0u : total;
    res.status = s_st[0] != HDLZ_OK ? s_st[0] : total > a.cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)HDLZ_OK;
    res.adler = s_st[0] != HDLZ_OK ? 0u : (s2 << 16) | s1;
    *a.result = res;
    if (a.cap >= STREAM_HEAD) { a.stream[0] = (uint8_t)HEAD0; a.stream[1] = (uint8_t)HEAD1; }
    if (s_st[0] == HDLZ_OK && total <= a.cap) {
        uint8_t* t = a.stream + end;
        t[0] = (uint8_t)FINAL_EMPTY; t[1] = 0;
        t[2] = (uint8_t)(s2 >> 8); t[3] = (uint8_t)s2; t[4] = (uint8_t)(s1 >> 8); t[5] = (uint8_t)s1;
    }
}

// ---- the gzip form (include/hdlz_gzip.h).  Its header is 10 = 8 + 2 bytes: k_join, pointed at stream + 8 with a capacity
// 8 smaller, puts every member where the gzip stream wants it and leaves the zlib form's index.  This kernel, in place of
// k_join_finish, lifts the index by 8 (every workgroup its share of d_off[0 .. nblocks); the word d_off[nblocks] is workgroup 0's:
// it reads the end from it) and, in workgroup 0, reduces the tiles' worst status and writes the header, the final block, the trailer
// -- the caller's CRC-32 word and N mod 2^32, little-endian -- and the result record.  a.stream / a.cap are k_join's view.
constexpr uint64_t GZ_HEAD = 10, GZ_LIFT = GZ_HEAD - STREAM_HEAD;
constexpr uint32_t GZ_TAIL = 10;                         // 03 00 + CRC-32 + ISIZE
__constant__ const uint8_t GZ_HEADER[GZ_HEAD] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF};      // CM 8, FLG 0, MTIME 0, XFL 0, OS 255

__global__ __launch_bounds__(256) void k_join_gzip_finish(JoinArgs a, uint32_t ntiles, const uint32_t* __restrict__ crc, uint8_t* gz,
                                                          uint64_t gz_cap, hdlz_join_gzip_result* result) {
    __shared__ uint32_t s_st[256];
    const uint32_t tid = threadIdx.x;
    for (uint64_t b = (uint64_t)blockIdx.x * 256u + tid; b < a.nblocks; b += (uint64_t)gridDim.x * 256u) a.off[b] += GZ_LIFT;
    if (blockIdx.x != 0u) return;
    uint32_t st = HDLZ_OK;
    for (uint32_t t = tid; t < ntiles; t += 256u) st = max(st, a.part[(size_t)PARTS * t + 3u]);
    s_st[tid] = st;
    __syncthreads();
    for (uint32_t o = 128u; o > 0u; o >>= 1) {
        if (tid < o) s_st[tid] = max(s_st[tid], s_st[tid + o]);
        __syncthreads();
    }
    if (tid != 0u) return;
    st = s_st[0];
    uint64_t N = 0;
    if (a.nblocks) N = a.in_off ? a.in_off[a.nblocks] - a.in_off[0] : a.nblocks * (uint64_t)a.in_len;
    const uint64_t end = (a.nblocks ? a.off[a.nblocks] : STREAM_HEAD) + GZ_LIFT;      // (k_join's last tile wrote it, in front of this launch)
    a.off[a.nblocks] = end;
    const uint64_t total = end + GZ_TAIL;
    const uint32_t c = crc[0], isize = (uint32_t)N;
    hdlz_join_gzip_result res;
    res.stream_len = st != HDLZ_OK ? 0u : total;
    res.status = st != HDLZ_OK ? st : total > gz_cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)HDLZ_OK;
    res.crc = st != HDLZ_OK ? 0u : c;
    *result = res;
    if (gz_cap >= GZ_HEAD)
        for (uint32_t k = 0; k < GZ_HEAD; k++) gz[k] = GZ_HEADER[k];
    if (st == HDLZ_OK && total <= gz_cap) {
        uint8_t* t = gz + end;
        t[0] = (uint8_t)FINAL_EMPTY; t[1] = 0;
        for (uint32_t k = 0; k < 4u; k++) { t[2u + k] = (uint8_t)(c >> (8u * k)); t[6u + k] = (uint8_t)(isize >> (8u * k)); }
    }
}

// ---- the BGZF form: one workgroup behind k_join<true>: the tiles' worst status and lowest failed row, the EOF member, the record
__global__ __launch_bounds__(256) void k_bgzf_join_finish(JoinArgs a, uint32_t ntiles, hdlz_bgzf_join_result* result) {
    __shared__ uint32_t s_st[256], s_f[256];
    const uint32_t tid = threadIdx.x;
    uint32_t st = HDLZ_OK, f = NONE_BAD;
    for (uint32_t t = tid; t < ntiles; t += 256u) {
        const uint32_t* q = a.part + (size_t)PARTS * t;
        st = max(st, q[3]); f = min(f, q[0]);
    }
    s_st[tid] = st; s_f[tid] = f;
    __syncthreads();
    for (uint32_t o = 128u; o > 0u; o >>= 1) {
        if (tid < o) { s_st[tid] = max(s_st[tid], s_st[tid + o]); s_f[tid] = min(s_f[tid], s_f[tid + o]); }
        __syncthreads();
    }
    st = s_st[0];
    if (a.nblocks == 0 && tid == 0u) a.off[0] = 0u;
    const uint64_t end = a.nblocks ? a.off[a.nblocks] : 0u;      // (k_join's last tile wrote it, in front of this launch)
    const uint64_t total = end + sizeof(BGZF_EOF);
    if (st == HDLZ_OK && total <= a.cap && tid < sizeof(BGZF_EOF)) a.stream[end + tid] = BGZF_EOF[tid];
    if (tid != 0u) return;
    hdlz_bgzf_join_result res;
    res.file_len = st != HDLZ_OK ? 0u : total;
    res.status = st != HDLZ_OK ? st : total > a.cap ? (uint32_t)HDLZ_E_OUT_CAPACITY : (uint32_t)HDLZ_OK;
    res.first_bad = s_f[0];
    *result = res;
}

static inline uint64_t join_tiles(uint64_t nblocks) { return (nblocks + JT - 1u) / JT; }

size_t join_work_bytes(uint64_t nblocks) {                     // ticket (+ pad), one 64-bit look-back word and PARTS words per tile
    const uint64_t ntiles = join_tiles(nblocks);
    return ntiles ? round256(sizeof(uint32_t) * (2u + (2u + PARTS) * (size_t)ntiles)) : 0u;
}

hipError_t launch_join(const uint8_t* rows, uint64_t pitch, const uint32_t* len, const uint64_t* end_bits, const uint32_t* status,
                       const uint64_t* in_off, uint32_t in_len, uint64_t nblocks, uint8_t* stream_out, uint64_t cap, uint64_t* off,
                       hdlz_join_result* result, void* work, hipStream_t stream) {
    const uint64_t ntiles = join_tiles(nblocks);
    uint32_t* ws = static_cast<uint32_t*>(work);
    JoinArgs a{rows, pitch, len, end_bits, status, in_off, in_len, nblocks, stream_out, cap, off, result, ws,
               reinterpret_cast<unsigned long long*>(ws + 2), ws + 2u + 2u * (size_t)ntiles};
    if (ntiles) {
        const hipError_t e = zero_words(ws, (uint32_t)(2u + 2u * ntiles), stream);      // the ticket and the look-back words
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_join<false>, dim3((unsigned)ntiles), dim3(256), 0, stream, a);
        const hipError_t e2 = hipGetLastError();
        if (e2 != hipSuccess) return e2;
    }
    hipLaunchKernelGGL(k_join_finish, dim3(1), dim3(256), 0, stream, a, (uint32_t)ntiles);
    return hipGetLastError();
}

hipError_t launch_join_gzip(const uint8_t* rows, uint64_t pitch, const uint32_t* len, const uint64_t* end_bits, const uint32_t* status,
                            const uint64_t* in_off, uint32_t in_len, uint64_t nblocks, const uint32_t* crc, uint8_t* stream_out,
                            uint64_t cap, uint64_t* off, hdlz_join_gzip_result* result, void* work, hipStream_t stream) {
    const uint64_t ntiles = join_tiles(nblocks);
    uint32_t* ws = static_cast<uint32_t*>(work);
    // k_join's view: the stream from byte 8 on (a capacity below 8 leaves it no room at all: it then writes no byte)
    JoinArgs a{rows, pitch, len, end_bits, status, in_off, in_len, nblocks, stream_out + GZ_LIFT, cap > GZ_LIFT ? cap - GZ_LIFT : 0u, off,
               nullptr, ws, reinterpret_cast<unsigned long long*>(ws + 2), ws + 2u + 2u * (size_t)ntiles};
    if (ntiles) {
        const hipError_t e = zero_words(ws, (uint32_t)(2u + 2u * ntiles), stream);      // the ticket and the look-back words
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_join<false>, dim3((unsigned)ntiles), dim3(256), 0, stream, a);
        const hipError_t e2 = hipGetLastError();
        if (e2 != hipSuccess) return e2;
    }
    const unsigned grid = (unsigned)(ntiles < 1024u ? (ntiles ? ntiles : 1u) : 1024u);
    hipLaunchKernelGGL(k_join_gzip_finish, dim3(grid), dim3(256), 0, stream, a, (uint32_t)ntiles, crc, stream_out, cap, result);
    return hipGetLastError();
}

hipError_t launch_bgzf_join(const uint8_t* rows, uint64_t pitch, const uint32_t* len, const uint32_t* status, const uint64_t* in_off,
                            uint32_t in_len, uint64_t nblocks, const uint32_t* crc, uint8_t* file, uint64_t cap, uint64_t* off,
                            hdlz_bgzf_join_result* result, void* work, hipStream_t stream) {
    const uint64_t ntiles = join_tiles(nblocks);
    uint32_t* ws = static_cast<uint32_t*>(work);
    JoinArgs a{rows, pitch, len, nullptr, status, in_off, in_len, nblocks, file, cap, off, nullptr, ws,
               reinterpret_cast<unsigned long long*>(ws + 2), ws + 2u + 2u * (size_t)ntiles, crc};
    if (ntiles) {
        const hipError_t e = zero_words(ws, (uint32_t)(2u + 2u * ntiles), stream);      // the ticket and the look-back words
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_join<true>, dim3((unsigned)ntiles), dim3(256), 0, stream, a);
        const hipError_t e2 = hipGetLastError();
        if (e2 != hipSuccess) return e2;
    }
    hipLaunchKernelGGL(k_bgzf_join_finish, dim3(1), dim3(256), 0, stream, a, (uint32_t)ntiles, result);
    return hipGetLastError();
}

}  // namespace hdlz
