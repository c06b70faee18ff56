// hdlz_api.hip -- the extern "C" surface of libhdlz.so (declared in include/hdlz.h).
// Host-side parameter checks + kernel launches; no CPU compute path exists here by design.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include "hdlz_device.h"

namespace {
thread_local char g_err[256] = "";

__global__ void k_set_result(uint32_t* out_len, uint32_t* status, uint32_t code) {
    *out_len = 0;
    *status = code;
}

int fail_param(const char* what) {
    snprintf(g_err, sizeof(g_err), "bad parameter: %s", what);
    return HDLZ_E_BAD_PARAM;
}
// The entry points that draw scratch from the library's pool (hipMallocFromPoolAsync / hipFreeAsync on the caller's stream) refuse a
// stream that is being captured: the calls would become graph memory nodes, and on ROCm 7.2 the memory such a node hands out does not
// keep what the graph's own kernel nodes write to it (tools/repro/graph_scratch.hip: a kernel node reads ZEROS where the node in front
// of it wrote, 2-3 million words in 60 replays, no libhdlz involved; with libhdlz: wrong bytes, a hang, and -- round 5 -- an abort in
// hipGraphLaunch when k_par_* followed garbage lists out of bounds; profiles/r06_graph_abort_cause.txt).  The _ws entry points
// allocate nothing and are capturable.
int refuse_capture(void* stream, const char* use) {
#ifdef HDLZ_ALLOW_POOL_IN_CAPTURE                         // (lib/libhdlz_poolcap.so: tools/repro/graph_abort.py shows what then happens)
    return HDLZ_OK;
#endif
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(static_cast<hipStream_t>(stream), &cs);
    if (e != hipSuccess) { (void)hipGetLastError(); return HDLZ_OK; }
    if (cs == hipStreamCaptureStatusNone) return HDLZ_OK;
    snprintf(g_err, sizeof(g_err), "bad parameter: the stream is being captured into a graph and this entry point allocates "
                                   "stream-ordered scratch: use %s (caller-owned scratch)", use);
    return HDLZ_E_BAD_PARAM;
}
int fail_hip(hipError_t e, const char* where) {
    snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
    return HDLZ_E_HIP;
}
int check_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail_hip(e, "hipGetDeviceCount");
    if (n <= 0) {
        snprintf(g_err, sizeof(g_err), "no HIP device visible: libhdlz has no CPU path");
        return HDLZ_E_HIP;
    }
    return HDLZ_OK;
}

// ---- The vocabulary of the parameter checks.  Every entry point states its OWN sequence of checks, one `if (...) return ...;` line
// each, in front of check_device(); what a check tests and how its refusal reads is written here once.  Twins -- two entry points
// whose sequences are the same line for line -- share one body (join_checks, member_index_impl, zip_index_impl, zip_inflate_impl,
// zip_write_impl); nothing else is shared, and no table drives a check.
// Behind the checks, what the container readers share is written once as well: Carver lays out a call's scratch (the size query and
// the call go through the same function), decode_members is the wave-per-member decode of a call's MemberView (with the CRC-32 of
// what decoded, where asked), inflate_one the batch call's path for a call of one stream.
template <class... P>
bool any_null(const P*... p) { return (... || !p); }
// is one of the pointers off a multiple of k (a power of two)?  A null pointer is aligned.
template <class... P>
bool misaligned(uintptr_t k, const P*... p) { return ((... | reinterpret_cast<uintptr_t>(p)) & (k - 1u)) != 0u; }
int fail_align(unsigned k, const char* names) {           // names: "a / b / c"
    snprintf(g_err, sizeof(g_err), "bad parameter: %s must be %u-byte aligned", names, k);
    return HDLZ_E_BAD_PARAM;
}
// the hipError_t of a launcher -> the call's status
int launched(hipError_t e, const char* where) { return e == hipSuccess ? HDLZ_OK : fail_hip(e, where); }
// the two knobs of the three compress entry points; false: refused, the message is set
bool window_ok(int cwindow, int maxmatch) {
    if (cwindow < 1 || cwindow > 256) fail_param("cwindow must be in [1,256]");
    else if (maxmatch != 5 && maxmatch != 10) fail_param("maxmatch must be 5 (MATCH10=False) or 10 (MATCH10=True)");
    else return true;
    return false;
}
// is the caller's scratch short of `need` bytes (0: none is needed and d_work may be null)?  true: refused, the message names the query
bool work_too_small(size_t need, const void* d_work, size_t work_bytes, const char* query) {
    if (need == 0u || (d_work && work_bytes >= need)) return false;
    snprintf(g_err, sizeof(g_err), "bad parameter: d_work smaller than %s", query);
    return true;
}
// The checks the four joins share, in their order (hdlz_join_batch_ws, hdlz_join_gzip_ws, hdlz_bgzf_join_ws, hdlz_bgzf_join_stored_ws).
// null_pointer: the entry point's own list of required pointers has a null in it; query: its size query, for the message; d_in_off:
// the BGZF forms hold it to 8 bytes as well (the other two pass null); d_crc: null where the form has none.
int join_checks(bool null_pointer, uint64_t nblocks, const void* d_off, const void* d_in_off, const void* d_result, const void* d_crc,
                const void* d_work, size_t work_bytes, const char* query, bool bgzf) {
    if (null_pointer) return fail_param("null device pointer");
    if (nblocks > 0x7FFFFFFFull) return fail_param("nblocks too large for one launch (2^31 - 1 rows)");   // (32-bit tile and word counts)
    if (work_too_small(hdlz::join_work_bytes(nblocks), d_work, work_bytes, query)) return HDLZ_E_BAD_PARAM;
    if (misaligned(8, d_work)) return fail_align(8, "d_work");
    if (misaligned(8, d_off, d_result) || (bgzf && misaligned(8, d_in_off))) return fail_align(8, bgzf ? "d_off / d_in_off / d_result" : "d_off / d_result");
    if (misaligned(4, d_crc)) return fail_align(4, "d_crc");
    return HDLZ_OK;
}
// hdlz_bgzf_index_ws and hdlz_gzip_members_index_ws (include/hdlz_gzip_members.h): the member index of a file, by either scan
template <class Result>
int member_index_impl(const uint8_t* d_file, uint64_t file_len, uint64_t member_cap, uint64_t* d_off, uint64_t* d_out_off, Result* d_result,
                      void* d_work, size_t work_bytes, void* stream, size_t need, const char* query,
                      hipError_t (*launch)(const uint8_t*, uint64_t, uint64_t, uint64_t*, uint64_t*, Result*, void*, hipStream_t), const char* kernel) {
    if (any_null(d_off, d_out_off, d_result) || (file_len && !d_file)) return fail_param("null device pointer");
    if (member_cap >= (1ull << 40)) return fail_param("member_cap too large (below 2^40)");
    if (work_too_small(need, d_work, work_bytes, query)) return HDLZ_E_BAD_PARAM;
    if (misaligned(8, d_off, d_out_off, d_result, d_work)) return fail_align(8, "d_off / d_out_off / d_result / d_work");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    return launched(launch(d_file, file_len, member_cap, d_off, d_out_off, d_result, d_work, static_cast<hipStream_t>(stream)), kernel);
}
// the scratch of a call: the caller's buffer (the _ws entry points), or the library's stream-ordered pool
hdlz::Work caller_work(void* d_work, size_t work_bytes) { return hdlz::Work{static_cast<uint8_t*>(d_work), d_work ? work_bytes : 0u, true}; }
hdlz::Work pooled_work() { return hdlz::Work{nullptr, 0u, false}; }
// A call's scratch, carved front to back.  The base is an integer: the size query carves from 0 through the same function as the
// call, and bytes() is its answer.  Pieces are packed; align256() starts the next one on a multiple of 256 bytes.
struct Carver {
    uintptr_t base;
    size_t at = 0;
    template <class T> T* take(size_t count) { const size_t o = at; at += sizeof(T) * count; return reinterpret_cast<T*>(base + o); }
    void align256() { at = hdlz::round256(at); }
    size_t bytes() const { return at; }
};
uintptr_t address(const void* p) { return reinterpret_cast<uintptr_t>(p); }
// what a layout that ends in a decoder's share answers: the bytes of it all, and the offset from which that share takes what is left
struct Laid { size_t bytes, decode; };
// What a caller's view of the member decoders differs in: the fields of hdlz::MemberArgs of the same names, and the decoder's flags
// (0: BFINAL is honoured, a member may hold any number of blocks of any type).  m_dst and m_dst_cap: the task view.
struct MemberView {
    const uint64_t *m_off, *m_end = nullptr, *m_out_off = nullptr;
    uint64_t m_out_cap = 0;
    uint32_t m_out_len = 0, m_gap = 0;
    uint8_t* const* m_dst = nullptr;
    const uint32_t* m_dst_cap = nullptr;
    uint32_t flags = 0;
};
// The member view of one flat input (hdlz::MemberArgs): n members seen through v, decoded into `out`, the three result arrays in scratch.
hdlz::MemberArgs member_args(const uint8_t* in, uint64_t n, uint8_t* out, uint32_t* len, uint32_t* status, uint32_t* end_bit, const MemberView& v) {
    hdlz::MemberArgs a{};
    a.in = in; a.nstreams = n; a.flags = v.flags; a.out = out; a.out_len = len; a.status = status; a.in_used = end_bit;
    a.m_off = v.m_off; a.m_end = v.m_end; a.m_out_off = v.m_out_off; a.m_out_len = v.m_out_len; a.m_out_cap = v.m_out_cap; a.m_gap = v.m_gap;
    a.m_dst = v.m_dst; a.m_dst_cap = v.m_dst_cap;
    return a;
}
// One decode step: a wave per member (k_inflate_dyn's member twin) over the n members of `in` seen through v.  crc: then the CRC-32 of
// what every member decoded, out + m_out_off[b] on, into crc[b] -- a member whose status is not HDLZ_OK is skipped.
int decode_members(const uint8_t* in, uint64_t n, uint8_t* out, uint32_t* len, uint32_t* status, uint32_t* end_bit, const MemberView& v, hipStream_t st,
                   uint32_t* crc = nullptr) {
    if (const int rc = launched(hdlz::launch_inflate_dyn_members(member_args(in, n, out, len, status, end_bit, v), st), "launch the member decode"); rc != HDLZ_OK) return rc;
    return crc ? launched(hdlz::launch_crc32_batch(out, v.m_out_off, 0, 0, n, crc, status, st), "launch k_crc32_batch") : HDLZ_OK;
}
}  // namespace

namespace hdlz {
__global__ __launch_bounds__(64) void k_zero_words(uint32_t* p, uint32_t n) {
    for (uint32_t i = threadIdx.x; i < n; i += 64u) p[i] = 0u;
}
hipError_t zero_words(uint32_t* p, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(64), 0, stream, p, n);
    return hipGetLastError();
}
// The library's own per-device pool for stream-ordered scratch.  Release threshold: SCRATCH_KEEP bytes stay cached between calls (the
// per-call lists of a 2^20-stream batch are 4 MB, the markers of a 16 MiB port stream 128 MB: neither pays a device allocation per
// call); anything above it goes back to the device at the next synchronisation point of the stream, so one 256 MiB single-stream
// inflate (2 GiB of markers) does not keep 2 GiB of HBM away from the caller's own allocator for the life of the process.
// hdlz_release_scratch() trims the rest.
constexpr uint64_t SCRATCH_KEEP = 256ull << 20;
static hipMemPool_t g_pools[64] = {nullptr};
static bool g_pool_tried[64] = {false};
static std::mutex g_pool_mu;                             // (callers may drive several streams / devices from several threads)
hipError_t scratch_alloc(void** p, size_t bytes, hipStream_t stream) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipGetLastError();
    std::lock_guard<std::mutex> lock(g_pool_mu);
    if (dev >= 0 && dev < 64 && !g_pool_tried[dev]) {
        g_pool_tried[dev] = true;
        hipMemPoolProps props;
        memset(&props, 0, sizeof(props));
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        hipMemPool_t pool = nullptr;
        if (hipMemPoolCreate(&pool, &props) == hipSuccess) {
            uint64_t keep = SCRATCH_KEEP;
            if (hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep) == hipSuccess) g_pools[dev] = pool;
            else (void)hipMemPoolDestroy(pool);
        }
        (void)hipGetLastError();
    }
    if (dev >= 0 && dev < 64 && g_pools[dev]) {
        const hipError_t e = hipMallocFromPoolAsync(p, bytes, g_pools[dev], stream);
        if (e == hipSuccess) return e;
        (void)hipGetLastError();
    }
    return hipMallocAsync(p, bytes, stream);
}
hipError_t scratch_release() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipGetLastError();
    std::lock_guard<std::mutex> lock(g_pool_mu);
    if (dev >= 0 && dev < 64 && g_pools[dev]) return hipMemPoolTrimTo(g_pools[dev], 0);
    return hipSuccess;
}
hipError_t Work::get(size_t need, hipStream_t stream, uint8_t** p) const {
    if (caller) {                                         // the caller's buffer or nothing: this call allocates no memory
        if (!base || need > bytes) return hipErrorOutOfMemory;
        *p = base;
        return hipSuccess;
    }
    return scratch_alloc(reinterpret_cast<void**>(p), need, stream);
}
hipError_t Work::put(uint8_t* p, hipStream_t stream) const { return caller ? hipSuccess : hipFreeAsync(p, stream); }
}  // namespace hdlz

extern "C" {

int hdlz_version(void) { return HDLZ_VERSION; }

const char* hdlz_last_error(void) { return g_err; }

const char* hdlz_status_string(int s) {
    switch (s) {
        case HDLZ_OK: return "OK";
        case HDLZ_E_SHORT_INPUT: return "SHORT_INPUT (N < 5)";
        case HDLZ_E_OUT_CAPACITY: return "OUT_CAPACITY";
        case HDLZ_E_BAD_BTYPE: return "BAD_BTYPE";
        case HDLZ_E_BAD_DISTANCE: return "BAD_DISTANCE";
        case HDLZ_E_NO_EOF: return "NO_EOF";
        case HDLZ_E_DYNAMIC_UNSUPPORTED: return "DYNAMIC_UNSUPPORTED";
        case HDLZ_E_BAD_SYMBOL: return "BAD_SYMBOL";
        case HDLZ_E_BAD_PARAM: return "BAD_PARAM";
        case HDLZ_E_HIP: return "HIP_ERROR";
        case HDLZ_E_BAD_TREE: return "BAD_TREE";
        case HDLZ_E_BAD_HEADER: return "BAD_HEADER";
        case HDLZ_E_BAD_CHECKSUM: return "BAD_CHECKSUM";
        default: return "?";
    }
}

int hdlz_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int good = 0;
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) good++;
    }
    return good;
}

size_t hdlz_out_bound(size_t n) { return 6 + (9 * n + 10 + 7) / 8; }

int hdlz_release_scratch(void) {
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    return launched(hdlz::scratch_release(), "hipMemPoolTrimTo");
}

static int compress_batch_impl(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len,
                               uint64_t nblocks, int cwindow, int maxmatch, uint8_t* d_out, uint64_t out_pitch,
                               uint32_t* d_out_len, uint32_t* d_status, uint64_t* d_end_bits, void* stream) {
    if (!window_ok(cwindow, maxmatch)) return HDLZ_E_BAD_PARAM;
    if (nblocks > 0x7FFFFFFFull) return fail_param("nblocks too large for one launch");
    if (nblocks && any_null(d_in, d_out, d_out_len, d_status)) return fail_param("null device pointer");
    if ((out_pitch & 3u) || misaligned(4, d_out)) return fail_align(4, "d_out / out_pitch");
    if (!d_in_off && in_len >= 0x80000000u) return fail_param("in_len too large");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hdlz::CompressArgs a{d_in, d_in_off, in_pitch, in_len, nblocks, cwindow, maxmatch, d_out, out_pitch, d_out_len, d_status, d_end_bits};
    return launched(hdlz::launch_compress(a, static_cast<hipStream_t>(stream)), "launch k_compress");
}

int hdlz_compress_batch(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len,
                        uint64_t nblocks, int cwindow, int maxmatch, uint8_t* d_out, uint64_t out_pitch,
                        uint32_t* d_out_len, uint32_t* d_status, void* stream) {
    return compress_batch_impl(d_in, d_in_off, in_pitch, in_len, nblocks, cwindow, maxmatch, d_out, out_pitch, d_out_len, d_status,
                               nullptr, stream);
}

// ---- include/hdlz_join.h: the batch call that also reports where every block ended, and the join of its rows into one zlib stream
int hdlz_compress_batch_bits(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len,
                             uint64_t nblocks, int cwindow, int maxmatch, uint8_t* d_out, uint64_t out_pitch,
                             uint32_t* d_out_len, uint32_t* d_status, uint64_t* d_end_bits, void* stream) {
    if (!d_end_bits) return fail_param("d_end_bits is required");
    if (misaligned(8, d_end_bits)) return fail_align(8, "d_end_bits");
    return compress_batch_impl(d_in, d_in_off, in_pitch, in_len, nblocks, cwindow, maxmatch, d_out, out_pitch, d_out_len, d_status,
                               d_end_bits, stream);
}

size_t hdlz_join_bound(uint64_t nblocks, uint32_t in_len) { return 8u + (size_t)nblocks * (hdlz_out_bound(in_len) - 1u); }

size_t hdlz_join_work_bytes(uint64_t nblocks) { return nblocks > 0x7FFFFFFFull ? 0u : hdlz::join_work_bytes(nblocks); }

int hdlz_join_batch_ws(const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_end_bits,
                       const uint32_t* d_status, const uint64_t* d_in_off, uint32_t in_len, uint64_t nblocks,
                       uint8_t* d_stream, uint64_t stream_cap, uint64_t* d_off, hdlz_join_result* d_result, void* d_work,
                       size_t work_bytes, void* stream) {
    const bool null_pointer = any_null(d_stream, d_off, d_result) || (nblocks && any_null(d_rows, d_len, d_end_bits, d_status));
    if (const int rc = join_checks(null_pointer, nblocks, d_off, nullptr, d_result, nullptr, d_work, work_bytes, "hdlz_join_work_bytes(nblocks)", false); rc != HDLZ_OK) return rc;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    const hdlz::JoinArgs a{d_rows, row_pitch, d_len, d_end_bits, d_status, d_in_off, in_len, nblocks, d_stream, stream_cap, d_off, d_result, {}};
    return launched(hdlz::launch_join(a, d_work, static_cast<hipStream_t>(stream)), "launch k_join");
}

#ifndef HDLZ_PAR_BATCH_SHORT_MAX
#define HDLZ_PAR_BATCH_SHORT_MAX HDLZ_INFLATE_PAR_BATCH_SHORT_MAX
#endif
#ifndef HDLZ_PAR_BATCH_MAX
#define HDLZ_PAR_BATCH_MAX HDLZ_INFLATE_PAR_BATCH_MAX      // (A/B builds override it: tools/bench_few_large_inflate.py)
#endif
}  // extern "C"

namespace {
constexpr uint32_t MAPPING_HINTS = HDLZ_INFLATE_LANE_PER_STREAM | HDLZ_INFLATE_WAVE_PER_STREAM | HDLZ_INFLATE_GROUP_PER_STREAM;
constexpr uint32_t INFLATE_FLAGS = MAPPING_HINTS | HDLZ_INFLATE_ASSUME_FIXED | HDLZ_INFLATE_ONEBLOCK | HDLZ_INFLATE_ONE_FIXED_BLOCK;

// the batch mapping of n streams (hdlz_inflate_batch_ws) or members (hdlz_unjoin_ws).  One LANE per stream (k_inflate_tok, 64 streams
// in lockstep per wave) needs ~10^5 streams to fill the GPU; up to HDLZ_INFLATE_WAVE_THRESHOLD streams one WAVE per stream
// (k_inflate_dyn, window decode) is faster, for any block type; in between, from HDLZ_INFLATE_GROUP_MIN to HDLZ_INFLATE_GROUP_MAX
// streams, 16 lanes per stream (k_inflate_grp) beat both.  A hint (at most one: the callers check) decides alone.
enum class Mapping { lane, group, wave };
Mapping mapping_of(uint64_t n, uint32_t flags) {
    const bool group = (flags & HDLZ_INFLATE_GROUP_PER_STREAM) ||
                       ((flags & MAPPING_HINTS) == 0u && n >= HDLZ_INFLATE_GROUP_MIN && n <= HDLZ_INFLATE_GROUP_MAX);
    const bool wave = (flags & HDLZ_INFLATE_WAVE_PER_STREAM) || (!(flags & HDLZ_INFLATE_LANE_PER_STREAM) && n <= HDLZ_INFLATE_WAVE_THRESHOLD);
    return group ? Mapping::group : wave ? Mapping::wave : Mapping::lane;
}

// does a batch of this shape take the whole-GPU path (hdlz_inflate_par.hip)?  ONE large stream: cut into pieces and decoded by the whole
// GPU.  A FEW large streams: the same chain with every kernel launched once for all of them (blockIdx.y = the stream): the batch kernels
// decode a stream as ONE serial chain (64 KiB: 5.9 ms, 1 MiB: 94 ms, however few there are); this path costs the launch chain once plus
// the streams' bytes at the rate of the single-stream path (profiles/r05_inflate_mapping.txt).  Streams below HDLZ_INFLATE_PAR_LONG bytes:
// up to HDLZ_INFLATE_PAR_BATCH_SHORT_MAX of them.  Ragged input: in_len is the caller's upper bound on the stream lengths (0 = not stated).
// The explicit mapping hints keep the batch kernels.
bool par_applies(uint64_t nstreams, uint32_t in_len, uint32_t flags) {
    if (in_len < HDLZ_INFLATE_PAR_MIN) return false;
    if (flags & (HDLZ_INFLATE_LANE_PER_STREAM | HDLZ_INFLATE_WAVE_PER_STREAM)) return false;
    if (nstreams == 1) return true;
    if (flags & HDLZ_INFLATE_GROUP_PER_STREAM) return false;
    return nstreams <= (in_len >= HDLZ_INFLATE_PAR_LONG ? HDLZ_PAR_BATCH_MAX : HDLZ_PAR_BATCH_SHORT_MAX);
}

int inflate_batch_impl(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len,
                       uint64_t nstreams, uint32_t flags, uint32_t obsize, uint8_t* d_out, uint64_t out_pitch,
                       uint32_t* d_out_len, uint32_t* d_status, const hdlz::Work& w, void* stream, uint32_t* d_in_used = nullptr) {
    if (nstreams > 0x7FFFFFFFull * 32) return fail_param("nstreams too large for one launch");
    if (nstreams && any_null(d_in, d_out, d_out_len, d_status)) return fail_param("null device pointer");
    if (flags & ~INFLATE_FLAGS) return fail_param("unknown flag");
    // the kernels keep stream lengths and bit positions in 32 bits (8 * length must not wrap)
    if (!d_in_off && in_len >= 0x10000000u) return fail_param("in_len too large (streams are limited to 256 MiB - 1)");
    if (d_in_off && in_len >= 0x10000000u) in_len = 0;      // ragged: a bound nobody can use is no bound
    if (!d_in_off && nstreams > 1 && in_pitch < in_len) return fail_param("in_pitch < in_len");
    {
        const uint32_t mf = flags & MAPPING_HINTS;
        if (mf & (mf - 1u)) return fail_param("contradictory mapping flags");
    }
    if ((out_pitch & 3u) || misaligned(4, d_out)) return fail_align(4, "d_out / out_pitch");
    if (w.caller && misaligned(256, w.base)) return fail_align(256, "d_work");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    if (nstreams == 0) return HDLZ_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hdlz::InflateArgs a{d_in, d_in_off, in_pitch, in_len, nstreams, flags, obsize, d_out, out_pitch, d_out_len, d_status, d_in_used};
    if ((flags & HDLZ_INFLATE_GROUP_PER_STREAM) && nstreams > 0x7FFFFFFFull * 16) return fail_param("nstreams too large for the 16-lanes-per-stream mapping");
    const Mapping map = mapping_of(nstreams, flags);
    if (par_applies(nstreams, in_len, flags)) {
        bool used = false;
        const int rc = launched(hdlz::launch_inflate_par(a, st, &used, w), "launch the whole-GPU inflate (k_par_*)");
        if (rc != HDLZ_OK || used) return rc;
        // (no scratch, or a shape the path leaves alone: the batch kernels below)
    }
    if (map == Mapping::wave) return launched(hdlz::launch_inflate_dyn(a, st, true), "launch k_inflate_dyn");
    // lane per stream, one TOKEN group per round (k_inflate_tok), or 16 lanes per stream
    if (const int rc = launched(map == Mapping::group ? hdlz::launch_inflate_grp(a, st) : hdlz::launch_inflate_tok(a, st, w), "launch k_inflate"); rc != HDLZ_OK) return rc;
    // second pass, same stream: streams in which pass 1 met a dynamic-tree block (status 6) are redone, again one lane each
    // (k_inflate_tok<true>); everything else is left untouched
    return launched(nstreams > 0xFFFFFFFFull ? hdlz::launch_inflate_dyn(a, st, false) : hdlz::launch_inflate_tok_dyn(a, st, false, w),
                    "launch the dynamic-tree pass");
}
// One stream (the .gz file of hdlz_gunzip_ws, the large entry of hdlz_zip_inflate_ws): the batch call's path over the two-word ragged
// index `idx` that the call's checks left on the device -- the whole-GPU chains for a large stream, their fallbacks, the wave for a
// small one.  in_len is the bound the call was given; the path takes what is left of the caller's scratch from `decode` on.
int inflate_one(const uint8_t* d_in, const uint64_t* idx, uint32_t in_len, uint8_t* d_out, uint64_t row, uint32_t* d_out_len, uint32_t* d_status,
                uint32_t* d_in_used, void* d_work, size_t work_bytes, size_t decode, void* stream) {
    return inflate_batch_impl(d_in, idx, 0, in_len, 1, 0, 0, d_out, row, d_out_len, d_status,
                              caller_work(static_cast<uint8_t*>(d_work) + decode, work_bytes - decode), stream, d_in_used);
}
}  // namespace

extern "C" {

size_t hdlz_inflate_work_bytes(uint64_t nstreams, uint32_t in_len, uint64_t out_pitch, uint32_t flags, int ragged) {
    if (nstreams == 0) return 0;
    size_t need = hdlz::inflate_tok_work_bytes(nstreams, ragged != 0);
    if (ragged && in_len >= 0x10000000u) in_len = 0;
    if (par_applies(nstreams, in_len, flags)) {
        const size_t p = hdlz::inflate_par_work_bytes(in_len, nstreams, out_pitch, flags);
        if (p > need) need = p;
    }
    return need < 256u ? 256u : need;
}

int hdlz_inflate_batch_ws(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len,
                          uint64_t nstreams, uint32_t flags, uint32_t obsize, uint8_t* d_out, uint64_t out_pitch,
                          uint32_t* d_out_len, uint32_t* d_status, void* d_work, size_t work_bytes, void* stream) {
    return inflate_batch_impl(d_in, d_in_off, in_pitch, in_len, nstreams, flags, obsize, d_out, out_pitch, d_out_len, d_status,
                              caller_work(d_work, work_bytes), stream);
}

int hdlz_inflate_batch(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len,
                       uint64_t nstreams, uint32_t flags, uint32_t obsize, uint8_t* d_out, uint64_t out_pitch,
                       uint32_t* d_out_len, uint32_t* d_status, void* stream) {
    if (const int rc = nstreams ? refuse_capture(stream, "hdlz_inflate_batch_ws") : HDLZ_OK; rc != HDLZ_OK) return rc;
    return inflate_batch_impl(d_in, d_in_off, in_pitch, in_len, nstreams, flags, obsize, d_out, out_pitch, d_out_len, d_status, pooled_work(), stream);
}

size_t hdlz_inflate_checked_work_bytes(uint64_t nstreams, uint32_t in_len, uint64_t out_pitch, uint32_t flags, int ragged) {
    if (nstreams == 0) return 0;
    return hdlz::judge_work_bytes(nstreams, out_pitch) + hdlz_inflate_work_bytes(nstreams, in_len, out_pitch, flags, ragged);
}

// The decode of hdlz_inflate_batch_ws with the end positions stored in d_in_used, then the judging pass behind it on the same stream
// (every decode path has joined its side stream when it returns).  The judging pass's share of the scratch comes off the front.
int hdlz_inflate_checked(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len,
                         uint64_t nstreams, uint32_t flags, uint32_t obsize, uint8_t* d_out, uint64_t out_pitch,
                         uint32_t* d_out_len, uint32_t* d_status, uint32_t* d_in_used, uint32_t* d_adler,
                         void* d_work, size_t work_bytes, void* stream) {
    if (!d_in_used) return fail_param("d_in_used is required");
    if (flags & ~INFLATE_FLAGS) return fail_param("unknown flag");
    if (flags & HDLZ_INFLATE_ONEBLOCK) return fail_param("HDLZ_INFLATE_ONEBLOCK: a stream cut at its first block has no trailer behind it");
    const size_t share = hdlz::judge_work_bytes(nstreams, out_pitch);
    if (work_too_small(share, d_work, work_bytes, "the judging pass's share (hdlz_inflate_checked_work_bytes - hdlz_inflate_work_bytes)")) return HDLZ_E_BAD_PARAM;
    uint8_t* wbase = static_cast<uint8_t*>(d_work);
    const hdlz::Work w = caller_work(wbase ? wbase + share : nullptr, work_bytes - share);
    const int rc = inflate_batch_impl(d_in, d_in_off, in_pitch, in_len, nstreams, flags, obsize, d_out, out_pitch, d_out_len, d_status, w, stream, d_in_used);
    if (rc != HDLZ_OK || nstreams == 0) return rc;
    const hdlz::JudgeArgs j{d_in, d_in_off, in_pitch, in_len, nstreams, d_out, out_pitch, d_out_len, d_status, d_in_used, d_adler,
                            share ? reinterpret_cast<uint2*>(wbase) : nullptr};
    return launched(hdlz::launch_judge(j, static_cast<hipStream_t>(stream)), "launch the judging pass (k_adler_*)");
}

int hdlz_compact_batch(const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_off,
                       uint64_t nblocks, uint8_t* d_archive, void* stream) {
    if (nblocks && any_null(d_rows, d_len, d_off, d_archive)) return fail_param("null device pointer");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    return launched(hdlz::launch_compact(d_rows, row_pitch, d_len, d_off, nblocks, d_archive, static_cast<hipStream_t>(stream)), "launch k_compact");
}

static int archive_impl(const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, uint64_t nblocks,
                        uint8_t* d_archive, uint64_t archive_cap, uint64_t* d_off, const hdlz::Work& w, void* stream) {
    if (!d_off || (nblocks && any_null(d_rows, d_len, d_archive))) return fail_param("null device pointer");
    if (nblocks > 0x7FFFFFFFull) return fail_param("nblocks too large for one launch (2^31 - 1 rows)");   // (32-bit tile and word counts)
    if (w.caller && work_too_small(hdlz::archive_work_bytes(nblocks), w.base, w.bytes, "hdlz_archive_work_bytes(nblocks)")) return HDLZ_E_BAD_PARAM;
    if (w.caller && misaligned(8, w.base)) return fail_align(8, "d_work");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    return launched(hdlz::launch_archive(d_rows, row_pitch, d_len, nblocks, d_archive, archive_cap, d_off, static_cast<hipStream_t>(stream), w), "launch k_archive");
}

size_t hdlz_archive_work_bytes(uint64_t nblocks) { return nblocks > 0x7FFFFFFFull ? 0u : hdlz::archive_work_bytes(nblocks); }

int hdlz_archive_batch_ws(const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, uint64_t nblocks,
                          uint8_t* d_archive, uint64_t archive_cap, uint64_t* d_off, void* d_work, size_t work_bytes, void* stream) {
    return archive_impl(d_rows, row_pitch, d_len, nblocks, d_archive, archive_cap, d_off, caller_work(d_work, work_bytes), stream);
}

int hdlz_archive_batch(const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, uint64_t nblocks,
                       uint8_t* d_archive, uint64_t archive_cap, uint64_t* d_off, void* stream) {
    if (const int rc = nblocks ? refuse_capture(stream, "hdlz_archive_batch_ws") : HDLZ_OK; rc != HDLZ_OK) return rc;
    return archive_impl(d_rows, row_pitch, d_len, nblocks, d_archive, archive_cap, d_off, pooled_work(), stream);
}

size_t hdlz_stream_work_bytes(size_t in_len) { return hdlz_streams_work_bytes(in_len, 1); }

size_t hdlz_streams_work_bytes(size_t in_len, uint64_t nblocks) {
    if (in_len >= 0x80000000ull || nblocks == 0 || nblocks > 0xFFFFFFFFull) return 0;
    if (((in_len + 2047) / 2048) * nblocks >= 0x80000000ull) return 0;          // tile indices are 32-bit
    return hdlz::stream_work_bytes((uint32_t)in_len, (uint32_t)nblocks);
}

int hdlz_compress_stream(const uint8_t* d_in, uint32_t in_len, int cwindow, int maxmatch, uint8_t* d_out,
                         uint64_t out_cap, uint32_t* d_out_len, uint32_t* d_status, void* d_work,
                         size_t work_bytes, void* stream) {
    return hdlz_compress_streams(d_in, 0, in_len, 1, cwindow, maxmatch, d_out, out_cap, d_out_len, d_status, d_work,
                                 work_bytes, stream);
}

int hdlz_compress_streams(const uint8_t* d_in, uint64_t in_pitch, uint32_t in_len, uint64_t nblocks, int cwindow,
                          int maxmatch, uint8_t* d_out, uint64_t out_pitch, uint32_t* d_out_len, uint32_t* d_status,
                          void* d_work, size_t work_bytes, void* stream) {
    if (!window_ok(cwindow, maxmatch)) return HDLZ_E_BAD_PARAM;
    if (nblocks == 0) return HDLZ_OK;
    if (any_null(d_in, d_out, d_out_len, d_status, d_work)) return fail_param("null device pointer");
    if (in_len >= 0x80000000u) return fail_param("in_len too large");
    if (misaligned(4, d_out)) return fail_align(4, "d_out");
    if (nblocks > 1 && (out_pitch & 3u)) return fail_param("out_pitch must be a multiple of 4");
    if (misaligned(8, d_work)) return fail_align(8, "d_work");
    const size_t need_work = hdlz_streams_work_bytes(in_len, nblocks);
    if (need_work == 0) return fail_param("in_len x nblocks too large for one call");
    if (work_too_small(need_work, d_work, work_bytes, "hdlz_streams_work_bytes(in_len, nblocks)")) return HDLZ_E_BAD_PARAM;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t need = ((uint64_t)hdlz::out_bound(in_len) + 3u) & ~3ull;
    if (in_len < 5u || out_pitch < need) {            // R0 / capacity: same per-stream status as the batch call
        if (nblocks > 1) return fail_param(in_len < 5u ? "in_len < 5" : "out_pitch smaller than hdlz_out_bound(in_len)");
        // (a kernel, not hipMemsetD32Async: 32-bit memsets did not survive HIP-graph capture on this stack)
        hipLaunchKernelGGL(k_set_result, dim3(1), dim3(1), 0, st, d_out_len, d_status,
                           in_len < 5u ? (uint32_t)HDLZ_E_SHORT_INPUT : (uint32_t)HDLZ_E_OUT_CAPACITY);
        return launched(hipGetLastError(), "launch k_set_result");
    }
    return launched(hdlz::launch_compress_streams(d_in, in_pitch, in_len, (uint32_t)nblocks, cwindow, maxmatch, d_out, out_pitch, d_out_len, d_status,
                                                  d_work, st), "launch k_stream_*");
}

int hdlz_compress_chunk(const uint8_t* d_in, uint32_t in_len, uint32_t q_end, int final, int cwindow, int maxmatch,
                        uint8_t* d_out, uint64_t out_cap, void* d_state, void* stream) {
    if (!window_ok(cwindow, maxmatch)) return HDLZ_E_BAD_PARAM;
    if (any_null(d_in, d_out, d_state)) return fail_param("null device pointer");
    if (in_len >= 0x80000000u) return fail_param("in_len too large");
    if (misaligned(4, d_out, d_state)) return fail_align(4, "d_out / d_state");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    return launched(hdlz::launch_compress_chunk(d_in, in_len, q_end, final, cwindow, maxmatch, d_out, out_cap, d_state, static_cast<hipStream_t>(stream)),
                    "launch k_compress_chunk");
}

int hdlz_inflate_chunk(const uint8_t* d_in, uint32_t in_len, int final, uint32_t flags, uint32_t obsize, uint8_t* d_out,
                       uint64_t out_cap, uint32_t out_limit, void* d_state, void* stream) {
    if (flags & ~(HDLZ_INFLATE_ASSUME_FIXED | HDLZ_INFLATE_ONEBLOCK)) return fail_param("unknown flag");
    if (any_null(d_in, d_out, d_state)) return fail_param("null device pointer");
    if (in_len >= 0x10000000u) return fail_param("in_len too large (streams are limited to 256 MiB - 1)");
    if (misaligned(4, d_out, d_state)) return fail_align(4, "d_out / d_state");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    return launched(hdlz::launch_inflate_chunk(d_in, in_len, final, flags, obsize, d_out, out_cap, out_limit, d_state, static_cast<hipStream_t>(stream)),
                    "launch k_inflate_dyn<stream>");
}

// ---- include/hdlz_unjoin.h: a joined stream read back member by member (the member view of the batch decoders; hdlz_unjoin.hip)
// (and include/hdlz_gzip.h: the gzip form differs in the checksum's share of the scratch and in what runs behind the decode)
// The scratch of hdlz_unjoin_ws / hdlz_unjoin_gzip_ws, laid out ONCE for the size query and the call: three words per member (length,
// status, end bit), the checksum's words per 32 KiB tile of the output (gzip: one CRC word; zlib: an (A, C) pair), the decoder's share,
// which takes what is left from `decode` on.
static Laid unjoin_layout(hdlz::UnjoinArgs& u, uintptr_t base, uint32_t flags, bool gzip) {
    Carver c{base};
    u.len = c.take<uint32_t>(u.nmembers); u.status = c.take<uint32_t>(u.nmembers); u.end_bit = c.take<uint32_t>(u.nmembers); c.align256();
    u.tiles = gzip ? reinterpret_cast<uint2*>(c.take<uint32_t>(hdlz::crc32_tiles(u.out_cap))) : c.take<uint2>(hdlz::unjoin_tiles(u.out_cap)); c.align256();
    const size_t decode = c.bytes();
    c.take<uint8_t>(hdlz::round256(hdlz_inflate_work_bytes(u.nmembers, 0, 0, flags, 1)));
    return {c.bytes(), decode};
}
static size_t unjoin_work_bytes(uint64_t nmembers, uint64_t total_out, uint32_t flags, bool gzip) {
    hdlz::UnjoinArgs u{nullptr, 0, nullptr, nullptr, 0, nmembers, nullptr, total_out};
    return nmembers > 0x7FFFFFFFull ? 0u : unjoin_layout(u, 0, flags, gzip).bytes;
}
size_t hdlz_unjoin_work_bytes(uint64_t nmembers, uint64_t total_out, uint32_t flags) { return unjoin_work_bytes(nmembers, total_out, flags, false); }
size_t hdlz_unjoin_gzip_work_bytes(uint64_t nmembers, uint64_t total_out, uint32_t flags) { return unjoin_work_bytes(nmembers, total_out, flags, true); }

static int unjoin_impl(const uint8_t* d_stream, uint64_t stream_len, const uint64_t* d_off, const uint64_t* d_out_off, uint32_t out_len,
                       uint64_t nmembers, uint32_t flags, uint8_t* d_out, uint64_t out_cap, uint32_t* d_member_status,
                       hdlz_unjoin_result* d_result, void* d_work, size_t work_bytes, void* stream, bool gzip) {
    if (any_null(d_stream, d_off, d_result) || (out_cap && !d_out)) return fail_param("null device pointer");
    if (nmembers > 0x7FFFFFFFull) return fail_param("nmembers too large for one call (2^31 - 1 members)");
    if (flags & ~MAPPING_HINTS) return fail_param("unknown flag (hdlz_unjoin_ws and hdlz_unjoin_gzip_ws take the three mapping hints only)");
    if (flags & (flags - 1u)) return fail_param("contradictory mapping flags");
    if (misaligned(4, d_out)) return fail_align(4, "d_out");
    if (misaligned(8, d_off, d_out_off, d_result)) return fail_align(8, "d_off / d_out_off / d_result");
    if (misaligned(256, d_work)) return fail_align(256, "d_work");
    hdlz::UnjoinArgs u{d_stream, stream_len, d_off, d_out_off, out_len, nmembers, d_out, out_cap, d_member_status, d_result};
    const Laid l = unjoin_layout(u, address(d_work), flags, gzip);
    if (work_too_small(l.bytes, d_work, work_bytes,
                       gzip ? "hdlz_unjoin_gzip_work_bytes(nmembers, out_cap, flags)" : "hdlz_unjoin_work_bytes(nmembers, out_cap, flags)")) return HDLZ_E_BAD_PARAM;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = launched(hdlz::launch_unjoin_index(u, st), "launch k_unjoin_index"); rc != HDLZ_OK) return rc;
    if (nmembers) {
        const MemberView v{d_off, nullptr, d_out_off, out_cap, out_len, 0, nullptr, nullptr, HDLZ_INFLATE_ONEBLOCK};   // (BFINAL is not read: a member is one block)
        const hdlz::MemberArgs a = member_args(d_stream, nmembers, d_out, u.len, u.status, u.end_bit, v);
        // the mapping: the thresholds of hdlz_inflate_batch_ws, or the hint; never the whole-GPU chains
        const Mapping map = mapping_of(nmembers, flags);
        const hdlz::Work w = caller_work(static_cast<uint8_t*>(d_work) + l.decode, work_bytes - l.decode);
        if (const int rc = launched(map == Mapping::wave ? hdlz::launch_inflate_dyn_members(a, st) : map == Mapping::group ? hdlz::launch_inflate_grp_members(a, st)
                                                                                                            : hdlz::launch_inflate_tok_members(a, st, w),
                      "launch the member decode"); rc != HDLZ_OK) return rc;
    }
    return launched(gzip ? hdlz::launch_unjoin_gzip_judge(u, st) : hdlz::launch_unjoin_judge(u, st), "launch k_unjoin_judge");
}

int hdlz_unjoin_ws(const uint8_t* d_stream, uint64_t stream_len, const uint64_t* d_off, const uint64_t* d_out_off, uint32_t out_len,
                   uint64_t nmembers, uint32_t flags, uint8_t* d_out, uint64_t out_cap, uint32_t* d_member_status,
                   hdlz_unjoin_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    return unjoin_impl(d_stream, stream_len, d_off, d_out_off, out_len, nmembers, flags, d_out, out_cap, d_member_status, d_result, d_work,
                       work_bytes, stream, false);
}

// ---- include/hdlz_gzip.h: CRC-32 on the device, the joined stream as one gzip member, and that member read back
int hdlz_unjoin_gzip_ws(const uint8_t* d_stream, uint64_t stream_len, const uint64_t* d_off, const uint64_t* d_out_off, uint32_t out_len,
                        uint64_t nmembers, uint32_t flags, uint8_t* d_out, uint64_t out_cap, uint32_t* d_member_status,
                        hdlz_unjoin_gzip_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    return unjoin_impl(d_stream, stream_len, d_off, d_out_off, out_len, nmembers, flags, d_out, out_cap, d_member_status,
                       reinterpret_cast<hdlz_unjoin_result*>(d_result), d_work, work_bytes, stream, true);      // (one record layout: hdlz_unjoin.hip)
}

size_t hdlz_crc32_work_bytes(uint64_t n) { return hdlz::round256(sizeof(uint32_t) * hdlz::crc32_tiles(n)); }

int hdlz_crc32_ws(const uint8_t* d_data, uint64_t n, uint32_t* d_crc, void* d_work, size_t work_bytes, void* stream) {
    if (!d_crc || (n && !d_data)) return fail_param("null device pointer");
    const size_t need = hdlz_crc32_work_bytes(n);
    if (work_too_small(need, d_work, work_bytes, "hdlz_crc32_work_bytes(n)")) return HDLZ_E_BAD_PARAM;
    if (misaligned(4, d_crc, d_work)) return fail_align(4, "d_crc / d_work");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    return launched(hdlz::launch_crc32(d_data, n, d_crc, static_cast<uint32_t*>(d_work), static_cast<hipStream_t>(stream)), "launch k_crc32_tiles");
}

size_t hdlz_join_gzip_bound(uint64_t nblocks, uint32_t in_len) { return hdlz_join_bound(nblocks, in_len) + 12u; }

size_t hdlz_join_gzip_work_bytes(uint64_t nblocks) { return hdlz_join_work_bytes(nblocks); }

int hdlz_join_gzip_ws(const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_end_bits,
                      const uint32_t* d_status, const uint64_t* d_in_off, uint32_t in_len, uint64_t nblocks, const uint32_t* d_crc,
                      uint8_t* d_stream, uint64_t stream_cap, uint64_t* d_off, hdlz_join_gzip_result* d_result, void* d_work,
                      size_t work_bytes, void* stream) {
    if (!d_crc) return fail_param("d_crc is required");
    const bool null_pointer = any_null(d_stream, d_off, d_result) || (nblocks && any_null(d_rows, d_len, d_end_bits, d_status));
    if (const int rc = join_checks(null_pointer, nblocks, d_off, nullptr, d_result, d_crc, d_work, work_bytes, "hdlz_join_gzip_work_bytes(nblocks)", false); rc != HDLZ_OK) return rc;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    const hdlz::JoinArgs a{d_rows, row_pitch, d_len, d_end_bits, d_status, d_in_off, in_len, nblocks, d_stream, stream_cap, d_off, nullptr, {}};
    return launched(hdlz::launch_join_gzip(a, d_crc, d_result, d_work, static_cast<hipStream_t>(stream)), "launch k_join");
}

// ---- include/hdlz_bgzf.h: the CRC-32 of every block of a batch, the BGZF writer, the member index and the reader
int hdlz_crc32_batch_ws(const uint8_t* d_data, const uint64_t* d_off, uint64_t pitch, uint32_t len, uint64_t nblocks, uint32_t* d_crc,
                        void* stream) {
    if (nblocks > 0x7FFFFFFFull) return fail_param("nblocks too large for one call (2^31 - 1 blocks)");
    if (nblocks && (!d_crc || (!d_data && (d_off || len)))) return fail_param("null device pointer");
    if (misaligned(4, d_crc)) return fail_align(4, "d_crc");
    if (misaligned(8, d_off)) return fail_align(8, "d_off");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    return launched(hdlz::launch_crc32_batch(d_data, d_off, pitch, len, nblocks, d_crc, nullptr, static_cast<hipStream_t>(stream)), "launch k_crc32_batch");
}

size_t hdlz_bgzf_bound(uint64_t nblocks, uint32_t in_len) { return 28u + (size_t)nblocks * (hdlz_out_bound(in_len) + 20u); }

size_t hdlz_bgzf_join_work_bytes(uint64_t nblocks) { return hdlz_join_work_bytes(nblocks); }

int hdlz_bgzf_join_ws(const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint32_t* d_status, const uint64_t* d_in_off,
                      uint32_t in_len, uint64_t nblocks, const uint32_t* d_crc, uint8_t* d_file, uint64_t file_cap, uint64_t* d_off,
                      hdlz_bgzf_join_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    const bool null_pointer = any_null(d_file, d_off, d_result) || (nblocks && any_null(d_rows, d_len, d_status, d_crc));
    if (const int rc = join_checks(null_pointer, nblocks, d_off, d_in_off, d_result, d_crc, d_work, work_bytes, "hdlz_bgzf_join_work_bytes(nblocks)", true); rc != HDLZ_OK) return rc;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    const hdlz::BgzfJoinArgs a{nullptr, d_in_off, 0u, in_len, d_rows, row_pitch, d_len, d_status, nblocks, d_crc, d_file, file_cap, d_off, nullptr, {}};
    return launched(hdlz::launch_bgzf_join(a, d_result, d_work, static_cast<hipStream_t>(stream)), "launch k_bgzf_join<fixed>");
}

// ---- include/hdlz_bgzf_stored.h: the BGZF writer that falls back to a stored member
size_t hdlz_bgzf_stored_bound(uint64_t nblocks, uint32_t in_len) {
    const size_t fixed = hdlz_out_bound(in_len) + 20u, stored = (size_t)in_len + 31u;
    return 28u + (size_t)nblocks * (fixed < stored ? fixed : stored);
}

size_t hdlz_bgzf_join_stored_work_bytes(uint64_t nblocks) { return hdlz_join_work_bytes(nblocks); }

int hdlz_bgzf_join_stored_ws(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len, const uint8_t* d_rows,
                             uint64_t row_pitch, const uint32_t* d_len, const uint32_t* d_status, uint64_t nblocks, const uint32_t* d_crc,
                             uint8_t* d_file, uint64_t file_cap, uint64_t* d_off, uint8_t* d_kind, hdlz_bgzf_stored_result* d_result,
                             void* d_work, size_t work_bytes, void* stream) {
    const bool null_pointer = any_null(d_file, d_off, d_result) || (nblocks && any_null(d_in, d_rows, d_len, d_status, d_crc));
    if (const int rc = join_checks(null_pointer, nblocks, d_off, d_in_off, d_result, d_crc, d_work, work_bytes, "hdlz_bgzf_join_stored_work_bytes(nblocks)", true); rc != HDLZ_OK) return rc;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    const hdlz::BgzfJoinArgs a{d_in, d_in_off, in_pitch, in_len, d_rows, row_pitch, d_len, d_status, nblocks, d_crc, d_file, file_cap, d_off, d_kind, {}};
    return launched(hdlz::launch_bgzf_join_stored(a, d_result, d_work, static_cast<hipStream_t>(stream)), "launch k_bgzf_join<stored>");
}

size_t hdlz_bgzf_index_work_bytes(uint64_t file_len) { return hdlz::bgzf_index_work_bytes(file_len); }

int hdlz_bgzf_index_ws(const uint8_t* d_file, uint64_t file_len, uint64_t member_cap, uint64_t* d_off, uint64_t* d_out_off,
                       hdlz_bgzf_index_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    return member_index_impl(d_file, file_len, member_cap, d_off, d_out_off, d_result, d_work, work_bytes, stream, hdlz::bgzf_index_work_bytes(file_len),
                             "hdlz_bgzf_index_work_bytes(file_len)", hdlz::launch_bgzf_index, "launch k_bgzf_scan");
}

// The scratch of hdlz_bgzf_inflate_ws, laid out once for the size query and the call: three words per member (length, status, end bit),
// the two shifted offset arrays of nmembers + 1 words (BgzfArgs::m_off, m_out_off), one CRC word per member.  No members: no scratch.
static size_t bgzf_inflate_layout(hdlz::BgzfArgs& u, uintptr_t base) {
    Carver c{base};
    u.len = c.take<uint32_t>(u.nmembers); u.status = c.take<uint32_t>(u.nmembers); u.end_bit = c.take<uint32_t>(u.nmembers); c.align256();
    u.m_off = c.take<uint64_t>(u.nmembers + 1u); u.m_out_off = c.take<uint64_t>(u.nmembers + 1u); c.align256();
    u.crc = c.take<uint32_t>(u.nmembers); c.align256();
    return u.nmembers ? c.bytes() : 0u;
}
size_t hdlz_bgzf_inflate_work_bytes(uint64_t nmembers, uint32_t flags) {
    hdlz::BgzfArgs u{nullptr, 0, nullptr, nullptr, nmembers};
    return nmembers > 0x7FFFFFFFull || flags != 0u ? 0u : bgzf_inflate_layout(u, 0);
}

int hdlz_bgzf_inflate_ws(const uint8_t* d_file, uint64_t file_len, const uint64_t* d_off, const uint64_t* d_out_off, uint64_t nmembers,
                         uint32_t flags, uint8_t* d_out, uint64_t out_cap, uint32_t* d_member_status, hdlz_bgzf_inflate_result* d_result,
                         void* d_work, size_t work_bytes, void* stream) {
    if (!d_result || (nmembers && any_null(d_file, d_off, d_out_off)) || (out_cap && !d_out)) return fail_param("null device pointer");
    if (nmembers > 0x7FFFFFFFull) return fail_param("nmembers too large for one call (2^31 - 1 members)");
    if (flags != 0u) return fail_param("flags must be 0 (hdlz_bgzf_inflate_ws decodes a wave per member: the mapping hints do not apply)");
    if (misaligned(8, d_off, d_out_off, d_result)) return fail_align(8, "d_off / d_out_off / d_result");
    if (misaligned(256, d_work)) return fail_align(256, "d_work");
    hdlz::BgzfArgs u{d_file, file_len, d_off, d_out_off, nmembers, d_out, out_cap, d_member_status, d_result};
    if (work_too_small(bgzf_inflate_layout(u, address(d_work)), d_work, work_bytes, "hdlz_bgzf_inflate_work_bytes(nmembers, flags)")) return HDLZ_E_BAD_PARAM;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = launched(hdlz::launch_bgzf_check(u, st), "launch k_bgzf_check"); rc != HDLZ_OK) return rc;
    if (nmembers) {
        const MemberView v{u.m_off, nullptr, u.m_out_off, out_cap, 0, 18u};                      // (m_gap: the next member's header)
        if (const int rc = decode_members(d_file, nmembers, d_out, u.len, u.status, u.end_bit, v, st, u.crc); rc != HDLZ_OK) return rc;
    }
    return launched(hdlz::launch_bgzf_judge(u, st), "launch k_bgzf_judge");
}

// ---- include/hdlz_bgzf_range.h: a batch of ranges of a BGZF file's data, by byte or virtual offset
size_t hdlz_bgzf_ranges_work_bytes(uint64_t nranges, uint64_t task_cap, uint32_t flags) {
    if (nranges > 0x7FFFFFFFull || task_cap > 0x7FFFFFFFull || (flags & ~HDLZ_BGZF_RANGE_VIRTUAL)) return 0;
    return hdlz::bgzf_ranges_work_bytes(nranges, task_cap);
}

int hdlz_bgzf_read_ranges_ws(const uint8_t* d_file, uint64_t file_len, const uint64_t* d_off, const uint64_t* d_out_off, uint64_t nmembers,
                             const uint64_t* d_ranges, uint64_t nranges, uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                             uint64_t* d_range_off, uint32_t* d_range_status, uint64_t task_cap, hdlz_bgzf_ranges_result* d_result,
                             void* d_work, size_t work_bytes, void* stream) {
    if (any_null(d_result, d_range_off) || (nranges && any_null(d_ranges, d_file, d_off, d_out_off)) || (out_cap && !d_out)) return fail_param("null device pointer");
    if (nranges > 0x7FFFFFFFull || nmembers > 0x7FFFFFFFull || task_cap > 0x7FFFFFFFull)
        return fail_param("nranges, nmembers and task_cap must be below 2^31");
    if (flags & ~HDLZ_BGZF_RANGE_VIRTUAL) return fail_param("flags: only HDLZ_BGZF_RANGE_VIRTUAL is defined");
    if (misaligned(8, d_off, d_out_off, d_ranges, d_range_off, d_result)) return fail_align(8, "d_off / d_out_off / d_ranges / d_range_off / d_result");
    if (misaligned(4, d_range_status)) return fail_align(4, "d_range_status");
    if (misaligned(256, d_work)) return fail_align(256, "d_work");
    if (work_too_small(hdlz::bgzf_ranges_work_bytes(nranges, task_cap), d_work, work_bytes, "hdlz_bgzf_ranges_work_bytes(nranges, task_cap, flags)")) return HDLZ_E_BAD_PARAM;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hdlz::RangeArgs u = hdlz::bgzf_ranges_args(d_work, nranges, task_cap);
    u.in = d_file; u.in_len = file_len; u.off = d_off; u.out_off = d_out_off; u.nmembers = nmembers;
    u.ranges = d_ranges; u.nranges = nranges; u.flags = flags; u.out = d_out; u.out_cap = out_cap;
    u.range_off = d_range_off; u.range_status = d_range_status; u.task_cap = task_cap; u.result = d_result;
    if (const int rc = launched(hdlz::launch_bgzf_ranges_plan(u, st), "launch the plan kernels (k_ranges_resolve, k_ranges_scan, k_ranges_expand)"); rc != HDLZ_OK) return rc;
    if (nranges && task_cap) {
        const MemberView v{u.t_off, u.t_end, nullptr, 0, 0, 0, u.t_dst, u.t_cap};                 // the task view (slots behind ntasks are marked as refused)
        if (const int rc = decode_members(d_file, task_cap, d_out, u.t_len, u.t_status, u.t_end_bit, v, st); rc != HDLZ_OK) return rc;
    }
    return launched(hdlz::launch_bgzf_ranges_finish(u, st),
                    "launch the finish kernels (k_ranges_crc, k_ranges_judge, k_ranges_slice, k_ranges_finish, k_ranges_record)");
}

// ---- include/hdlz_seek.h: the seek index of a gzip or zlib stream and batched ranges through it (hdlz_seek.hip)
// The scratch of hdlz_seek_index_ws, laid out once for the size query and the call: a head (the count of written points; behind it the
// decoder's two sink words), the one stream's words (length, status, end, and the header walk's three), the walk's two-word index, the
// recorded points, the checksum's tile words.
struct SeekIndexWork {
    uint64_t *head, *sink_head, *idx, *pt_bit, *pt_pos;
    uint32_t* words;             // out_len, status, in_used, p, verdict, crcw
    uint8_t* tiles;
    size_t decode;               // from here on: what the decode path takes
};
static uint64_t seek_row(uint64_t out_cap) { return (out_cap & ~3ull) < 0xFFFFFE00ull ? out_cap & ~3ull : 0xFFFFFE00ull; }
static size_t seek_index_layout(SeekIndexWork& w, uintptr_t base, uint64_t file_len, bool gzip, uint64_t row, uint64_t point_cap) {
    Carver c{base};
    w.head = c.take<uint64_t>(16); w.sink_head = c.take<uint64_t>(16); c.align256();
    w.words = c.take<uint32_t>(64); c.align256();
    w.idx = c.take<uint64_t>(32); c.align256();
    w.pt_bit = c.take<uint64_t>(point_cap); c.align256();
    w.pt_pos = c.take<uint64_t>(point_cap); c.align256();
    w.tiles = c.take<uint8_t>(8u * (size_t)((row + 32767u) / 32768u)); c.align256();
    w.decode = c.bytes();
    c.take<uint8_t>(hdlz::round256(hdlz_inflate_work_bytes(1, (uint32_t)file_len, row, 0, gzip ? 1 : 0)));      // the share of the batch call's path
    return c.bytes();
}
static bool seek_index_shape_ok(uint64_t file_len, uint32_t flags, uint32_t span, uint64_t point_cap) {
    return (flags == HDLZ_SEEK_ZLIB || flags == HDLZ_SEEK_GZIP) && span != 0u && file_len < 0x10000000ull && point_cap <= 0x7FFFFFFFull;
}
static bool seek_ranges_shape_ok(uint64_t nranges, uint64_t task_cap, uint64_t seg_cap, uint32_t flags) {
    return nranges <= 0x7FFFFFFFull && task_cap <= 0x7FFFFFFFull && seg_cap <= 0xFFFFFE00ull && flags == 0u;
}
static size_t seek_ranges_bytes(uint64_t nranges, uint64_t task_cap, uint64_t seg_cap) {
    if (nranges == 0) return 0;
    return hdlz::bgzf_ranges_work_bytes(nranges, task_cap, hdlz::round256(seg_cap)) + 3u * hdlz::round256(4u * (size_t)task_cap);
}

size_t hdlz_seek_index_work_bytes(uint64_t file_len, uint32_t flags, uint64_t out_cap, uint64_t point_cap) {
    if (!seek_index_shape_ok(file_len, flags, 1u, point_cap)) return 0;
    SeekIndexWork w;
    return seek_index_layout(w, 0, file_len, flags == HDLZ_SEEK_GZIP, seek_row(out_cap), point_cap);
}

int hdlz_seek_index_ws(const uint8_t* d_file, uint64_t file_len, uint32_t flags, uint32_t span, uint8_t* d_out, uint64_t out_cap,
                       uint64_t* d_bit, uint64_t* d_pos, uint32_t* d_crc, uint8_t* d_win, uint64_t point_cap, hdlz_seek_result* d_result,
                       void* d_work, size_t work_bytes, void* stream) {
    if (!d_result) return fail_param("null device pointer");
    if (flags != HDLZ_SEEK_ZLIB && flags != HDLZ_SEEK_GZIP) return fail_param("flags: exactly one of HDLZ_SEEK_ZLIB and HDLZ_SEEK_GZIP");
    if (span == 0u) return fail_param("span must be at least 1");
    if (file_len >= 0x10000000ull) return fail_param("file_len too large (streams are limited to 256 MiB - 1)");
    if (point_cap > 0x7FFFFFFFull) return fail_param("point_cap must be below 2^31");
    if ((file_len && !d_file) || (out_cap && !d_out) || (point_cap && any_null(d_bit, d_pos, d_crc, d_win))) return fail_param("null device pointer");
    if (misaligned(8, d_bit, d_pos, d_result)) return fail_align(8, "d_bit / d_pos / d_result");
    if (misaligned(4, d_crc, d_out)) return fail_align(4, "d_crc / d_out");
    if (misaligned(16, d_win)) return fail_align(16, "d_win");
    if (misaligned(256, d_work)) return fail_align(256, "d_work");
    const uint64_t row = seek_row(out_cap);
    SeekIndexWork w;
    const bool gzip = flags == HDLZ_SEEK_GZIP;
    if (work_too_small(seek_index_layout(w, address(d_work), file_len, gzip, row, point_cap), d_work, work_bytes, "hdlz_seek_index_work_bytes(file_len, flags, out_cap, point_cap)")) return HDLZ_E_BAD_PARAM;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t *out_len = w.words, *status = w.words + 1, *in_used = w.words + 2;
    const hdlz::PointSink sink{w.sink_head, w.pt_bit, w.pt_pos, (uint32_t)point_cap, span};
    if (const int rc = launched(hdlz::zero_words(reinterpret_cast<uint32_t*>(w.sink_head), 8u, st), "launch k_zero_words"); rc != HDLZ_OK) return rc;
    hdlz::GunzipArgs g{d_file, nullptr, 0, (uint32_t)file_len, 1, d_out, row, out_len, status, in_used, nullptr};
    if (gzip) {
        g.p = w.words + 3; g.verdict = w.words + 4; g.crcw = w.words + 5; g.idx = w.idx;
        g.tiles = hdlz::gunzip_tile_words(1, row) ? reinterpret_cast<uint32_t*>(w.tiles) : nullptr;
        g.single = true;
        if (const int rc = launched(hdlz::launch_gunzip_heads(g, st), "launch k_gunzip_heads"); rc != HDLZ_OK) return rc;
    }
    // the decode of the one stream -- the file (zlib), or the walk's ragged index (gzip) -- on the path of the one-stream calls: the
    // whole-GPU chains where they apply, which fill the sink themselves or hand on to the recording view of the wave decoder; else that view
    const hdlz::InflateArgs a{d_file, gzip ? w.idx : nullptr, 0, (uint32_t)file_len, 1, 0, 0, d_out, row, out_len, status, in_used, sink};
    bool used = false;
    if (par_applies(1, (uint32_t)file_len, 0)) {
        const hdlz::Work share = caller_work(static_cast<uint8_t*>(d_work) + w.decode, work_bytes - w.decode);
        if (const int rc = launched(hdlz::launch_inflate_par(a, st, &used, share), "launch the whole-GPU inflate (k_par_*)"); rc != HDLZ_OK) return rc;
    }
    if (!used)
        if (const int rc = launched(hdlz::launch_inflate_dyn_record(a, st), "launch k_inflate_dyn (the recording view)"); rc != HDLZ_OK) return rc;
    if (gzip) {
        if (const int rc = launched(hdlz::launch_gunzip_crc(g, st), "launch k_gunzip_crc_*"); rc != HDLZ_OK) return rc;
        if (const int rc = launched(hdlz::launch_gunzip_judge(g, st), "launch k_gunzip_judge"); rc != HDLZ_OK) return rc;
    } else {
        const hdlz::JudgeArgs j{d_file, nullptr, 0, (uint32_t)file_len, 1, d_out, row, out_len, status, in_used, nullptr,
                                hdlz::judge_work_bytes(1, row) ? reinterpret_cast<uint2*>(w.tiles) : nullptr};
        if (const int rc = launched(hdlz::launch_judge(j, st), "launch the judging pass (k_adler_*)"); rc != HDLZ_OK) return rc;
    }
    const hdlz::SeekIndexArgs s{d_out, out_len, status, sink, d_bit, d_pos, d_crc, d_win, point_cap, d_result, w.head};
    return launched(hdlz::launch_seek_index_finish(s, st), "launch the index kernels (k_seek_points, k_seek_windows, k_seek_crc)");
}

size_t hdlz_seek_ranges_work_bytes(uint64_t nranges, uint64_t task_cap, uint64_t seg_cap, uint32_t flags) {
    return seek_ranges_shape_ok(nranges, task_cap, seg_cap, flags) ? seek_ranges_bytes(nranges, task_cap, seg_cap) : 0;
}

int hdlz_seek_read_ranges_ws(const uint8_t* d_file, uint64_t file_len, const uint64_t* d_bit, const uint64_t* d_pos, const uint32_t* d_crc,
                             const uint8_t* d_win, uint64_t npoints, const uint64_t* d_ranges, uint64_t nranges, uint32_t flags, uint64_t seg_cap,
                             uint8_t* d_out, uint64_t out_cap, uint64_t* d_range_off, uint32_t* d_range_status, uint64_t task_cap,
                             hdlz_seek_ranges_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    if (any_null(d_result, d_range_off) || (nranges && any_null(d_ranges, d_file, d_bit, d_pos, d_crc, d_win)) || (out_cap && !d_out)) return fail_param("null device pointer");
    if (nranges > 0x7FFFFFFFull || npoints > 0x7FFFFFFFull || task_cap > 0x7FFFFFFFull) return fail_param("nranges, npoints and task_cap must be below 2^31");
    if (nranges && npoints == 0) return fail_param("npoints: an index has at least one point");
    if (file_len >= 0x10000000ull) return fail_param("file_len too large (streams are limited to 256 MiB - 1)");
    if (seg_cap > 0xFFFFFE00ull) return fail_param("seg_cap too large (at most 2^32 - 512)");
    if (flags) return fail_param("flags: none is defined");
    if (misaligned(8, d_bit, d_pos, d_ranges, d_range_off, d_result)) return fail_align(8, "d_bit / d_pos / d_ranges / d_range_off / d_result");
    if (misaligned(4, d_crc, d_range_status)) return fail_align(4, "d_crc / d_range_status");
    if (misaligned(256, d_work)) return fail_align(256, "d_work");
    if (work_too_small(seek_ranges_bytes(nranges, task_cap, seg_cap), d_work, work_bytes, "hdlz_seek_ranges_work_bytes(nranges, task_cap, seg_cap, flags)")) return HDLZ_E_BAD_PARAM;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t slot = hdlz::round256(seg_cap);
    hdlz::SeekRangeArgs s{};
    hdlz::RangeArgs& u = s.r;
    u = hdlz::bgzf_ranges_args(d_work, nranges, task_cap, slot);
    u.in = d_file; u.in_len = file_len; u.off = nullptr; u.out_off = d_pos; u.nmembers = npoints;
    u.ranges = d_ranges; u.nranges = nranges; u.flags = 0; u.out = d_out; u.out_cap = out_cap;
    u.range_off = d_range_off; u.range_status = d_range_status; u.task_cap = task_cap; u.result = d_result;
    s.bit = d_bit; s.crc = d_crc; s.win = d_win; s.seg_cap = seg_cap;
    {
        Carver c{address(u.slots) + (size_t)(2u * slot) * (size_t)nranges};      // behind the slots: the three words per task of this call
        s.t_sbit = c.take<uint32_t>(task_cap); c.align256();
        s.t_hist = c.take<uint32_t>(task_cap); c.align256();
        s.t_k = c.take<uint32_t>(task_cap);
    }
    if (const int rc = launched(hdlz::launch_ranges_resolve_scan(u, st), "launch the plan kernels (k_ranges_resolve, k_ranges_scan)"); rc != HDLZ_OK) return rc;
    if (nranges && task_cap) {
        if (const int rc = launched(hdlz::launch_seek_expand(s, st), "launch k_seek_expand"); rc != HDLZ_OK) return rc;
        hdlz::SegArgs a{};
        a.in = d_file; a.nstreams = task_cap; a.out = d_out; a.out_len = u.t_len; a.status = u.t_status; a.in_used = u.t_end_bit;
        a.t_off = u.t_off; a.t_end = u.t_end; a.t_dst = u.t_dst; a.t_cap = u.t_cap; a.t_sbit = s.t_sbit; a.t_hist = s.t_hist; a.t_k = s.t_k; a.win = d_win; a.bit = d_bit;
        if (const int rc = launched(hdlz::launch_inflate_dyn_segments(a, st), "launch k_inflate_dyn (the segment view)"); rc != HDLZ_OK) return rc;
        if (const int rc = launched(hdlz::launch_ranges_crc(u, st), "launch k_ranges_crc"); rc != HDLZ_OK) return rc;
        if (const int rc = launched(hdlz::launch_seek_judge(s, st), "launch k_seek_judge"); rc != HDLZ_OK) return rc;
    }
    return launched(hdlz::launch_ranges_deliver(u, st), "launch the finish kernels (k_ranges_slice, k_ranges_finish, k_ranges_record)");
}

// ---- include/hdlz_gunzip.h: gzip members of any writer, one per stream (hdlz_gunzip.hip)
// The scratch of hdlz_gunzip_ws, laid out once for the size query and the call: three words per stream (p, the header's verdict, the
// CRC-32), the decoder's view of 2 nstreams offsets, one CRC word per 32 KiB tile of row capacity where the rows are tiled, and -- one
// stream -- the share of the batch call's path, which takes what is left from `decode` on.
static Laid gunzip_layout(hdlz::GunzipArgs& g, uintptr_t base) {
    Carver c{base};
    g.p = c.take<uint32_t>(g.nstreams); g.verdict = c.take<uint32_t>(g.nstreams); g.crcw = c.take<uint32_t>(g.nstreams); c.align256();
    g.idx = c.take<uint64_t>(2u * g.nstreams); c.align256();
    const size_t words = hdlz::gunzip_tile_words(g.nstreams, g.out_pitch);
    g.tiles = words ? c.take<uint32_t>(words) : nullptr; c.align256();
    const size_t decode = c.bytes();
    if (g.nstreams == 1) c.take<uint8_t>(hdlz::round256(hdlz_inflate_work_bytes(1, g.in_len, g.out_pitch, 0, 1)));
    return {c.bytes(), decode};
}
size_t hdlz_gunzip_work_bytes(uint64_t nstreams, uint32_t in_len, uint64_t out_pitch, int ragged) {
    if (nstreams == 0 || nstreams > 0x7FFFFFFFull || (!ragged && in_len >= 0x10000000u) || (nstreams > 1 && out_pitch > 0xFFFFFFFFull)) return 0;
    hdlz::GunzipArgs g{nullptr, nullptr, 0, in_len, nstreams, nullptr, out_pitch};
    return gunzip_layout(g, 0).bytes;
}

int hdlz_gunzip_ws(const uint8_t* d_in, const uint64_t* d_in_off, uint64_t in_pitch, uint32_t in_len, uint64_t nstreams, uint8_t* d_out,
                   uint64_t out_pitch, uint32_t* d_out_len, uint32_t* d_status, uint32_t* d_in_used, uint32_t* d_crc, void* d_work,
                   size_t work_bytes, void* stream) {
    if (!d_in_used) return fail_param("d_in_used is required");
    if (nstreams > 0x7FFFFFFFull) return fail_param("nstreams too large for one call (2^31 - 1 streams)");
    if (nstreams && any_null(d_in, d_out, d_out_len, d_status)) return fail_param("null device pointer");
    if (!d_in_off && in_len >= 0x10000000u) return fail_param("in_len too large (streams are limited to 256 MiB - 1)");
    if (!d_in_off && nstreams > 1 && in_pitch < in_len) return fail_param("in_pitch < in_len");
    if (nstreams > 1 && out_pitch > 0xFFFFFFFFull) return fail_param("out_pitch too large for more than one stream (below 2^32)");
    if ((out_pitch & 3u) || misaligned(4, d_out)) return fail_align(4, "d_out / out_pitch");
    if (misaligned(8, d_in_off)) return fail_align(8, "d_in_off");
    if (misaligned(4, d_out_len, d_status, d_in_used, d_crc)) return fail_align(4, "d_out_len / d_status / d_in_used / d_crc");
    if (misaligned(256, d_work)) return fail_align(256, "d_work");
    hdlz::GunzipArgs g{d_in, d_in_off, in_pitch, in_len, nstreams, d_out, out_pitch, d_out_len, d_status, d_in_used, d_crc};
    const Laid l = gunzip_layout(g, address(d_work));
    if (nstreams && work_too_small(l.bytes, d_work, work_bytes, "hdlz_gunzip_work_bytes(nstreams, in_len, out_pitch, ragged)")) return HDLZ_E_BAD_PARAM;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    if (nstreams == 0) return HDLZ_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool single = g.single = nstreams == 1;
    if (const int rc = launched(hdlz::launch_gunzip_heads(g, st), "launch k_gunzip_heads"); rc != HDLZ_OK) return rc;
    if (single) {                                                                                 // the .gz file
        if (const int rc = inflate_one(d_in, g.idx, in_len, d_out, out_pitch, d_out_len, d_status, d_in_used, d_work, work_bytes, l.decode, stream); rc != HDLZ_OK) return rc;
    } else {
        const MemberView v{g.idx, g.idx + nstreams, nullptr, nstreams * out_pitch, (uint32_t)out_pitch};   // (rows: member b decodes to d_out + b * out_pitch)
        if (const int rc = decode_members(d_in, nstreams, d_out, d_out_len, d_status, d_in_used, v, st); rc != HDLZ_OK) return rc;
    }
    if (const int rc = launched(hdlz::launch_gunzip_crc(g, st), "launch k_gunzip_crc_*"); rc != HDLZ_OK) return rc;
    return launched(hdlz::launch_gunzip_judge(g, st), "launch k_gunzip_judge");
}

// ---- include/hdlz_gzip_members.h: a gzip file of many members, indexed by a guess and read verified (hdlz_gzip_members.hip)
size_t hdlz_gzip_members_index_work_bytes(uint64_t file_len) { return hdlz::gzip_members_index_work_bytes(file_len); }

int hdlz_gzip_members_index_ws(const uint8_t* d_file, uint64_t file_len, uint64_t member_cap, uint64_t* d_off, uint64_t* d_out_off,
                               hdlz_gzip_members_index_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    return member_index_impl(d_file, file_len, member_cap, d_off, d_out_off, d_result, d_work, work_bytes, stream, hdlz::gzip_members_index_work_bytes(file_len),
                             "hdlz_gzip_members_index_work_bytes(file_len)", hdlz::launch_gzip_members_index, "launch k_gzm_scan");
}

// The scratch of hdlz_gzip_members_inflate_ws, laid out once for the size query and the call: five words per member (length, status,
// end bit, p, the CRC-32), then the decoder's view: m_off and m_end of nmembers words, m_out_off of nmembers + 1.  No members: no scratch.
static size_t gzip_members_layout(hdlz::GzipMembersArgs& u, uintptr_t base) {
    Carver c{base};
    u.len = c.take<uint32_t>(u.nmembers); u.status = c.take<uint32_t>(u.nmembers); u.end_bit = c.take<uint32_t>(u.nmembers);
    u.p = c.take<uint32_t>(u.nmembers); u.crc = c.take<uint32_t>(u.nmembers); c.align256();
    u.m_off = c.take<uint64_t>(u.nmembers); u.m_end = c.take<uint64_t>(u.nmembers); u.m_out_off = c.take<uint64_t>(u.nmembers + 1u); c.align256();
    return u.nmembers ? c.bytes() : 0u;
}
size_t hdlz_gzip_members_inflate_work_bytes(uint64_t nmembers) {
    hdlz::GzipMembersArgs u{nullptr, 0, nullptr, nullptr, nmembers};
    return nmembers > 0x7FFFFFFFull ? 0u : gzip_members_layout(u, 0);
}

int hdlz_gzip_members_inflate_ws(const uint8_t* d_file, uint64_t file_len, const uint64_t* d_off, const uint64_t* d_out_off, uint64_t nmembers,
                                 uint8_t* d_out, uint64_t out_cap, uint32_t* d_member_status, hdlz_gzip_members_inflate_result* d_result,
                                 void* d_work, size_t work_bytes, void* stream) {
    if (!d_result || (nmembers && any_null(d_file, d_off, d_out_off)) || (out_cap && !d_out)) return fail_param("null device pointer");
    if (nmembers > 0x7FFFFFFFull) return fail_param("nmembers too large for one call (2^31 - 1 members)");
    if (misaligned(8, d_off, d_out_off, d_result)) return fail_align(8, "d_off / d_out_off / d_result");
    if (misaligned(4, d_member_status)) return fail_align(4, "d_member_status");
    if (misaligned(256, d_work)) return fail_align(256, "d_work");
    hdlz::GzipMembersArgs u{d_file, file_len, d_off, d_out_off, nmembers, out_cap, d_member_status, d_result};
    if (work_too_small(gzip_members_layout(u, address(d_work)), d_work, work_bytes, "hdlz_gzip_members_inflate_work_bytes(nmembers)")) return HDLZ_E_BAD_PARAM;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nmembers) {
        if (const int rc = launched(hdlz::launch_gzip_members_heads(u, st), "launch k_gzm_heads"); rc != HDLZ_OK) return rc;
        const MemberView v{u.m_off, u.m_end, u.m_out_off, out_cap};
        if (const int rc = decode_members(d_file, nmembers, d_out, u.len, u.status, u.end_bit, v, st, u.crc); rc != HDLZ_OK) return rc;
    }
    return launched(hdlz::launch_gzip_members_judge(u, st), "launch k_gzm_judge");
}

}  // extern "C"
// hdlz_zip_index_ws and hdlz_zip64_index_ws (include/hdlz_zip64.h; Rec: hdlz_zip_entry or hdlz_zip64_entry): the classic form ends at
// 2^32 bytes and records, the wide one at 2^31 records
template <class Rec>
static int zip_index_impl(const uint8_t* d_file, uint64_t file_len, uint64_t entry_cap, uint32_t out_align, Rec* d_entries, hdlz_zip_index_result* d_result,
                          void* d_work, size_t work_bytes, void* stream, size_t need, const char* query,
                          hipError_t (*launch)(const uint8_t*, uint64_t, uint64_t, uint32_t, Rec*, hdlz_zip_index_result*, void*, hipStream_t), const char* kernel) {
    constexpr bool wide = sizeof(Rec) != sizeof(hdlz_zip_entry);
    if (!d_result || (file_len && !d_file)) return fail_param("null device pointer");
    if (entry_cap && !d_entries) return fail_param("d_entries is null with entry_cap > 0");
    if (!wide && file_len > 0xFFFFFFFFull) return fail_param("file_len too large (below 2^32: ZIP64 is out of scope)");
    if (entry_cap > (wide ? 0x7FFFFFFFull : 0xFFFFFFFFull)) return fail_param(wide ? "entry_cap too large (below 2^31)" : "entry_cap too large (below 2^32)");
    if (out_align == 0u || out_align > 256u || (out_align & (out_align - 1u))) return fail_param("out_align must be a power of two in [1, 256]");
    if (work_too_small(need, d_work, work_bytes, query)) return HDLZ_E_BAD_PARAM;
    if (misaligned(8, d_entries, d_result, d_work)) return fail_align(8, "d_entries / d_result / d_work");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    return launched(launch(d_file, file_len, entry_cap, out_align, d_entries, d_result, d_work, static_cast<hipStream_t>(stream)), kernel);
}
// The scratch of hdlz_zip_inflate_ws and hdlz_zip64_inflate_ws, laid out once for the size query and the call: six words per entry
// (length, status, end bit, room, CRC-32, the checks' verdict), three 64-bit words per entry (the decoder's view: start, end,
// destination) and -- one entry -- a CRC word per 32 KiB tile of out_cap and the share of the batch call's path, which takes what is
// left from `decode` on.  `row`: what the one-stream path is given of out_cap (hdlz_zip_inflate_ws: all of it, in whole words)
template <class Rec>
static Laid zip_layout(hdlz::ZipArgsT<Rec>& z, uintptr_t base, uint64_t row) {
    Carver c{base};
    z.len = c.take<uint32_t>(z.count); z.status = c.take<uint32_t>(z.count); z.end_bit = c.take<uint32_t>(z.count);
    z.cap = c.take<uint32_t>(z.count); z.crc = c.take<uint32_t>(z.count); z.verdict = c.take<uint32_t>(z.count); c.align256();
    z.m_off = c.take<uint64_t>(z.count); z.m_end = c.take<uint64_t>(z.count); z.m_dst = c.take<uint8_t*>(z.count); c.align256();
    const size_t words = z.count == 1 ? hdlz::crc32_tiles(z.out_cap) : 0u;
    z.tiles = words ? c.take<uint32_t>(words) : nullptr; c.align256();
    const size_t decode = c.bytes();
    if (z.count == 1) c.take<uint8_t>(hdlz::round256(hdlz_inflate_work_bytes(1, z.bound, row, 0, 1)));
    return {c.bytes(), decode};
}
static size_t zip_inflate_work_bytes(uint64_t count, uint32_t in_len, uint64_t out_cap, uint64_t row) {
    hdlz::ZipArgs z{nullptr, 0, nullptr, count, in_len, nullptr, out_cap};
    return count == 0 || count > 0x7FFFFFFFull ? 0u : zip_layout(z, 0, row).bytes;
}
// the row the one-stream path is given: the decoders' room ends at 2^32 - 512 (a stored entry needs none of it)
static uint64_t zip64_row(uint64_t out_cap) { return (out_cap & ~3ull) < 0xFFFFFE00ull ? out_cap & ~3ull : 0xFFFFFE00ull; }
// hdlz_zip_inflate_ws and hdlz_zip64_inflate_ws (include/hdlz_zip64.h): `row` is what the one-stream path is given of out_cap
template <class Rec>
static int zip_inflate_impl(const uint8_t* d_file, uint64_t file_len, const Rec* d_entries, uint64_t first, uint64_t count, uint32_t in_len,
                            uint8_t* d_out, uint64_t out_cap, uint64_t row, uint32_t* d_entry_status, hdlz_zip_inflate_result* d_result,
                            void* d_work, size_t work_bytes, void* stream, const char* query) {
    if (!d_result) return fail_param("d_result is required");
    if (count && any_null(d_file, d_entries)) return fail_param("null device pointer");
    if (out_cap && !d_out) return fail_param("d_out is null with out_cap > 0");
    if (first > 0x7FFFFFFFull || count > 0x7FFFFFFFull || first + count > 0x7FFFFFFFull) return fail_param("first + count too large (below 2^31)");
    if (sizeof(Rec) == sizeof(hdlz_zip_entry) && file_len > 0xFFFFFFFFull) return fail_param("file_len too large (below 2^32: ZIP64 is out of scope)");
    if (misaligned(8, d_entries, d_result)) return fail_align(8, "d_entries / d_result");
    if (misaligned(4, d_entry_status)) return fail_align(4, "d_entry_status");
    if (misaligned(256, d_work)) return fail_align(256, "d_work");
    hdlz::ZipArgsT<Rec> z{d_file, file_len, d_entries ? d_entries + first : nullptr, count, in_len, d_out, out_cap, d_entry_status, d_result};
    const Laid l = zip_layout(z, address(d_work), row);
    if (count && work_too_small(l.bytes, d_work, work_bytes, query)) return HDLZ_E_BAD_PARAM;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // one entry takes the batch call's path, which stores words, when its row is one that path accepts; else the task view
    const bool single = z.single = count == 1 && out_cap >= 4u && !misaligned(4, d_out);
    if (!single) z.tiles = nullptr;
    if (const int rc = launched(hdlz::launch_zip_check(z, st), "launch k_zip_check"); rc != HDLZ_OK) return rc;
    if (single) {                                                                                 // a large entry (m_off[0], m_end[0]: its ragged index)
        if (const int rc = inflate_one(d_file, z.m_off, in_len, d_out, row, z.len, z.status, z.end_bit, d_work, work_bytes, l.decode, stream); rc != HDLZ_OK) return rc;
    } else if (count) {
        const MemberView v{z.m_off, z.m_end, nullptr, 0, 0, 0, z.m_dst, z.cap};                        // the task view
        if (const int rc = decode_members(d_file, count, d_out, z.len, z.status, z.end_bit, v, st); rc != HDLZ_OK) return rc;
    }
    if (const int rc = launched(hdlz::launch_zip_copy(z, st), "launch k_zip_copy"); rc != HDLZ_OK) return rc;
    if (const int rc = launched(hdlz::launch_zip_crc(z, st), "launch k_zip_crc_*"); rc != HDLZ_OK) return rc;
    return launched(hdlz::launch_zip_judge(z, st), "launch k_zip_judge");
}

extern "C" {

// ---- include/hdlz_zip.h: ZIP archives, the directory indexed and the entries read on the device (hdlz_zip.hip)
size_t hdlz_zip_index_work_bytes(uint64_t file_len, uint64_t entry_cap) {
    (void)entry_cap;
    return file_len > 0xFFFFFFFFull ? 0u : hdlz::zip_index_work_bytes();
}

int hdlz_zip_index_ws(const uint8_t* d_file, uint64_t file_len, uint64_t entry_cap, uint32_t out_align, hdlz_zip_entry* d_entries,
                      hdlz_zip_index_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    return zip_index_impl(d_file, file_len, entry_cap, out_align, d_entries, d_result, d_work, work_bytes, stream, hdlz::zip_index_work_bytes(),
                          "hdlz_zip_index_work_bytes(file_len, entry_cap)", hdlz::launch_zip_index, "launch k_zip_end");
}

size_t hdlz_zip_inflate_work_bytes(uint64_t count, uint32_t in_len, uint64_t out_cap) { return zip_inflate_work_bytes(count, in_len, out_cap, out_cap & ~3ull); }

int hdlz_zip_inflate_ws(const uint8_t* d_file, uint64_t file_len, const hdlz_zip_entry* d_entries, uint64_t first, uint64_t count,
                        uint32_t in_len, uint8_t* d_out, uint64_t out_cap, uint32_t* d_entry_status, hdlz_zip_inflate_result* d_result,
                        void* d_work, size_t work_bytes, void* stream) {
    return zip_inflate_impl(d_file, file_len, d_entries, first, count, in_len, d_out, out_cap, out_cap & ~3ull, d_entry_status, d_result, d_work,
                            work_bytes, stream, "hdlz_zip_inflate_work_bytes(count, in_len, out_cap)");
}

// ---- include/hdlz_zip64.h: ZIP64 indexed and read; written: further down (the generalised index kernels of hdlz_zip.hip, and its read kernels over the 64-byte record)
size_t hdlz_zip64_index_work_bytes(uint64_t file_len, uint64_t entry_cap) {
    (void)file_len;
    return entry_cap > 0x7FFFFFFFull ? 0u : hdlz::zip64_index_work_bytes(entry_cap);
}

int hdlz_zip64_index_ws(const uint8_t* d_file, uint64_t file_len, uint64_t entry_cap, uint32_t out_align, hdlz_zip64_entry* d_entries,
                        hdlz_zip_index_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    return zip_index_impl(d_file, file_len, entry_cap, out_align, d_entries, d_result, d_work, work_bytes, stream, hdlz::zip64_index_work_bytes(entry_cap),
                          "hdlz_zip64_index_work_bytes(file_len, entry_cap)", hdlz::launch_zip64_index, "launch k_zip64_end");
}

size_t hdlz_zip64_inflate_work_bytes(uint64_t count, uint32_t in_len, uint64_t out_cap) { return zip_inflate_work_bytes(count, in_len, out_cap, zip64_row(out_cap)); }

int hdlz_zip64_inflate_ws(const uint8_t* d_file, uint64_t file_len, const hdlz_zip64_entry* d_entries, uint64_t first, uint64_t count,
                          uint32_t in_len, uint8_t* d_out, uint64_t out_cap, uint32_t* d_entry_status, hdlz_zip_inflate_result* d_result,
                          void* d_work, size_t work_bytes, void* stream) {
    return zip_inflate_impl(d_file, file_len, d_entries, first, count, in_len, d_out, out_cap, zip64_row(out_cap), d_entry_status, d_result, d_work,
                            work_bytes, stream, "hdlz_zip64_inflate_work_bytes(count, in_len, out_cap)");
}

// ---- include/hdlz_zip_write.h: a ZIP archive written from the rows of one compress batch (hdlz_zip_write.hip)
size_t hdlz_zip_write_bound(uint64_t nentries, uint64_t nblocks, uint32_t block_len, uint64_t total_in, uint64_t names_len) {
    (void)nblocks; (void)block_len;                          // (a payload is never longer than its entry)
    return 22u + 76u * (size_t)nentries + 2u * (size_t)names_len + (size_t)total_in;
}

size_t hdlz_zip_write_work_bytes(uint64_t nentries, uint64_t nblocks) {
    return nentries > 65535u || nblocks > 0x7FFFFFFFull ? 0u : hdlz::zip_write_work_bytes(nentries, nblocks);
}

// hdlz_zip_write_ws and hdlz_zip64_write_ws (include/hdlz_zip64.h: wide, with its records in d_entries64 and its zip64_from)
static int zip_write_impl(const uint8_t* d_in, const uint64_t* d_ent_off, const uint8_t* d_names, const uint64_t* d_name_off, uint64_t nentries,
                          const uint64_t* d_in_off, const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_end_bits,
                          const uint32_t* d_status, uint64_t nblocks, const uint64_t* d_blk_first, const uint32_t* d_crc, uint32_t flags,
                          uint32_t dos_datetime, uint32_t out_align, uint64_t total_in, uint8_t* d_file, uint64_t file_cap, hdlz_zip_entry* d_entries,
                          hdlz_zip64_entry* d_entries64, hdlz_zip_write_result* d_result, void* d_work, size_t work_bytes, void* stream, bool wide,
                          uint64_t zip64_from) {
    if (!d_result) return fail_param("d_result is required");
    if (nentries > (wide ? 0x7FFFFFFFull : 65535u)) return fail_param(wide ? "nentries too large (2^31 - 1 entries)" : "nentries too large (at most 65535: ZIP64 is out of scope)");
    if (nblocks > 0x7FFFFFFFull || (nblocks && !nentries)) return fail_param("nblocks too large for one launch (2^31 - 1 rows), or rows without entries");
    if (nentries && (any_null(d_in, d_names, d_crc) || any_null(d_ent_off, d_name_off, d_blk_first))) return fail_param("null device pointer (the entries)");
    if (nblocks && (any_null(d_in_off, d_end_bits) || any_null(d_len, d_status) || !d_rows)) return fail_param("null device pointer (the rows)");
    if (file_cap && !d_file) return fail_param("d_file is null with file_cap > 0");
    if (flags & ~(uint32_t)HDLZ_ZIP_FLAG_UTF8) return fail_param("flags: only HDLZ_ZIP_FLAG_UTF8 may be set");
    if (out_align == 0u || out_align > 256u || (out_align & (out_align - 1u))) return fail_param("out_align must be a power of two in [1, 256]");
    if (zip64_from > 0xFFFFFFFFull) return fail_param("zip64_from must be at most FFFFFFFF");
    if (work_too_small(hdlz::zip_write_work_bytes(nentries, nblocks, wide), d_work, work_bytes,
                       wide ? "hdlz_zip64_write_work_bytes(nentries, nblocks)" : "hdlz_zip_write_work_bytes(nentries, nblocks)")) return HDLZ_E_BAD_PARAM;
    if (misaligned(8, d_ent_off, d_name_off, d_in_off, d_end_bits, d_blk_first) || misaligned(8, d_entries, d_entries64) || misaligned(8, d_result) || misaligned(8, d_work))
        return fail_align(8, "d_ent_off / d_name_off / d_in_off / d_end_bits / d_blk_first / d_entries / d_result / d_work");
    if (misaligned(4, d_len, d_status, d_crc)) return fail_align(4, "d_len / d_status / d_crc");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hdlz::ZipWriteArgs a{d_in, d_ent_off, d_names, d_name_off, nentries, d_in_off, d_rows, row_pitch, d_len, d_end_bits, d_status, nblocks,
                         d_blk_first, d_crc, flags, dos_datetime, out_align, total_in, d_file, file_cap, d_entries, d_result, {}, d_entries64, zip64_from};
    return launched(hdlz::launch_zip_write(a, d_work, static_cast<hipStream_t>(stream), wide), wide ? "launch k_zipw64_*" : "launch k_zipw_*");
}

int hdlz_zip_write_ws(const uint8_t* d_in, const uint64_t* d_ent_off, const uint8_t* d_names, const uint64_t* d_name_off, uint64_t nentries,
                      const uint64_t* d_in_off, const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_end_bits,
                      const uint32_t* d_status, uint64_t nblocks, const uint64_t* d_blk_first, const uint32_t* d_crc, uint32_t flags,
                      uint32_t dos_datetime, uint32_t out_align, uint64_t total_in, uint8_t* d_file, uint64_t file_cap,
                      hdlz_zip_entry* d_entries, hdlz_zip_write_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    return zip_write_impl(d_in, d_ent_off, d_names, d_name_off, nentries, d_in_off, d_rows, row_pitch, d_len, d_end_bits, d_status, nblocks, d_blk_first, d_crc,
                          flags, dos_datetime, out_align, total_in, d_file, file_cap, d_entries, nullptr, d_result, d_work, work_bytes, stream, false,
                          0xFFFFFFFFull);                    // (the args record's default: the classic form has no zip64_from)
}

// ---- include/hdlz_zip64.h: ZIP64 written (the scan and the gather of hdlz_zip_write.hip, a plan for any number of entries)
size_t hdlz_zip64_write_bound(uint64_t nentries, uint64_t nblocks, uint32_t block_len, uint64_t total_in, uint64_t names_len) {
    (void)nblocks; (void)block_len;
    return 98u + 124u * (size_t)nentries + 2u * (size_t)names_len + (size_t)total_in;
}

size_t hdlz_zip64_write_work_bytes(uint64_t nentries, uint64_t nblocks) {
    return nentries > 0x7FFFFFFFull || nblocks > 0x7FFFFFFFull ? 0u : hdlz::zip_write_work_bytes(nentries, nblocks, true);
}

int hdlz_zip64_write_ws(const uint8_t* d_in, const uint64_t* d_ent_off, const uint8_t* d_names, const uint64_t* d_name_off, uint64_t nentries,
                        const uint64_t* d_in_off, const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_end_bits,
                        const uint32_t* d_status, uint64_t nblocks, const uint64_t* d_blk_first, const uint32_t* d_crc, uint32_t flags,
                        uint32_t dos_datetime, uint32_t out_align, uint64_t zip64_from, uint64_t total_in, uint8_t* d_file, uint64_t file_cap,
                        hdlz_zip64_entry* d_entries, hdlz_zip_write_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    return zip_write_impl(d_in, d_ent_off, d_names, d_name_off, nentries, d_in_off, d_rows, row_pitch, d_len, d_end_bits, d_status, nblocks, d_blk_first, d_crc,
                          flags, dos_datetime, out_align, total_in, d_file, file_cap, nullptr, d_entries, d_result, d_work, work_bytes, stream, true, zip64_from);
}

}  // extern "C"

// ---- include/hdlz_png.h: PNG images, the chunks walked, the pixels inflated and unfiltered on the device (hdlz_png.hip)
// The scratch of hdlz_png_decode_ws, laid out once for the size query and the call (the header states the closed form).  The one-stream
// path takes what is left from `decode` on; `row` is what it is given of the decoded streams' room.
static uint32_t png_bound(uint64_t z_bytes) { return z_bytes < 0x0FFFFFFFull ? (uint32_t)z_bytes : 0x0FFFFFFFu; }
static uint64_t png_row(uint64_t raw_bytes) { return (raw_bytes & ~3ull) < 0xFFFFFE00ull ? raw_bytes & ~3ull : 0xFFFFFE00ull; }
static Laid png_layout(hdlz::PngArgs& g, uintptr_t base) {
    Carver c{base};
    const size_t n = (size_t)g.count;
    g.len = c.take<uint32_t>(n); g.status = c.take<uint32_t>(n); g.end_bit = c.take<uint32_t>(n); g.cap = c.take<uint32_t>(n);
    g.verdict = c.take<uint32_t>(n); g.crcbad = c.take<uint32_t>(n); g.fltbad = c.take<uint32_t>(n); g.fin = c.take<uint32_t>(n); c.align256();
    g.m_off = c.take<uint64_t>(n); g.m_end = c.take<uint64_t>(n); g.m_dst = c.take<uint8_t*>(n);
    g.cbase = c.take<uint64_t>(n + 1u); g.tb = c.take<uint64_t>(n + 1u); g.zb = c.take<uint64_t>(n + 1u); g.sb = c.take<uint64_t>(n + 1u);
    g.head = c.take<uint64_t>(32); c.align256();
    g.c_src = c.take<uint64_t>((size_t)g.list_cap); g.c_dst = c.take<uint64_t>((size_t)g.list_cap);
    g.c_len = c.take<uint32_t>((size_t)g.list_cap); g.c_img = c.take<uint32_t>((size_t)g.list_cap); c.align256();
    g.tiles = c.take<uint2>((size_t)g.tile_cap); c.align256();
    g.z = c.take<uint8_t>((size_t)g.z_bytes); c.align256();
    g.raw = c.take<uint8_t>((size_t)g.raw_bytes); c.align256();
    const size_t decode = c.bytes();
    if (g.count == 1) c.take<uint8_t>(hdlz::round256(hdlz_inflate_work_bytes(1, png_bound(g.z_bytes), png_row(g.raw_bytes), 0, 1)));
    return {c.bytes(), decode};
}
static hdlz::PngArgs png_args(uint64_t count, uint64_t idat_cap, uint64_t z_bytes, uint64_t raw_bytes) {
    hdlz::PngArgs g{};
    g.count = count; g.list_cap = idat_cap + 4u * count; g.tile_cap = raw_bytes / 32768u + count; g.z_bytes = z_bytes; g.raw_bytes = raw_bytes;
    return g;
}
static bool png_caps_ok(uint64_t idat_cap, uint64_t z_bytes, uint64_t raw_bytes) { return idat_cap < (1ull << 40) && z_bytes < (1ull << 40) && raw_bytes < (1ull << 40); }

extern "C" {

size_t hdlz_png_index_work_bytes(uint64_t n, uint64_t image_cap) {
    (void)image_cap;
    return n == 0 || n > 0x7FFFFFFFull ? 0u : hdlz::png_index_work_bytes(n);
}

int hdlz_png_index_ws(const uint8_t* d_files, uint64_t files_len, const uint64_t* d_file_off, const uint64_t* d_file_len, uint64_t n,
                      uint32_t flags, uint32_t out_align, uint64_t image_cap, hdlz_png_image* d_images, hdlz_png_index_result* d_result,
                      void* d_work, size_t work_bytes, void* stream) {
    if (!d_result || (n && any_null(d_files, d_file_off, d_file_len))) return fail_param("null device pointer");
    if (image_cap && !d_images) return fail_param("d_images is null with image_cap > 0");
    if (n > 0x7FFFFFFFull) return fail_param("n too large (below 2^31)");
    if (image_cap > 0x7FFFFFFFull) return fail_param("image_cap too large (below 2^31)");
    if (flags & ~(HDLZ_PNG_EXPAND | HDLZ_PNG_ADAM7)) return fail_param("flags must be HDLZ_PNG_RAW or HDLZ_PNG_EXPAND, with or without HDLZ_PNG_ADAM7");
    if (out_align == 0u || out_align > 256u || (out_align & (out_align - 1u))) return fail_param("out_align must be a power of two in [1, 256]");
    if (work_too_small(hdlz_png_index_work_bytes(n, image_cap), d_work, work_bytes, "hdlz_png_index_work_bytes(n, image_cap)")) return HDLZ_E_BAD_PARAM;
    if (misaligned(8, d_file_off, d_file_len, d_images, d_result) || misaligned(8, d_work)) return fail_align(8, "d_file_off / d_file_len / d_images / d_result / d_work");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    return launched(hdlz::launch_png_index(d_files, files_len, d_file_off, d_file_len, n, flags, out_align, image_cap, d_images, d_result, d_work,
                                           static_cast<hipStream_t>(stream)), "launch k_png_parse");
}

size_t hdlz_png_decode_work_bytes(uint64_t count, uint64_t idat_cap, uint64_t z_bytes, uint64_t raw_bytes) {
    if (count == 0 || count > 0x7FFFFFFFull || !png_caps_ok(idat_cap, z_bytes, raw_bytes)) return 0u;
    hdlz::PngArgs g = png_args(count, idat_cap, z_bytes, raw_bytes);
    return png_layout(g, 0).bytes;
}

int hdlz_png_decode_ws(const uint8_t* d_files, uint64_t files_len, const hdlz_png_image* d_images, uint64_t first, uint64_t count,
                       uint32_t flags, uint64_t idat_cap, uint64_t z_bytes, uint64_t raw_bytes, uint8_t* d_out, uint64_t out_cap,
                       uint32_t* d_image_status, hdlz_png_decode_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    if (!d_result) return fail_param("d_result is required");
    if (count && any_null(d_files, d_images)) return fail_param("null device pointer");
    if (out_cap && !d_out) return fail_param("d_out is null with out_cap > 0");
    if (first > 0x7FFFFFFFull || count > 0x7FFFFFFFull || first + count > 0x7FFFFFFFull) return fail_param("first + count too large (below 2^31)");
    if (flags & ~(HDLZ_PNG_EXPAND | HDLZ_PNG_ADAM7)) return fail_param("flags must be HDLZ_PNG_RAW or HDLZ_PNG_EXPAND, with or without HDLZ_PNG_ADAM7");
    if (!png_caps_ok(idat_cap, z_bytes, raw_bytes)) return fail_param("idat_cap, z_bytes or raw_bytes too large (below 2^40)");
    if (misaligned(8, d_images, d_result)) return fail_align(8, "d_images / d_result");
    if (misaligned(4, d_image_status)) return fail_align(4, "d_image_status");
    if (misaligned(256, d_work)) return fail_align(256, "d_work");
    hdlz::PngArgs g = png_args(count, idat_cap, z_bytes, raw_bytes);
    g.in = d_files; g.in_len = files_len; g.images = d_images ? d_images + first : nullptr; g.flags = flags;
    g.out = d_out; g.out_cap = out_cap; g.image_status = d_image_status; g.result = d_result;
    const Laid l = png_layout(g, address(d_work));
    if (count && work_too_small(l.bytes, d_work, work_bytes, "hdlz_png_decode_work_bytes(count, idat_cap, z_bytes, raw_bytes)")) return HDLZ_E_BAD_PARAM;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool single = g.single = count == 1 && png_row(raw_bytes) >= 4u;
    if (const int rc = launched(hdlz::launch_png_front(g, st), "launch k_png_plan"); rc != HDLZ_OK) return rc;
    if (single) {                                                                                 // a large image (m_off[0], m_end[0]: its ragged index)
        if (const int rc = inflate_one(g.z, g.m_off, png_bound(z_bytes), g.raw, png_row(raw_bytes), g.len, g.status, g.end_bit, d_work, work_bytes, l.decode, stream); rc != HDLZ_OK) return rc;
    } else if (count) {
        const MemberView v{g.m_off, g.m_end, nullptr, 0, 0, 0, g.m_dst, g.cap};                        // the task view
        if (const int rc = decode_members(g.z, count, g.raw, g.len, g.status, g.end_bit, v, st); rc != HDLZ_OK) return rc;
    }
    return launched(hdlz::launch_png_back(g, st), "launch k_png_unfilter");
}

}  // extern "C"

// ---- include/hdlz_png_write.h: PNG files written on the device (hdlz_png_write.hip)
extern "C" {

size_t hdlz_png_filter_work_bytes(uint64_t n) { return n == 0 || n > 0x7FFFFFFFull ? 0u : hdlz::png_filter_work_bytes(n); }

int hdlz_png_filter_ws(const uint8_t* d_pix, uint64_t pix_len, const hdlz_png_spec* d_specs, uint64_t n, uint32_t mode, uint64_t total_rows,
                       uint8_t* d_raw, uint64_t raw_cap, uint8_t* d_row_filter, uint32_t* d_status, uint64_t* d_raw_off, void* d_work,
                       size_t work_bytes, void* stream) {
    if (n && (any_null(d_specs) || any_null(d_status) || any_null(d_raw_off))) return fail_param("null device pointer");
    if (pix_len && !d_pix) return fail_param("d_pix is null with pix_len > 0");
    if (raw_cap && !d_raw) return fail_param("d_raw is null with raw_cap > 0");
    if (n > 0x7FFFFFFFull) return fail_param("n too large (below 2^31)");
    if (mode > HDLZ_PNG_FILTER_ADAPTIVE) return fail_param("mode must be a filter 0 .. 4 or HDLZ_PNG_FILTER_ADAPTIVE");
    if (total_rows >= (1ull << 40)) return fail_param("total_rows too large (below 2^40)");
    if (work_too_small(hdlz_png_filter_work_bytes(n), d_work, work_bytes, "hdlz_png_filter_work_bytes(n)")) return HDLZ_E_BAD_PARAM;
    if (misaligned(8, d_specs) || misaligned(8, d_raw_off) || misaligned(8, d_work)) return fail_align(8, "d_specs / d_raw_off / d_work");
    if (misaligned(4, d_status)) return fail_align(4, "d_status");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hdlz::PngFilterArgs a{d_pix, pix_len, d_specs, n, mode, total_rows, d_raw, raw_cap, d_row_filter, d_status, d_raw_off, nullptr, nullptr};
    return launched(hdlz::launch_png_filter(a, d_work, static_cast<hipStream_t>(stream)), "launch k_pngw_filter");
}

size_t hdlz_png_write_bound(uint64_t n, uint64_t total_raw, uint64_t nblocks, uint32_t block_len, uint32_t idat_len) {
    (void)total_raw;
    if (idat_len == 0u) return 0u;
    const size_t Z = 15u * (size_t)n + (size_t)nblocks * (hdlz_out_bound(block_len) - 1u);
    return Z + 12u * (Z / idat_len) + 57u * (size_t)n;
}

size_t hdlz_png_write_work_bytes(uint64_t n, uint64_t nblocks) {
    return n == 0 || n > 0x7FFFFFFFull || nblocks > 0x7FFFFFFFull ? 0u : hdlz::png_write_work_bytes(n, nblocks);
}

int hdlz_png_write_ws(const hdlz_png_spec* d_specs, uint64_t n, const uint8_t* d_raw, const uint64_t* d_raw_off, const uint32_t* d_filter_status,
                      const uint64_t* d_in_off, const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_end_bits,
                      const uint32_t* d_status, uint64_t nblocks, const uint64_t* d_blk_first, uint32_t idat_len, uint32_t flags, uint32_t out_align,
                      uint8_t* d_file, uint64_t file_cap, uint64_t* d_file_off, uint64_t* d_file_len, uint32_t* d_image_status,
                      hdlz_png_image* d_images, hdlz_png_write_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    if (!d_result) return fail_param("d_result is required");
    if (n > 0x7FFFFFFFull) return fail_param("n too large (below 2^31)");
    if (nblocks > 0x7FFFFFFFull || (nblocks && !n)) return fail_param("nblocks too large for one launch (2^31 - 1 rows), or rows without images");
    if (n && (any_null(d_specs) || any_null(d_raw_off, d_blk_first, d_file_off, d_file_len))) return fail_param("null device pointer (the images)");
    if (nblocks && (any_null(d_in_off, d_end_bits) || any_null(d_len, d_status) || !d_rows)) return fail_param("null device pointer (the rows)");
    if (file_cap && !d_file) return fail_param("d_file is null with file_cap > 0");
    if (idat_len == 0u || idat_len > 0x7FFFFFFFu) return fail_param("idat_len must be in [1, 2^31 - 1]");
    if (flags > HDLZ_PNG_EXPAND) return fail_param("flags must be HDLZ_PNG_RAW or HDLZ_PNG_EXPAND");
    if (out_align == 0u || out_align > 256u || (out_align & (out_align - 1u))) return fail_param("out_align must be a power of two in [1, 256]");
    if (work_too_small(hdlz_png_write_work_bytes(n, nblocks), d_work, work_bytes, "hdlz_png_write_work_bytes(n, nblocks)")) return HDLZ_E_BAD_PARAM;
    if (misaligned(8, d_raw_off, d_in_off, d_end_bits, d_blk_first, d_file_off, d_file_len) || misaligned(8, d_specs) || misaligned(8, d_images) ||
        misaligned(8, d_result) || misaligned(8, d_work))
        return fail_align(8, "d_specs / d_raw_off / d_in_off / d_end_bits / d_blk_first / d_file_off / d_file_len / d_images / d_result / d_work");
    if (misaligned(4, d_len, d_status, d_filter_status, d_image_status)) return fail_align(4, "d_len / d_status / d_filter_status / d_image_status");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hdlz::PngWriteArgs a{};
    a.specs = d_specs; a.n = n; a.raw = d_raw; a.raw_off = d_raw_off; a.fstatus = d_filter_status; a.in_off = d_in_off; a.rows = d_rows;
    a.pitch = row_pitch; a.len = d_len; a.end_bits = d_end_bits; a.status = d_status; a.nblocks = nblocks; a.blk_first = d_blk_first;
    a.idat = idat_len; a.flags = flags; a.out_align = out_align; a.file = d_file; a.cap = file_cap; a.file_off = d_file_off; a.file_len = d_file_len;
    a.image_status = d_image_status; a.images = d_images; a.result = d_result;
    return launched(hdlz::launch_png_write(a, d_work, static_cast<hipStream_t>(stream)), "launch k_pngw_*");
}

}  // extern "C"

// ---- include/hdlz_tiff.h: TIFF images, the directory walked, the strips and tiles inflated and the predictor undone on the device (hdlz_tiff.hip)
// The scratch of hdlz_tiff_decode_ws, laid out once for the size query and the call (the header states the closed form).  The one-chunk
// route takes what is left from `decode` on; `row` is what it is given of the decoded chunks' room, `bound` what it sizes itself from.
static uint32_t tiff_bound(uint64_t raw_bytes) { return 2u * raw_bytes + 64u < 0x0FFFFFFFull ? (uint32_t)(2u * raw_bytes + 64u) : 0x0FFFFFFFu; }
static bool tiff_one(const hdlz::TiffArgs& g) { return g.count == 1 && g.chunk_cap == 1; }
static Laid tiff_layout(hdlz::TiffArgs& g, uintptr_t base) {
    Carver c{base};
    const size_t n = (size_t)g.count, k = (size_t)g.chunk_cap;
    g.verdict = c.take<uint32_t>(n); g.fin = c.take<uint32_t>(n); c.align256();
    g.cb = c.take<uint64_t>(n + 1u); g.tb = c.take<uint64_t>(n + 1u); g.head = c.take<uint64_t>(32); c.align256();
    g.m_off = c.take<uint64_t>(k); g.m_end = c.take<uint64_t>(k); g.m_dst = c.take<uint8_t*>(k); c.align256();
    g.cap = c.take<uint32_t>(k); g.len = c.take<uint32_t>(k); g.status = c.take<uint32_t>(k); g.end_bit = c.take<uint32_t>(k); g.cst = c.take<uint32_t>(k); c.align256();
    g.tiles = c.take<uint2>((size_t)g.tile_cap); c.align256();
    g.raw = c.take<uint8_t>((size_t)g.raw_bytes); c.align256();
    const size_t decode = c.bytes();
    if (tiff_one(g)) c.take<uint8_t>(hdlz::round256(hdlz_inflate_work_bytes(1, tiff_bound(g.raw_bytes), png_row(g.raw_bytes), 0, 1)));
    return {c.bytes(), decode};
}
static hdlz::TiffArgs tiff_args(uint64_t count, uint64_t chunk_cap, uint64_t raw_bytes) {
    hdlz::TiffArgs g{};
    g.count = count; g.chunk_cap = chunk_cap; g.tile_cap = raw_bytes / 32768u + chunk_cap; g.raw_bytes = raw_bytes;
    return g;
}
static bool tiff_caps_ok(uint64_t chunk_cap, uint64_t raw_bytes) { return chunk_cap <= 0x7FFFFFFFull && raw_bytes < (1ull << 40); }

extern "C" {

size_t hdlz_tiff_index_work_bytes(uint64_t n, uint64_t image_cap) {
    (void)image_cap;
    return n == 0 || n > 0x7FFFFFFFull ? 0u : hdlz::tiff_index_work_bytes(n);
}

int hdlz_tiff_index_ws(const uint8_t* d_files, uint64_t files_len, const uint64_t* d_file_off, const uint64_t* d_file_len, const uint32_t* d_page,
                       uint64_t n, uint32_t out_align, uint64_t image_cap, hdlz_tiff_image* d_images, hdlz_tiff_index_result* d_result,
                       void* d_work, size_t work_bytes, void* stream) {
    if (!d_result || (n && any_null(d_files, d_file_off, d_file_len))) return fail_param("null device pointer");
    if (image_cap && !d_images) return fail_param("d_images is null with image_cap > 0");
    if (n > 0x7FFFFFFFull) return fail_param("n too large (below 2^31)");
    if (image_cap > 0x7FFFFFFFull) return fail_param("image_cap too large (below 2^31)");
    if (out_align == 0u || out_align > 256u || (out_align & (out_align - 1u))) return fail_param("out_align must be a power of two in [1, 256]");
    if (work_too_small(hdlz_tiff_index_work_bytes(n, image_cap), d_work, work_bytes, "hdlz_tiff_index_work_bytes(n, image_cap)")) return HDLZ_E_BAD_PARAM;
    if (misaligned(8, d_file_off, d_file_len, d_images, d_result) || misaligned(8, d_work)) return fail_align(8, "d_file_off / d_file_len / d_images / d_result / d_work");
    if (misaligned(4, d_page)) return fail_align(4, "d_page");
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    return launched(hdlz::launch_tiff_index(d_files, files_len, d_file_off, d_file_len, d_page, n, out_align, image_cap, d_images, d_result, d_work,
                                            static_cast<hipStream_t>(stream)), "launch k_tiff_parse");
}

size_t hdlz_tiff_decode_work_bytes(uint64_t count, uint64_t chunk_cap, uint64_t raw_bytes) {
    if (count == 0 || count > 0x7FFFFFFFull || !tiff_caps_ok(chunk_cap, raw_bytes)) return 0u;
    hdlz::TiffArgs g = tiff_args(count, chunk_cap, raw_bytes);
    return tiff_layout(g, 0).bytes;
}

int hdlz_tiff_decode_ws(const uint8_t* d_files, uint64_t files_len, const hdlz_tiff_image* d_images, uint64_t first, uint64_t count,
                        uint64_t chunk_cap, uint64_t raw_bytes, uint8_t* d_out, uint64_t out_cap, uint32_t* d_image_status,
                        hdlz_tiff_decode_result* d_result, void* d_work, size_t work_bytes, void* stream) {
    if (!d_result) return fail_param("d_result is required");
    if (count && any_null(d_files, d_images)) return fail_param("null device pointer");
    if (out_cap && !d_out) return fail_param("d_out is null with out_cap > 0");
    if (first > 0x7FFFFFFFull || count > 0x7FFFFFFFull || first + count > 0x7FFFFFFFull) return fail_param("first + count too large (below 2^31)");
    if (!tiff_caps_ok(chunk_cap, raw_bytes)) return fail_param("chunk_cap (below 2^31) or raw_bytes (below 2^40) too large");
    if (misaligned(8, d_images, d_result)) return fail_align(8, "d_images / d_result");
    if (misaligned(4, d_image_status)) return fail_align(4, "d_image_status");
    if (misaligned(256, d_work)) return fail_align(256, "d_work");
    hdlz::TiffArgs g = tiff_args(count, chunk_cap, raw_bytes);
    g.in = d_files; g.in_len = files_len; g.images = d_images ? d_images + first : nullptr;
    g.out = d_out; g.out_cap = out_cap; g.image_status = d_image_status; g.result = d_result;
    const Laid l = tiff_layout(g, address(d_work));
    if (count && work_too_small(l.bytes, d_work, work_bytes, "hdlz_tiff_decode_work_bytes(count, chunk_cap, raw_bytes)")) return HDLZ_E_BAD_PARAM;
    if (const int rc = check_device(); rc != HDLZ_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool single = g.single = tiff_one(g) && png_row(raw_bytes) >= 4u;
    g.bound = tiff_bound(raw_bytes);
    if (const int rc = launched(hdlz::launch_tiff_front(g, st), "launch k_tiff_plan"); rc != HDLZ_OK) return rc;
    if (single) {                                                                                 // a single-strip image (m_off[0], m_end[0]: its ragged index)
        if (const int rc = inflate_one(d_files, g.m_off, g.bound, g.raw, png_row(raw_bytes), g.len, g.status, g.end_bit, d_work, work_bytes, l.decode, stream); rc != HDLZ_OK) return rc;
    } else if (count && chunk_cap) {
        const MemberView v{g.m_off, g.m_end, nullptr, 0, 0, 0, g.m_dst, g.cap};                        // the task view: a task a chunk
        if (const int rc = decode_members(d_files, chunk_cap, g.raw, g.len, g.status, g.end_bit, v, st); rc != HDLZ_OK) return rc;
    }
    return launched(hdlz::launch_tiff_back(g, st), "launch k_tiff_unpredict");
}

}  // extern "C"
