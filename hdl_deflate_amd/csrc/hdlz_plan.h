// hdlz_plan.h -- what the one-workgroup planner kernels in front of the container calls are made of, each once: a thread's strip of
// the items, the scan of a wave and of the workgroup over 64-bit sums, the binary searches in the prefix arrays a planner leaves, and
// the verdict over a range of compressed rows.  The planners: k_zip_offsets, k_zip64_offsets (hdlz_zip.hip), k_zipw_plan, k_zipw64_plan
// (hdlz_zip_write.hip), k_png_offsets, k_png_plan (hdlz_png.hip), k_pngw_plan, k_pngw_scan, k_pngw_layout (hdlz_png_write.hip),
// k_gzm_seam (hdlz_gzip_members.hip).  What a kernel that is launched per item could not take from here without another instruction
// sequence stands in that kernel and is listed in profiles/planner_shared.txt, section 3.
#pragma once
#include "hdlz_device.h"

namespace hdlz {

// ---- thread tid of `threads` takes the items [lo, hi) of n: per = ceil(n / threads) consecutive ones, clamped to n (the last threads'
// strips may be empty); returns per
__device__ __forceinline__ uint64_t strip(uint64_t n, uint32_t threads, uint32_t tid, uint64_t& lo, uint64_t& hi) {
    const uint64_t per = (n + threads - 1u) / threads;
    lo = tid * per < n ? tid * per : n;
    hi = lo + per < n ? lo + per : n;
    return per;
}

// ---- the inclusive sum over the lanes of a wave, up to and with this one
__device__ __forceinline__ uint64_t wave_scan_add(uint64_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(v, o, 64);
        if (lane >= (uint32_t)o) v += t;
    }
    return v;
}

// ---- the exclusive prefix of every thread's mine[0 .. Q) over a workgroup of THREADS -> base; total: the Q sums, in every thread.
// lds: uint64_t[Q][THREADS / 64] (or more rows).  EVERY thread of the workgroup calls it, one with an empty strip too.  Two barriers:
// one in front of the stores to lds -- so a second scan may use the same array, and what the caller stored to LDS of its own before
// the call is visible to all behind it --, one between the stores and the loads.
template <int Q, uint32_t THREADS>
__device__ __forceinline__ void block_scan(const uint64_t (&mine)[Q], uint64_t (&base)[Q], uint64_t (&total)[Q], uint64_t (*lds)[THREADS / 64u]) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t v[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) v[q] = wave_scan_add(mine[q]);
    __syncthreads();
    if (lane == 63u) {
#pragma unroll
        for (int q = 0; q < Q; q++) lds[q][wave] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; q++) {
        base[q] = v[q] - mine[q];
        total[q] = 0u;
        for (uint32_t k = 0; k < THREADS / 64u; k++) {
            if (k < wave) base[q] += lds[q][k];
            total[q] += lds[q][k];
        }
    }
}

// ---- searches in an ascending a[0 .. n): the first i with a[i] > v (upper) or a[i] >= v (lower); n when there is none.  The index
// has the type of n: 32 bits where the caller's count has them
template <class T, class I>
__device__ __forceinline__ I upper(const T* __restrict__ a, I n, uint64_t v) {
    I lo = 0, hi = n;
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if ((uint64_t)a[mid] > v) hi = mid; else lo = mid + 1u;
    }
    return lo;
}
template <class T, class I>
__device__ __forceinline__ I lower(const T* __restrict__ a, I n, uint64_t v) {
    I lo = 0, hi = n;
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if ((uint64_t)a[mid] < v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}
// the item that owns slot g of a list, base being the exclusive prefix of the items' shares: the largest i < count with base[i] <= g,
// that is upper(base, count, g) - 1.  base[0] <= g; base[0] is not loaded
template <class T>
__device__ __forceinline__ uint64_t owner(const T* __restrict__ base, uint64_t count, uint64_t g) {
    uint64_t lo = 0, hi = count;
    while (hi - lo > 1u) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)base[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the verdict over the compressed rows [F0, F1) of an entry or an image (F0 < F1 <= the rows of the call).  A row scan
// (k_zipw_scan, k_pngw_scan) leaves in cnt the exclusive prefix of two counts in one word: rows whose status is not HDLZ_OK (bits
// 0 .. COUNT_BITS - 1) and rows whose length, end bit and pitch contradict each other (the bits above; nblocks < 2^31, so both fit
// under the two state bits of a look-back word).  Both counts ascend, so the halves of two prefixes subtract without a borrow.
// A range with a failed row walks its rows for the largest status: the one serial loop, on the failing path only.
constexpr uint32_t COUNT_BITS = 31u;
constexpr uint64_t COUNT_MASK = (1ull << COUNT_BITS) - 1u;
__device__ __forceinline__ uint32_t rows_verdict(const uint64_t* __restrict__ cnt, const uint32_t* __restrict__ status, uint64_t F0, uint64_t F1) {
    const uint64_t k = cnt[F1] - cnt[F0];
    uint32_t st = HDLZ_OK;
    if (k & COUNT_MASK) {
        for (uint64_t b = F0; b < F1; b++) st = max(st, status[b]);
    } else if (k >> COUNT_BITS) st = HDLZ_E_BAD_PARAM;
    return st;
}

}  // namespace hdlz
