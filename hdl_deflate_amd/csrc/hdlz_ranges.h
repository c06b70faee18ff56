// hdlz_ranges.h -- what the range kernels of hdlz_bgzf_range.hip and the two of hdlz_seek.hip that stand in for its expand and judge
// share: the workgroup size, the head's words of RangeArgs (hdlz_device.h) and the two binary searches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hdlz {
namespace bgzf {

constexpr uint32_t RT = 256u;                      // threads of the per-range and per-task kernels, and of the scan
constexpr uint32_t H_TOTAL = 0u, H_NTASKS = 1u, H_CAPACITY = 2u, H_FIRST = 3u;      // the head's words

// the first i in [0, n) with a[i] > v (upper) or a[i] >= v (lower); n when there is none
__device__ __forceinline__ uint64_t upper(const uint64_t* __restrict__ a, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint64_t lower(const uint64_t* __restrict__ a, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

}  // namespace bgzf
}  // namespace hdlz
