// hdlz_ranges.h -- what the range kernels of hdlz_bgzf_range.hip and the two of hdlz_seek.hip that stand in for its expand and judge
// share: the workgroup size and the head's words of RangeArgs (hdlz_device.h); the binary searches are those of hdlz_plan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hdlz_plan.h"

namespace hdlz {
namespace bgzf {

constexpr uint32_t RT = 256u;                      // threads of the per-range and per-task kernels, and of the scan
constexpr uint32_t H_TOTAL = 0u, H_NTASKS = 1u, H_CAPACITY = 2u, H_FIRST = 3u;      // the head's words

}  // namespace bgzf
}  // namespace hdlz
