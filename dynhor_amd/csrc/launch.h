// What every launch function repeats: the 1-D grid of a grid-stride loop, and the status of the launches just enqueued.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dynhor_hip.h"

namespace dh {

// workgroups of `threads` for n items: at least one (a launch over nothing runs an empty loop), at most 2^20 (the kernel's
// grid-stride loop covers the rest)
inline unsigned grid_1d(int64_t n, int threads) {
    const int64_t b = (n + threads - 1) / threads;
    return (unsigned)(b < 1 ? 1 : (b < (1 << 20) ? b : (1 << 20)));
}

inline int launch_status() { return hipGetLastError() == hipSuccess ? DH_OK : DH_ERR_LAUNCH; }

}  // namespace dh
