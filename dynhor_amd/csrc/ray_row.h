// A ray's row of the sample arrays and the mid depth m_k of a sample, for the per-ray kernels that read both sample layouts
// (prior_loss.hip, warp_loss.hip): dense [B,n], or the occupancy-grid sampler's packed segments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dh {
namespace {
struct PriorRow { int64_t rb; int n; };

// the ray's row of the sample arrays: dense [B,n], or its packed segment (at most max_samples of it, as the packed scan clamps)
__device__ __forceinline__ PriorRow prior_row(int64_t ray, int n, const int64_t* __restrict__ seg_off,
                                              const int32_t* __restrict__ seg_cnt, int max_samples) {
    PriorRow r;
    if (seg_off) {
        r.rb = seg_off[ray];
        r.n = min(max(seg_cnt[ray], 0), max_samples);
    } else {
        r.rb = ray * n;
        r.n = n;
    }
    return r;
}

// m_k of the scans: z_k + 0.5 (z_{k+1} - z_k), sample_dist for the last interval; packed: every interval is sample_dist long
__device__ __forceinline__ float prior_mid(const float* __restrict__ z, int64_t rb, int k, int n, bool packed, float sample_dist) {
    const float zc = z[rb + k];
    const float dist = (packed || k + 1 >= n) ? sample_dist : z[rb + k + 1] - zc;
    return zc + 0.5f * dist;
}
}  // namespace
}  // namespace dh
