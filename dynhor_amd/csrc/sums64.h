// The reproducible fp64 sum of the mesh kernels: K sums per workgroup (icp.hip, sil.hip) or per wave (mesh_simplify.hip), with no
// atomics and every addition in a fixed order.  Each lane first adds its own items in ascending order into acc[K]; then
//   sum64_wave:         a fixed xor butterfly (sum64_lanes: offsets 32, 16, .. 1) folds the 64 lanes; every lane ends with the wave's
//                       sums.  Every lane of the wave must be active: call it outside any divergent branch or early exit.
//   sum64_block_store:  the butterfly, then the SUM64_THREADS / 64 waves added in order through LDS, and one partial of K doubles
//                       stored per workgroup.  Called by all SUM64_THREADS threads of the workgroup.
//   launch_sum64_reduce (kernels.h, icp.hip): adds a group's partials in block order.
// sum64_blocks gives the workgroups per group; it depends on the item count alone, so a result is bitwise the same from launch to
// launch and however the groups are chunked over launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dh {
namespace {
constexpr int SUM64_THREADS = 256;

// clamp(ceil(n / SUM64_THREADS), 1, max_blocks)
inline int64_t sum64_blocks(int64_t n, int64_t max_blocks) {
    const int64_t b = (n + SUM64_THREADS - 1) / SUM64_THREADS;
    return b < 1 ? 1 : (b < max_blocks ? b : max_blocks);
}

__device__ __forceinline__ double sum64_lanes(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int K>
__device__ __forceinline__ void sum64_wave(double (&acc)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = sum64_lanes(acc[k]);
}

template <int K>
__device__ __forceinline__ void sum64_block_store(const double (&acc)[K], double* __restrict__ partial) {
    __shared__ double wave_sum[SUM64_THREADS / 64][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = sum64_lanes(acc[k]);
        if (lane == 0) wave_sum[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double v = wave_sum[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < SUM64_THREADS / 64; ++w) v += wave_sum[w][threadIdx.x];
        partial[threadIdx.x] = v;
    }
}
}  // namespace
}  // namespace dh
