// Volumetric fusion of depth maps (dynhor_amd/depth_fuse.py): every frame's depth map, read at the projection of every grid point,
// summed over the frames into a weighted truncated signed distance per point.
//
// tsdf_integrate_kernel: one lane per point, looping over the frames of the call; the frame's R, T (and the depth image's K) are read
// at a wave-uniform address (the loop counter alone), so they sit in scalar registers.  The point's state (num, den, obs) is read once
// before the loop, lives in registers and is written once after it.  Per frame, in fp32:
//   projection: mk_project (mesh_raster.h); the pair is skipped unless c_2 > 1e-3
//   nearest pixel, as dh_mvs_check: xf = floor(u + 0.5), yf = floor(w + 0.5); skipped unless 0 <= xf <= W - 1 and 0 <= yf <= H - 1,
//     compared as floats before any conversion (every comparison is false for a NaN, and a huge value never reaches the conversion)
//   zd = depth[f, y, x], wt = weight[f, y, x]; skipped when wt == 0, zd is not finite or zd <= 1e-3
//   d = zd - c_2; skipped when d < -trunc (the point is hidden behind the surface: this frame says nothing about it)
//   t = min(d / trunc, 1) (one IEEE division), q = rint(t * 65536) as int32, in [-65536, 65536]
//   num += (int64) wt * q, den += wt, obs += 1
// The sums are integers: the state after any set of frames is the same bits for every order of the frames and every split of them
// into calls.  |num| <= 255 * 2^16 * frames (int64: never reached); den <= 255 * frames fits in int32 up to 8.4e6 frames.
// The depth and the weight are loaded unconditionally, at pixel 0 of the frame when the point does not project into it (as the hull
// kernel loads its four taps): the loads of consecutive frames then do not wait behind a branch, and the frame loop has no divergent
// control flow at all; a pair that is skipped adds zeros.  No atomics, no LDS, no scratch, no inline assembly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "mesh_raster.h"

namespace dh {

namespace {
constexpr int TS_THREADS = 256;
}

__global__ __launch_bounds__(TS_THREADS) void tsdf_integrate_kernel(const float* __restrict__ pts, int64_t n, const float* __restrict__ depth,
                                                                    const uint8_t* __restrict__ weight, const float* __restrict__ R,
                                                                    const float* __restrict__ T, const float* __restrict__ K, int n_frames,
                                                                    int H, int W, float trunc, int64_t* __restrict__ num,
                                                                    int32_t* __restrict__ den, int32_t* __restrict__ obs) {
    const int64_t i = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
    if (i >= n) return;
    const float px = pts[i * 3 + 0], py = pts[i * 3 + 1], pz = pts[i * 3 + 2];
    const float k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5];
    const float umax = (float)(W - 1), wmax = (float)(H - 1);
    const int64_t HW = (int64_t)H * W;
    int64_t a = num[i];
    int32_t dn = den[i], ob = obs[i];
#pragma unroll 2
    for (int f = 0; f < n_frames; ++f) {
        const Cam c = mk_project(R + (int64_t)f * 9, T + (int64_t)f * 3, k00, k01, k02, k10, k11, k12, px, py, pz);
        const float xf = floorf(c.u + 0.5f), yf = floorf(c.w + 0.5f);
        const bool in = (c.c2 > 1e-3f) & (xf >= 0.f) & (xf <= umax) & (yf >= 0.f) & (yf <= wmax);      // bitwise: no branch
        const int x = in ? (int)xf : 0, y = in ? (int)yf : 0;                                          // inside the frame either way
        const int64_t at = (int64_t)f * HW + (int64_t)y * W + x;
        const float zd = depth[at];
        const int32_t wt = weight[at];
        const float d = zd - c.c2;
        const bool ok = in & (wt != 0) & (fabsf(zd) < INFINITY) & (zd > 1e-3f) & !(d < -trunc);
        const float t = fminf((ok ? d : 0.f) / trunc, 1.f);
        const int32_t q = __float2int_rn(t * 65536.f);
        const int32_t w = ok ? wt : 0;
        a += (int64_t)(w * q);                  // |w q| <= 255 * 65536: the product fits in int32
        dn += w;
        ob += ok;
    }
    num[i] = a;
    den[i] = dn;
    obs[i] = ob;
}

int launch_tsdf_integrate(const float* pts, int64_t n, const float* depth, const uint8_t* weight, const float* R, const float* T,
                          const float* K, int n_frames, int H, int W, float trunc, int64_t* num, int32_t* den, int32_t* obs,
                          hipStream_t st) {
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((n + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, st, pts, n, depth,
                       weight, R, T, K, n_frames, H, W, trunc, num, den, obs);
    return launch_status();
}

}  // namespace dh
