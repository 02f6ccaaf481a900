// Visual hull carving (dynhor_amd/visual_hull.py): the signed pixel distance of every frame's mask, read at the projection of every
// grid point, reduced over the frames to the m largest values per point.
//
// hull_accumulate_kernel<M>: one lane per point, looping over the frames of the chunk; the frame's R, T (and the sequence's K) are
// read at a wave-uniform address (the loop counter alone), so they sit in scalar registers.  Per frame, in fp32:
//   projection: mk_project (mesh_raster.h), the order of dh_mesh_mask_votes
//   seen: c_2 > 1e-6 and 0 <= u <= W - 1 and 0 <= w <= H - 1 (every comparison is false for a NaN)
//   x0 = min(floor(u), W - 2), y0 = min(floor(w), H - 2), fx = u - x0, fy = w - y0 (so the last column / row is read with fx = 1)
//   top = fma(fx, s01 - s00, s00), bot = fma(fx, s11 - s10, s10), val = fma(fy, bot - top, top)
//   g = ((val * c_2) / K00) + 0  (pixels into object units at the point's depth; the + 0 turns a -0 into +0, so that equal values
//   are equal bits and the order of the frames cannot show in the result)
// The four taps are loaded unconditionally (the frame's pixel 0 when the point is not seen) so that the loads of consecutive frames
// do not wait behind a branch; a frame that does not see the point then enters the insertion as -inf, which changes nothing.
// The M largest values live in registers, sorted descending: one max and one min per slot, fully unrolled (M is a template
// parameter: a run-time indexed per-thread array would live in scratch).  arg follows the largest value and prefers the lower frame
// on exactly equal values; together with the sorted insertion every output is a function of the multiset of frames: any split of
// the frames into calls, in any order, gives the same bits.  No atomics, no LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "mesh_raster.h"

namespace dh {

namespace {
constexpr int VH_THREADS = 256;
}

template <int M>
__global__ __launch_bounds__(VH_THREADS) void hull_accumulate_kernel(const float* __restrict__ pts, int64_t n, const float* __restrict__ sd,
                                                                     const float* __restrict__ R, const float* __restrict__ T,
                                                                     const float* __restrict__ K, int n_frames, int H, int W, int frame0,
                                                                     float* __restrict__ topk, int32_t* __restrict__ arg,
                                                                     int32_t* __restrict__ seen) {
    const int64_t i = (int64_t)blockIdx.x * VH_THREADS + threadIdx.x;
    if (i >= n) return;
    const float px = pts[i * 3 + 0], py = pts[i * 3 + 1], pz = pts[i * 3 + 2];
    const float k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5];
    const float umax = (float)(W - 1), wmax = (float)(H - 1), xcap = (float)(W - 2), ycap = (float)(H - 2);
    const int64_t HW = (int64_t)H * W;
    float t[M];
#pragma unroll
    for (int j = 0; j < M; ++j) t[j] = topk[i * M + j];
    int32_t a = arg[i], ns = seen[i];
#pragma unroll 2
    for (int f = 0; f < n_frames; ++f) {
        const Cam c = mk_project(R + (int64_t)f * 9, T + (int64_t)f * 3, k00, k01, k02, k10, k11, k12, px, py, pz);
        const bool in = (c.c2 > 1e-6f) & (c.u >= 0.f) & (c.u <= umax) & (c.w >= 0.f) & (c.w <= wmax);     // bitwise: no branch
        const float x0f = in ? fminf(floorf(c.u), xcap) : 0.f, y0f = in ? fminf(floorf(c.w), ycap) : 0.f;
        const float fx = c.u - x0f, fy = c.w - y0f;
        const float* s = sd + (int64_t)f * HW + (int64_t)(int)y0f * W + (int)x0f;     // H, W >= 2: the four taps lie inside the frame
        const float s00 = s[0], s01 = s[1], s10 = s[W], s11 = s[W + 1];
        const float top = __builtin_fmaf(fx, s01 - s00, s00), bot = __builtin_fmaf(fx, s11 - s10, s10);
        const float val = __builtin_fmaf(fy, bot - top, top);
        const float g = ((val * c.c2) / k00) + 0.f;
        const int32_t fg = frame0 + f;
        ns += in;
        a = (in & ((g > t[0]) | ((g == t[0]) & (fg < a)))) ? fg : a;
        float v = in ? g : -INFINITY;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const float hi = fmaxf(t[j], v), lo = fminf(t[j], v);
            t[j] = hi;
            v = lo;
        }
    }
#pragma unroll
    for (int j = 0; j < M; ++j) topk[i * M + j] = t[j];
    arg[i] = a;
    seen[i] = ns;
}

template <int M>
static int launch_hull_m(const float* pts, int64_t n, const float* sd, const float* R, const float* T, const float* K, int n_frames, int H,
                         int W, int frame0, float* topk, int32_t* arg, int32_t* seen, hipStream_t st) {
    hipLaunchKernelGGL(hull_accumulate_kernel<M>, dim3((unsigned)((n + VH_THREADS - 1) / VH_THREADS)), dim3(VH_THREADS), 0, st, pts, n, sd,
                       R, T, K, n_frames, H, W, frame0, topk, arg, seen);
    return launch_status();
}

int launch_hull_accumulate(const float* pts, int64_t n, const float* sd, const float* R, const float* T, const float* K, int n_frames,
                           int H, int W, int frame0, int m, float* topk, int32_t* arg, int32_t* seen, hipStream_t st) {
    switch (m) {
        case 1: return launch_hull_m<1>(pts, n, sd, R, T, K, n_frames, H, W, frame0, topk, arg, seen, st);
        case 2: return launch_hull_m<2>(pts, n, sd, R, T, K, n_frames, H, W, frame0, topk, arg, seen, st);
        case 3: return launch_hull_m<3>(pts, n, sd, R, T, K, n_frames, H, W, frame0, topk, arg, seen, st);
        case 4: return launch_hull_m<4>(pts, n, sd, R, T, K, n_frames, H, W, frame0, topk, arg, seen, st);
        case 5: return launch_hull_m<5>(pts, n, sd, R, T, K, n_frames, H, W, frame0, topk, arg, seen, st);
        case 6: return launch_hull_m<6>(pts, n, sd, R, T, K, n_frames, H, W, frame0, topk, arg, seen, st);
        case 7: return launch_hull_m<7>(pts, n, sd, R, T, K, n_frames, H, W, frame0, topk, arg, seen, st);
        case 8: return launch_hull_m<8>(pts, n, sd, R, T, K, n_frames, H, W, frame0, topk, arg, seen, st);
    }
    return DH_ERR_BAD_ARG;
}

}  // namespace dh
