// Mesh colouring (dynhor_amd/mesh_color.py): a z-buffer of the mesh in every frame, then per-vertex colours gathered from the
// frames that see the vertex.
//
// mesh_raster_kernel: the face walker of mesh_raster.h (which states the projection, the skip rule, the coverage rule and the wave
// phase) with mk_pixel as its per-pixel operation.  Perspective-correct depth of a covered pixel centre:
//   z = (e0 + e1 + e2) / fma(e2, 1/z2, fma(e1, 1/z1, e0 * (1/z0)))
// (normalised by the sum of the three edge values, so z is a weighted harmonic mean of z0, z1, z2 whatever the rounding).  The key
// (float_bits(z) << 32) | face goes in by a 64-bit agent-scope atomic minimum: z > 0, so the bits order as the depths do; the
// minimum does not depend on the order of arrival, so the buffer is bitwise reproducible, and on a depth tie the smaller face wins.
//
// mesh_bake_kernel: one thread per vertex, looping over the frames in ascending order and adding onto the caller's acc / n_views
// (read once, written once: a fixed sequential fp32 sum per vertex, no float atomics).  A frame contributes when c_2 > 1e-3, the
// nearest pixel (floor(u + 0.5), floor(w + 0.5)) lies in the image (range-checked as floats), usable[pixel] != 0, mk_view sees the
// vertex through the z-buffer's key at that pixel (mesh_shade.h states the depth test and cos = <n, d> / |d|, d = C - v the direction
// to the camera centre; dh_texture_bake shares it), and cos >= min_cos:
//   acc.rgb = fma(cos, rgb / 255, acc.rgb),  acc.w += cos,  n_views += 1
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "mesh_shade.h"

namespace dh {

namespace {
struct MkDepth {
    static constexpr int N = 9;
    static constexpr bool FACE_TEST = false;
    __device__ __forceinline__ void pixel(const Tri<9>& t, int x, int y, uint32_t face, uint64_t* zrow) const {
        float e0, e1, e2;
        if (!mk_covers(t, (float)x, (float)y, e0, e1, e2)) return;
        const float z = (e0 + e1 + e2) / __builtin_fmaf(e2, t.iz[2], __builtin_fmaf(e1, t.iz[1], e0 * t.iz[0]));
        const uint64_t key = ((uint64_t)__float_as_uint(z) << 32) | face;
        __hip_atomic_fetch_min(zrow + x, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
}  // namespace

__global__ __launch_bounds__(MK_THREADS) void mesh_raster_kernel(const float* __restrict__ verts, int64_t nv,
                                                                 const int64_t* __restrict__ faces, int64_t nf,
                                                                 const float* __restrict__ R, const float* __restrict__ T,
                                                                 const float* __restrict__ K, int64_t n_frames, int H, int W,
                                                                 uint64_t* zbuf) {
    mk_walk_faces(verts, nv, faces, nf, R, T, K, n_frames, H, W, 0.f, zbuf, MkDepth{});
}

__global__ __launch_bounds__(MK_THREADS) void mesh_bake_kernel(const float* __restrict__ verts, const float* __restrict__ normals,
                                                               int64_t nv, const uint8_t* __restrict__ rgb,
                                                               const uint8_t* __restrict__ usable, const uint64_t* __restrict__ zbuf,
                                                               const float* __restrict__ R, const float* __restrict__ T,
                                                               const float* __restrict__ K, int64_t n_frames, int H, int W,
                                                               float depth_eps, float min_cos, float* __restrict__ acc,
                                                               int32_t* __restrict__ n_views) {
    const int64_t i = (int64_t)blockIdx.x * MK_THREADS + threadIdx.x;
    if (i >= nv) return;
    const float vx = verts[i * 3 + 0], vy = verts[i * 3 + 1], vz = verts[i * 3 + 2];
    const float nx = normals[i * 3 + 0], ny = normals[i * 3 + 1], nz = normals[i * 3 + 2];
    const float k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5];
    const float fw = (float)W, fh = (float)H;
    const int64_t HW = (int64_t)H * W;
    float ar = acc[i * 4 + 0], ag = acc[i * 4 + 1], ab = acc[i * 4 + 2], aw = acc[i * 4 + 3];
    int32_t cnt = n_views[i];
    for (int64_t f = 0; f < n_frames; ++f) {
        const float* Rf = R + f * 9;
        const float* Tf = T + f * 3;
        const Cam c = mk_project(Rf, Tf, k00, k01, k02, k10, k11, k12, vx, vy, vz);
        const float px = floorf(c.u + 0.5f), py = floorf(c.w + 0.5f);
        const bool in = (c.c2 > 1e-3f) & (px >= 0.f) & (px < fw) & (py >= 0.f) & (py < fh);
        const int64_t pix = f * HW + (in ? (int64_t)(int)py * W + (int)px : 0);
        const uint8_t us = usable[pix];
        const View v = mk_view(zbuf[pix], c.c2, depth_eps, Rf, Tf, vx, vy, vz, nx, ny, nz);
        const float cs = v.cos;
        if (in & (us != 0) & v.seen & (cs >= min_cos)) {
            ar = __builtin_fmaf(cs, (float)rgb[pix * 3 + 0] / 255.f, ar);
            ag = __builtin_fmaf(cs, (float)rgb[pix * 3 + 1] / 255.f, ag);
            ab = __builtin_fmaf(cs, (float)rgb[pix * 3 + 2] / 255.f, ab);
            aw += cs;
            cnt += 1;
        }
    }
    acc[i * 4 + 0] = ar;
    acc[i * 4 + 1] = ag;
    acc[i * 4 + 2] = ab;
    acc[i * 4 + 3] = aw;
    n_views[i] = cnt;
}

int launch_mesh_raster_depth(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R, const float* T,
                             const float* K, int64_t n_frames, int H, int W, uint64_t* zbuf, hipStream_t st) {
    hipLaunchKernelGGL(mesh_raster_kernel, dim3(grid_1d(n_frames * nf, MK_THREADS)), dim3(MK_THREADS), 0, st, verts, nv, faces, nf, R, T, K,
                       n_frames, H, W, zbuf);
    return launch_status();
}

int launch_mesh_bake_colors(const float* verts, const float* normals, int64_t nv, const uint8_t* rgb, const uint8_t* usable,
                            const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                            float depth_eps, float min_cos, float* acc, int32_t* n_views, hipStream_t st) {
    hipLaunchKernelGGL(mesh_bake_kernel, dim3((unsigned)((nv + MK_THREADS - 1) / MK_THREADS)), dim3(MK_THREADS), 0, st, verts, normals,
                       nv, rgb, usable, zbuf, R, T, K, n_frames, H, W, depth_eps, min_cos, acc, n_views);
    return launch_status();
}

}  // namespace dh
