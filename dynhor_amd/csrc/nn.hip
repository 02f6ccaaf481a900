// Exact nearest-neighbour squared distance between two point clouds (mesh evaluation: dynhor_amd/metrics.py; Chamfer distance and
// F-score need, for every surface sample of one mesh, its distance to the nearest sample of the other: ~10^6 x 10^6 pairs).
//
// Brute force, every pair, in the direct form d = fma(dz, dz, fma(dy, dy, dx * dx)) with dx = q.x - r.x (fp32, this operation order,
// no expanded |q|^2 - 2 q.r + |r|^2: that form cancels to ~1.5e-8 absolute near a 0.5-radius object, several percent of d at
// distances below 1e-3).  Each lane holds NN_K queries in registers; the workgroup stages the reference points through LDS in tiles
// of float4 and every lane reads the SAME address (a broadcast: no bank conflict), so one ds_read_b128 feeds NN_K queries.
// Determinism: a lane sweeps the references in ascending order with a strict `<`, so it keeps the smallest index among ties -- no
// cross-lane reduction, bitwise the same result on every launch.
// Small query counts (e.g. 37 x 10^6) would leave most CUs idle: the reference range is then cut into S slabs (grid.y), each slab
// writes its (d, idx) pair into the caller's scratch, and nn_merge_kernel takes the lexicographic minimum over the slabs in ascending
// order -- the same pair the one-slab sweep finds, bit for bit.
// The sweep is one body, nn_sweep<XF>: nn_sqdist_kernel is its plain form; icp_correspond_kernel (dynhor_amd/mesh_align.py: the
// correspondence search of similarity ICP) is the same sweep for H hypotheses in grid.z, each transforming the query point on load.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"

namespace dh {

namespace {
constexpr int NN_THREADS = 256;
constexpr int NN_K = 8;                               // queries per lane
constexpr int64_t NN_QPB = NN_THREADS * NN_K;         // queries per workgroup
constexpr int NN_TILE = 1024;                         // reference points per LDS tile (16 KB of float4)
constexpr int NN_UNROLL = 4;
// slab split: aim at this many workgroups (4 per CU on MI355X's 256 CUs) when the queries alone give fewer, but never cut the
// references finer than NN_MIN_SLAB points per slab (a slab's fixed cost -- query loads, one partial store -- stays small)
constexpr int64_t NN_TARGET_BLOCKS = 1024;
constexpr int64_t NN_MIN_SLAB = 8 * NN_TILE;

struct NnPlan {
    int64_t slabs, slab_len;
};

// h: launches of the same sweep side by side (grid.z: the hypotheses of icp_correspond_kernel; 1 for nn_sqdist_kernel)
NnPlan nn_plan(int64_t nq, int64_t nr, int64_t h = 1) {
    const int64_t qb = (nq + NN_QPB - 1) / NN_QPB * h;
    int64_t s = 1;
    if (qb > 0 && qb < NN_TARGET_BLOCKS && nr > 0) {
        s = (NN_TARGET_BLOCKS + qb - 1) / qb;
        const int64_t smax = (nr + NN_MIN_SLAB - 1) / NN_MIN_SLAB;
        s = s < smax ? s : smax;
    }
    if (s <= 1) return {1, nr};
    // tile-aligned slabs; the count actually needed follows from the rounded length
    int64_t len = (nr + s - 1) / s;
    len = (len + NN_TILE - 1) / NN_TILE * NN_TILE;
    return {(nr + len - 1) / len, len};
}
}  // namespace

// The sweep of one workgroup: NN_QPB queries against the references of slab blockIdx.y, [s * slab_len, min(nr, (s + 1) * slab_len)); the
// pairs go to od / oi (oi may be null: distances only).  XF: the query is x = A p + t of the point p read from q, with xf = A row-major
// (9) then t (3), in fp32 and in this order for every row r: x_r = fma(A_r2, p.z, fma(A_r1, p.y, fma(A_r0, p.x, t_r))).  Both kernels
// below are this one body, so a transformed sweep gives the bits nn_sqdist_kernel gives on points transformed by that formula.
template <bool XF>
__device__ __forceinline__ void nn_sweep(float4* __restrict__ tile, const float* __restrict__ q, int64_t nq, const float* __restrict__ ref,
                                         int64_t nr, int64_t slab_len, const float* __restrict__ xf, float* __restrict__ od,
                                         int32_t* __restrict__ oi) {
    const int t = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * NN_QPB + t;
    float qx[NN_K], qy[NN_K], qz[NN_K], best[NN_K];
    int bi[NN_K];
#pragma unroll
    for (int k = 0; k < NN_K; ++k) {
        const int64_t i = q0 + (int64_t)k * NN_THREADS;
        const bool in = i < nq;
        qx[k] = in ? q[i * 3 + 0] : 0.f;
        qy[k] = in ? q[i * 3 + 1] : 0.f;
        qz[k] = in ? q[i * 3 + 2] : 0.f;
        if (XF) {
            const float px = qx[k], py = qy[k], pz = qz[k];
            qx[k] = __builtin_fmaf(xf[2], pz, __builtin_fmaf(xf[1], py, __builtin_fmaf(xf[0], px, xf[9])));
            qy[k] = __builtin_fmaf(xf[5], pz, __builtin_fmaf(xf[4], py, __builtin_fmaf(xf[3], px, xf[10])));
            qz[k] = __builtin_fmaf(xf[8], pz, __builtin_fmaf(xf[7], py, __builtin_fmaf(xf[6], px, xf[11])));
        }
        best[k] = INFINITY;
        bi[k] = -1;
    }
    const int64_t r0 = (int64_t)blockIdx.y * slab_len;
    const int64_t r1 = r0 + slab_len < nr ? r0 + slab_len : nr;
    for (int64_t base = r0; base < r1; base += NN_TILE) {
        const int64_t left = r1 - base;
        __syncthreads();                                          // the previous tile has been read by every wave
        for (int j = t; j < NN_TILE; j += NN_THREADS) {
            const int64_t g = base + j;
            // past the slab end: +inf coordinates, whose distance (+inf, or NaN for a non-finite query) never passes the strict `<`
            tile[j] = g < r1 ? make_float4(ref[g * 3 + 0], ref[g * 3 + 1], ref[g * 3 + 2], 0.f)
                             : make_float4(INFINITY, INFINITY, INFINITY, 0.f);
        }
        __syncthreads();
        const int n = left < NN_TILE ? (int)((left + NN_UNROLL - 1) / NN_UNROLL * NN_UNROLL) : NN_TILE;
        const int jb = (int)base;                                 // nr < 2^31 (api.hip)
        for (int j = 0; j < n; j += NN_UNROLL) {
#pragma unroll
            for (int u = 0; u < NN_UNROLL; ++u) {
                const float4 r = tile[j + u];
#pragma unroll
                for (int k = 0; k < NN_K; ++k) {
                    const float dx = qx[k] - r.x, dy = qy[k] - r.y, dz = qz[k] - r.z;
                    const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                    if (d < best[k]) {
                        best[k] = d;
                        bi[k] = jb + j + u;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NN_K; ++k) {
        const int64_t i = q0 + (int64_t)k * NN_THREADS;
        if (i < nq) {
            od[i] = best[k];
            if (oi) oi[i] = bi[k];
        }
    }
}

// grid (query blocks, slabs).  Slab s writes its pairs at d2 + s * out_stride / idx + s * out_stride (idx may be null).
__global__ __launch_bounds__(NN_THREADS) void nn_sqdist_kernel(const float* __restrict__ q, int64_t nq, const float* __restrict__ ref,
                                                               int64_t nr, int64_t slab_len, float* __restrict__ d2,
                                                               int32_t* __restrict__ idx, int64_t out_stride) {
    __shared__ float4 tile[NN_TILE];
    nn_sweep<false>(tile, q, nq, ref, nr, slab_len, nullptr, d2 + (int64_t)blockIdx.y * out_stride,
                    idx ? idx + (int64_t)blockIdx.y * out_stride : nullptr);
}

// ICP correspondences (dynhor_amd/mesh_align.py): grid (source blocks, slabs, hypotheses).  Hypothesis h transforms the source by
// xf + 12 h on load and writes slab s at d2 + (h * gridDim.y + s) * n (one slab: the caller's [H,N] arrays themselves).
__global__ __launch_bounds__(NN_THREADS) void icp_correspond_kernel(const float* __restrict__ src, int64_t n, const float* __restrict__ tgt,
                                                                    int64_t m, int64_t slab_len, const float* __restrict__ xf,
                                                                    float* __restrict__ d2, int32_t* __restrict__ idx) {
    __shared__ float4 tile[NN_TILE];
    const int64_t o = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * n;
    nn_sweep<true>(tile, src, n, tgt, m, slab_len, xf + 12 * (int64_t)blockIdx.z, d2 + o, idx + o);
}

// lexicographic minimum of the slabs' (d, idx) pairs, slabs in ascending order with a strict `<`: ties keep the lower slab, whose
// indices are the smaller ones
__global__ __launch_bounds__(256) void nn_merge_kernel(const float* __restrict__ pd, const int32_t* __restrict__ pi, int64_t nq, int slabs,
                                                       float* __restrict__ d2, int32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    // blockIdx.y: the hypothesis of an ICP launch (its slabs lie together); 0 for dh_nearest_sqdist
    pd += (int64_t)blockIdx.y * slabs * nq;
    pi += (int64_t)blockIdx.y * slabs * nq;
    float b = pd[i];
    int32_t bi = pi[i];
    for (int s = 1; s < slabs; ++s) {
        const float d = pd[(int64_t)s * nq + i];
        if (d < b) {
            b = d;
            bi = pi[(int64_t)s * nq + i];
        }
    }
    d2[(int64_t)blockIdx.y * nq + i] = b;
    if (idx) idx[(int64_t)blockIdx.y * nq + i] = bi;
}

int64_t nearest_sqdist_workspace(int64_t nq, int64_t nr) {
    const NnPlan p = nn_plan(nq, nr);
    return p.slabs > 1 ? p.slabs * nq * (int64_t)(sizeof(float) + sizeof(int32_t)) : 0;
}

int launch_nearest_sqdist(const float* q, int64_t nq, const float* ref, int64_t nr, float* d2, int32_t* idx, void* ws, hipStream_t st) {
    const int64_t qb = (nq + NN_QPB - 1) / NN_QPB;
    const NnPlan p = ws ? nn_plan(nq, nr) : NnPlan{1, nr};
    if (p.slabs == 1) {
        hipLaunchKernelGGL(nn_sqdist_kernel, dim3((unsigned)qb, 1), dim3(NN_THREADS), 0, st, q, nq, ref, nr, nr, d2, idx, (int64_t)0);
        return launch_status();
    }
    // scratch: the slabs' distances [slabs, nq] floats, then their indices [slabs, nq] int32
    float* pd = static_cast<float*>(ws);
    int32_t* pi = reinterpret_cast<int32_t*>(pd + p.slabs * nq);
    hipLaunchKernelGGL(nn_sqdist_kernel, dim3((unsigned)qb, (unsigned)p.slabs), dim3(NN_THREADS), 0, st, q, nq, ref, nr, p.slab_len, pd,
                       pi, nq);
    if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, pd, pi, nq, (int)p.slabs, d2, idx);
    return launch_status();
}

int64_t icp_correspond_workspace(int64_t n, int64_t m, int64_t h) {
    const NnPlan p = nn_plan(n, m, h);
    return p.slabs > 1 ? h * p.slabs * n * (int64_t)(sizeof(float) + sizeof(int32_t)) : 0;
}

int launch_icp_correspond(const float* src, int64_t n, const float* tgt, int64_t m, const float* xf, int64_t h, float* d2, int32_t* idx,
                          void* ws, hipStream_t st) {
    const int64_t qb = (n + NN_QPB - 1) / NN_QPB;
    const NnPlan p = ws ? nn_plan(n, m, h) : NnPlan{1, m};
    if (p.slabs == 1) {
        hipLaunchKernelGGL((icp_correspond_kernel), dim3((unsigned)qb, 1, (unsigned)h), dim3(NN_THREADS), 0, st, src, n, tgt, m, m, xf, d2,
                           idx);
        return launch_status();
    }
    // scratch: the slabs' distances [h, slabs, n] floats, then their indices [h, slabs, n] int32
    float* pd = static_cast<float*>(ws);
    int32_t* pi = reinterpret_cast<int32_t*>(pd + h * p.slabs * n);
    hipLaunchKernelGGL((icp_correspond_kernel), dim3((unsigned)qb, (unsigned)p.slabs, (unsigned)h), dim3(NN_THREADS), 0, st, src, n, tgt, m,
                       p.slab_len, xf, pd, pi);
    if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)h), dim3(256), 0, st, pd, pi, n, (int)p.slabs, d2, idx);
    return launch_status();
}

}  // namespace dh
