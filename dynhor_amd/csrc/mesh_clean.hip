// Mesh cleaning (dynhor_amd/mesh_clean.py): silhouette culling against the per-frame label maps, and connected components.
//
// label_dilate_*: keep[f,y,x] = 1 where a (2r+1)^2 window, clipped to the image, holds a label != 0 (object OR hand: a hand pixel
// hides what lies behind it, so it never votes "background").  Two separable passes (rows into the caller's tmp, then columns).
//
// mesh_votes_kernel: one thread per vertex, looping over the frames; the frame's R, T (and the sequence's K) are read at a
// wave-uniform address.  Projection: mk_project (mesh_raster.h), for every vertex and frame.
//   seen: c_2 > 0 and (floor(u + 0.5), floor(w + 0.5)) inside the image, range-checked as floats before any integer conversion
// The label byte is loaded unconditionally (pixel 0 of the frame when the vertex is not seen) so that the loads of consecutive frames
// do not wait behind a branch.  Counts are integers: bitwise reproducible.
//
// Components: lock-free union-find on labels[] (the parent array).  uf_union_kernel, one thread per face, unites (a,b) and (a,c),
// always hooking the larger root under the smaller one by an agent-scope compare-exchange.  MI355X's eight XCD L2s are not coherent
// with one another for plain stores, so inside that launch every access of the parent array is an agent-scope atomic -- the path
// halving of find() included, done as a compare-exchange that only ever moves a pointer to an ancestor.  Every parent is smaller than
// its child, so each tree's root is the smallest index of its component.  uf_jump_kernel then resolves every vertex to its root by
// pointer jumping, after the kernel boundary, with plain accesses: ceil(log2 nv) launches bound any depth (a 10^6-vertex path
// included); a read that sees another lane's newer pointer only jumps further towards the same root.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "mesh_raster.h"

namespace dh {

namespace {
constexpr int MC_THREADS = 256;

__device__ inline int32_t uf_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline bool uf_cas(int32_t* p, int32_t expected, int32_t desired) {
    return __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline int32_t uf_find(int32_t* par, int32_t x) {
    while (true) {
        const int32_t p = uf_load(par + x);
        if (p == x) return x;
        const int32_t gp = uf_load(par + p);
        if (gp == p) return p;
        uf_cas(par + x, p, gp);                              // path halving; a failed exchange means another lane moved it further
        x = gp;
    }
}

__device__ inline void uf_unite(int32_t* par, int32_t a, int32_t b) {
    while (true) {
        a = uf_find(par, a);
        b = uf_find(par, b);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (uf_cas(par + hi, hi, lo)) return;
        a = hi;                                              // hi was hooked meanwhile: find both roots again
        b = lo;
    }
}
}  // namespace

// grid (n_frames * H image rows, column blocks): no 64-bit division per pixel
__global__ __launch_bounds__(MC_THREADS) void label_dilate_rows_kernel(const int8_t* __restrict__ label, int W, int r,
                                                                        uint8_t* __restrict__ tmp) {
    const int x = (int)blockIdx.y * MC_THREADS + threadIdx.x;
    if (x >= W) return;
    const int64_t row = (int64_t)blockIdx.x * W;
    const int x0 = x - r > 0 ? x - r : 0, x1 = x < W - 1 - r ? x + r : W - 1;
    uint8_t any = 0;
    for (int xx = x0; xx <= x1; ++xx) any |= label[row + xx] != 0;
    tmp[row + x] = any;
}

__global__ __launch_bounds__(MC_THREADS) void label_dilate_cols_kernel(const uint8_t* __restrict__ tmp, int H, int W, int r,
                                                                        uint8_t* __restrict__ keep) {
    const int x = (int)blockIdx.y * MC_THREADS + threadIdx.x;
    if (x >= W) return;
    const int y = (int)(blockIdx.x % (unsigned)H);
    const int64_t col = ((int64_t)blockIdx.x - y) * W + x;   // this frame's row 0, this column
    const int y0 = y - r > 0 ? y - r : 0, y1 = y < H - 1 - r ? y + r : H - 1;
    uint8_t any = 0;
    for (int yy = y0; yy <= y1; ++yy) any |= tmp[col + (int64_t)yy * W];
    keep[col + (int64_t)y * W] = any;
}

__global__ __launch_bounds__(MC_THREADS) void mesh_votes_kernel(const float* __restrict__ verts, int64_t nv, const uint8_t* __restrict__ keep,
                                                                const float* __restrict__ R, const float* __restrict__ T,
                                                                const float* __restrict__ K, int64_t n_frames, int H, int W,
                                                                int32_t* __restrict__ bg_votes, int32_t* __restrict__ seen) {
    const int64_t i = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= nv) return;
    const float vx = verts[i * 3 + 0], vy = verts[i * 3 + 1], vz = verts[i * 3 + 2];
    const float k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5];
    const float fw = (float)W, fh = (float)H;
    const int64_t HW = (int64_t)H * W;
    int32_t nb = 0, ns = 0;
#pragma unroll 4
    for (int64_t f = 0; f < n_frames; ++f) {
        const float* Rf = R + f * 9;
        const float* Tf = T + f * 3;
        const Cam c = mk_project(Rf, Tf, k00, k01, k02, k10, k11, k12, vx, vy, vz);
        const float px = floorf(c.u + 0.5f), py = floorf(c.w + 0.5f);
        // every comparison is false for a NaN: a vertex with z ~ 0 (u, w huge, infinite or NaN) is not seen
        const bool in = (c.c2 > 0.f) & (px >= 0.f) & (px < fw) & (py >= 0.f) & (py < fh);     // bitwise: no branch
        const int64_t pix = in ? (int64_t)(int)py * W + (int)px : 0;
        const uint8_t k = keep[f * HW + pix];
        ns += in;
        nb += in & (k == 0);
    }
    bg_votes[i] = nb;
    seen[i] = ns;
}

__global__ __launch_bounds__(MC_THREADS) void uf_init_kernel(int32_t* __restrict__ par, int64_t nv) {
    for (int64_t i = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * MC_THREADS) par[i] = (int32_t)i;
}

__global__ __launch_bounds__(MC_THREADS) void uf_union_kernel(const int64_t* __restrict__ faces, int64_t nf, int64_t nv, int32_t* par) {
    for (int64_t i = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x; i < nf; i += (int64_t)gridDim.x * MC_THREADS) {
        int64_t a, b, c;
        if (!mk_face_in_range(faces, i, nv, a, b, c)) continue;     // a bad index never reaches the parent array
        uf_unite(par, (int32_t)a, (int32_t)b);
        uf_unite(par, (int32_t)a, (int32_t)c);
    }
}

__global__ __launch_bounds__(MC_THREADS) void uf_jump_kernel(int32_t* par, int64_t nv) {
    for (int64_t i = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * MC_THREADS) {
        const int32_t p = par[i];
        par[i] = par[p];
    }
}

int launch_label_dilate(const int8_t* label, int64_t n_frames, int H, int W, int radius, uint8_t* tmp, uint8_t* keep, hipStream_t st) {
    const dim3 grid((unsigned)(n_frames * H), (unsigned)((W + MC_THREADS - 1) / MC_THREADS));   // api.hip: n_frames * H < 2^31
    hipLaunchKernelGGL(label_dilate_rows_kernel, grid, dim3(MC_THREADS), 0, st, label, W, radius, tmp);
    if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    hipLaunchKernelGGL(label_dilate_cols_kernel, grid, dim3(MC_THREADS), 0, st, tmp, H, W, radius, keep);
    return launch_status();
}

int launch_mesh_mask_votes(const float* verts, int64_t nv, const uint8_t* keep, const float* R, const float* T, const float* K,
                           int64_t n_frames, int H, int W, int32_t* bg_votes, int32_t* seen, hipStream_t st) {
    hipLaunchKernelGGL(mesh_votes_kernel, dim3((unsigned)((nv + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, st, verts, nv, keep,
                       R, T, K, n_frames, H, W, bg_votes, seen);
    return launch_status();
}

int launch_mesh_components(const int64_t* faces, int64_t nf, int64_t nv, int32_t* labels, hipStream_t st) {
    hipLaunchKernelGGL(uf_init_kernel, dim3(grid_1d(nv, MC_THREADS)), dim3(MC_THREADS), 0, st, labels, nv);
    if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    if (nf > 0) {
        hipLaunchKernelGGL(uf_union_kernel, dim3(grid_1d(nf, MC_THREADS)), dim3(MC_THREADS), 0, st, faces, nf, nv, labels);
        if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    }
    // after k jumps every pointer is min(2^k, distance to the root) steps up; a tree holds at most nv - 1 edges
    for (int64_t reach = 1; reach < nv - 1; reach *= 2) {
        hipLaunchKernelGGL(uf_jump_kernel, dim3(grid_1d(nv, MC_THREADS)), dim3(MC_THREADS), 0, st, labels, nv);
        if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    }
    return 0;
}

}  // namespace dh
