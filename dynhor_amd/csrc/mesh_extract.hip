// Block-sparse marching cubes (dynhor_amd/mesh_extract.py; the rules are in include/dynhor_hip.h): only the blocks of B^3 cells that can
// hold a crossing are sampled, at their (B+1)^3 grid points, and each is triangulated by one workgroup of 256 threads.
//   mc_block_points_kernel: one thread per sample, coordinates READ from the caller's axis arrays (the dense grid's bits).
//   mc_count_kernel / mc_emit_kernel: v = u - threshold staged in LDS ((B+1)^3 floats, dynamic: 2.9 KB at B = 8, 19.6 KB at B = 16);
//   thread t owns the cells [t c, (t + 1) c) of the B^3 cells in (i, j, k) order, c = ceil(B^3 / 256); case bit n = v(corner n) > 0 in
//   mesh.py's corner order; the table is the caller's u8 [256,16].  count: triangles per block (wave shuffles, four partial sums in
//   LDS), the non-finite flag, the cut faces towards culled blocks (one integer atomic per block).  emit: an exclusive scan of the
//   per-thread counts places every triangle at offsets[block] + (triangles of the earlier cells): no atomics.
// A triangle corner lies on a cube edge whose lower end g and axis are packed five bits per edge into EDGE_CODES from mesh.py's corner /
// edge lists.  t = min(max(v0 / (v0 - v1), 0), 1) with IEEE division, pos = g with t added along the axis: the bits of the dense
// p0 + t * (p1 - p0), p1 - p0 being a unit vector.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"

namespace dh {

namespace {
constexpr int MX_THREADS = 256;
constexpr int MX_WAVES = MX_THREADS / 64;

// corner n -> (x, y, z) offsets and edge e -> its two corners: the numbering of dynhor_amd/mesh.py (_MC_CORNERS, _MC_EDGES)
constexpr int CORNER_XYZ[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
constexpr int EDGE_ENDS[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};

// five bits per edge: x | y << 1 | z << 2 of the lower end, key axis << 3 (0 = along z, 1 = along y, 2 = along x)
constexpr uint64_t edge_codes() {
    uint64_t all = 0;
    for (int e = 0; e < 12; ++e) {
        const int a = EDGE_ENDS[e][0], b = EDGE_ENDS[e][1];
        uint64_t code = 0;
        int axis = 0;
        for (int d = 0; d < 3; ++d) {
            const int lo = CORNER_XYZ[a][d] < CORNER_XYZ[b][d] ? CORNER_XYZ[a][d] : CORNER_XYZ[b][d];
            code |= (uint64_t)lo << d;
            if (CORNER_XYZ[a][d] != CORNER_XYZ[b][d]) axis = 2 - d;
        }
        all |= (code | (uint64_t)axis << 3) << (5 * e);
    }
    return all;
}
constexpr uint64_t EDGE_CODES = edge_codes();

struct BlockGeom {
    int bx, by, bz;      // block coordinates
    int ex, ey, ez;      // cells of the block along each axis (B, fewer in a clipped end block, 0 for a block outside the grid)
};

__device__ inline BlockGeom block_geom(const int32_t* __restrict__ blocks, int64_t b, int N, int B, int nbk) {
    BlockGeom g;
    g.bx = blocks[b * 3 + 0]; g.by = blocks[b * 3 + 1]; g.bz = blocks[b * 3 + 2];
    const bool ok = g.bx >= 0 && g.bx < nbk && g.by >= 0 && g.by < nbk && g.bz >= 0 && g.bz < nbk;
    const int rx = N - 1 - g.bx * B, ry = N - 1 - g.by * B, rz = N - 1 - g.bz * B;
    g.ex = ok ? (rx < B ? rx : B) : 0;
    g.ey = ok ? (ry < B ? ry : B) : 0;
    g.ez = ok ? (rz < B ? rz : B) : 0;
    return g;
}

// stages v = u - threshold of one block; returns whether this thread saw a non-finite u
__device__ inline bool stage_block(const float* __restrict__ vals, int P3, float threshold, float* s) {
    bool bad = false;
    for (int i = threadIdx.x; i < P3; i += MX_THREADS) {
        const float u = vals[i];
        bad |= !(fabsf(u) <= 3.402823466e38f);                // NaN compares false
        s[i] = u - threshold;
    }
    return bad;
}

__device__ inline int cell_case(const float* s, int P, int li, int lj, int lk) {
    const int o = (li * P + lj) * P + lk, sx = P * P, sy = P;
    return (int)(s[o] > 0.f) | (int)(s[o + sx] > 0.f) << 1 | (int)(s[o + sx + sy] > 0.f) << 2 | (int)(s[o + sy] > 0.f) << 3 |
           (int)(s[o + 1] > 0.f) << 4 | (int)(s[o + sx + 1] > 0.f) << 5 | (int)(s[o + sx + sy + 1] > 0.f) << 6 |
           (int)(s[o + sy + 1] > 0.f) << 7;
}

// triangles of cell c of the block (0 for a cell outside the clipped extent); *cs = its case
__device__ inline int cell_triangles(const float* s, const uint8_t* __restrict__ table, const BlockGeom& g, int B, int c, int* cs) {
    const int li = c / (B * B), lj = (c / B) % B, lk = c % B;
    *cs = 0;
    if (li >= g.ex || lj >= g.ey || lk >= g.ez) return 0;
    *cs = cell_case(s, B + 1, li, lj, lk);
    const int n = table[*cs * 16 + 15];
    return n < 5 ? n : 5;                                     // (a row holds five triangles: a bad table never reads past it)
}

__device__ inline int wave_sum(int v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
}  // namespace

__global__ __launch_bounds__(MX_THREADS) void mc_block_points_kernel(const float* __restrict__ ax, const float* __restrict__ ay,
                                                                      const float* __restrict__ az, int N, const int32_t* __restrict__ blocks,
                                                                      int64_t n_pts, int B, float* __restrict__ pts) {
    const int P = B + 1, P3 = P * P * P;
    for (int64_t i = (int64_t)blockIdx.x * MX_THREADS + threadIdx.x; i < n_pts; i += (int64_t)gridDim.x * MX_THREADS) {
        const int64_t b = i / P3;
        const int l = (int)(i - b * P3);
        int gx = blocks[b * 3 + 0] * B + l / (P * P), gy = blocks[b * 3 + 1] * B + (l / P) % P, gz = blocks[b * 3 + 2] * B + l % P;
        gx = gx < 0 ? 0 : (gx > N - 1 ? N - 1 : gx);
        gy = gy < 0 ? 0 : (gy > N - 1 ? N - 1 : gy);
        gz = gz < 0 ? 0 : (gz > N - 1 ? N - 1 : gz);
        pts[i * 3 + 0] = ax[gx];
        pts[i * 3 + 1] = ay[gy];
        pts[i * 3 + 2] = az[gz];
    }
}

__global__ __launch_bounds__(MX_THREADS) void mc_count_kernel(const float* __restrict__ vals, const int32_t* __restrict__ blocks, int N, int B,
                                                               float threshold, const uint8_t* __restrict__ table,
                                                               const int32_t* __restrict__ block_map, int32_t* __restrict__ counts,
                                                               int32_t* cut_faces, int32_t* nonfinite) {
    extern __shared__ float s[];
    __shared__ int part[2][MX_WAVES];
    const int P = B + 1, P3 = P * P * P, nbk = (N - 2) / B + 1;
    const int64_t b = blockIdx.x;
    const BlockGeom g = block_geom(blocks, b, N, B, nbk);
    const bool bad = stage_block(vals + b * P3, P3, threshold, s);
    __syncthreads();
    // triangles
    const int cells = B * B * B, per = (cells + MX_THREADS - 1) / MX_THREADS;
    int ntri = 0;
    for (int c = threadIdx.x * per; c < (threadIdx.x + 1) * per && c < cells; ++c) {
        int cs;
        ntri += cell_triangles(s, table, g, B, c, &cs);
    }
    // cut faces on the six sides: side = 2 axis + (1 for the far side); (a, b) run over the two other axes in x < y < z order
    int ncut = 0;
    for (int f = threadIdx.x; f < 6 * B * B; f += MX_THREADS) {
        const int side = f / (B * B), a = (f / B) % B, c = f % B, axis = side >> 1, far = side & 1;
        const int nx = g.bx + (axis == 0 ? 2 * far - 1 : 0), ny = g.by + (axis == 1 ? 2 * far - 1 : 0), nz = g.bz + (axis == 2 ? 2 * far - 1 : 0);
        if (nx < 0 || nx >= nbk || ny < 0 || ny >= nbk || nz < 0 || nz >= nbk) continue;       // the grid's own boundary
        const int ea = axis == 0 ? g.ey : g.ex, ec = axis == 2 ? g.ey : g.ez;
        if (a >= ea || c >= ec || g.ex == 0) continue;
        // (a far neighbour inside the grid means this block is not clipped along the axis: its far plane is sample index B)
        const int p = far ? B : 0;
        const int li = axis == 0 ? p : a, lj = axis == 1 ? p : (axis == 0 ? a : c), lk = axis == 2 ? p : c;
        const int sa = axis == 0 ? P : P * P, sc = axis == 2 ? P : 1;                           // strides of the face's two axes
        const int o = (li * P + lj) * P + lk;
        const int in = (int)(s[o] > 0.f) + (int)(s[o + sa] > 0.f) + (int)(s[o + sc] > 0.f) + (int)(s[o + sa + sc] > 0.f);
        if (in == 0 || in == 4) continue;
        ncut += block_map[((int64_t)nx * nbk + ny) * nbk + nz] < 0;
    }
    ntri = wave_sum(ntri);
    ncut = wave_sum(ncut);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { part[0][wave] = ntri; part[1][wave] = ncut; }
    if (__any(bad) && lane == 0) atomicOr(nonfinite, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0, k = 0;
        for (int w = 0; w < MX_WAVES; ++w) { t += part[0][w]; k += part[1][w]; }
        counts[b] = t;
        if (k) atomicAdd(cut_faces, k);
    }
}

__global__ __launch_bounds__(MX_THREADS) void mc_emit_kernel(const float* __restrict__ vals, const int32_t* __restrict__ blocks, int N, int B,
                                                              float threshold, const uint8_t* __restrict__ table,
                                                              const int64_t* __restrict__ offsets, int64_t n_tri,
                                                              int64_t* __restrict__ keys, float* __restrict__ pos) {
    extern __shared__ float s[];
    __shared__ int part[MX_WAVES];
    const int P = B + 1, P3 = P * P * P, nbk = (N - 2) / B + 1;
    const int64_t b = blockIdx.x;
    const BlockGeom g = block_geom(blocks, b, N, B, nbk);
    stage_block(vals + b * P3, P3, threshold, s);
    __syncthreads();
    const int cells = B * B * B, per = (cells + MX_THREADS - 1) / MX_THREADS;
    const int c0 = threadIdx.x * per, c1 = (c0 + per < cells) ? c0 + per : cells;
    int mine = 0;
    for (int c = c0; c < c1; ++c) {
        int cs;
        mine += cell_triangles(s, table, g, B, c, &cs);
    }
    // exclusive scan of `mine` over the workgroup: inclusive within the wave, then the earlier waves' totals
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    int before = incl - mine;
    for (int w = 0; w < MX_WAVES; ++w) before += w < wave ? part[w] : 0;
    if (mine == 0) return;
    int64_t tri = offsets[b] + before;
    for (int c = c0; c < c1; ++c) {
        int cs;
        const int n = cell_triangles(s, table, g, B, c, &cs);
        const int li = c / (B * B), lj = (c / B) % B, lk = c % B;
        for (int t = 0; t < n; ++t, ++tri) {
            if (tri >= n_tri) return;                         // (offsets that do not belong to these values: never write past the output)
            for (int k = 0; k < 3; ++k) {
                const int e = table[cs * 16 + t * 3 + k];
                const int code = (int)(EDGE_CODES >> (5 * (e < 12 ? e : 0))) & 31, axis = code >> 3;
                const int ci = li + (code & 1), cj = lj + (code >> 1 & 1), ck = lk + (code >> 2 & 1);
                const int o = (ci * P + cj) * P + ck;
                const float v0 = s[o], v1 = s[o + (axis == 2 ? P * P : (axis == 1 ? P : 1))];
                const float t01 = fminf(fmaxf(v0 / (v0 - v1), 0.f), 1.f);
                const int gx = g.bx * B + ci, gy = g.by * B + cj, gz = g.bz * B + ck;
                const int64_t row = tri * 3 + k;
                keys[row] = (((int64_t)gx * N + gy) * N + gz) * 3 + axis;
                pos[row * 3 + 0] = (float)gx + (axis == 2 ? t01 : 0.f);
                pos[row * 3 + 1] = (float)gy + (axis == 1 ? t01 : 0.f);
                pos[row * 3 + 2] = (float)gz + (axis == 0 ? t01 : 0.f);
            }
        }
    }
}

int launch_mc_block_points(const float* ax, const float* ay, const float* az, int N, const int32_t* blocks, int64_t nb, int B, float* pts,
                           hipStream_t st) {
    const int P = B + 1;
    const int64_t n_pts = nb * P * P * P, wg = (n_pts + MX_THREADS - 1) / MX_THREADS;
    hipLaunchKernelGGL(mc_block_points_kernel, dim3((unsigned)(wg < (1 << 20) ? wg : (1 << 20))), dim3(MX_THREADS), 0, st, ax, ay, az, N,
                       blocks, n_pts, B, pts);
    return launch_status();
}

int launch_mc_count(const float* vals, const int32_t* blocks, int64_t nb, int N, int B, float threshold, const uint8_t* table,
                    const int32_t* block_map, int32_t* counts, int32_t* cut_faces, int32_t* nonfinite, hipStream_t st) {
    const int P = B + 1;
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)nb), dim3(MX_THREADS), (size_t)P * P * P * sizeof(float), st, vals, blocks, N, B,
                       threshold, table, block_map, counts, cut_faces, nonfinite);
    return launch_status();
}

int launch_mc_emit(const float* vals, const int32_t* blocks, int64_t nb, int N, int B, float threshold, const uint8_t* table,
                   const int64_t* offsets, int64_t n_tri, int64_t* keys, float* pos, hipStream_t st) {
    const int P = B + 1;
    hipLaunchKernelGGL(mc_emit_kernel, dim3((unsigned)nb), dim3(MX_THREADS), (size_t)P * P * P * sizeof(float), st, vals, blocks, N, B,
                       threshold, table, offsets, n_tri, keys, pos);
    return launch_status();
}

}  // namespace dh
