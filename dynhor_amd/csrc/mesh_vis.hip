// Mesh overlay (dynhor_amd/mesh_vis.py): the mesh shaded from a z-buffer of dh_mesh_raster_depth, composited over the frames, and
// the silhouette agreement with the object labels counted in the same pass.
//
// mesh_shade_kernel: a flat index over the n_frames * H * W pixels, four consecutive pixels per lane (the 12 bytes of rgb / out
// and the 4 of label then move as whole dwords, the 32 of zbuf as two 16-byte loads; a group of four starts at a multiple of 12
// bytes).  A wave walks a contiguous span of tiles of 64 such groups, so a frame's counts stay in the wave's scalar accumulators
// until the frame changes: one integer atomic per wave, frame and count, after a reduction by ballot and population count.
//
// A pixel is covered when its key is not empty, its face index i = key & 0xffffffff is < nf and the face's vertices lie in [0, nv)
// (the face is read only then).  For a covered pixel centre p = (x, y) of frame f and face (a, b, c) = (v0, v1, v2):
//   the three vertices are projected by mk_project and the edge values e0 = edge(v1, v2, p), e1 = edge(v2, v0, p),
//   e2 = edge(v0, v1, p) taken by mk_edge, both the rasteriser's own code (mesh_raster.h);
//   den = fma(e2, 1/z2, fma(e1, 1/z1, e0 * (1/z0)))      (the denominator of the rasteriser's depth),
//   l_j = (e_j * (1/z_j)) * (1 / den)                    (1/3 each if den is 0 or not finite: a z-buffer that is not this mesh's),
//   n = sum_j l_j n_j,  nz = fma(R_f8, n_z, fma(R_f7, n_y, R_f6 * n_x)),  s = |nz| / |n| (0 when |n| is 0 or NaN),
//   base = colors ? sum_j l_j colors_j / 255 : (0.8, 0.46, 0.51),  c = clamp(base * fma(0.7, s, 0.3), 0, 1),
//   o = fma(alpha, c, (1 - alpha) * bg),  bg = rgb / 255 (1 without frames),  out = min(floor(fma(255, o, 0.5)), 255).
// An uncovered pixel copies its background bytes (255 without frames).  With labels, over the pixels with label >= 0:
//   counts[f] += (covered & label == 1, covered & label == 0, !covered & label == 1).
// Everything is integer or per pixel: the output and the counts are bitwise reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "mesh_raster.h"

namespace dh {

namespace {
constexpr int MS_THREADS = 256;
constexpr int MS_WAVES = MS_THREADS / 64;
constexpr int MS_TILE = 64 * 4;            // pixels of one wave step
constexpr float MS_INV255 = 1.f / 255.f;

__device__ inline bool ms_face(uint64_t key, const int64_t* __restrict__ faces, int64_t nf, int64_t nv, int64_t& a, int64_t& b,
                               int64_t& c) {
    const int64_t i = (int64_t)(key & 0xffffffffu);
    if (key == MK_EMPTY || i >= nf) return false;
    a = faces[i * 3 + 0];
    b = faces[i * 3 + 1];
    c = faces[i * 3 + 2];
    return a >= 0 && a < nv && b >= 0 && b < nv && c >= 0 && c < nv;
}

__device__ inline uint32_t ms_byte(float o) {
    return (uint32_t)fminf(floorf(__builtin_fmaf(255.f, o, 0.5f)), 255.f);
}

// The three composited bytes of a covered pixel, packed as r | g << 8 | b << 16.
__device__ inline uint32_t ms_shade(const float* __restrict__ verts, const float* __restrict__ normals,
                                    const uint8_t* __restrict__ colors, int64_t a, int64_t b, int64_t c, const float* Rf,
                                    const float* Tf, float k00, float k01, float k02, float k10, float k11, float k12, int x, int y,
                                    uint32_t bg, float alpha) {
    const Cam p0 = mk_project(Rf, Tf, k00, k01, k02, k10, k11, k12, verts[a * 3], verts[a * 3 + 1], verts[a * 3 + 2]);
    const Cam p1 = mk_project(Rf, Tf, k00, k01, k02, k10, k11, k12, verts[b * 3], verts[b * 3 + 1], verts[b * 3 + 2]);
    const Cam p2 = mk_project(Rf, Tf, k00, k01, k02, k10, k11, k12, verts[c * 3], verts[c * 3 + 1], verts[c * 3 + 2]);
    const float iz0 = 1.f / p0.c2, iz1 = 1.f / p1.c2, iz2 = 1.f / p2.c2;
    const float px = (float)x, py = (float)y;
    const float e0 = mk_edge(p1.u, p1.w, p2.u, p2.w, px, py);
    const float e1 = mk_edge(p2.u, p2.w, p0.u, p0.w, px, py);
    const float e2 = mk_edge(p0.u, p0.w, p1.u, p1.w, px, py);
    const float den = __builtin_fmaf(e2, iz2, __builtin_fmaf(e1, iz1, e0 * iz0));
    const bool ok = (fabsf(den) > 0.f) & (fabsf(den) < 3.0e38f);
    const float rden = 1.f / den;
    const float l0 = ok ? (e0 * iz0) * rden : 1.f / 3.f;
    const float l1 = ok ? (e1 * iz1) * rden : 1.f / 3.f;
    const float l2 = ok ? (e2 * iz2) * rden : 1.f / 3.f;
    const float nx = __builtin_fmaf(l2, normals[c * 3 + 0], __builtin_fmaf(l1, normals[b * 3 + 0], l0 * normals[a * 3 + 0]));
    const float ny = __builtin_fmaf(l2, normals[c * 3 + 1], __builtin_fmaf(l1, normals[b * 3 + 1], l0 * normals[a * 3 + 1]));
    const float nz = __builtin_fmaf(l2, normals[c * 3 + 2], __builtin_fmaf(l1, normals[b * 3 + 2], l0 * normals[a * 3 + 2]));
    const float ncz = __builtin_fmaf(Rf[8], nz, __builtin_fmaf(Rf[7], ny, Rf[6] * nx));
    const float len = sqrtf(__builtin_fmaf(nz, nz, __builtin_fmaf(ny, ny, nx * nx)));
    const float s = len > 0.f ? fabsf(ncz) / len : 0.f;
    const float shade = __builtin_fmaf(0.7f, s, 0.3f);
    float base[3] = {0.8f, 0.46f, 0.51f};
    if (colors) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            base[k] = __builtin_fmaf(l2, (float)colors[c * 3 + k], __builtin_fmaf(l1, (float)colors[b * 3 + k],
                                                                                   l0 * (float)colors[a * 3 + k])) * MS_INV255;
    }
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float col = fmaxf(fminf(1.f, base[k] * shade), 0.f);          // fminf / fmaxf take the number over a NaN
        const float bk = (float)((bg >> (8 * k)) & 0xffu) * MS_INV255;
        o |= ms_byte(__builtin_fmaf(alpha, col, (1.f - alpha) * bk)) << (8 * k);
    }
    return o;
}

__device__ inline void ms_flush(int64_t* counts, int f, unsigned long long tp, unsigned long long fp, unsigned long long fn) {
    unsigned long long* cf = reinterpret_cast<unsigned long long*>(counts + (int64_t)f * 3);
    if (tp) atomicAdd(cf + 0, tp);
    if (fp) atomicAdd(cf + 1, fp);
    if (fn) atomicAdd(cf + 2, fn);
}
}  // namespace

// VEC: rgb, label and out are 4-byte aligned and zbuf 16-byte aligned, so a full group moves as dwords; otherwise bytes.
template <bool VEC>
__global__ __launch_bounds__(MS_THREADS) void mesh_shade_kernel(const float* __restrict__ verts, const float* __restrict__ normals,
                                                                const uint8_t* __restrict__ colors, int64_t nv,
                                                                const int64_t* __restrict__ faces, int64_t nf,
                                                                const uint64_t* __restrict__ zbuf, const float* __restrict__ R,
                                                                const float* __restrict__ T, const float* __restrict__ K, int H,
                                                                int W, int64_t n_pix, const uint8_t* __restrict__ rgb,
                                                                const int8_t* __restrict__ label, float alpha,
                                                                uint8_t* __restrict__ out, int64_t* __restrict__ counts,
                                                                int64_t tiles_per_wave) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * MS_WAVES + (threadIdx.x >> 6);
    const int64_t n_tiles = (n_pix + MS_TILE - 1) / MS_TILE;
    const int64_t t0 = wave * tiles_per_wave;
    const int64_t t1 = t0 + tiles_per_wave < n_tiles ? t0 + tiles_per_wave : n_tiles;
    if (t0 >= t1) return;                                       // the whole wave
    const float k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5];
    const int64_t HW = (int64_t)H * W;
    // (frame, row, column) of this lane's first pixel; a wave step advances it by MS_TILE = qf HW + qy W + qx pixels
    int f, y, x;
    {
        const int64_t p = t0 * MS_TILE + lane * 4;
        const int64_t ff = p / HW, r = p - ff * HW, yy = r / W;
        f = (int)ff; y = (int)yy; x = (int)(r - yy * W);
    }
    const int64_t qf = MS_TILE / HW, rq = MS_TILE - qf * HW;
    const int qy = (int)(rq / W), qx = (int)(rq - (int64_t)qy * W);
    int cur = -1;                                               // the frame the wave's counts belong to
    unsigned long long ctp = 0, cfp = 0, cfn = 0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t p = t * MS_TILE + lane * 4;
        const int64_t left = n_pix - p;
        const int nval = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
        uint64_t key[4] = {MK_EMPTY, MK_EMPTY, MK_EMPTY, MK_EMPTY};
        uint32_t cw[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
        uint32_t lw = 0;
        if (VEC && nval == 4) {
            const ulonglong2 k01v = reinterpret_cast<const ulonglong2*>(zbuf + p)[0];
            const ulonglong2 k23v = reinterpret_cast<const ulonglong2*>(zbuf + p)[1];
            key[0] = k01v.x; key[1] = k01v.y; key[2] = k23v.x; key[3] = k23v.y;
            if (rgb) {
                const uint32_t* cp = reinterpret_cast<const uint32_t*>(rgb + p * 3);
                cw[0] = cp[0]; cw[1] = cp[1]; cw[2] = cp[2];
            }
            if (label) lw = *reinterpret_cast<const uint32_t*>(label + p);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nval) {
                    key[j] = zbuf[p + j];
                    if (rgb) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const int byte = j * 3 + k;
                            cw[byte >> 2] = (cw[byte >> 2] & ~(0xffu << (8 * (byte & 3)))) |
                                            ((uint32_t)rgb[(p + j) * 3 + k] << (8 * (byte & 3)));
                        }
                    }
                    if (label) lw |= (uint32_t)(uint8_t)label[p + j] << (8 * j);
                }
            }
        }
        // one pixel at a time (a rolled loop: one copy of the gathers and the shading is live), its 3 bytes at byte 3j of the group
        uint32_t ow0 = 0u, ow1 = 0u, ow2 = 0u;
        unsigned covm = 0u;
        int fj = f, yj = y, xj = x;
#pragma unroll 1
        for (int j = 0; j < nval; ++j) {
            const uint64_t kj = j == 0 ? key[0] : (j == 1 ? key[1] : (j == 2 ? key[2] : key[3]));
            const uint32_t bg = (j == 0 ? cw[0] : (j == 1 ? (cw[0] >> 24) | (cw[1] << 8)
                                                          : (j == 2 ? (cw[1] >> 16) | (cw[2] << 16) : cw[2] >> 8))) & 0xffffffu;
            int64_t a = 0, b = 0, c = 0;
            const bool cv = ms_face(kj, faces, nf, nv, a, b, c);
            const uint32_t o = cv ? ms_shade(verts, normals, colors, a, b, c, R + (int64_t)fj * 9, T + (int64_t)fj * 3, k00, k01, k02,
                                             k10, k11, k12, xj, yj, bg, alpha)
                                  : bg;
            covm |= (unsigned)cv << j;
            if (j == 0) { ow0 |= o; }
            else if (j == 1) { ow0 |= o << 24; ow1 |= o >> 8; }
            else if (j == 2) { ow1 |= o << 16; ow2 |= o >> 16; }
            else { ow2 |= o << 8; }
            if (++xj == W) {
                xj = 0;
                if (++yj == H) { yj = 0; ++fj; }
            }
        }
        const uint32_t ow[3] = {ow0, ow1, ow2};
        if (VEC && nval == 4) {
            uint32_t* op = reinterpret_cast<uint32_t*>(out + p * 3);
            op[0] = ow[0]; op[1] = ow[1]; op[2] = ow[2];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nval) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int byte = j * 3 + k;
                        out[(p + j) * 3 + k] = (uint8_t)(ow[byte >> 2] >> (8 * (byte & 3)));
                    }
                }
        }
        if (counts) {
            // frames are ascending over the lanes and their pixels: the tile holds frames flo..fhi
            int pf[4];
            {
                int ff = f, yy = y, xx = x;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pf[j] = ff;
                    if (++xx == W) {
                        xx = 0;
                        if (++yy == H) { yy = 0; ++ff; }
                    }
                }
            }
            const int64_t rest = (n_pix - 1 - t * MS_TILE) >> 2;
            const int last_lane = rest < 63 ? (int)rest : 63;
            const int fl = nval > 3 ? pf[3] : (nval > 2 ? pf[2] : (nval > 1 ? pf[1] : pf[0]));
            const int flo = __shfl(pf[0], 0), fhi = __shfl(fl, last_lane);
            for (int F = flo; F <= fhi; ++F) {
                if (F != cur) {
                    if (cur >= 0 && lane == 0) ms_flush(counts, cur, ctp, cfp, cfn);
                    cur = F;
                    ctp = cfp = cfn = 0;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int lab = (int)(int8_t)(lw >> (8 * j));
                    const bool in = (j < nval) & (pf[j] == F);
                    const bool cv = (covm >> j) & 1u;
                    ctp += __popcll(__ballot(in & cv & (lab == 1)));
                    cfp += __popcll(__ballot(in & cv & (lab == 0)));
                    cfn += __popcll(__ballot(in & !cv & (lab == 1)));
                }
            }
        }
        x += qx; y += qy; f += (int)qf;
        if (x >= W) { x -= W; ++y; }
        if (y >= H) { y -= H; ++f; }
    }
    if (counts && cur >= 0 && lane == 0) ms_flush(counts, cur, ctp, cfp, cfn);
}

// The workgroups that are resident at once on the current device (CUs x the kernel's occupancy), asked once per device: the grid is
// one such round, each wave walking an equal span of tiles, so no second round of waves starts after the first has finished.
template <bool VEC>
static int64_t ms_resident_blocks() {
    static int64_t cache[16] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 1024;
    int64_t n = cache[dev];                                  // (a benign race: every thread writes the same value)
    if (n == 0) {
        int cus = 0, per = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, mesh_shade_kernel<VEC>, MS_THREADS, 0) != hipSuccess || per < 1) per = 1;
        n = (int64_t)cus * per;
        cache[dev] = n;
    }
    return n;
}

template <bool VEC>
static int ms_launch(const float* verts, const float* normals, const uint8_t* colors, int64_t nv, const int64_t* faces, int64_t nf,
                     const uint64_t* zbuf, const float* R, const float* T, const float* K, int H, int W, int64_t n_pix,
                     const uint8_t* rgb, const int8_t* label, float alpha, uint8_t* out, int64_t* counts, hipStream_t st) {
    const int64_t n_tiles = (n_pix + MS_TILE - 1) / MS_TILE;
    const int64_t most = ms_resident_blocks<VEC>();
    int64_t blocks = (n_tiles + MS_WAVES - 1) / MS_WAVES;
    blocks = blocks < most ? blocks : most;
    const int64_t per = (n_tiles + blocks * MS_WAVES - 1) / (blocks * MS_WAVES);
    blocks = (n_tiles + per * MS_WAVES - 1) / (per * MS_WAVES);
    hipLaunchKernelGGL(mesh_shade_kernel<VEC>, dim3((unsigned)blocks), dim3(MS_THREADS), 0, st, verts, normals, colors, nv, faces, nf,
                       zbuf, R, T, K, H, W, n_pix, rgb, label, alpha, out, counts, per);
    return launch_status();
}

int launch_mesh_shade(const float* verts, const float* normals, const uint8_t* colors, int64_t nv, const int64_t* faces, int64_t nf,
                      const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                      const uint8_t* rgb, const int8_t* label, float alpha, uint8_t* out, int64_t* counts, hipStream_t st) {
    const int64_t n_pix = n_frames * H * W;
    const bool vec = ((uintptr_t)zbuf % 16 == 0) && ((uintptr_t)rgb % 4 == 0) && ((uintptr_t)label % 4 == 0) && ((uintptr_t)out % 4 == 0);
    return vec ? ms_launch<true>(verts, normals, colors, nv, faces, nf, zbuf, R, T, K, H, W, n_pix, rgb, label, alpha, out, counts, st)
               : ms_launch<false>(verts, normals, colors, nv, faces, nf, zbuf, R, T, K, H, W, n_pix, rgb, label, alpha, out, counts, st);
}

}  // namespace dh
