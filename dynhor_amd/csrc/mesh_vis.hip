// Mesh overlay (dynhor_amd/mesh_vis.py): the mesh shaded from a z-buffer of dh_mesh_raster_depth, composited over the frames, and
// the silhouette agreement with the object labels counted in the same pass.
//
// mesh_shade_kernel: a flat index over the n_frames * H * W pixels, four consecutive pixels per lane (the 12 bytes of rgb / out
// and the 4 of label then move as whole dwords, the 32 of zbuf as two 16-byte loads; a group of four starts at a multiple of 12
// bytes).  A wave walks a contiguous span of tiles of 64 such groups, so a frame's counts stay in the wave's scalar accumulators
// until the frame changes: one integer atomic per wave, frame and count, after a reduction by ballot and population count.
//
// A pixel is covered by mk_key_face.  A covered pixel takes its weights l_j from mk_pixel_weights and its light from mk_headlight, and
// per channel mk_composite(base, shade, alpha, bg) with base = colors ? fma(l2, c2, fma(l1, c1, l0 c0)) / 255 : (0.8, 0.46, 0.51) and
// bg the frame's byte (255 without frames): mesh_shade.h states the four rules, which dh_mesh_shade_tex shares.
// An uncovered pixel copies its background bytes (255 without frames).  With labels, over the pixels with label >= 0:
//   counts[f] += (covered & label == 1, covered & label == 0, !covered & label == 1).
// Everything is integer or per pixel: the output and the counts are bitwise reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "mesh_shade.h"

namespace dh {

namespace {
constexpr int MS_THREADS = 256;
constexpr int MS_WAVES = MS_THREADS / 64;
constexpr int MS_TILE = 64 * 4;            // pixels of one wave step

// The three composited bytes of a covered pixel, packed as r | g << 8 | b << 16.
__device__ inline uint32_t ms_shade(const float* __restrict__ verts, const float* __restrict__ normals,
                                    const uint8_t* __restrict__ colors, int64_t a, int64_t b, int64_t c, const float* Rf,
                                    const float* Tf, float k00, float k01, float k02, float k10, float k11, float k12, int x, int y,
                                    uint32_t bg, float alpha) {
    float l0, l1, l2;
    mk_pixel_weights(verts, a, b, c, Rf, Tf, k00, k01, k02, k10, k11, k12, x, y, l0, l1, l2);
    const float shade = mk_headlight(normals, a, b, c, l0, l1, l2, Rf);
    float base[3] = {0.8f, 0.46f, 0.51f};
    if (colors) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            base[k] = __builtin_fmaf(l2, (float)colors[c * 3 + k], __builtin_fmaf(l1, (float)colors[b * 3 + k],
                                                                                   l0 * (float)colors[a * 3 + k])) * MK_INV255;
    }
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) o |= mk_composite(base[k], shade, alpha, (bg >> (8 * k)) & 0xffu) << (8 * k);
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
            const bool cv = mk_key_face(kj, faces, nf, nv, a, b, c);
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
