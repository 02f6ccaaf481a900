// Texture atlas of a mesh (dynhor_amd/mesh_texture.py): the atlas baked from the frames that see each texel, and the mesh drawn with it.
//
// texture_bake_kernel: one lane per texel of the S x S atlas.  A workgroup of 256 covers 16 x 16 texels, each of its waves an 8 x 8
// tile: the 64 lanes of a wave lie in one or two faces of one atlas cell, so their face data comes from the same few cache lines and
// their projections land on neighbouring pixels of a frame.  The frame loop is wave-uniform (camera rows through the scalar unit).
// A texel (x, y) is worked on when o = owner[y S + x] lies in [0, nf), the three vertex indices of faces[o] lie in [0, nv) and the UV
// area = edge(uv0, uv1, uv2) is not 0 (mk_edge, mesh_raster.h).  With q = (x + 0.5, y + 0.5), in fp32 and in this order:
//   e0 = edge(uv1, uv2, q), e1 = edge(uv2, uv0, q), e2 = edge(uv0, uv1, q),  b_i = max(e_i / area, 0),  b_i = b_i / ((b0 + b1) + b2)
//   p = fma(b2, v2, fma(b1, v1, b0 v0)),  n = fma(b2, n2, fma(b1, n1, b0 n0))     (a gutter texel repeats the nearest edge)
// and for every frame f in ascending order: (c, u, w) = mk_project(p).  The frame contributes when c_2 > 1e-3, 0 <= u <= W - 1 and
// 0 <= w <= H - 1, usable at the nearest pixel (floor(u + 0.5), floor(w + 0.5)) is set, mk_view (mesh_shade.h, shared with
// mesh_bake_kernel) sees p through the z-buffer's key there, and cosv = mk_view's cos / |n| >= min_cos.  weight = cosv squared
// `sharpen` times.  The colour is mk_bilinear_u8 at (u, w): x0 = floor(u), x1 = min(x0 + 1, W - 1), fx = u - x0, likewise y;
//   acc.rgb = fma(weight, col, acc.rgb),  acc.w += weight,  n_views += 1
// acc / n_views are read once and written once: a fixed sequential fp32 sum per texel, no float atomics.
//
// mesh_shade_tex_kernel: one lane per pixel, four pixels per lane 256 apart, every workgroup inside one frame.  Coverage, the weights
// l_j, the headlight and the composite are dh_mesh_shade's (mk_key_face, mk_pixel_weights, mk_headlight, mk_composite of mesh_shade.h);
// (s, t) = fma(l2, uv2, fma(l1, uv1, l0 uv0)); col = mk_bilinear_u8 of tex u8 [Sh,Sw,3]: i0 = floor(s - 0.5), fx = (s - 0.5) - i0, taps
// i0 and i0 + 1 clamped to [0, Sw - 1], likewise t;  out = mk_composite(col, lit ? shade : 1, alpha, bg).
// With usable and sums, over the covered pixels with usable set: sums[f] += (sum_channels (out - rgb)^2, 1), reduced over the wave by
// integer shuffles, over the workgroup through LDS, then one 64-bit integer atomic each: bitwise reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "mesh_shade.h"

namespace dh {

namespace {
constexpr int TX_TILE = 16;                 // texels per workgroup edge of the bake (four 8 x 8 wave tiles)
constexpr int TS_THREADS = 256;
constexpr int TS_PER_LANE = 4;              // pixels per lane of the textured shade
}  // namespace

__global__ __launch_bounds__(TX_TILE* TX_TILE) void texture_bake_kernel(
    const float* __restrict__ verts, const float* __restrict__ normals, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
    const float* __restrict__ uv, const int32_t* __restrict__ owner, int S, const uint8_t* __restrict__ rgb,
    const uint8_t* __restrict__ usable, const uint64_t* __restrict__ zbuf, const float* __restrict__ R, const float* __restrict__ T,
    const float* __restrict__ K, int64_t n_frames, int H, int W, float depth_eps, float min_cos, int sharpen, float* __restrict__ acc,
    int32_t* __restrict__ n_views) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * TX_TILE + (wave & 1) * 8 + (lane & 7);
    const int y = blockIdx.y * TX_TILE + (wave >> 1) * 8 + (lane >> 3);
    if (x >= S || y >= S) return;
    const int64_t t = (int64_t)y * S + x;
    const int64_t o = owner[t];
    if (o < 0 || o >= nf) return;
    int64_t ia, ib, ic;
    if (!mk_face_in_range(faces, o, nv, ia, ib, ic)) return;
    const float u0 = uv[o * 6 + 0], w0 = uv[o * 6 + 1], u1 = uv[o * 6 + 2], w1 = uv[o * 6 + 3], u2 = uv[o * 6 + 4], w2 = uv[o * 6 + 5];
    const float area = mk_edge(u0, w0, u1, w1, u2, w2);
    if (!(fabsf(area) > 0.f)) return;                            // 0 or NaN
    const float qx = (float)x + 0.5f, qy = (float)y + 0.5f;
    float b0 = fmaxf(mk_edge(u1, w1, u2, w2, qx, qy) / area, 0.f);
    float b1 = fmaxf(mk_edge(u2, w2, u0, w0, qx, qy) / area, 0.f);
    float b2 = fmaxf(mk_edge(u0, w0, u1, w1, qx, qy) / area, 0.f);
    const float bs = (b0 + b1) + b2;
    b0 /= bs; b1 /= bs; b2 /= bs;
    float p[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = __builtin_fmaf(b2, verts[ic * 3 + k], __builtin_fmaf(b1, verts[ib * 3 + k], b0 * verts[ia * 3 + k]));
        n[k] = __builtin_fmaf(b2, normals[ic * 3 + k], __builtin_fmaf(b1, normals[ib * 3 + k], b0 * normals[ia * 3 + k]));
    }
    const float nlen = sqrtf(__builtin_fmaf(n[2], n[2], __builtin_fmaf(n[1], n[1], n[0] * n[0])));
    const float k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5];
    const float umax = (float)(W - 1), wmax = (float)(H - 1);
    const int64_t HW = (int64_t)H * W;
    float4 a = reinterpret_cast<const float4*>(acc)[t];
    int32_t cnt = n_views[t];
    for (int64_t f = 0; f < n_frames; ++f) {
        const float* Rf = R + f * 9;
        const float* Tf = T + f * 3;
        const Cam c = mk_project(Rf, Tf, k00, k01, k02, k10, k11, k12, p[0], p[1], p[2]);
        if (!((c.c2 > 1e-3f) & (c.u >= 0.f) & (c.u <= umax) & (c.w >= 0.f) & (c.w <= wmax))) continue;     // false for a NaN
        // 0 <= u <= W - 1: the nearest pixel and both taps of the fetch lie in the image
        const int64_t pix = f * HW + (int64_t)(int)floorf(c.w + 0.5f) * W + (int)floorf(c.u + 0.5f);
        if (usable[pix] == 0) continue;
        const View v = mk_view(zbuf[pix], c.c2, depth_eps, Rf, Tf, p[0], p[1], p[2], n[0], n[1], n[2]);
        if (!v.seen) continue;
        const float cs = v.cos / nlen;
        if (!(cs >= min_cos)) continue;
        float wgt = cs;
        for (int k = 0; k < sharpen; ++k) wgt *= wgt;
        const float fx0 = floorf(c.u), fy0 = floorf(c.w);
        const int x0 = (int)fx0, y0 = (int)fy0;
        const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
        const float fx = c.u - fx0, fy = c.w - fy0;
        float col[3];
        mk_bilinear_u8(rgb + f * HW * 3, W, x0, x1, y0, y1, fx, fy, col);
        a.x = __builtin_fmaf(wgt, col[0], a.x);
        a.y = __builtin_fmaf(wgt, col[1], a.y);
        a.z = __builtin_fmaf(wgt, col[2], a.z);
        a.w += wgt;
        cnt += 1;
    }
    reinterpret_cast<float4*>(acc)[t] = a;
    n_views[t] = cnt;
}

__global__ __launch_bounds__(TS_THREADS) void mesh_shade_tex_kernel(
    const float* __restrict__ verts, const float* __restrict__ normals, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
    const float* __restrict__ uv, const uint8_t* __restrict__ tex, int Sh, int Sw, const uint64_t* __restrict__ zbuf,
    const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ K, int H, int W, int blocks_per_frame,
    const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ usable, float alpha, int lit, uint8_t* __restrict__ out,
    int64_t* __restrict__ sums) {
    __shared__ unsigned long long part[TS_THREADS / 64][2];
    const int64_t f = blockIdx.x / blocks_per_frame;             // block-uniform: a workgroup never leaves its frame
    const int64_t HW = (int64_t)H * W;
    const int64_t base = (int64_t)(blockIdx.x - f * blocks_per_frame) * (TS_THREADS * TS_PER_LANE);
    const float* Rf = R + f * 9;
    const float* Tf = T + f * 3;
    const float k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5];
    const float smax = (float)(Sw - 1), tmax = (float)(Sh - 1);
    uint32_t sse = 0, cntp = 0;
    for (int j = 0; j < TS_PER_LANE; ++j) {
        const int64_t r = base + (int64_t)j * TS_THREADS + threadIdx.x;
        if (r >= HW) break;
        const int64_t pidx = f * HW + r;
        const int yy = (int)(r / W), xx = (int)(r - (int64_t)yy * W);
        uint32_t bg[3] = {255u, 255u, 255u};
        if (rgb) {
            bg[0] = rgb[pidx * 3 + 0]; bg[1] = rgb[pidx * 3 + 1]; bg[2] = rgb[pidx * 3 + 2];
        }
        const uint64_t key = zbuf[pidx];
        int64_t ia = 0, ib = 0, ic = 0;
        const bool cv = mk_key_face(key, faces, nf, nv, ia, ib, ic);
        uint32_t o[3] = {bg[0], bg[1], bg[2]};
        if (cv) {
            float l0, l1, l2;
            mk_pixel_weights(verts, ia, ib, ic, Rf, Tf, k00, k01, k02, k10, k11, k12, xx, yy, l0, l1, l2);
            const float shade = lit ? mk_headlight(normals, ia, ib, ic, l0, l1, l2, Rf) : 1.f;
            const float* uf = uv + (int64_t)(key & 0xffffffffu) * 6;
            const float s = __builtin_fmaf(l2, uf[4], __builtin_fmaf(l1, uf[2], l0 * uf[0])) - 0.5f;
            const float tt = __builtin_fmaf(l2, uf[5], __builtin_fmaf(l1, uf[3], l0 * uf[1])) - 0.5f;
            const float si = floorf(s), ti = floorf(tt);
            const float fx = s - si, fy = tt - ti;
            // fmaxf / fminf take the number over a NaN: the four taps always lie in the texture
            const int i0 = (int)fminf(fmaxf(si, 0.f), smax), i1 = (int)fminf(fmaxf(si + 1.f, 0.f), smax);
            const int j0 = (int)fminf(fmaxf(ti, 0.f), tmax), j1 = (int)fminf(fmaxf(ti + 1.f, 0.f), tmax);
            float col[3];
            mk_bilinear_u8(tex, Sw, i0, i1, j0, j1, fx, fy, col);
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = mk_composite(col[k], shade, alpha, bg[k]);
        }
        out[pidx * 3 + 0] = (uint8_t)o[0]; out[pidx * 3 + 1] = (uint8_t)o[1]; out[pidx * 3 + 2] = (uint8_t)o[2];
        if (sums && cv && usable[pidx] != 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int d = (int)o[k] - (int)bg[k];
                sse += (uint32_t)(d * d);
            }
            cntp += 1;
        }
    }
    if (sums) {                                                  // kernel-uniform; every lane of the workgroup arrives here
        // per lane at most 4 * 3 * 255^2 < 2^20, per wave < 2^26
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            sse += (uint32_t)__shfl_xor((int)sse, m);
            cntp += (uint32_t)__shfl_xor((int)cntp, m);
        }
        if ((threadIdx.x & 63) == 0) {
            part[threadIdx.x >> 6][0] = sse;
            part[threadIdx.x >> 6][1] = cntp;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long s0 = 0, s1 = 0;
#pragma unroll
            for (int w = 0; w < TS_THREADS / 64; ++w) {
                s0 += part[w][0];
                s1 += part[w][1];
            }
            unsigned long long* sf = reinterpret_cast<unsigned long long*>(sums + f * 2);
            if (s0) atomicAdd(sf + 0, s0);
            if (s1) atomicAdd(sf + 1, s1);
        }
    }
}

int launch_texture_bake(const float* verts, const float* normals, int64_t nv, const int64_t* faces, int64_t nf, const float* uv,
                        const int32_t* owner, int S, const uint8_t* rgb, const uint8_t* usable, const uint64_t* zbuf, const float* R,
                        const float* T, const float* K, int64_t n_frames, int H, int W, float depth_eps, float min_cos, int sharpen,
                        float* acc, int32_t* n_views, hipStream_t st) {
    const unsigned g = (unsigned)((S + TX_TILE - 1) / TX_TILE);
    hipLaunchKernelGGL(texture_bake_kernel, dim3(g, g), dim3(TX_TILE * TX_TILE), 0, st, verts, normals, nv, faces, nf, uv, owner, S, rgb,
                       usable, zbuf, R, T, K, n_frames, H, W, depth_eps, min_cos, sharpen, acc, n_views);
    return launch_status();
}

int64_t shade_tex_blocks_per_frame(int H, int W) {
    return ((int64_t)H * W + TS_THREADS * TS_PER_LANE - 1) / (TS_THREADS * TS_PER_LANE);
}

int launch_mesh_shade_tex(const float* verts, const float* normals, int64_t nv, const int64_t* faces, int64_t nf, const float* uv,
                          const uint8_t* tex, int Sh, int Sw, const uint64_t* zbuf, const float* R, const float* T, const float* K,
                          int64_t n_frames, int H, int W, const uint8_t* rgb, const uint8_t* usable, float alpha, int lit, uint8_t* out,
                          int64_t* sums, hipStream_t st) {
    const int64_t bpf = shade_tex_blocks_per_frame(H, W);
    hipLaunchKernelGGL(mesh_shade_tex_kernel, dim3((unsigned)(n_frames * bpf)), dim3(TS_THREADS), 0, st, verts, normals, nv, faces, nf, uv,
                       tex, Sh, Sw, zbuf, R, T, K, H, W, (int)bpf, rgb, usable, alpha, lit, out, sums);
    return launch_status();
}

}  // namespace dh
