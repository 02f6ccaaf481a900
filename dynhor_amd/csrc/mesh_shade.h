// What the mesh kernels share about a z-buffer of dh_mesh_raster_depth once it is filled: the covered test of a key, the weights of a
// covered pixel, the headlight, the composite, the view test of the bakes and the bilinear byte fetch.  Each rule is written once,
// here, so the vertex-colour path (csrc/mesh_vis.hip, csrc/mesh_color.hip) and the texture path (csrc/mesh_texture.hip) agree bit for
// bit by construction.  All fp32, in the order written; a multiply that feeds an fma is a product of its own.
//
// mk_key_face: a pixel is covered when its key is not empty, its face index i = key & 0xffffffff is < nf and the face's vertices lie
// in [0, nv) (the face is read only then).
// mk_pixel_weights, for the pixel centre p = (x, y) of a frame and the face (a, b, c) = (v0, v1, v2): the vertices projected by
// mk_project, e0 = edge(v1, v2, p), e1 = edge(v2, v0, p), e2 = edge(v0, v1, p) by mk_edge (the rasteriser's own code, mesh_raster.h),
//   den = fma(e2, 1/z2, fma(e1, 1/z1, e0 * (1/z0)))      (the denominator of the rasteriser's depth),
//   l_j = (e_j * (1/z_j)) * (1 / den)                    (1/3 each if den is 0 or not finite: a z-buffer that is not this mesh's).
// mk_headlight: n = fma(l2, n2, fma(l1, n1, l0 n0)),  nz = fma(R_8, n_z, fma(R_7, n_y, R_6 * n_x)),  s = |nz| / |n| (0 when |n| is 0
// or NaN), shade = fma(0.7, s, 0.3): a double-sided light along the optical axis.
// mk_composite, per channel: c = clamp(base * shade, 0, 1),  o = fma(alpha, c, (1 - alpha) * (bg / 255)),
//   byte = min(floor(fma(255, o, 0.5)), 255)   (mk_byte).
// mk_view, for a surface point p with normal n whose nearest pixel holds `key`, at camera depth c_2: depth = the float in the key's
// high word; seen = the key is not empty and c_2 <= depth + depth_eps; and with C = -R^T T the camera centre and d = C - p:
//   C_k = -fma(R_2k, T_2, fma(R_1k, T_1, R_0k * T_0)),   |d| = sqrt(fma(d_z, d_z, fma(d_y, d_y, d_x * d_x)))
//   cos = fma(n_z, d_z, fma(n_y, d_y, n_x * d_x)) / |d|.
// mk_bilinear_u8, the three channels of a u8 image [.., stride, 3] at the columns x0, x1 and rows y0, y1 (the caller clamps them into
// the image) with fractions fx, fy:
//   top = fma(fx, c10 - c00, c00), bot = fma(fx, c11 - c01, c01), col = fma(fy, bot - top, top) * (1/255)   (c..: the bytes as floats).
#pragma once
#include "mesh_raster.h"

namespace dh {
namespace {
constexpr float MK_INV255 = 1.f / 255.f;

__device__ __forceinline__ bool mk_key_face(uint64_t key, const int64_t* __restrict__ faces, int64_t nf, int64_t nv, int64_t& a,
                                            int64_t& b, int64_t& c) {
    const int64_t i = (int64_t)(key & 0xffffffffu);
    return key != MK_EMPTY && i < nf && mk_face_in_range(faces, i, nv, a, b, c);
}

__device__ __forceinline__ void mk_pixel_weights(const float* __restrict__ verts, int64_t a, int64_t b, int64_t c, const float* Rf,
                                                 const float* Tf, float k00, float k01, float k02, float k10, float k11, float k12,
                                                 int x, int y, float& l0, float& l1, float& l2) {
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
    const float rden = 1.f / den, third = 1.f / 3.f;
    l0 = ok ? (e0 * iz0) * rden : third;
    l1 = ok ? (e1 * iz1) * rden : third;
    l2 = ok ? (e2 * iz2) * rden : third;
}

__device__ __forceinline__ float mk_headlight(const float* __restrict__ normals, int64_t a, int64_t b, int64_t c, float l0, float l1,
                                              float l2, const float* Rf) {
    const float nx = __builtin_fmaf(l2, normals[c * 3 + 0], __builtin_fmaf(l1, normals[b * 3 + 0], l0 * normals[a * 3 + 0]));
    const float ny = __builtin_fmaf(l2, normals[c * 3 + 1], __builtin_fmaf(l1, normals[b * 3 + 1], l0 * normals[a * 3 + 1]));
    const float nz = __builtin_fmaf(l2, normals[c * 3 + 2], __builtin_fmaf(l1, normals[b * 3 + 2], l0 * normals[a * 3 + 2]));
    const float ncz = __builtin_fmaf(Rf[8], nz, __builtin_fmaf(Rf[7], ny, Rf[6] * nx));
    const float len = sqrtf(__builtin_fmaf(nz, nz, __builtin_fmaf(ny, ny, nx * nx)));
    const float s = len > 0.f ? fabsf(ncz) / len : 0.f;
    return __builtin_fmaf(0.7f, s, 0.3f);
}

__device__ __forceinline__ uint32_t mk_byte(float o) {
    return (uint32_t)fminf(floorf(__builtin_fmaf(255.f, o, 0.5f)), 255.f);
}

// One channel of a covered pixel over the background byte bg.
__device__ __forceinline__ uint32_t mk_composite(float base, float shade, float alpha, uint32_t bg) {
    const float col = fmaxf(fminf(1.f, base * shade), 0.f);                  // fminf / fmaxf take the number over a NaN
    return mk_byte(__builtin_fmaf(alpha, col, (1.f - alpha) * ((float)bg * MK_INV255)));
}

struct View {
    float depth, cos;
    bool seen;
};

__device__ __forceinline__ View mk_view(uint64_t key, float c2, float depth_eps, const float* Rf, const float* Tf, float px, float py,
                                        float pz, float nx, float ny, float nz) {
    View v;
    v.depth = __uint_as_float((uint32_t)(key >> 32));
    v.seen = (key != MK_EMPTY) & (c2 <= v.depth + depth_eps);
    const float cx = -__builtin_fmaf(Rf[6], Tf[2], __builtin_fmaf(Rf[3], Tf[1], Rf[0] * Tf[0]));
    const float cy = -__builtin_fmaf(Rf[7], Tf[2], __builtin_fmaf(Rf[4], Tf[1], Rf[1] * Tf[0]));
    const float cz = -__builtin_fmaf(Rf[8], Tf[2], __builtin_fmaf(Rf[5], Tf[1], Rf[2] * Tf[0]));
    const float dx = cx - px, dy = cy - py, dz = cz - pz;
    const float len = sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
    v.cos = __builtin_fmaf(nz, dz, __builtin_fmaf(ny, dy, nx * dx)) / len;
    return v;
}

__device__ __forceinline__ void mk_bilinear_u8(const uint8_t* __restrict__ img, int stride, int x0, int x1, int y0, int y1, float fx,
                                               float fy, float col[3]) {
    const uint8_t* c00 = img + ((int64_t)y0 * stride + x0) * 3;
    const uint8_t* c10 = img + ((int64_t)y0 * stride + x1) * 3;
    const uint8_t* c01 = img + ((int64_t)y1 * stride + x0) * 3;
    const uint8_t* c11 = img + ((int64_t)y1 * stride + x1) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float top = __builtin_fmaf(fx, (float)c10[k] - (float)c00[k], (float)c00[k]);
        const float bot = __builtin_fmaf(fx, (float)c11[k] - (float)c01[k], (float)c01[k]);
        col[k] = __builtin_fmaf(fy, bot - top, top) * MK_INV255;
    }
}
}  // namespace
}  // namespace dh
