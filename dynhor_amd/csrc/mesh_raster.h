// What the mesh kernels share about a face on the screen: the projection, the edge function, the face-index check and the face walker.
// Every user evaluates a pixel centre with the same fp32 operations in the same order, so the z-buffer (csrc/mesh_color.hip), the
// silhouette's covered set (csrc/sil.hip) and the coverage and barycentrics of the shade (csrc/mesh_vis.hip) agree bit for bit.
//
// Projection, in fp32 and in this order (mk_project):
//   c_r = fma(R_r2, z, fma(R_r1, y, R_r0 * x)) + T_r            (r = 0, 1, 2: x_cam = R v + T)
//   u = fma(K02, c_2, fma(K01, c_1, K00 * c_0)) / c_2,   w = fma(K12, c_2, fma(K11, c_1, K10 * c_0)) / c_2
// Pixel centres sit at integer (u, w).  Edge functions in fp32 (mk_edge, mk_covers):
//   edge(a, b, p) = fma(b.u - a.u, p.w - a.w, -((b.w - a.w) * (p.u - a.u)))
//   e0 = edge(v1, v2, p), e1 = edge(v2, v0, p), e2 = edge(v0, v1, p), area = edge(v0, v1, v2)
// The pixel centre p is covered when e0, e1, e2 are all >= 0 or all <= 0 (double-sided, edges included) and their sum is not 0.
//
// mk_walk_faces: one lane per (frame, face), frame-major.  A face is skipped when an index lies outside [0, nv), when a vertex has
// c_2 <= 1e-3 or a non-finite (u, w), when its screen area is 0, or when its box of pixel centres, grown by `grow` pixels and clipped
// to the image, is empty; an operation with FACE_TEST may also skip a face after a look at its box (op.work).  A lane walks its
// face's box alone when the box is at most MK_SMALL_BOX pixels wide and tall.  A larger face is deferred to the wave phase that
// follows in the same loop iteration: the wave takes its deferred faces one after the other (ballot order) and spreads each face's
// box over its 64 lanes, so a coarse mesh with large faces never serialises one lane.  Per pixel of the box the walker calls
// op.pixel(tri, x, y, face, row) with row the image row y of the frame's 64-bit buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace dh {
namespace {
constexpr uint64_t MK_EMPTY = ~(uint64_t)0;
constexpr int MK_THREADS = 256;             // workgroup of the kernels that run mk_walk_faces
constexpr int MK_SMALL_BOX = 32;

struct Cam {
    float c0, c1, c2, u, w;
};

__device__ inline Cam mk_project(const float* Rf, const float* Tf, float k00, float k01, float k02, float k10, float k11, float k12,
                                 float x, float y, float z) {
    Cam c;
    c.c0 = __builtin_fmaf(Rf[2], z, __builtin_fmaf(Rf[1], y, Rf[0] * x)) + Tf[0];
    c.c1 = __builtin_fmaf(Rf[5], z, __builtin_fmaf(Rf[4], y, Rf[3] * x)) + Tf[1];
    c.c2 = __builtin_fmaf(Rf[8], z, __builtin_fmaf(Rf[7], y, Rf[6] * x)) + Tf[2];
    c.u = __builtin_fmaf(k02, c.c2, __builtin_fmaf(k01, c.c1, k00 * c.c0)) / c.c2;
    c.w = __builtin_fmaf(k12, c.c2, __builtin_fmaf(k11, c.c1, k10 * c.c0)) / c.c2;
    return c;
}

__device__ inline float mk_edge(float au, float aw, float bu, float bw, float pu, float pw) {
    return __builtin_fmaf(bu - au, pw - aw, -((bw - aw) * (pu - au)));
}

// The three vertex indices of face fi, and whether all of them lie in [0, nv).
__device__ __forceinline__ bool mk_face_in_range(const int64_t* __restrict__ faces, int64_t fi, int64_t nv, int64_t& a, int64_t& b,
                                                 int64_t& c) {
    a = faces[fi * 3 + 0]; b = faces[fi * 3 + 1]; c = faces[fi * 3 + 2];
    return a >= 0 && a < nv && b >= 0 && b < nv && c >= 0 && c < nv;
}

// The screen-space face one lane (or, in the wave phase, the whole wave) walks.  N = 6: the corners only; N = 9: with the reciprocal
// camera depths of the corners, which only an operation that interpolates depth takes along (and shuffles in the wave phase).
template <int N>
struct Tri {
    float u0, w0, u1, w1, u2, w2;
    float iz[N - 6];
};
template <>
struct Tri<6> {
    float u0, w0, u1, w1, u2, w2;
};

template <int N>
__device__ __forceinline__ bool mk_covers(const Tri<N>& t, float px, float py, float& e0, float& e1, float& e2) {
    e0 = mk_edge(t.u1, t.w1, t.u2, t.w2, px, py);
    e1 = mk_edge(t.u2, t.w2, t.u0, t.w0, px, py);
    e2 = mk_edge(t.u0, t.w0, t.u1, t.w1, px, py);
    const bool pos = (e0 >= 0.f) & (e1 >= 0.f) & (e2 >= 0.f), neg = (e0 <= 0.f) & (e1 <= 0.f) & (e2 <= 0.f);
    return (pos | neg) && e0 + e1 + e2 != 0.f;
}

// Op: static constexpr int N (Tri<N>), static constexpr bool FACE_TEST, pixel(tri, x, y, face, row), and with FACE_TEST
// work(frame, x0, x1, y0, y1).  Called by every thread of a MK_THREADS workgroup of a 1-D grid (the wave phase needs whole waves).
template <class Op>
__device__ __forceinline__ void mk_walk_faces(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                              const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ K,
                                              int64_t n_frames, int H, int W, float grow, uint64_t* buf, const Op& op) {
    constexpr int N = Op::N;
    const float k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5];
    const int64_t total = n_frames * nf, HW = (int64_t)H * W;
    const int lane = threadIdx.x & 63;
    // the loop bound is block-uniform, so every lane of a wave reaches the ballot of every iteration
    for (int64_t base = (int64_t)blockIdx.x * MK_THREADS; base < total; base += (int64_t)gridDim.x * MK_THREADS) {
        const int64_t i = base + threadIdx.x;
        bool big = false;
        Tri<N> t = {};
        int64_t f = 0;
        uint32_t face = 0;
        int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
        if (i < total) {
            f = i / nf;
            const int64_t fi = i - f * nf;
            face = (uint32_t)fi;
            int64_t a, b, c;
            if (mk_face_in_range(faces, fi, nv, a, b, c)) {
                const float* Rf = R + f * 9;
                const float* Tf = T + f * 3;
                const Cam p0 = mk_project(Rf, Tf, k00, k01, k02, k10, k11, k12, verts[a * 3], verts[a * 3 + 1], verts[a * 3 + 2]);
                const Cam p1 = mk_project(Rf, Tf, k00, k01, k02, k10, k11, k12, verts[b * 3], verts[b * 3 + 1], verts[b * 3 + 2]);
                const Cam p2 = mk_project(Rf, Tf, k00, k01, k02, k10, k11, k12, verts[c * 3], verts[c * 3 + 1], verts[c * 3 + 2]);
                t.u0 = p0.u; t.w0 = p0.w; t.u1 = p1.u; t.w1 = p1.w; t.u2 = p2.u; t.w2 = p2.w;
                if constexpr (N == 9) {
                    t.iz[0] = 1.f / p0.c2; t.iz[1] = 1.f / p1.c2; t.iz[2] = 1.f / p2.c2;
                }
                const float lim = 3.0e38f;    // |u|, |w| < lim: finite, and every comparison below is false for a NaN
                const bool ok = (p0.c2 > 1e-3f) & (p1.c2 > 1e-3f) & (p2.c2 > 1e-3f) & (fabsf(p0.u) < lim) & (fabsf(p0.w) < lim) &
                                (fabsf(p1.u) < lim) & (fabsf(p1.w) < lim) & (fabsf(p2.u) < lim) & (fabsf(p2.w) < lim) &
                                (mk_edge(p0.u, p0.w, p1.u, p1.w, p2.u, p2.w) != 0.f);
                const float fx0 = fmaxf(ceilf(fminf(fminf(p0.u, p1.u), p2.u) - grow), 0.f);
                const float fx1 = fminf(floorf(fmaxf(fmaxf(p0.u, p1.u), p2.u) + grow), (float)(W - 1));
                const float fy0 = fmaxf(ceilf(fminf(fminf(p0.w, p1.w), p2.w) - grow), 0.f);
                const float fy1 = fminf(floorf(fmaxf(fmaxf(p0.w, p1.w), p2.w) + grow), (float)(H - 1));
                if (ok && fx0 <= fx1 && fy0 <= fy1) {
                    x0 = (int)fx0; x1 = (int)fx1; y0 = (int)fy0; y1 = (int)fy1;
                    bool work = true;
                    if constexpr (Op::FACE_TEST) work = op.work(f, x0, x1, y0, y1);
                    big = work & ((x1 - x0 >= MK_SMALL_BOX) | (y1 - y0 >= MK_SMALL_BOX));
                    if (work & !big) {
                        uint64_t* zf = buf + f * HW;
                        for (int y = y0; y <= y1; ++y)
                            for (int x = x0; x <= x1; ++x) op.pixel(t, x, y, face, zf + (int64_t)y * W);
                    }
                }
            }
        }
        // wave phase: the deferred faces of this wave, one at a time, their boxes spread over the 64 lanes
        uint64_t todo = __ballot(big);
        while (todo) {
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            Tri<N> s;
            s.u0 = __shfl(t.u0, src); s.w0 = __shfl(t.w0, src); s.u1 = __shfl(t.u1, src); s.w1 = __shfl(t.w1, src);
            s.u2 = __shfl(t.u2, src); s.w2 = __shfl(t.w2, src);
            if constexpr (N == 9) {
                s.iz[0] = __shfl(t.iz[0], src); s.iz[1] = __shfl(t.iz[1], src); s.iz[2] = __shfl(t.iz[2], src);
            }
            const uint32_t sface = (uint32_t)__shfl((int)face, src);
            const int64_t sf = (int64_t)__shfl((int)f, src);          // f < n_frames < 2^31 (api.hip)
            const int sx0 = __shfl(x0, src), sx1 = __shfl(x1, src), sy0 = __shfl(y0, src), sy1 = __shfl(y1, src);
            const int bw = sx1 - sx0 + 1;
            const int64_t npix = (int64_t)bw * (sy1 - sy0 + 1);
            uint64_t* zf = buf + sf * HW;
            for (int64_t p = lane; p < npix; p += 64) {
                const int y = sy0 + (int)(p / bw), x = sx0 + (int)(p % bw);
                op.pixel(s, x, y, sface, zf + (int64_t)y * W);
            }
        }
    }
}
}  // namespace
}  // namespace dh
