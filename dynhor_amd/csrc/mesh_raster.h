// The rasteriser's projection and edge function (csrc/mesh_color.hip), shared with the shading kernel (csrc/mesh_vis.hip) so that
// both evaluate a pixel centre with the same fp32 operations in the same order: coverage and barycentrics of the shade agree with the
// z-buffer bit for bit.  The formulas are stated at the top of mesh_color.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dh {
namespace {
constexpr uint64_t MK_EMPTY = ~(uint64_t)0;

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
}  // namespace
}  // namespace dh
