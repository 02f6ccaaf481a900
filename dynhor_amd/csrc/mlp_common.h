// Helpers shared by the forward and backward MLP chain kernels.
#pragma once
#include "tile.h"
#include "tile16.h"

namespace dh {

// ------------------------------------------------------------------------------------------------
// positional embedding of 128 points into the LDS aux image: [x, sin(2^k x), cos(2^k x)]_{k<6}  (App. A.1)
// 256 threads: thread handles point tid&127 and frequencies 3*(tid>>7) .. +2.
// ------------------------------------------------------------------------------------------------
constexpr int TPP = 256 / TM;      // threads per point in the per-point VALU phases (2 or 4)
__device__ __forceinline__ void embed_tile(const float* __restrict__ pts, int64_t base, int64_t npts, float* aux, int tid) {
    const int p = tid & (TM - 1), part = tid / TM;
    const int64_t gp = base + p;
    float x[3] = {0.f, 0.f, 0.f};
    if (gp < npts) { x[0] = pts[gp * 3 + 0]; x[1] = pts[gp * 3 + 1]; x[2] = pts[gp * 3 + 2]; }
    float* row = aux + p * LDA;
    if (part == 0) { row[0] = x[0]; row[1] = x[1]; row[2] = x[2]; }
    if (part == 1) { for (int c = 39; c < LDA; ++c) row[c] = 0.f; }
    for (int k = part; k < 6; k += TPP) {
        const float f = (float)(1 << k);
        DH_UNROLL for (int c = 0; c < 3; ++c) {
            float s, co;
            sincosf(x[c] * f, &s, &co);
            row[3 + 6 * k + c] = s;
            row[3 + 6 * k + 3 + c] = co;
        }
    }
}

template <class F>
__device__ __forceinline__ void acc_map(f32x16 (&acc)[MT][2], F f) {
    DH_UNROLL for (int m = 0; m < MT; ++m)
        DH_UNROLL for (int t = 0; t < 2; ++t)
            DH_UNROLL for (int r = 0; r < 16; ++r) acc[m][t][r] = f(m, t, r, acc[m][t][r]);
}

// per-point dot of the LDS main tile rows with a 256-vector: TPP threads per point (point = tid / TPP), result
// valid on every thread of the group
__device__ __forceinline__ float row_dot256(const float* main, const float* __restrict__ w, int tid) {
    constexpr int SEG = 256 / TPP;
    const int p = tid / TPP, part = tid % TPP;
    const f32x4* xr = reinterpret_cast<const f32x4*>(main + p * LDX + part * SEG);
    const f32x4* wr = reinterpret_cast<const f32x4*>(w + part * SEG);
    float s = 0.f;
    DH_UNROLL for (int i = 0; i < SEG / 4; ++i) {
        const f32x4 a = xr[i], b = wr[i];
        s = fmaf(a[0], b[0], s); s = fmaf(a[1], b[1], s); s = fmaf(a[2], b[2], s); s = fmaf(a[3], b[3], s);
    }
    DH_UNROLL for (int off = 1; off < TPP; off <<= 1) s += __shfl_xor(s, off);
    return s;
}

struct SdfPtrs {
    const f32x4* fwd_main[N_SDF];
    const f32x4* fwd_aux[N_SDF];
    const f32x4* rev_main[N_SDF];
    const f32x4* rev_aux[N_SDF];
    const float* bias[N_SDF];
    const float* w8row0;
    const float* b8_0;
};

static inline SdfPtrs make_sdf_ptrs(const float* packed) {
    SdfPtrs P;
    for (int l = 0; l < N_SDF; ++l) {
        P.fwd_main[l] = reinterpret_cast<const f32x4*>(packed + PACK.sdf_fwd_main[l]);
        P.fwd_aux[l] = reinterpret_cast<const f32x4*>(packed + PACK.sdf_fwd_aux[l]);
        P.rev_main[l] = reinterpret_cast<const f32x4*>(packed + PACK.sdf_rev_main[l]);
        P.rev_aux[l] = reinterpret_cast<const f32x4*>(packed + PACK.sdf_rev_aux[l]);
        P.bias[l] = packed + PACK.sdf_bias[l];
    }
    P.w8row0 = packed + PACK.sdf_w8row0;
    P.b8_0 = packed + PACK.sdf_b8_0;
    return P;
}

struct ColPtrs {
    const f32x4* fwd_main[4];
    const f32x4* rev_main[4];
    const f32x4* fwd_aux0;
    const f32x4* rev_aux0;
    const float* bias[4];
    const float* w4;
    const float* b4;
};
static inline ColPtrs make_col_ptrs(const float* packed) {
    ColPtrs C;
    for (int l = 0; l < 4; ++l) {
        C.fwd_main[l] = reinterpret_cast<const f32x4*>(packed + PACK.col_fwd_main[l]);
        C.rev_main[l] = reinterpret_cast<const f32x4*>(packed + PACK.col_rev_main[l]);
        C.bias[l] = packed + PACK.col_bias[l];
    }
    C.fwd_aux0 = reinterpret_cast<const f32x4*>(packed + PACK.col_fwd_aux0);
    C.rev_aux0 = reinterpret_cast<const f32x4*>(packed + PACK.col_rev_aux0);
    C.w4 = packed + PACK.col_w4;
    C.b4 = packed + PACK.col_b4;
    return C;
}


// ---- pointers into the split-bf16 packed weights (layout.h PACK16): the members of SdfPtrs / ColPtrs
struct Sdf16Ptrs {
    const bf16x8* fwd_main[N_SDF];
    const bf16x8* fwd_aux[N_SDF];
    const bf16x8* rev_main[N_SDF];
    const bf16x8* rev_aux[N_SDF];
    const float* bias[N_SDF];
    const float* w8row0;
    const float* b8_0;
};
static inline Sdf16Ptrs make_sdf16_ptrs(const float* packed) {
    Sdf16Ptrs P;
    for (int l = 0; l < N_SDF; ++l) {
        P.fwd_main[l] = reinterpret_cast<const bf16x8*>(packed + PACK16.sdf_fwd_main[l]);
        P.fwd_aux[l] = reinterpret_cast<const bf16x8*>(packed + PACK16.sdf_fwd_aux[l]);
        P.rev_main[l] = reinterpret_cast<const bf16x8*>(packed + PACK16.sdf_rev_main[l]);
        P.rev_aux[l] = reinterpret_cast<const bf16x8*>(packed + PACK16.sdf_rev_aux[l]);
        P.bias[l] = packed + PACK.sdf_bias[l];
    }
    P.w8row0 = packed + PACK.sdf_w8row0;
    P.b8_0 = packed + PACK.sdf_b8_0;
    return P;
}

struct Col16Ptrs {
    const bf16x8* fwd_main[4];
    const bf16x8* rev_main[4];
    const bf16x8* fwd_aux0;
    const bf16x8* rev_aux0;
    const float* bias[4];
    const float* w4;
    const float* b4;
};
static inline Col16Ptrs make_col16_ptrs(const float* packed) {
    Col16Ptrs C;
    for (int l = 0; l < 4; ++l) {
        C.fwd_main[l] = reinterpret_cast<const bf16x8*>(packed + PACK16.col_fwd_main[l]);
        C.rev_main[l] = reinterpret_cast<const bf16x8*>(packed + PACK16.col_rev_main[l]);
        C.bias[l] = packed + PACK.col_bias[l];
    }
    C.fwd_aux0 = reinterpret_cast<const bf16x8*>(packed + PACK16.col_fwd_aux0);
    C.rev_aux0 = reinterpret_cast<const bf16x8*>(packed + PACK16.col_rev_aux0);
    C.w4 = packed + PACK.col_w4;
    C.b4 = packed + PACK.col_b4;
    return C;
}

// ---- GEMM cores of the fp32-MFMA and split-bf16 tile chains (kernels_mlp.hip, kernels_mlp_bwd.hip: one body per stage, templated
// on the core).  A core carries what the two arithmetics do differently: the weight-pointer structs, the k-step counts of a 256-deep
// input, of layer 4's 217 main columns and of the aux image, the next layer's B-fragment prefetch (fp32 only; an empty no-op in the
// bf16 core), and how the tangent and SDF-backward chains stream their saved tiles (fp32 plain, bf16 non-temporal).  STAMPS: the
// chain carries the -DDH_STAMPS phase stamps (stamps.h).
struct CoreF32 {                                  // tile.h: v_mfma_f32_32x32x2_f32, k-groups of 8
    typedef SdfPtrs Sdf;
    typedef ColPtrs Col;
    static constexpr int K_MAIN = 32, K_L4 = 28, K_AUX = 5;
    static constexpr bool STAMPS = false;
    typedef BFrag Pre;
    static __device__ __forceinline__ Pre prefetch(const f32x4* wp, int wave, int lane) { return gemm_b_prefetch(wp, wave, lane); }
    static __device__ __forceinline__ void rows(f32x16 (&acc)[MT][2], const float* xs, int ldx, int nk, const f32x4* wp, int wave,
                                                int lane, const Pre& pre) {
        gemm_rows(acc, xs, ldx, nk, wp, wave, lane, pre);
    }
    static __device__ __forceinline__ void rows(f32x16 (&acc)[MT][2], const float* xs, int ldx, int nk, const f32x4* wp, int wave,
                                                int lane) {
        gemm_rows(acc, xs, ldx, nk, wp, wave, lane);
    }
    static __device__ __forceinline__ void auxout(f32x16 (&acc2)[AUX_NTW], const float* xs, const f32x4* wp, int wave, int lane) {
        gemm_auxout(acc2, xs, K_MAIN, wp, wave, lane);
    }
    static __device__ __forceinline__ f32x4 saved_ld(const f32x4* p) { return *p; }
    static __device__ __forceinline__ void saved_st(f32x4* p, const f32x4& v) { *p = v; }
};
struct CoreBf16 {                                 // tile16.h: split-on-fetch, k-chunks of 16
    typedef Sdf16Ptrs Sdf;
    typedef Col16Ptrs Col;
    static constexpr int K_MAIN = 16, K_L4 = 14, K_AUX = AUX_KC;
    static constexpr bool STAMPS = true;
    struct Pre {};
    static __device__ __forceinline__ Pre prefetch(const bf16x8*, int, int) { return Pre(); }
    static __device__ __forceinline__ void rows(f32x16 (&acc)[MT][2], const float* xs, int ldx, int nk, const bf16x8* wp, int wave,
                                                int lane, const Pre& = Pre()) {
        gemm_rows_s(acc, xs, ldx, nk, wp, wave, lane);
    }
    static __device__ __forceinline__ void auxout(f32x16 (&acc2)[AUX_NTW], const float* xs, const bf16x8* wp, int wave, int lane) {
        gemm_auxout_s(acc2, xs, K_MAIN, wp, wave, lane);
    }
    static __device__ __forceinline__ f32x4 saved_ld(const f32x4* p) { return DH_TILE_LD(p); }
    static __device__ __forceinline__ void saved_st(f32x4* p, const f32x4& v) { DH_TILE_ST(p, v); }
};

// column sums of a [TM x 256] accumulator tile -> dst[256]
__device__ __forceinline__ void tile_colsum(const f32x16 (&acc)[MT][2], float* __restrict__ dst, int wave, int lane) {
    DH_UNROLL for (int t = 0; t < 2; ++t) {
        float s = 0.f;
        DH_UNROLL for (int m = 0; m < MT; ++m)
            DH_UNROLL for (int r = 0; r < 16; ++r) s += acc[m][t][r];
        s += __shfl_xor(s, 32);
        if (lane < 32) dst[64 * wave + 32 * t + lane] = s;
    }
}

// ---- per-point tails of the fp32-MFMA / split-bf16 chains that end in the aux image, one point per call.  The split-fp16 tile and
// pair kernels (kernels_mlp_h.hip, chain_pair.hip) keep their own copies of this text: calling these there changes their listings.
// aux accumulators, columns < ncol -> the LDS aux image
__device__ __forceinline__ void aux_acc_to_lds(const f32x16 (&a2)[AUX_NTW], float* aux, int ncol, int wave, int lane) {
    DH_UNROLL for (int tt = 0; tt < AUX_NTW; ++tt) {
        const int col = aux_col(wave, tt, lane);
        if (col < ncol) {
            DH_UNROLL for (int r = 0; r < 16; ++r) aux[aux_row(wave, r, lane) * LDA + col] = a2[tt][r];
        }
    }
}
// input gradient: n = J_e(x)^T ge of point gp, g = its ge row (d sdf / d embedding); save == 2 also keeps ge (pose refinement)
__device__ __forceinline__ void point_normal(const float* g, const float* pts, int64_t gp, float* normals, int save, float* gesave) {
    float n[3];
    DH_UNROLL for (int c = 0; c < 3; ++c) {
        const float x = pts[gp * 3 + c];
        float v = g[c];
        DH_UNROLL for (int k = 0; k < 6; ++k) {
            const float f = (float)(1 << k);
            float s, co; sincosf(x * f, &s, &co);
            v += f * (co * g[3 + 6 * k + c] - s * g[3 + 6 * k + 3 + c]);
        }
        n[c] = v;
    }
    normals[gp * 3 + 0] = n[0]; normals[gp * 3 + 1] = n[1]; normals[gp * 3 + 2] = n[2];
    if (save == 2) { for (int c = 0; c < 40; ++c) gesave[gp * 40 + c] = c < EMB ? g[c] : 0.f; }
}
// colour backward, pose refinement: row = point gp's adjoint of the extras [p, embed_4(view), n] -> the adjoints of the sample point
// (columns 0..2, WRITTEN to d_pts) and of the ray direction through the view embedding (columns 3..29, written to d_dirs_pts)
__device__ __forceinline__ void point_view_adjoint(const float* row, const float* dirs, int n_per_ray, int64_t gp, float* d_pts,
                                                   float* d_dirs_pts) {
    const int64_t ray = gp / n_per_ray;
    DH_UNROLL for (int c = 0; c < 3; ++c) {
        d_pts[gp * 3 + c] = row[c];
        const float dv = dirs[ray * 3 + c];
        float v = row[3 + c];
        DH_UNROLL for (int kf = 0; kf < 4; ++kf) {
            const float f = (float)(1 << kf);
            float sn, co; sincosf(dv * f, &sn, &co);
            v += f * (co * row[6 + 6 * kf + c] - sn * row[6 + 6 * kf + 3 + c]);
        }
        d_dirs_pts[gp * 3 + c] = v;
    }
}
// SDF backward, pose refinement: e = point gp's ebar row (adjoint of the embedding) ->
//   xbar = J_e(x)^T ebar + nbar * d/dx [J_e(x)^T] ge,  ACCUMULATED onto d_pts  (ge: gesave, kept by the input gradient's save == 2)
__device__ __forceinline__ void point_sdf_adjoint(const float* e, const float* pts, const float* d_normals, const float* gesave,
                                                  int64_t gp, float* d_pts) {
    const float* ge = gesave + gp * 40;
    DH_UNROLL for (int c = 0; c < 3; ++c) {
        const float x = pts[gp * 3 + c], nb = d_normals[gp * 3 + c];
        float v = e[c], dn = 0.f;
        DH_UNROLL for (int k = 0; k < 6; ++k) {
            const float f = (float)(1 << k);
            float sn, co; sincosf(x * f, &sn, &co);
            v += f * (co * e[3 + 6 * k + c] - sn * e[3 + 6 * k + 3 + c]);
            dn -= f * f * (sn * ge[3 + 6 * k + c] + co * ge[3 + 6 * k + 3 + c]);
        }
        d_pts[gp * 3 + c] += v + nb * dn;
    }
}

}  // namespace dh
