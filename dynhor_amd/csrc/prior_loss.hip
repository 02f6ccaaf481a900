// Depth prior and validity-masked normal prior of the training step (include/dynhor_hip.h: dh_prior_loss, dh_prior_loss_packed).
//
// Three launches, no atomics, no host read:
//   1. prior_ray_kernel    grid over rays, ONE WAVE PER RAY (as render_fwd_kernel).  Lane l adds its samples l, l + 64, .. of
//                          t^ = sum_k w_k m_k in ascending k (fp64 fma of the fp32 w_k and m_k), so a row of z and weights is read
//                          coalesced; the 64 lanes then fold in a fixed xor butterfly (offsets 32 .. 1) with every lane active -- the
//                          sample loop is the only divergent part and ends before it, and the ray loop's condition is the same for
//                          the whole wave.  e, rho and rho' are fp64 per ray, the normal cost fp32 as in loss_kernel; lane 0 adds the
//                          ray's values into fp64 sums, sum64_block_store (sums64.h) folds lanes and waves and stores one partial per
//                          workgroup.  The ray's un-normalised coefficient v rho'(e) c_z goes to the workspace as fp32.
//   2. sum64_reduce_kernel (icp.hip) adds the partials in block order.
//   3. prior_write_kernel  one wave per ray again: d_weights[r,k] = depth_weight coef_r / (sum v + 1e-5) m_k, coalesced; lane 0
//                          writes the ray's d_normal_map; thread 0 of workgroup 0 writes stats.
// Workgroup g owns the rays 4 g + wave + 4 j gridDim; the grid depends on B alone, so a result is bitwise the same from launch to
// launch.  Packed rays (occupancy-grid marching): ray r owns [seg_off[r], seg_off[r] + min(seg_cnt[r], max_samples)) of the packed
// arrays and m_k = t_start[k] + 0.5 step, the packed scan's own mid-point (render_elem in kernels_ray.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "ray_row.h"
#include "sums64.h"

namespace dh {

namespace {
constexpr int PR_THREADS = SUM64_THREADS;
constexpr int PR_WAVES = PR_THREADS / 64;         // rays per workgroup and trip
constexpr int PR_SUMS = 5;                        // sum v rho, sum v, sum v |e|, sum nw (l1 + 1 - cos), sum nw
constexpr int PR_SUMS_PAD = 8;                    // doubles kept for the reduced sums (the coefficients after them stay 16-byte aligned)
constexpr int64_t PR_MAX_BLOCKS = 1024;           // 4 workgroups per CU; more rays loop

inline int64_t prior_blocks(int64_t B) {
    const int64_t b = (B + PR_WAVES - 1) / PR_WAVES;
    return b < 1 ? 1 : (b < PR_MAX_BLOCKS ? b : PR_MAX_BLOCKS);
}

__device__ __forceinline__ float sgn(float e) { return e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f); }

// the normal prior of one ray, loss_kernel's (optim.hip) operations: cost = L1 + (1 - cos) between normalize(R n) and mono;
// with grad also normal_w * weight / nsum * d cost / d n (object frame), exact zeros where the weight is 0
struct PriorNormal { float cost, wgt; };
__device__ __forceinline__ PriorNormal prior_normal(const float* __restrict__ rays, const float* __restrict__ nmap,
                                                    const float (&Rm)[9], int64_t ray, float m, bool grad, float normal_w,
                                                    float nsum, float (&d_no)[3]) {
    float no[3], nc[3], mono[3], nh[3], dnh[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { no[c] = nmap[ray * 3 + c]; mono[c] = rays[ray * 14 + 11 + c]; }
    const float has = (mono[0] * mono[0] + mono[1] * mono[1] + mono[2] * mono[2] >= 0.25f) ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) nc[i] = Rm[i * 3] * no[0] + Rm[i * 3 + 1] * no[1] + Rm[i * 3 + 2] * no[2];
    const float nn = sqrtf(nc[0] * nc[0] + nc[1] * nc[1] + nc[2] * nc[2]);
    const float nrm = nn + 1e-6f;
    PriorNormal r;
    r.wgt = m * has;
    float l1 = 0.f, cs = 0.f, dd = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        nh[i] = nc[i] / nrm;
        const float e = nh[i] - mono[i];
        l1 += fabsf(e);
        cs += nh[i] * mono[i];
        dnh[i] = normal_w * r.wgt / nsum * (sgn(e) - mono[i]);
        dd += dnh[i] * nc[i];
    }
    r.cost = r.wgt > 0.f ? (l1 + 1.f - cs) * r.wgt : 0.f;     // a ray without a normal adds an exact zero whatever its map holds
    if (grad) {
        float dnc[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) dnc[i] = dnh[i] / nrm - (nn > 0.f ? nc[i] * dd / (nn * nrm * nrm) : 0.f);
#pragma unroll
        for (int j = 0; j < 3; ++j) d_no[j] = r.wgt > 0.f ? Rm[j] * dnc[0] + Rm[3 + j] * dnc[1] + Rm[6 + j] * dnc[2] : 0.f;
    }
    return r;
}
}  // namespace

static_assert(PR_SUMS <= PR_THREADS && PR_SUMS <= PR_SUMS_PAD, "sum64_block_store stores one sum per thread");

// partial [gridDim.x, PR_SUMS] doubles, coef [B]
__global__ __launch_bounds__(PR_THREADS) void prior_ray_kernel(const float* __restrict__ rays, const float* __restrict__ R,
                                                               const float* __restrict__ z, const float* __restrict__ weights,
                                                               const float* __restrict__ nmap, const float* __restrict__ prior,
                                                               int64_t B, int n, const int64_t* __restrict__ seg_off,
                                                               const int32_t* __restrict__ seg_cnt, int max_samples,
                                                               float sample_dist, float delta, double* __restrict__ partial,
                                                               float* __restrict__ coef) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool packed = seg_off != nullptr;
    float Rm[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rm[i] = R[i];
    double acc[PR_SUMS];
#pragma unroll
    for (int k = 0; k < PR_SUMS; ++k) acc[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * PR_WAVES;
    for (int64_t ray = (int64_t)blockIdx.x * PR_WAVES + wave; ray < B; ray += stride) {      // the same trip count for a whole wave
        const float m = rays[ray * 14 + 9] * rays[ray * 14 + 10];                            // obj * keep
        if (prior) {
            const PriorRow row = prior_row(ray, n, seg_off, seg_cnt, max_samples);
            // fp64 from the fp32 inputs: e is what is left of z^ - prior, a few thousandths of a depth near 2, and rho' = e / delta on the
            // quadratic branch passes its relative error on to the whole d_weights row
            double t = 0.0;
            for (int k = lane; k < row.n; k += 64)
                t = fma((double)weights[row.rb + k], (double)prior_mid(z, row.rb, k, row.n, packed, sample_dist), t);
            t = sum64_lanes(t);                                                               // every lane: t^
            const double cz = (double)Rm[6] * rays[ray * 14 + 3] + (double)Rm[7] * rays[ray * 14 + 4] + (double)Rm[8] * rays[ray * 14 + 5];
            const float p = prior[ray];
            const bool v = (m > 0.f) && (p > 1e-3f) && (p < __builtin_inff()) && (row.n >= 1);   // NaN fails both comparisons
            const double e = v ? t * cz - (double)p : 0.0;
            const double a = fabs(e), dl = (double)delta;
            const bool in = a <= dl;
            const double rho = in ? e * e / (2.0 * dl) : a - 0.5 * dl;
            const double drho = in ? e / dl : (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0));
            if (lane == 0) {
                coef[ray] = v ? (float)(drho * cz) : 0.f;
                if (v) { acc[0] += rho; acc[1] += 1.0; acc[2] += a; }
            }
        }
        if (nmap) {
            float unused[3];
            const PriorNormal pn = prior_normal(rays, nmap, Rm, ray, m, false, 0.f, 1.f, unused);
            if (lane == 0) { acc[3] += (double)pn.cost; acc[4] += (double)pn.wgt; }
        }
    }
    sum64_block_store(acc, partial + (int64_t)blockIdx.x * PR_SUMS);
}

__global__ __launch_bounds__(PR_THREADS) void prior_write_kernel(const float* __restrict__ rays, const float* __restrict__ R,
                                                                 const float* __restrict__ z, const float* __restrict__ nmap,
                                                                 int64_t B, int n, const int64_t* __restrict__ seg_off,
                                                                 const int32_t* __restrict__ seg_cnt, int max_samples,
                                                                 float sample_dist, float depth_w, float normal_w, int accumulate,
                                                                 const double* __restrict__ sums, const float* __restrict__ coef,
                                                                 float* __restrict__ stats, float* __restrict__ d_weights,
                                                                 float* __restrict__ d_nmap) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool packed = seg_off != nullptr;
    const float vsum = (float)sums[1] + 1e-5f, nsum = (float)sums[4] + 1e-5f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const float ld = (float)sums[0] / vsum, ln = (float)sums[3] / nsum;
        stats[0] = ld; stats[1] = (float)sums[1]; stats[2] = (float)sums[2] / vsum; stats[3] = depth_w * ld;
        stats[4] = ln; stats[5] = (float)sums[4]; stats[6] = normal_w * ln; stats[7] = 0.f;
    }
    float Rm[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rm[i] = R[i];
    const int64_t stride = (int64_t)gridDim.x * PR_WAVES;
    for (int64_t ray = (int64_t)blockIdx.x * PR_WAVES + wave; ray < B; ray += stride) {
        if (d_weights) {
            const PriorRow row = prior_row(ray, n, seg_off, seg_cnt, max_samples);
            const float c = depth_w * coef[ray] / vsum;
            if (!accumulate) {
                for (int k = lane; k < row.n; k += 64) d_weights[row.rb + k] = c != 0.f ? c * prior_mid(z, row.rb, k, row.n, packed, sample_dist) : 0.f;
            } else if (c != 0.f) {                       // adding nothing leaves the buffer's bits alone (-0 + 0 would not)
                for (int k = lane; k < row.n; k += 64) d_weights[row.rb + k] += c * prior_mid(z, row.rb, k, row.n, packed, sample_dist);
            }
        }
        if (d_nmap && lane == 0) {
            const float m = rays[ray * 14 + 9] * rays[ray * 14 + 10];
            float d_no[3];
            prior_normal(rays, nmap, Rm, ray, m, true, normal_w, nsum, d_no);
#pragma unroll
            for (int j = 0; j < 3; ++j) d_nmap[ray * 3 + j] = d_no[j];
        }
    }
}

int64_t prior_loss_workspace(int64_t B) {
    return (prior_blocks(B) * PR_SUMS + PR_SUMS_PAD) * (int64_t)sizeof(double) + B * (int64_t)sizeof(float);
}

int launch_prior_loss(const float* rays, const float* R, const float* z, const float* weights, const float* nmap, const float* prior,
                      int64_t B, int n, const int64_t* seg_off, const int32_t* seg_cnt, int max_samples, float sample_dist,
                      float depth_w, float delta, float normal_w, int accumulate, float* stats, float* d_weights, float* d_nmap,
                      void* ws, hipStream_t st) {
    const int64_t blocks = prior_blocks(B);
    double* partial = static_cast<double*>(ws);
    double* sums = partial + blocks * PR_SUMS;
    float* coef = reinterpret_cast<float*>(sums + PR_SUMS_PAD);
    hipLaunchKernelGGL(prior_ray_kernel, dim3((unsigned)blocks), dim3(PR_THREADS), 0, st, rays, R, z, weights, nmap, prior, B, n, seg_off,
                       seg_cnt, max_samples, sample_dist, delta, partial, coef);
    if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    const int rc = launch_sum64_reduce(partial, 1, (int)blocks, PR_SUMS, sums, st);
    if (rc != DH_OK) return rc;
    hipLaunchKernelGGL(prior_write_kernel, dim3((unsigned)blocks), dim3(PR_THREADS), 0, st, rays, R, z, nmap, B, n, seg_off, seg_cnt,
                       max_samples, sample_dist, depth_w, normal_w, accumulate, sums, coef, stats, prior ? d_weights : nullptr,
                       nmap && normal_w > 0.f ? d_nmap : nullptr);
    return launch_status();
}

}  // namespace dh
