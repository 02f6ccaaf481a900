// Sphere tracing of the SDF for novel views and depth maps (dynhor_amd/surface_render.py; DESIGN_NEXT_ROWS.md section 17).
//
// The network query itself is dh_sdf_nograd / dh_hash_sdf_nograd; these kernels are the per-ray work around it: rays of F poses at
// once (trace_init), one step of the marching / bracketing state machine for the listed rays (trace_step), order-preserving
// compaction of the live rays (trace_compact: per-block counts, one scan, emit -- the packed order is the order of the incoming
// list, no atomics, so the same inputs give the same bits) and the image buffers (trace_compose).
// Every kernel is stateless: the per-ray state lives in caller-owned structure-of-arrays buffers, one thread per ray.
// HBM-bound / latency-bound fp32 work -- no MFMA here by design.
//
// The state machine's products go through a one-instruction asm (mul_rn.h, as march.hip's do) so that nothing is contracted into an
// fma: tests/trace_util.py restates the step in separately rounded fp32 operations and the two agree bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "mul_rn.h"

namespace dh {

namespace {

enum : uint8_t { T_MARCH = 0, T_REFINE = 1, T_HIT = 2, T_MISS = 3, T_FAIL = 4 };
enum : uint8_t { TF_INSIDE = 1, TF_CAPPED = 2 };

__device__ __forceinline__ bool tr_live(uint8_t st) { return st == T_MARCH || st == T_REFINE; }

// count of `flag` over the threads of a 256-thread block before this one (the return value), and the block's total
__device__ __forceinline__ int block_prefix(bool flag, int& total) {
    __shared__ int wave_cnt[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        before += w < wave ? wave_cnt[w] : 0;
        total += wave_cnt[w];
    }
    return before + __popcll(m & ((1ull << lane) - 1ull));      // exclusive prefix
}

}  // namespace

// ---------------------------------------------------------------- rays of F poses
// o, d: gen_rays_kernel's expressions (kernels_ray.hip), term for term.  near / far: the true intersection with the sphere of radius
// `bound`, in fp64 from the fp32 o and d (b^2 and |o|^2 - bound^2 cancel to a few 1e-7 in fp32, which the square root of a small
// discriminant would magnify).
__global__ __launch_bounds__(256) void trace_init_kernel(const float* __restrict__ R, const float* __restrict__ T,
                                                         const float* __restrict__ Kinv, int h, int w, int level, float bound,
                                                         int64_t N, float* __restrict__ o_out, float* __restrict__ d_out,
                                                         float* __restrict__ t, float* __restrict__ t_far, uint8_t* __restrict__ state) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int64_t hw = (int64_t)h * w;
    const int64_t frame = i / hw, rem = i - frame * hw;
    const int64_t y = (rem / w) * level, x = (rem % w) * level;
    const float u = (float)x, v = (float)y;
    float p[3], dcam[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = Kinv[r * 3 + 0] * u + Kinv[r * 3 + 1] * v + Kinv[r * 3 + 2];
    const float inv = 1.f / sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) dcam[r] = p[r] * inv;
    const float* Rf = R + frame * 9;
    const float* Tf = T + frame * 3;
    float o[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {          // d = R^T dcam ; o = -R^T T
        d[c] = Rf[0 * 3 + c] * dcam[0] + Rf[1 * 3 + c] * dcam[1] + Rf[2 * 3 + c] * dcam[2];
        o[c] = -(Rf[0 * 3 + c] * Tf[0] + Rf[1 * 3 + c] * Tf[1] + Rf[2 * 3 + c] * Tf[2]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) d_out[i * 3 + c] = d[c];
    if (rem == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o_out[frame * 3 + c] = o[c];
    }
    const double b = (double)o[0] * d[0] + (double)o[1] * d[1] + (double)o[2] * d[2];
    const double cc = (double)o[0] * o[0] + (double)o[1] * o[1] + (double)o[2] * o[2] - (double)bound * (double)bound;
    const double disc = b * b - cc;
    float tn = 0.f, tf = 0.f;
    uint8_t st = T_MISS;
    if (disc > 0.0) {
        const double sq = sqrt(disc);
        const double near = -b - sq, far = -b + sq;
        tn = (float)(near > 0.0 ? near : 0.0);
        tf = (float)far;
        if (far > 0.0) st = T_MARCH;
    }
    t[i] = tn;
    t_far[i] = tf;
    state[i] = st;
}

// ---------------------------------------------------------------- one step of the state machine
struct TraceArrays {
    float* t; const float* t_far; float* t_lo; float* s_lo; float* t_hi; float* s_hi;
    uint8_t* state; uint16_t* nq; uint8_t* nref; uint8_t* flags;
};

__global__ __launch_bounds__(256) void trace_step_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ count,
                                                         const float* __restrict__ s_in, const float* __restrict__ o,
                                                         const float* __restrict__ d, int64_t rays_per_view, int64_t N, TraceArrays a,
                                                         float eps, float relax, float min_step, float max_step, int refine_steps,
                                                         int64_t n_max, float* __restrict__ pts) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_max || (count && k >= (int64_t)*count)) return;
    const int64_t r = idx[k];
    if (r < 0 || r >= N) return;                         // (a list that does not belong to these arrays: touch nothing)
    uint8_t st = a.state[r];
    float t = a.t[r];
    if (tr_live(st)) {
        const float s = s_in[k];
        const uint16_t q = a.nq[r];
        uint8_t fl = a.flags[r];
        bool secant = false;
        float t_lo = a.t_lo[r], s_lo = a.s_lo[r], t_hi = a.t_hi[r], s_hi = a.s_hi[r];
        if (!(fabsf(s) <= 3.4028234663852886e38f)) {     // NaN or +-inf
            st = T_FAIL;
        } else if (fabsf(s) <= eps) {
            st = T_HIT;
        } else if (st == T_MARCH) {
            if (s < 0.f) {
                if (q == 0) {
                    st = T_HIT;
                    fl |= TF_INSIDE;
                } else {
                    t_hi = t; s_hi = s;
                    st = T_REFINE;
                    secant = true;
                }
            } else {
                t_lo = t; s_lo = s;
                float stp = mul_rn(relax, s);
                stp = stp < min_step ? min_step : (stp > max_step ? max_step : stp);
                const float tn = t + stp;
                if (tn > a.t_far[r]) st = T_MISS; else t = tn;
            }
        } else {
            if (s > 0.f) { t_lo = t; s_lo = s; } else { t_hi = t; s_hi = s; }
            const int c = (int)a.nref[r] + 1;
            a.nref[r] = (uint8_t)(c > 255 ? 255 : c);
            if (c >= refine_steps) {
                st = T_HIT;
                fl |= TF_CAPPED;
            } else if (t_hi - t_lo <= eps) {
                st = T_HIT;
            } else {
                secant = true;
            }
        }
        if (secant) {
            const float w = t_hi - t_lo;
            const float m = mul_rn(0.1f, w);
            const float lo = t_lo + m, hi = t_hi - m;
            float tn = t_lo + mul_rn(w, s_lo / (s_lo - s_hi));
            tn = tn >= lo ? tn : lo;                     // (a NaN secant point lands on lo)
            tn = tn <= hi ? tn : hi;
            t = tn;
        }
        a.t[r] = t;
        a.t_lo[r] = t_lo; a.s_lo[r] = s_lo; a.t_hi[r] = t_hi; a.s_hi[r] = s_hi;
        a.state[r] = st;
        a.flags[r] = fl;
        a.nq[r] = q == 65535 ? q : (uint16_t)(q + 1);
    }
    const int64_t view = r / rays_per_view;
#pragma unroll
    for (int c = 0; c < 3; ++c) pts[k * 3 + c] = __fmaf_rn(t, d[r * 3 + c], o[view * 3 + c]);   // one rounding: |t d| > |p|
}

// ---------------------------------------------------------------- the query points of listed rays, whatever their state
__global__ __launch_bounds__(256) void trace_points_kernel(const int32_t* __restrict__ idx, const float* __restrict__ o,
                                                           const float* __restrict__ d, const float* __restrict__ t,
                                                           int64_t rays_per_view, int64_t N, int64_t n, float* __restrict__ pts) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t r = idx[k];
    if (r < 0 || r >= N) return;
    const int64_t view = r / rays_per_view;
    const float tt = t[r];
#pragma unroll
    for (int c = 0; c < 3; ++c) pts[k * 3 + c] = __fmaf_rn(tt, d[r * 3 + c], o[view * 3 + c]);
}

// ---------------------------------------------------------------- order-preserving compaction of the live rays
// MODE 0: survivors per block of 256 list entries; MODE 1: the survivors' indices and next query points, densely, in list order.
// idx == null: the list is 0 .. n_max-1.
template <int MODE>
__global__ __launch_bounds__(256) void trace_compact_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ count,
                                                            const uint8_t* __restrict__ state, const float* __restrict__ o,
                                                            const float* __restrict__ d, const float* __restrict__ t,
                                                            int64_t rays_per_view, int64_t N, int64_t n_max,
                                                            int32_t* __restrict__ block_off, int32_t* __restrict__ idx_out,
                                                            float* __restrict__ pts_out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = count ? (int64_t)*count : n_max;
    int64_t r = -1;
    if (k < n_max && k < n) r = idx ? (int64_t)idx[k] : k;
    const bool keep = r >= 0 && r < N && tr_live(state[r]);
    int total;
    const int before = block_prefix(keep, total);
    if (MODE == 0) {
        if (threadIdx.x == 0) block_off[blockIdx.x] = total;
    } else if (keep) {
        const int64_t pos = (int64_t)block_off[blockIdx.x] + before;
        idx_out[pos] = (int32_t)r;
        const int64_t view = r / rays_per_view;
        const float tt = t[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) pts_out[pos * 3 + c] = __fmaf_rn(tt, d[r * 3 + c], o[view * 3 + c]);
    }
}

// exclusive scan of the nb per-block counts in place, the total to count_out: one block of 1024 threads, every thread a contiguous
// run of ceil(nb / 1024) counts
__global__ __launch_bounds__(1024) void trace_scan_kernel(int32_t* __restrict__ block_off, int64_t nb, int32_t* __restrict__ count_out) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (nb + 1023) / 1024;
    const int64_t b0 = tid * per, b1 = b0 + per < nb ? b0 + per : nb;
    int sum = 0;
    for (int64_t b = b0; b < b1; ++b) sum += block_off[b];
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;                                  // exclusive prefix of this thread's run
    for (int64_t b = b0; b < b1; ++b) {
        const int c = block_off[b];
        block_off[b] = run;
        run += c;
    }
    if (tid == 1023) *count_out = part[1023];
}

// ---------------------------------------------------------------- image buffers
// One thread per ray.  depth = t (R d)_z, the camera z of the hit (the camera sits at o); the products are rounded separately so
// that a tensor expression of the same operations gives the same bits.
__global__ __launch_bounds__(256) void trace_compose_kernel(const uint8_t* __restrict__ state, const float* __restrict__ t,
                                                            const float* __restrict__ d, const int32_t* __restrict__ slot,
                                                            const float* __restrict__ normals, const float* __restrict__ colors,
                                                            int64_t n_hits, const float* __restrict__ R, int h, int w, int level,
                                                            int H, int W, int background, const uint8_t* __restrict__ frame_rgb,
                                                            const int32_t* __restrict__ frame_idx, int n_frames, int64_t N,
                                                            uint8_t* __restrict__ rgb, float* __restrict__ depth,
                                                            uint8_t* __restrict__ normal, uint8_t* __restrict__ hit) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int64_t hw = (int64_t)h * w;
    const int64_t view = i / hw, rem = i - view * hw;
    const int64_t sl = state[i] == T_HIT ? (int64_t)slot[i] : -1;
    const bool is_hit = sl >= 0 && sl < n_hits;
    hit[i] = is_hit ? 1 : 0;
    if (is_hit) {
        const float* Rv = R + view * 9;
        const float dz = (mul_rn(Rv[6], d[i * 3 + 0]) + mul_rn(Rv[7], d[i * 3 + 1])) + mul_rn(Rv[8], d[i * 3 + 2]);
        depth[i] = mul_rn(t[i], dz);
        const float n0 = normals[sl * 3 + 0], n1 = normals[sl * 3 + 1], n2 = normals[sl * 3 + 2];
        float nc[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) nc[r] = (mul_rn(Rv[r * 3 + 0], n0) + mul_rn(Rv[r * 3 + 1], n1)) + mul_rn(Rv[r * 3 + 2], n2);
        const float len = sqrtf((mul_rn(nc[0], nc[0]) + mul_rn(nc[1], nc[1])) + mul_rn(nc[2], nc[2])) + 1e-6f;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            float e = mul_rn(nc[r] / len, 0.5f) + 0.5f;
            e = e >= 0.f ? e : 0.f;                                   // (NaN -> 0)
            e = e <= 1.f ? e : 1.f;
            normal[i * 3 + r] = (uint8_t)mul_rn(e, 255.f);            // truncation: validate_image's encoding
            float c = colors[sl * 3 + r];
            c = c >= 0.f ? c : 0.f;
            c = c <= 1.f ? c : 1.f;
            rgb[i * 3 + r] = (uint8_t)rintf(mul_rn(c, 255.f));
        }
    } else {
        depth[i] = __builtin_inff();
#pragma unroll
        for (int r = 0; r < 3; ++r) normal[i * 3 + r] = 127;                // (a zero normal in the same encoding)
        if (background == 2) {
            const int64_t y = (rem / w) * level, x = (rem % w) * level;
            const int64_t fi = frame_idx[view];
            const int64_t pix = ((fi * H + y) * W + x) * 3;
#pragma unroll
            for (int r = 0; r < 3; ++r) rgb[i * 3 + r] = fi >= 0 && fi < n_frames ? frame_rgb[pix + r] : 0;   // (no frame: black)
        } else {
            const uint8_t v = background == 0 ? 255 : 0;
#pragma unroll
            for (int r = 0; r < 3; ++r) rgb[i * 3 + r] = v;
        }
    }
}

// ---------------------------------------------------------------- launchers
static inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

int launch_trace_init(const float* R, const float* T, const float* Kinv, int h, int w, int level, float bound, int64_t N, float* o,
                      float* d, float* t, float* t_far, uint8_t* state, hipStream_t st) {
    hipLaunchKernelGGL(trace_init_kernel, dim3(blocks256(N)), dim3(256), 0, st, R, T, Kinv, h, w, level, bound, N, o, d, t, t_far, state);
    return ok();
}

int launch_trace_step(const int32_t* idx, const int32_t* count, const float* s, const float* o, const float* d, int64_t rays_per_view,
                      int64_t N, float* t, const float* t_far, float* t_lo, float* s_lo, float* t_hi, float* s_hi, uint8_t* state,
                      uint16_t* nq, uint8_t* nref, uint8_t* flags, float eps, float relax, float min_step, float max_step,
                      int refine_steps, int64_t n_max, float* pts, hipStream_t st) {
    TraceArrays a{t, t_far, t_lo, s_lo, t_hi, s_hi, state, nq, nref, flags};
    hipLaunchKernelGGL(trace_step_kernel, dim3(blocks256(n_max)), dim3(256), 0, st, idx, count, s, o, d, rays_per_view, N, a, eps,
                       relax, min_step, max_step, refine_steps, n_max, pts);
    return ok();
}

int launch_trace_points(const int32_t* idx, const float* o, const float* d, const float* t, int64_t rays_per_view, int64_t N, int64_t n,
                        float* pts, hipStream_t st) {
    hipLaunchKernelGGL(trace_points_kernel, dim3(blocks256(n)), dim3(256), 0, st, idx, o, d, t, rays_per_view, N, n, pts);
    return ok();
}

int launch_trace_compact(const int32_t* idx, const int32_t* count, const uint8_t* state, const float* o, const float* d, const float* t,
                         int64_t rays_per_view, int64_t N, int64_t n_max, int32_t* block_off, int32_t* idx_out, int32_t* count_out,
                         float* pts_out, hipStream_t st) {
    const unsigned nb = blocks256(n_max);
    if (nb > 0)
        hipLaunchKernelGGL(trace_compact_kernel<0>, dim3(nb), dim3(256), 0, st, idx, count, state, o, d, t, rays_per_view, N, n_max,
                           block_off, idx_out, pts_out);
    hipLaunchKernelGGL(trace_scan_kernel, dim3(1), dim3(1024), 0, st, block_off, (int64_t)nb, count_out);
    if (nb > 0)
        hipLaunchKernelGGL(trace_compact_kernel<1>, dim3(nb), dim3(256), 0, st, idx, count, state, o, d, t, rays_per_view, N, n_max,
                           block_off, idx_out, pts_out);
    return ok();
}

int launch_trace_compose(const uint8_t* state, const float* t, const float* d, const int32_t* slot, const float* normals,
                         const float* colors, int64_t n_hits, const float* R, int h, int w, int level, int H, int W, int background,
                         const uint8_t* frame_rgb, const int32_t* frame_idx, int n_frames, int64_t N, uint8_t* rgb, float* depth,
                         uint8_t* normal, uint8_t* hit, hipStream_t st) {
    hipLaunchKernelGGL(trace_compose_kernel, dim3(blocks256(N)), dim3(256), 0, st, state, t, d, slot, normals, colors, n_hits, R, h, w,
                       level, H, W, background, frame_rgb, frame_idx, n_frames, N, rgb, depth, normal, hit);
    return ok();
}

}  // namespace dh
