// Multi-view photometric consistency on the training path (include/dynhor_hip.h: dh_ray_depth, dh_warp_loss, dh_ray_depth_bwd;
// DESIGN_NEXT_ROWS.md section 30): the grey patch about a ray's pixel is carried into the neighbouring frames by the homography of the
// plane through the ray's surface point with the rendered normal, scored by normalised cross-correlation, and the mean of the best
// few 1 - score is differentiated with respect to the ray's depth and normal.
//
//   ray_depth_kernel      ONE WAVE PER RAY (as prior_ray_kernel).  Lane l adds its samples l, l + 64, .. of W = sum w_k and
//                         sum w_k m_k in ascending k in fp64, the lanes fold in sums64.h's fixed xor butterfly; t = the quotient,
//                         z = t c_z.
//   warp_ray_kernel       one wave per ray, tap lane + 64 s of the (2P+1)^2 patch in slot s of a lane (one slot at P <= 3, two up to
//                         P = 5, four at P = 7).  The source bytes, the tap's pixel and sigma stay in registers for all
//                         neighbours: nothing is staged in LDS.  Per neighbour (a loop uniform over the wave):
//                           pass 1  the tap's homography in fp32 with no contraction, the four bytes of `valid` and of `gray`, the
//                                   bilinear value b in fp32; a ballot ends the neighbour when any tap failed; sum b, sum b^2 and
//                                   sum a b are fp64 butterflies with every lane active;
//                           pass 2  s_t = d l / d b of the lane's taps from the b it kept, times the tap's grad b . d q / d sigma (fp64 of
//                                   the fp32 coordinates); with rho = (n_c . u) / (n_c . e) in fp64, sum s rho and sum s (u - rho e)
//                                   are reduced: g_z and g_n of the neighbour.
//                         Lane jn (< 8) keeps neighbour jn's l, score and gradient; the top-k choice is a rank by eight broadcasts and
//                         the chosen are added by a three-step butterfly over those eight lanes.  Lane 0 writes the ray's outputs and
//                         adds it to the fp64 sums of its workgroup (sum64_block_store).
//   sum64_reduce_kernel   (icp.hip) adds the partials in block order; warp_stats_kernel turns them into stats [8].
//   ray_depth_bwd_kernel  one wave per ray: d_weights[r,k] (+)= c_r (m_k - t_r) coalesced, lanes 0..2 write d_nmap.
// Workgroup g owns the rays 4 g + wave + 4 j gridDim; the grid depends on B alone.  No atomics, no LDS beyond the block sums, no
// scratch; a ray's outputs depend on that ray's inputs alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "ray_row.h"
#include "sums64.h"

#pragma clang fp contract(off)

namespace dh {

namespace {
constexpr int WL_THREADS = SUM64_THREADS;
constexpr int WL_WAVES = WL_THREADS / 64;          // rays per workgroup and trip
constexpr int WL_MAX_P = 7, WL_MAX_NBR = 8;
constexpr int WL_SLOTS = 4;                        // 15 * 15 = 225 taps <= 4 * 64
constexpr int WL_SUMS = 7;                         // sum l, count, sum mean score, rays with flag 1, 2, 8, 16
constexpr int WL_SUMS_PAD = 8;
constexpr int64_t WL_MAX_BLOCKS = 1024;
constexpr float WL_NONE = -2.0f;
constexpr float WL_Z_MIN = 1e-3f;

inline int64_t warp_blocks(int64_t B) {
    const int64_t b = (B + WL_WAVES - 1) / WL_WAVES;
    return b < 1 ? 1 : (b < WL_MAX_BLOCKS ? b : WL_MAX_BLOCKS);
}

// (a . b) as ((a0 b0 + a1 b1) + a2 b2)
__device__ __forceinline__ float wl_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

__device__ __forceinline__ uint32_t wl_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// the sum over the eight lanes 8 g .. 8 g + 7 of a wave, in every one of them: offsets 4, 2, 1
__device__ __forceinline__ double wl_sum8(double v) {
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
}  // namespace

static_assert(WL_SUMS <= WL_THREADS && WL_SUMS <= WL_SUMS_PAD, "sum64_block_store stores one sum per thread");
static_assert((2 * WL_MAX_P + 1) * (2 * WL_MAX_P + 1) <= 64 * WL_SLOTS, "a tap per lane and slot");

__global__ __launch_bounds__(WL_THREADS) void ray_depth_kernel(const float* __restrict__ rays, const float* __restrict__ R,
                                                               const float* __restrict__ z, const float* __restrict__ weights, int64_t B,
                                                               int n, const int64_t* __restrict__ seg_off,
                                                               const int32_t* __restrict__ seg_cnt, int max_samples, float sample_dist,
                                                               float* __restrict__ t_out, float* __restrict__ w_out,
                                                               float* __restrict__ z_out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool packed = seg_off != nullptr;
    const double r6 = (double)R[6], r7 = (double)R[7], r8 = (double)R[8];
    const int64_t stride = (int64_t)gridDim.x * WL_WAVES;
    for (int64_t ray = (int64_t)blockIdx.x * WL_WAVES + wave; ray < B; ray += stride) {      // the same trip count for a whole wave
        const PriorRow row = prior_row(ray, n, seg_off, seg_cnt, max_samples);
        double sw = 0.0, swm = 0.0;
        for (int k = lane; k < row.n; k += 64) {
            const double w = (double)weights[row.rb + k];
            sw += w;
            swm = fma(w, (double)prior_mid(z, row.rb, k, row.n, packed, sample_dist), swm);
        }
        sw = sum64_lanes(sw);
        swm = sum64_lanes(swm);
        const double cz = r6 * rays[ray * 14 + 3] + r7 * rays[ray * 14 + 4] + r8 * rays[ray * 14 + 5];
        const double t = sw > 0.0 ? swm / sw : 0.0;
        if (lane == 0) {
            t_out[ray] = (float)t;
            w_out[ray] = (float)sw;
            z_out[ray] = (float)(t * cz);
        }
    }
}

__global__ __launch_bounds__(WL_THREADS) void ray_depth_bwd_kernel(const float* __restrict__ rays, const float* __restrict__ R,
                                                                   const float* __restrict__ z, const float* __restrict__ t_in,
                                                                   const float* __restrict__ w_in, const float* __restrict__ ray_f,
                                                                   const float* __restrict__ stats, int64_t B, int n,
                                                                   const int64_t* __restrict__ seg_off,
                                                                   const int32_t* __restrict__ seg_cnt, int max_samples, float sample_dist,
                                                                   float warp_w, int accumulate, float* __restrict__ d_weights,
                                                                   float* __restrict__ d_nmap) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool packed = seg_off != nullptr;
    const double r6 = (double)R[6], r7 = (double)R[7], r8 = (double)R[8];
    const float count = stats[1];
    const double scale = (double)warp_w / (double)(count > 1.f ? count : 1.f);
    const int64_t stride = (int64_t)gridDim.x * WL_WAVES;
    for (int64_t ray = (int64_t)blockIdx.x * WL_WAVES + wave; ray < B; ray += stride) {
        if (d_weights) {
            const PriorRow row = prior_row(ray, n, seg_off, seg_cnt, max_samples);
            const float gz = ray_f[ray * 8 + 1], ws = w_in[ray], tt = t_in[ray];
            const double cz = r6 * rays[ray * 14 + 3] + r7 * rays[ray * 14 + 4] + r8 * rays[ray * 14 + 5];
            const float c = (gz != 0.f && ws > 0.f) ? (float)(scale * (double)gz * cz / (double)ws) : 0.f;
            if (!(accumulate & 1)) {
                for (int k = lane; k < row.n; k += 64)
                    d_weights[row.rb + k] = c != 0.f ? c * (prior_mid(z, row.rb, k, row.n, packed, sample_dist) - tt) : 0.f;
            } else if (c != 0.f) {                       // adding nothing leaves the buffer's bits alone
                for (int k = lane; k < row.n; k += 64)
                    d_weights[row.rb + k] += c * (prior_mid(z, row.rb, k, row.n, packed, sample_dist) - tt);
            }
        }
        if (d_nmap && lane < 3) {
            const float g = (float)(scale * (double)ray_f[ray * 8 + 2 + lane]);
            if (!(accumulate & 2)) d_nmap[ray * 3 + lane] = g;
            else if (g != 0.f) d_nmap[ray * 3 + lane] += g;
        }
    }
}

// partial [gridDim.x, WL_SUMS] doubles; NS = the slots of a lane: N <= 64 NS taps
template <int NS>
__global__ __launch_bounds__(WL_THREADS) void warp_ray_kernel(
    const uint8_t* __restrict__ gray, const uint8_t* __restrict__ valid, int F, int H, int W, const float* __restrict__ Rm,
    const float* __restrict__ Tm, const float* __restrict__ Km, const float* __restrict__ Kim, const int32_t* __restrict__ nbr, int Nn,
    int fi, const int32_t* __restrict__ pix, const float* __restrict__ zin, const float* __restrict__ win, const float* __restrict__ nin,
    int64_t B, int P, int64_t min_va, float min_vb, int topk, int min_views, float min_cos, float min_wsum, float* __restrict__ out_f,
    int32_t* __restrict__ out_i, double* __restrict__ partial) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int S = 2 * P + 1, N = S * S;
    const int64_t HW = (int64_t)H * W;
    const float K[9] = {Km[0], Km[1], Km[2], Km[3], Km[4], Km[5], Km[6], Km[7], Km[8]};
    const float Ki[9] = {Kim[0], Kim[1], Kim[2], Kim[3], Kim[4], Kim[5], Kim[6], Kim[7], Kim[8]};
    const float* Ri = Rm + (int64_t)fi * 9;
    const float* Ti = Tm + (int64_t)fi * 3;
    const uint8_t* gi = gray + (int64_t)fi * HW;
    const uint8_t* vi = valid + (int64_t)fi * HW;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const double dN = (double)N;
    double acc[WL_SUMS];
#pragma unroll
    for (int k = 0; k < WL_SUMS; ++k) acc[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * WL_WAVES;
    for (int64_t ray = (int64_t)blockIdx.x * WL_WAVES + wave; ray < B; ray += stride) {      // the same trip count for a whole wave
        const int px = pix[ray * 2], py = pix[ray * 2 + 1];

        // ---- the source patch: this lane's taps stay in registers
        float av[NS];
        bool bad = false;
        uint32_t sa = 0, sa2 = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int ti = lane + 64 * s;
            av[s] = 0.f;
            if (ti < N) {
                const int r = ti / S, c = ti - r * S;
                const int64_t x = (int64_t)px - P + c, y = (int64_t)py - P + r;
                bool ok = false;
                uint32_t b = 0;
                if (x >= 0 && x < W && y >= 0 && y < H) {
                    const int64_t at = y * W + x;
                    if (vi[at] != 0) {
                        ok = true;
                        b = gi[at];
                    }
                }
                bad |= !ok;
                sa += b;
                sa2 += b * b;
                av[s] = (float)b;
            }
        }
        const bool src_bad = __ballot(bad) != 0ull;
        sa = wl_sum_u32(sa);
        sa2 = wl_sum_u32(sa2);
        const int64_t va = (int64_t)N * sa2 - (int64_t)sa * sa;
        int flags = 0;
        if (src_bad || va < min_va) flags |= 1;
        if (!(win[ray] >= min_wsum)) flags |= 16;                                             // a NaN fails

        // ---- the plane
        const float z0 = zin[ray], n0 = nin[ray * 3], n1 = nin[ray * 3 + 1], n2 = nin[ray * 3 + 2];
        const float fx = (float)px, fy = (float)py;
        const float e0 = (Ki[0] * fx + Ki[1] * fy) + Ki[2], e1 = (Ki[3] * fx + Ki[4] * fy) + Ki[5], e2 = (Ki[6] * fx + Ki[7] * fy) + Ki[8];
        const float c0 = wl_dot3(Ri[0], Ri[1], Ri[2], n0, n1, n2), c1 = wl_dot3(Ri[3], Ri[4], Ri[5], n0, n1, n2),
                    c2 = wl_dot3(Ri[6], Ri[7], Ri[8], n0, n1, n2);
        const float ne = wl_dot3(c0, c1, c2, e0, e1, e2);
        const float nn = sqrtf(wl_dot3(c0, c1, c2, c0, c1, c2)), en = sqrtf(wl_dot3(e0, e1, e2, e0, e1, e2));
        const float cosv = -ne / (nn * en);
        if (!__builtin_isfinite(z0) || !(z0 > WL_Z_MIN) || !(nn > 1e-6f) || !(cosv >= min_cos)) flags |= 8;
        const float g = z0 * ne;

        // ---- the neighbours; lane jn keeps neighbour jn's results
        double lj = (double)__builtin_inff(), scj = (double)WL_NONE, gzj = 0.0, gj0 = 0.0, gj1 = 0.0, gj2 = 0.0;
        int nvalid = 0;
        if (flags == 0) {                                                                     // uniform over the wave
            float tx_[NS], ty_[NS], sg[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int ti = lane + 64 * s;
                tx_[s] = ty_[s] = sg[s] = 0.f;
                if (ti < N) {
                    const int r = ti / S, c = ti - r * S;
                    const float x = (float)(px + (c - P)), y = (float)(py + (r - P));
                    tx_[s] = x;
                    ty_[s] = y;
                    const float u0 = (Ki[0] * x + Ki[1] * y) + Ki[2], u1 = (Ki[3] * x + Ki[4] * y) + Ki[5], u2 = (Ki[6] * x + Ki[7] * y) + Ki[8];
                    sg[s] = wl_dot3(c0, c1, c2, u0, u1, u2) / g;
                }
            }
            // the plane again in fp64 of the fp32 inputs, for the derivative: d sigma / d n_c = (u - rho e) / g with rho = (n_c . u) /
            // (n_c . e) is what is left of two nearly equal vectors, and the fp32 sigma would leave its rounding in it
            const double E0 = ((double)Ki[0] * px + (double)Ki[1] * py) + (double)Ki[2], E1 = ((double)Ki[3] * px + (double)Ki[4] * py) + (double)Ki[5],
                         E2 = ((double)Ki[6] * px + (double)Ki[7] * py) + (double)Ki[8];
            const double C0 = ((double)Ri[0] * n0 + (double)Ri[1] * n1) + (double)Ri[2] * n2, C1 = ((double)Ri[3] * n0 + (double)Ri[4] * n1) + (double)Ri[5] * n2,
                         C2 = ((double)Ri[6] * n0 + (double)Ri[7] * n1) + (double)Ri[8] * n2;
            const double NE = (C0 * E0 + C1 * E1) + C2 * E2, G64 = (double)z0 * NE;
            for (int jn = 0; jn < Nn; ++jn) {
                const int j = nbr[(int64_t)fi * Nn + jn];
                if (j < 0 || j >= F) continue;
                const float* Rj = Rm + (int64_t)j * 9;
                const float* Tj = Tm + (int64_t)j * 3;
                float Rij[9], t[3], G[9], A[9], bv[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) Rij[r * 3 + c] = wl_dot3(Rj[r * 3], Rj[r * 3 + 1], Rj[r * 3 + 2], Ri[c * 3], Ri[c * 3 + 1], Ri[c * 3 + 2]);
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) t[r] = Tj[r] - wl_dot3(Rij[r * 3], Rij[r * 3 + 1], Rij[r * 3 + 2], Ti[0], Ti[1], Ti[2]);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) G[r * 3 + c] = wl_dot3(K[r * 3], K[r * 3 + 1], K[r * 3 + 2], Rij[c], Rij[3 + c], Rij[6 + c]);
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) A[r * 3 + c] = wl_dot3(G[r * 3], G[r * 3 + 1], G[r * 3 + 2], Ki[c], Ki[3 + c], Ki[6 + c]);
                    bv[r] = wl_dot3(K[r * 3], K[r * 3 + 1], K[r * 3 + 2], t[0], t[1], t[2]);
                }
                const uint8_t* gj = gray + (int64_t)j * HW;
                const uint8_t* vj = valid + (int64_t)j * HW;

                // pass 1: b per tap, and grad b . d q / d sigma for pass 2
                float bt[NS];
                double wt[NS];
                double psb = 0.0, psb2 = 0.0, psab = 0.0;
                bool fail = false;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    bt[s] = 0.f;
                    wt[s] = 0.0;
                    if (lane + 64 * s < N) {
                        const float x = tx_[s], y = ty_[s], sgm = sg[s];
                        const float h0 = ((A[0] * x + A[1] * y) + A[2]) + bv[0] * sgm;
                        const float h1 = ((A[3] * x + A[4] * y) + A[5]) + bv[1] * sgm;
                        const float h2 = ((A[6] * x + A[7] * y) + A[8]) + bv[2] * sgm;
                        bool ok = h2 > WL_Z_MIN;
                        if (ok) {
                            const float tx = h0 / h2, ty = h1 / h2;
                            ok = tx >= 0.f && tx < xmax && ty >= 0.f && ty < ymax;                // NaN fails; x0 + 1 <= W - 1, y0 + 1 <= H - 1
                            if (ok) {
                                const float flx = floorf(tx), fly = floorf(ty);
                                const int64_t at = (int64_t)(int)fly * W + (int)flx;
                                ok = vj[at] != 0 && vj[at + 1] != 0 && vj[at + W] != 0 && vj[at + W + 1] != 0;
                                if (ok) {
                                    const float g00 = (float)gj[at], g01 = (float)gj[at + 1], g10 = (float)gj[at + W], g11 = (float)gj[at + W + 1];
                                    const float wx = tx - flx, wy = ty - fly;
                                    const float top = g00 + wx * (g01 - g00), bot = g10 + wx * (g11 - g10);
                                    const float b = top + wy * (bot - top);
                                    bt[s] = b;
                                    const double gbx = (double)(g01 - g00) + (double)wy * ((double)(g11 - g10) - (double)(g01 - g00));
                                    const double gby = (double)(g10 - g00) + (double)wx * ((double)(g11 - g10) - (double)(g01 - g00));
                                    const double dtx = ((double)bv[0] - (double)tx * (double)bv[2]) / (double)h2;
                                    const double dty = ((double)bv[1] - (double)ty * (double)bv[2]) / (double)h2;
                                    wt[s] = gbx * dtx + gby * dty;
                                    psb += (double)b;
                                    psb2 += (double)b * (double)b;
                                    psab += (double)av[s] * (double)b;
                                }
                            }
                        }
                        fail |= !ok;
                    }
                }
                if (__ballot(fail) != 0ull) continue;                                         // uniform
                const double sb = sum64_lanes(psb), sb2 = sum64_lanes(psb2), sab = sum64_lanes(psab);
                const double vb = dN * sb2 - sb * sb;
                if (!(vb >= (double)min_vb)) continue;
                const double D = sqrt((double)va * vb);
                const double score = (dN * sab - (double)sa * sb) / D;

                // pass 2: s_t = d l / d b_t (grad b . d q / d sigma); sum s sigma, sum s u
                double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (lane + 64 * s < N) {
                        const double dl = score * (dN * (double)bt[s] - sb) / vb - (dN * (double)av[s] - (double)sa) / D;
                        const double st = dl * wt[s];
                        const double x = (double)tx_[s], y = (double)ty_[s];
                        const double U0 = ((double)Ki[0] * x + (double)Ki[1] * y) + (double)Ki[2], U1 = ((double)Ki[3] * x + (double)Ki[4] * y) + (double)Ki[5],
                                     U2 = ((double)Ki[6] * x + (double)Ki[7] * y) + (double)Ki[8];
                        const double rho = ((C0 * U0 + C1 * U1) + C2 * U2) / NE;
                        q0 += st * rho;
                        q1 += st * (U0 - rho * E0);
                        q2 += st * (U1 - rho * E1);
                        q3 += st * (U2 - rho * E2);
                    }
                }
                q0 = sum64_lanes(q0);
                q1 = sum64_lanes(q1);
                q2 = sum64_lanes(q2);
                q3 = sum64_lanes(q3);
                if (lane == jn) {
                    lj = 1.0 - score;
                    scj = score;
                    gzj = -q0 / ((double)z0 * (double)z0);           // sigma = rho / z: g_z = -sum s sigma / z
                    gj0 = q1 / G64;
                    gj1 = q2 / G64;
                    gj2 = q3 / G64;
                }
                ++nvalid;
            }
        }

        // ---- the top-k choice over lanes 0..7 (every lane takes part in the shuffles)
        int rank = 0;
#pragma unroll
        for (int i = 0; i < WL_MAX_NBR; ++i) {
            const double li = __shfl(lj, i, 64);
            if (li < lj || (li == lj && i < lane)) ++rank;
        }
        const bool counts = flags == 0 && nvalid >= min_views && nvalid > 0;
        const int kk = topk < nvalid ? topk : nvalid;
        const bool chosen = counts && lane < WL_MAX_NBR && lj < (double)__builtin_inff() && rank < kk;
        const uint32_t mask = (uint32_t)(__ballot(chosen) & 0xffull);
        const double sl = wl_sum8(chosen ? lj : 0.0), ss = wl_sum8(chosen ? scj : 0.0), sz = wl_sum8(chosen ? gzj : 0.0);
        const double s0 = wl_sum8(chosen ? gj0 : 0.0), s1 = wl_sum8(chosen ? gj1 : 0.0), s2 = wl_sum8(chosen ? gj2 : 0.0);
        double best = (lane < WL_MAX_NBR) ? scj : (double)WL_NONE;
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            best = ob > best ? ob : best;
        }
        if (lane == 0) {
            float* of = out_f + ray * 8;
            int32_t* oi = out_i + ray * 4;
            int fl = flags;
            if (counts) {
                const double inv = 1.0 / (double)kk;
                const float lr = (float)(sl * inv), ms = (float)(ss * inv);
                const double a0 = s0 * inv, a1 = s1 * inv, a2 = s2 * inv;
                of[0] = lr;
                of[1] = (float)(sz * inv);
                of[2] = (float)(((double)Ri[0] * a0 + (double)Ri[3] * a1) + (double)Ri[6] * a2);
                of[3] = (float)(((double)Ri[1] * a0 + (double)Ri[4] * a1) + (double)Ri[7] * a2);
                of[4] = (float)(((double)Ri[2] * a0 + (double)Ri[5] * a1) + (double)Ri[8] * a2);
                of[5] = ms;
                of[6] = (float)best;
                of[7] = 0.f;
                oi[0] = nvalid; oi[1] = kk; oi[2] = 0; oi[3] = (int32_t)mask;
                acc[0] += (double)lr;
                acc[1] += 1.0;
                acc[2] += (double)ms;
            } else {
                if (fl == 0) fl = 2;
                of[0] = 0.f; of[1] = 0.f; of[2] = 0.f; of[3] = 0.f; of[4] = 0.f; of[5] = WL_NONE; of[6] = WL_NONE; of[7] = 0.f;
                oi[0] = nvalid; oi[1] = 0; oi[2] = fl; oi[3] = 0;
            }
            if (fl & 1) acc[3] += 1.0;
            if (fl & 2) acc[4] += 1.0;
            if (fl & 8) acc[5] += 1.0;
            if (fl & 16) acc[6] += 1.0;
        }
    }
    sum64_block_store(acc, partial + (int64_t)blockIdx.x * WL_SUMS);
}

__global__ void warp_stats_kernel(const double* __restrict__ sums, float warp_w, float* __restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double cnt = sums[1] > 1.0 ? sums[1] : 1.0;
    const float L = (float)(sums[0] / cnt);
    stats[0] = L;
    stats[1] = (float)sums[1];
    stats[2] = (float)(sums[2] / cnt);
    stats[3] = warp_w * L;
    stats[4] = (float)sums[3];
    stats[5] = (float)sums[4];
    stats[6] = (float)sums[5];
    stats[7] = (float)sums[6];
}

int warp_max_patch() { return WL_MAX_P; }
int warp_max_neighbours() { return WL_MAX_NBR; }

int64_t warp_loss_workspace(int64_t B) { return (warp_blocks(B) * WL_SUMS + WL_SUMS_PAD) * (int64_t)sizeof(double); }

int launch_ray_depth(const float* rays, const float* R, const float* z, const float* weights, int64_t B, int n, const int64_t* seg_off,
                     const int32_t* seg_cnt, int max_samples, float sample_dist, float* t_out, float* w_out, float* z_out, hipStream_t st) {
    hipLaunchKernelGGL(ray_depth_kernel, dim3((unsigned)warp_blocks(B)), dim3(WL_THREADS), 0, st, rays, R, z, weights, B, n, seg_off,
                       seg_cnt, max_samples, sample_dist, t_out, w_out, z_out);
    return launch_status();
}

int launch_ray_depth_bwd(const float* rays, const float* R, const float* z, const float* t_in, const float* w_in, const float* ray_f,
                         const float* stats, int64_t B, int n, const int64_t* seg_off, const int32_t* seg_cnt, int max_samples,
                         float sample_dist, float warp_w, int accumulate, float* d_weights, float* d_nmap, hipStream_t st) {
    hipLaunchKernelGGL(ray_depth_bwd_kernel, dim3((unsigned)warp_blocks(B)), dim3(WL_THREADS), 0, st, rays, R, z, t_in, w_in, ray_f, stats,
                       B, n, seg_off, seg_cnt, max_samples, sample_dist, warp_w, accumulate, d_weights, d_nmap);
    return launch_status();
}

int launch_warp_loss(const uint8_t* gray, const uint8_t* valid, int n_frames, int H, int W, const float* R, const float* T, const float* K,
                     const float* Kinv, const int32_t* nbr, int n_nbr, int frame, const int32_t* pix, const float* z, const float* wsum,
                     const float* normal, int64_t B, int P, int64_t min_va, float min_vb, int topk, int min_views, float min_cos,
                     float min_wsum, float warp_w, float* out_f, int32_t* out_i, float* stats, void* ws, hipStream_t st) {
    const int64_t blocks = warp_blocks(B);
    double* partial = static_cast<double*>(ws);
    double* sums = partial + blocks * WL_SUMS;
    const int N = (2 * P + 1) * (2 * P + 1);
#define DH_WARP_LAUNCH(NS)                                                                                                             \
    hipLaunchKernelGGL(warp_ray_kernel<NS>, dim3((unsigned)blocks), dim3(WL_THREADS), 0, st, gray, valid, n_frames, H, W, R, T, K, Kinv, \
                       nbr, n_nbr, frame, pix, z, wsum, normal, B, P, min_va, min_vb, topk, min_views, min_cos, min_wsum, out_f, out_i,  \
                       partial)
    if (N <= 64) DH_WARP_LAUNCH(1);
    else if (N <= 128) DH_WARP_LAUNCH(2);
    else DH_WARP_LAUNCH(WL_SLOTS);
#undef DH_WARP_LAUNCH
    if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    const int rc = launch_sum64_reduce(partial, 1, (int)blocks, WL_SUMS, sums, st);
    if (rc != DH_OK) return rc;
    hipLaunchKernelGGL(warp_stats_kernel, dim3(1), dim3(64), 0, st, sums, warp_w, stats);
    return launch_status();
}

}  // namespace dh
