// Multi-view stereo (dynhor_amd/mvs.py): a mesh-guided plane sweep scored by zero-mean normalised cross-correlation on match.hip's 8-bit
// grey frames, and a geometric consistency count between depth maps (include/dynhor_hip.h states both rules in full).
//
// mvs_sweep_kernel: a lane per (pixel, hypothesis).  A wave is cut into 64 / SW slots of SW = the power of two >= D lanes (D <= 63), a
// slot per pixel, lane k of a slot the hypothesis k; MV_WAVES waves per workgroup.
//   source  a wave stages the (2P+1)^2 patches of its slots as bytes in LDS (a slot's row of MV_SRC_STRIDE bytes: 57 words, so the slots
//           of a wave start on different banks), 64 taps a step; a ballot per slot says whether every tap was inside and valid.  Every
//           lane then adds its slot's sum a and sum a^2 as integers (the lanes of a slot read one address: a broadcast).
//   sweep   per neighbour the lane forms R_ij, t_ij, the plane's homography at its depth, the centre q and the 2 x 2 Jacobian A, all in
//           fp32 with the operations written out (no contraction), and walks the taps in row-major order: four bytes of `valid`, four of
//           `gray`, the bilinear value, the three fp32 sums.  A tap with a pixel outside or invalid ends the neighbour for this lane.
//           Neighbouring lanes of a slot fetch along the epipolar line.
//   select  the best (score, then lowest k), the second peak beyond |k - k*| > 1 and the count by xor butterflies of width SW with every
//           lane of the wave active (lanes beyond D or beyond n carry NONE); the parabola reads the two neighbours' scores by shuffles.
// No atomics, no scratch; a pixel's outputs depend on that pixel's inputs alone, whatever slot it lands in.
//
// mvs_check_kernel: a lane per pixel of a depth map; integer counts, no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"

#pragma clang fp contract(off)

namespace dh {

namespace {
constexpr int MV_THREADS = 256;
constexpr int MV_WAVES = MV_THREADS / 64;
constexpr int MV_MAX_P = 7, MV_MAX_D = 63, MV_MAX_NBR = 8;
constexpr int MV_MAX_SLOTS = 16;                               // D = 3: SW = 4
constexpr int MV_SRC_STRIDE = 228;                             // >= 15 * 15 bytes, 57 words
constexpr float MV_NONE = -2.0f;                               // the score of an invalid hypothesis; real scores lie in [-1, 1]
constexpr float MV_Z_MIN = 1e-3f;

__device__ __forceinline__ bool mv_better(float s, int k, float s0, int k0) { return s > s0 || (s == s0 && k < k0); }

// (a . b) as ((a0 b0 + a1 b1) + a2 b2)
__device__ __forceinline__ float mv_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}
}  // namespace

__global__ __launch_bounds__(MV_THREADS) void mvs_sweep_kernel(
    const uint8_t* __restrict__ gray, const uint8_t* __restrict__ valid, int F, int H, int W, const float* __restrict__ Rm,
    const float* __restrict__ Tm, const float* __restrict__ Km, const float* __restrict__ Kim, const int32_t* __restrict__ pix,
    const float* __restrict__ guide, int64_t n, const int32_t* __restrict__ nbr, int Nn, int D, int SW, float step, int P, int64_t min_va,
    float min_vb, int min_views, float min_cos, float* __restrict__ out_f, int32_t* __restrict__ out_i) {
    __shared__ __attribute__((aligned(16))) uint8_t src[MV_WAVES * MV_MAX_SLOTS * MV_SRC_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slots = 64 / SW, slot = lane / SW, k = lane - slot * SW;
    const int S = 2 * P + 1, N = S * S;
    const int64_t HW = (int64_t)H * W;
    const int64_t first = ((int64_t)blockIdx.x * MV_WAVES + wave) * slots;      // the wave's first pixel
    const int64_t me = first + slot;
    const bool have = me < n;
    uint8_t* wsrc = src + wave * (MV_MAX_SLOTS * MV_SRC_STRIDE);

    // ---- the source patches of the wave's slots
    bool src_bad = true;
    for (int s = 0; s < slots; ++s) {
        const int64_t q = first + s;                                            // uniform over the wave
        bool bad = false;
        if (q < n) {
            const int fi = pix[q * 3], px = pix[q * 3 + 1], py = pix[q * 3 + 2];
            for (int t = lane; t < N; t += 64) {
                const int r = t / S, c = t - r * S;
                const int64_t x = (int64_t)px - P + c, y = (int64_t)py - P + r;
                uint8_t b = 0;
                bool ok = false;
                if (fi >= 0 && fi < F && x >= 0 && x < W && y >= 0 && y < H) {
                    const int64_t at = (int64_t)fi * HW + y * W + x;
                    if (valid[at] != 0) {
                        ok = true;
                        b = gray[at];
                    }
                }
                bad |= !ok;
                wsrc[s * MV_SRC_STRIDE + t] = b;
            }
        }
        const bool any_bad = __ballot(bad) != 0ull;
        if (s == slot) src_bad = any_bad;
    }
    __syncthreads();

    // ---- per lane: the pixel, the guide, sum a and sum a^2
    const uint8_t* a = wsrc + slot * MV_SRC_STRIDE;
    int fi = 0, px = 0, py = 0;
    float z0 = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
    if (have) {
        fi = pix[me * 3]; px = pix[me * 3 + 1]; py = pix[me * 3 + 2];
        z0 = guide[me * 4]; n0 = guide[me * 4 + 1]; n1 = guide[me * 4 + 2]; n2 = guide[me * 4 + 3];
    }
    int64_t va = 0;
    uint32_t sa = 0;
    if (have && !src_bad) {
        uint32_t sa2 = 0;
        for (int t = 0; t < N; ++t) {
            const uint32_t v = a[t];
            sa += v;
            sa2 += v * v;
        }
        va = (int64_t)N * sa2 - (int64_t)sa * sa;
    }
    int flags = 0;
    if (src_bad || va < min_va) flags |= 1;
    const float Ki[9] = {Kim[0], Kim[1], Kim[2], Kim[3], Kim[4], Kim[5], Kim[6], Kim[7], Kim[8]};
    const float K[9] = {Km[0], Km[1], Km[2], Km[3], Km[4], Km[5], Km[6], Km[7], Km[8]};
    const float fx = (float)px, fy = (float)py;
    const float e0 = (Ki[0] * fx + Ki[1] * fy) + Ki[2], e1 = (Ki[3] * fx + Ki[4] * fy) + Ki[5], e2 = (Ki[6] * fx + Ki[7] * fy) + Ki[8];
    const float ne = mv_dot3(n0, n1, n2, e0, e1, e2);
    const float cosv = -ne / sqrtf(mv_dot3(e0, e1, e2, e0, e1, e2));
    if (!__builtin_isfinite(z0) || !(z0 > MV_Z_MIN) || !(cosv >= min_cos)) flags |= 8;          // the first test fails NaN and inf
    const bool live = have && flags == 0 && k < D;

    // ---- the sweep: this lane's hypothesis against every neighbour
    const int half = (D - 1) / 2;
    const float zk = z0 + (float)(k - half) * step;
    const float X0 = zk * e0, X1 = zk * e1, X2 = zk * e2;
    const float d = mv_dot3(n0, n1, n2, X0, X1, X2);
    const float s0 = n0 / d, s1 = n1 / d, s2 = n2 / d;
    const float fva = (float)va, fN = (float)N, fsa = (float)sa;
    float csum = 0.f;
    int views = 0;
    if (live && zk > MV_Z_MIN) {
        const float* Ri = Rm + (int64_t)fi * 9;
        const float* Ti = Tm + (int64_t)fi * 3;
        for (int jn = 0; jn < Nn; ++jn) {
            const int j = nbr[(int64_t)fi * Nn + jn];
            if (j < 0 || j >= F) continue;
            const float* Rj = Rm + (int64_t)j * 9;
            const float* Tj = Tm + (int64_t)j * 3;
            float Rij[9], t[3], M[9], G[9], Hm[9];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) Rij[r * 3 + c] = mv_dot3(Rj[r * 3], Rj[r * 3 + 1], Rj[r * 3 + 2], Ri[c * 3], Ri[c * 3 + 1], Ri[c * 3 + 2]);
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) t[r] = Tj[r] - mv_dot3(Rij[r * 3], Rij[r * 3 + 1], Rij[r * 3 + 2], Ti[0], Ti[1], Ti[2]);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                M[r * 3] = Rij[r * 3] + t[r] * s0;
                M[r * 3 + 1] = Rij[r * 3 + 1] + t[r] * s1;
                M[r * 3 + 2] = Rij[r * 3 + 2] + t[r] * s2;
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) G[r * 3 + c] = mv_dot3(K[r * 3], K[r * 3 + 1], K[r * 3 + 2], M[c], M[3 + c], M[6 + c]);
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) Hm[r * 3 + c] = mv_dot3(G[r * 3], G[r * 3 + 1], G[r * 3 + 2], Ki[c], Ki[3 + c], Ki[6 + c]);
            }
            const float h0 = (Hm[0] * fx + Hm[1] * fy) + Hm[2], h1 = (Hm[3] * fx + Hm[4] * fy) + Hm[5], h2 = (Hm[6] * fx + Hm[7] * fy) + Hm[8];
            if (!(h2 > MV_Z_MIN)) continue;
            const float qx = h0 / h2, qy = h1 / h2;
            const float A00 = (Hm[0] - qx * Hm[6]) / h2, A01 = (Hm[1] - qx * Hm[7]) / h2;
            const float A10 = (Hm[3] - qy * Hm[6]) / h2, A11 = (Hm[4] - qy * Hm[7]) / h2;
            const uint8_t* gj = gray + (int64_t)j * HW;
            const uint8_t* vj = valid + (int64_t)j * HW;
            const float xmax = (float)(W - 1), ymax = (float)(H - 1);
            float sb = 0.f, sb2 = 0.f, sab = 0.f;
            bool ok = true;
            int ti = 0;
            for (int r = -P; r <= P && ok; ++r) {
                const float fr = (float)r;
                for (int c = -P; c <= P; ++c, ++ti) {
                    const float fc = (float)c;
                    const float tx = qx + (A00 * fc + A01 * fr), ty = qy + (A10 * fc + A11 * fr);
                    if (!(tx >= 0.f && tx < xmax && ty >= 0.f && ty < ymax)) {                // NaN fails; x0 + 1 <= W - 1, y0 + 1 <= H - 1
                        ok = false;
                        break;
                    }
                    const float flx = floorf(tx), fly = floorf(ty);
                    const int64_t at = (int64_t)(int)fly * W + (int)flx;
                    if (vj[at] == 0 || vj[at + 1] == 0 || vj[at + W] == 0 || vj[at + W + 1] == 0) {
                        ok = false;
                        break;
                    }
                    const float g00 = (float)gj[at], g01 = (float)gj[at + 1], g10 = (float)gj[at + W], g11 = (float)gj[at + W + 1];
                    const float wx = tx - flx, wy = ty - fly;
                    const float top = g00 + wx * (g01 - g00), bot = g10 + wx * (g11 - g10);
                    const float b = top + wy * (bot - top);
                    const float av = (float)a[ti];
                    sb = sb + b;
                    sb2 = sb2 + b * b;
                    sab = sab + av * b;
                }
            }
            if (!ok) continue;
            const float vb = fN * sb2 - sb * sb;
            if (!(vb >= min_vb)) continue;
            csum = csum + (fN * sab - fsa * sb) / sqrtf(fva * vb);
            ++views;
        }
    }
    float ck = MV_NONE;
    if (live && views >= min_views && views > 0) ck = csum / (float)views;

    // ---- the best hypothesis of every slot: every lane of the wave takes part
    float best = ck;
    int best_k = ck > -1.5f ? k : 0x7fffffff, count = ck > -1.5f ? 1 : 0;
    for (int o = SW >> 1; o >= 1; o >>= 1) {
        const float s = __shfl_xor(best, o);
        const int c = __shfl_xor(best_k, o);
        count += __shfl_xor(count, o);
        if (mv_better(s, c, best, best_k)) {
            best = s;
            best_k = c;
        }
    }
    const int kb = count > 0 ? best_k : 0;
    const int dk = k > kb ? k - kb : kb - k;
    float sec = dk > 1 ? ck : MV_NONE;
    for (int o = SW >> 1; o >= 1; o >>= 1) {
        const float s = __shfl_xor(sec, o);
        sec = s > sec ? s : sec;
    }
    const int base = lane - k;
    const float cm = __shfl(ck, base + (kb > 0 ? kb - 1 : 0));
    const float cp = __shfl(ck, base + (kb < SW - 1 ? kb + 1 : kb));
    const int vbest = __shfl(views, base + kb);
    if (!have || k != 0) return;

    float* of = out_f + me * 4;
    int32_t* oi = out_i + me * 4;
    if (flags != 0 || count == 0) {
        of[0] = 0.f; of[1] = MV_NONE; of[2] = MV_NONE; of[3] = 0.f;
        oi[0] = 0; oi[1] = 0; oi[2] = flags != 0 ? flags : 2; oi[3] = 0;
        return;
    }
    const bool border = kb == 0 || kb == D - 1;
    float sub = 0.f;
    if (!border && cm > -1.5f && cp > -1.5f) {
        const float den = (cm - 2.f * best) + cp;
        if (den < 0.f) {
            const float tt = (0.5f * (cm - cp)) / den;
            sub = tt < -0.5f ? -0.5f : (tt > 0.5f ? 0.5f : tt);
        }
    }
    of[0] = z0 + ((float)(kb - half) + sub) * step; of[1] = best; of[2] = sec; of[3] = sub;
    oi[0] = kb; oi[1] = vbest; oi[2] = border ? 4 : 0; oi[3] = count;
}

__global__ __launch_bounds__(MV_THREADS) void mvs_check_kernel(const float* __restrict__ depth, int F, int H, int W,
                                                                const float* __restrict__ Rm, const float* __restrict__ Tm,
                                                                const float* __restrict__ Km, const float* __restrict__ Kim,
                                                                const int32_t* __restrict__ nbr, int Nn, float depth_rel,
                                                                uint8_t* __restrict__ count) {
    const int64_t HW = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * MV_THREADS + threadIdx.x;
    if (i >= (int64_t)F * HW) return;
    const int f = (int)(i / HW);
    const int64_t rem = i - (int64_t)f * HW;
    const int py = (int)(rem / W), px = (int)(rem - (int64_t)py * W);
    const float z = depth[i];
    int cnt = 0;
    if (__builtin_isfinite(z)) {                                                   // NaN and inf: no depth
        const float fx = (float)px, fy = (float)py;
        const float c0 = z * ((Kim[0] * fx + Kim[1] * fy) + Kim[2]) - Tm[(int64_t)f * 3];
        const float c1 = z * ((Kim[3] * fx + Kim[4] * fy) + Kim[5]) - Tm[(int64_t)f * 3 + 1];
        const float c2 = z * ((Kim[6] * fx + Kim[7] * fy) + Kim[8]) - Tm[(int64_t)f * 3 + 2];
        const float* Ri = Rm + (int64_t)f * 9;
        const float X0 = mv_dot3(Ri[0], Ri[3], Ri[6], c0, c1, c2), X1 = mv_dot3(Ri[1], Ri[4], Ri[7], c0, c1, c2),
                    X2 = mv_dot3(Ri[2], Ri[5], Ri[8], c0, c1, c2);
        for (int jn = 0; jn < Nn; ++jn) {
            const int j = nbr[(int64_t)f * Nn + jn];
            if (j < 0 || j >= F) continue;
            const float* Rj = Rm + (int64_t)j * 9;
            const float y0 = mv_dot3(Rj[0], Rj[1], Rj[2], X0, X1, X2) + Tm[(int64_t)j * 3];
            const float y1 = mv_dot3(Rj[3], Rj[4], Rj[5], X0, X1, X2) + Tm[(int64_t)j * 3 + 1];
            const float y2 = mv_dot3(Rj[6], Rj[7], Rj[8], X0, X1, X2) + Tm[(int64_t)j * 3 + 2];
            if (!(y2 > MV_Z_MIN)) continue;
            const float u = floorf(mv_dot3(Km[0], Km[1], Km[2], y0, y1, y2) / y2 + 0.5f);
            const float w = floorf(mv_dot3(Km[3], Km[4], Km[5], y0, y1, y2) / y2 + 0.5f);
            if (!(u >= 0.f && u < (float)W && w >= 0.f && w < (float)H)) continue;
            const float zj = depth[(int64_t)j * HW + (int64_t)(int)w * W + (int)u];
            if (!__builtin_isfinite(zj)) continue;
            if (fabsf(y2 - zj) <= depth_rel * zj) ++cnt;
        }
    }
    count[i] = (uint8_t)cnt;
}

int mvs_max_patch() { return MV_MAX_P; }
int mvs_max_depths() { return MV_MAX_D; }
int mvs_max_neighbours() { return MV_MAX_NBR; }

int launch_mvs_sweep(const uint8_t* gray, const uint8_t* valid, int n_frames, int H, int W, const float* R, const float* T, const float* K,
                     const float* Kinv, const int32_t* pix, const float* guide, int64_t n, const int32_t* nbr, int n_nbr, int D, float step,
                     int P, int64_t min_va, float min_vb, int min_views, float min_cos, float* out_f, int32_t* out_i, hipStream_t st) {
    int SW = 4;
    while (SW < D) SW *= 2;
    const int64_t per_block = (int64_t)MV_WAVES * (64 / SW);
    const int64_t blocks = (n + per_block - 1) / per_block;
    hipLaunchKernelGGL(mvs_sweep_kernel, dim3((unsigned)blocks), dim3(MV_THREADS), 0, st, gray, valid, n_frames, H, W, R, T, K, Kinv, pix,
                       guide, n, nbr, n_nbr, D, SW, step, P, min_va, min_vb, min_views, min_cos, out_f, out_i);
    return launch_status();
}

int launch_mvs_check(const float* depth, int n_frames, int H, int W, const float* R, const float* T, const float* K, const float* Kinv,
                     const int32_t* nbr, int n_nbr, float depth_rel, uint8_t* count, hipStream_t st) {
    const int64_t total = (int64_t)n_frames * H * W;
    const int64_t blocks = (total + MV_THREADS - 1) / MV_THREADS;
    hipLaunchKernelGGL(mvs_check_kernel, dim3((unsigned)blocks), dim3(MV_THREADS), 0, st, depth, n_frames, H, W, R, T, K, Kinv, nbr, n_nbr,
                       depth_rel, count);
    return launch_status();
}

}  // namespace dh
