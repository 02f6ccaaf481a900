// Dense frame matching (dynhor_amd/match.py): block matching by zero-mean normalised cross-correlation on 8-bit grey frames, guided by
// a guess per query (include/dynhor_hip.h states both rules in full).
//
// match_gray_kernel: one lane per pixel of dh_image_blur's output; every operation is an fp32 IEEE operation written out (fmaf), so a
// float32 restatement gives the same bytes.
//
// match_search_kernel<P, WARP>: one workgroup of MS_THREADS lanes per query, dynamic LDS sized by (P, R):
//   source  the (2P+1)^2 patch about (px, py) of frame fi, rows padded with zero bytes to NW = ceil((2P+1) / 4) words; after a barrier
//           every lane keeps all of it in registers (P is a template argument: the rows are unrolled).  A patch with a pixel that is
//           invalid or outside the image, or with va < min_va, ends the query (flag 1) before any search.  WARP (dh_match_search_warp,
//           queries of 10 words): the lane of cell (c, r) samples frame fi at (px, py) + A (c, r), A the query's 2 x 2 map in Q16, from
//           up to four bytes with 8-bit bilinear weights (ms_warp_cell); only this staging differs, the registers, the window and the
//           search are those of the plain kernel.
//   window  the (2(R+P)+1)^2 pixels about (gx, gy) of frame fj: a wave stages one row per step, lane = column, the bytes of `gray`
//           (0 where invalid or outside) at a row stride that is a multiple of 4 with NW+1 words readable from every candidate's
//           column, and the wave's ballot of `valid` as the row's bit mask (no atomics).
//   rows    per window row y and candidate column cx: the sums of b and b^2 over the 2P+1 pixels right of cx, packed into one word
//           (b^2 << 12 | b: 20 + 12 bits), or ~0 when the mask shows an invalid pixel among them.
//   search  a lane walks the candidates c = lane, lane + MS_THREADS, ... (consecutive lanes: consecutive columns): 2P+1 row words give
//           sum b, sum b^2 and validity; sum ab is v_dot4_u32_u8 over the source words and the window words, which v_alignbyte_b32
//           forms from two aligned words for the candidate's byte offset (DH_MATCH_NO_DOT4: the same loop with plain multiply-adds,
//           for an A/B).  The score goes to LDS (-2 for an invalid candidate) and into the lane's running best.
//   select  the best (score, then smallest c) and the count over the workgroup (xor butterfly in every wave, all lanes active, then the
//           MS_THREADS / 64 wave results through LDS), the second peak outside `excl` the same way, the sub-pixel step by lane 0.
// All sums are integers and every lane combines in a fixed order: the outputs do not depend on scheduling.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"

#pragma clang fp contract(off)

namespace dh {

namespace {
constexpr int MG_THREADS = 256;
constexpr int MS_THREADS = 256;
constexpr int MS_WAVES = MS_THREADS / 64;
constexpr int MS_MAX_P = 7, MS_MAX_R = 32;
constexpr int MS_MAX_AFFINE = 1 << 19;         // Q16: a scale of 8
constexpr double MS_NONE = -2.0;               // the score of an invalid candidate; real scores lie in [-1, 1]
constexpr uint32_t MS_ROW_BAD = 0xFFFFFFFFu;   // no valid row packs to this: sum b^2 <= 15 * 255^2 < 0xEE210 leaves the top bits short of all ones

__device__ __forceinline__ uint32_t ms_dot4(uint32_t a, uint32_t b, uint32_t c) {
#ifdef DH_MATCH_NO_DOT4
    return c + (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u) +
           (a >> 24) * (b >> 24);
#else
    return __builtin_amdgcn_udot4(a, b, c, false);
#endif
}

struct MsGeom {
    int C, WS, stride, vw;                     // candidates per axis, window size, byte stride of a window row, mask words per row
    size_t off_rows, off_mask, off_win, off_src, off_red, bytes;
};

__host__ __device__ inline MsGeom ms_geom(int P, int R) {
    MsGeom g;
    const int S = 2 * P + 1, NW = (S + 3) / 4;
    g.C = 2 * R + 1;
    g.WS = g.C + 2 * P;
    g.stride = ((2 * R) & ~3) + 4 * (NW + 1);                       // >= WS; candidate column cx reads the words [cx & ~3, .. + 4 (NW+1))
    g.vw = 2 * ((g.stride + 63) / 64);
    size_t o = (size_t)g.C * g.C * sizeof(double);                   // scores first: 8-byte aligned
    g.off_rows = o;  o += (size_t)g.WS * g.C * 4;
    g.off_mask = o;  o += (size_t)g.WS * g.vw * 4;
    g.off_win = o;   o += (size_t)g.WS * g.stride;                   // stride is a multiple of 4
    g.off_src = o;   o += (size_t)S * NW * 4;
    o = (o + 7) & ~(size_t)7;
    g.off_red = o;   o += (size_t)MS_WAVES * 16;
    g.bytes = o;
    return g;
}

// One cell of a warped source patch: the sample of frame f (gray, valid at its first pixel) at (X, Y) / 65536, X = px 65536 + a00 c + a01 r,
// Y = py 65536 + a10 c + a11 r in int64.  (x0, y0) = floor, the fractions' top 8 bits weigh the four neighbours by (256 - fx, fx) x
// (256 - fy, fy); a neighbour of weight 0 is not read.  False when a neighbour that is read lies outside the image or is invalid; else
// *out = (sum w gray + 32768) >> 16 (the weights sum to 65536: the sum stays below 2^24).
__device__ __forceinline__ bool ms_warp_cell(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ valid, int H, int W, int64_t X,
                                             int64_t Y, uint8_t* out) {
    const int64_t x0 = X >> 16, y0 = Y >> 16;
    const uint32_t fx = (uint32_t)(X & 0xFFFF) >> 8, fy = (uint32_t)(Y & 0xFFFF) >> 8;
    const uint32_t wx[2] = {256u - fx, fx}, wy[2] = {256u - fy, fy};
    uint32_t sum = 32768u;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t w = wx[i] * wy[j];
            if (w == 0u) continue;
            const int64_t x = x0 + i, y = y0 + j;
            if (x < 0 || x >= W || y < 0 || y >= H) {
                ok = false;
                continue;
            }
            const int64_t pix = y * W + x;
            if (valid[pix] == 0) ok = false;
            else sum += w * gray[pix];
        }
    }
    *out = (uint8_t)(sum >> 16);
    return ok;
}

// (score, candidate) order of the selection: the larger score, then the smaller index
__device__ __forceinline__ bool ms_better(double s, int c, double s0, int c0) { return s > s0 || (s == s0 && c < c0); }
}  // namespace

__global__ __launch_bounds__(MG_THREADS) void match_gray_kernel(const float4* __restrict__ img, int64_t n, float a_min,
                                                                 uint8_t* __restrict__ gray, uint8_t* __restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * MG_THREADS + threadIdx.x;
    if (i >= n) return;
    const float4 v = img[i];
    const bool ok = v.w >= a_min;
    float y = floorf(__builtin_fmaf(255.f, __builtin_fmaf(0.114f, v.z, __builtin_fmaf(0.587f, v.y, 0.299f * v.x)), 0.5f));
    y = y < 0.f ? 0.f : (y > 255.f ? 255.f : y);
    valid[i] = ok ? 1 : 0;
    gray[i] = ok ? (uint8_t)(int)y : (uint8_t)0;
}

// *bad (zeroed by the caller) becomes 1 when a query names a frame outside [0, n_frames) or, WARP, has an affine entry beyond
// +-MS_MAX_AFFINE
template <bool WARP>
__global__ __launch_bounds__(MG_THREADS) void match_check_kernel(const int32_t* __restrict__ queries, int64_t n, int n_frames,
                                                                  int32_t* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * MG_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t* Q = queries + i * (WARP ? 10 : 6);
    const int fi = Q[0], fj = Q[1];
    bool wrong = fi < 0 || fi >= n_frames || fj < 0 || fj >= n_frames;
    if constexpr (WARP) {
#pragma unroll
        for (int k = 6; k < 10; ++k) wrong |= Q[k] > MS_MAX_AFFINE || Q[k] < -MS_MAX_AFFINE;
    }
    if (wrong) atomicOr(bad, 1);
}

template <int P, bool WARP>
__global__ __launch_bounds__(MS_THREADS) void match_search_kernel(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ valid,
                                                                   int H, int W, const int32_t* __restrict__ queries, int R, int excl,
                                                                   int64_t min_va, int32_t* __restrict__ out_i,
                                                                   double* __restrict__ out_f) {
    constexpr int S = 2 * P + 1, N = S * S, NW = (S + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const MsGeom g = ms_geom(P, R);
    double* sc = reinterpret_cast<double*>(lds);
    uint32_t* rows = reinterpret_cast<uint32_t*>(lds + g.off_rows);
    uint32_t* mask = reinterpret_cast<uint32_t*>(lds + g.off_mask);
    uint8_t* win = lds + g.off_win;
    uint8_t* src = lds + g.off_src;
    double* red_s = reinterpret_cast<double*>(lds + g.off_red);
    int* red_c = reinterpret_cast<int*>(lds + g.off_red + MS_WAVES * 8);
    int* red_n = red_c + MS_WAVES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int32_t* Q = queries + q * (WARP ? 10 : 6);
    const int fi = Q[0], fj = Q[1], px = Q[2], py = Q[3], gx = Q[4], gy = Q[5];
    const int64_t HW = (int64_t)H * W;
    int32_t* oi = out_i + q * 4;
    double* of = out_f + q * 4;

    // ---- the source patch: S rows of 4 NW bytes, zero beyond column S
    bool src_ok = false;
    if (tid < S * 4 * NW) {
        const int r = tid / (4 * NW), c = tid - r * (4 * NW);
        uint8_t b = 0;
        if (c < S) {
            if constexpr (WARP) {
                const int64_t cc = c - P, rr = r - P;
                const int64_t X = (int64_t)px * 65536 + (int64_t)Q[6] * cc + (int64_t)Q[7] * rr;
                const int64_t Y = (int64_t)py * 65536 + (int64_t)Q[8] * cc + (int64_t)Q[9] * rr;
                uint8_t v;
                src_ok = ms_warp_cell(gray + (int64_t)fi * HW, valid + (int64_t)fi * HW, H, W, X, Y, &v);
                if (src_ok) b = v;
            } else {
                const int64_t x = (int64_t)px - P + c, y = (int64_t)py - P + r;
                if (x >= 0 && x < W && y >= 0 && y < H) {
                    const int64_t pix = (int64_t)fi * HW + y * W + x;
                    if (valid[pix] != 0) {
                        src_ok = true;
                        b = gray[pix];
                    }
                }
            }
        }
        src[tid] = b;
    }
    const int n_src = __syncthreads_count(src_ok);
    uint32_t a[S][NW];
    uint32_t sa = 0, sa2 = 0;
#pragma unroll
    for (int r = 0; r < S; ++r) {
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            a[r][w] = reinterpret_cast<const uint32_t*>(src)[r * NW + w];
            sa = ms_dot4(a[r][w], 0x01010101u, sa);
            sa2 = ms_dot4(a[r][w], a[r][w], sa2);
        }
    }
    const int64_t va = (int64_t)N * sa2 - (int64_t)sa * sa;
    if (n_src != N || va < min_va) {                                 // uniform over the workgroup
        if (tid == 0) {
            oi[0] = gx; oi[1] = gy; oi[2] = 1; oi[3] = 0;
            of[0] = MS_NONE; of[1] = MS_NONE; of[2] = 0.0; of[3] = 0.0;
        }
        return;
    }

    // ---- the window: a wave per row, a lane per column
    const int chunks = g.vw / 2;
    for (int wy = wave; wy < g.WS; wy += MS_WAVES) {
        const int64_t y = (int64_t)gy - R - P + wy;
        for (int ch = 0; ch < chunks; ++ch) {
            const int wx = ch * 64 + lane;
            const int64_t x = (int64_t)gx - R - P + wx;
            bool ok = false;
            uint8_t b = 0;
            if (wx < g.WS && x >= 0 && x < W && y >= 0 && y < H) {
                const int64_t pix = (int64_t)fj * HW + y * W + x;
                ok = valid[pix] != 0;
                if (ok) b = gray[pix];
            }
            if (wx < g.stride) win[wy * g.stride + wx] = b;
            const uint64_t m = __ballot(ok);
            if (lane == 0) {
                mask[wy * g.vw + 2 * ch] = (uint32_t)m;
                mask[wy * g.vw + 2 * ch + 1] = (uint32_t)(m >> 32);
            }
        }
    }
    __syncthreads();

    // ---- per window row and candidate column: sum b, sum b^2 over the S pixels to the right, or MS_ROW_BAD
    for (int e = tid; e < g.WS * g.C; e += MS_THREADS) {
        const int y = e / g.C, cx = e - y * g.C;
        const int wi = cx >> 5;
        const uint64_t lo = mask[y * g.vw + wi], hi = wi + 1 < g.vw ? mask[y * g.vw + wi + 1] : 0u;
        const uint32_t m = (uint32_t)(((hi << 32) | lo) >> (cx & 31)) & ((1u << S) - 1u);
        uint32_t sb = 0, sb2 = 0;
        const uint8_t* p = win + y * g.stride + cx;
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const uint32_t b = p[k];
            sb += b;
            sb2 += b * b;
        }
        rows[e] = m == (1u << S) - 1u ? (sb2 << 12) | sb : MS_ROW_BAD;
    }
    __syncthreads();

    // ---- the candidates
    const int n_cand = g.C * g.C;
    double best = MS_NONE;
    int best_c = 0x7fffffff, count = 0;
    for (int c = tid; c < n_cand; c += MS_THREADS) {
        const int cy = c / g.C, cx = c - cy * g.C;
        uint32_t sb = 0, sb2 = 0;
        bool ok = true;
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const uint32_t r = rows[(cy + k) * g.C + cx];
            ok &= r != MS_ROW_BAD;
            sb += r & 0xFFFu;
            sb2 += r >> 12;
        }
        const int64_t vb = (int64_t)N * sb2 - (int64_t)sb * sb;
        ok &= vb >= min_va;
        double s = MS_NONE;
        if (ok) {
            const uint32_t sh = (uint32_t)cx & 3u;
            const uint32_t* wrow = reinterpret_cast<const uint32_t*>(win + cy * g.stride + (cx & ~3));
            uint32_t sab = 0;
#pragma unroll
            for (int r = 0; r < S; ++r) {
                uint32_t wd[NW + 1];
#pragma unroll
                for (int w = 0; w <= NW; ++w) wd[w] = wrow[w];
#pragma unroll
                for (int w = 0; w < NW; ++w) sab = ms_dot4(a[r][w], __builtin_amdgcn_alignbyte(wd[w + 1], wd[w], sh), sab);
                wrow += g.stride / 4;
            }
            const int64_t num = (int64_t)N * sab - (int64_t)sa * sb;
            s = (double)num / sqrt((double)va * (double)vb);
            ++count;
            if (s > best) {                                         // ascending c: a lane's own ties keep the smaller index
                best = s;
                best_c = c;
            }
        }
        sc[c] = s;
    }

    // ---- best score, smallest index on a tie, and the number of valid candidates
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double s = __shfl_xor(best, o);
        const int c = __shfl_xor(best_c, o);
        count += __shfl_xor(count, o);
        if (ms_better(s, c, best, best_c)) {
            best = s;
            best_c = c;
        }
    }
    if (lane == 0) {
        red_s[wave] = best;
        red_c[wave] = best_c;
        red_n[wave] = count;
    }
    __syncthreads();                                                 // also: every score is in LDS
    best = red_s[0]; best_c = red_c[0]; count = red_n[0];
#pragma unroll
    for (int w = 1; w < MS_WAVES; ++w) {
        count += red_n[w];
        if (ms_better(red_s[w], red_c[w], best, best_c)) {
            best = red_s[w];
            best_c = red_c[w];
        }
    }
    if (count == 0) {
        if (tid == 0) {
            oi[0] = gx; oi[1] = gy; oi[2] = 2; oi[3] = 0;
            of[0] = MS_NONE; of[1] = MS_NONE; of[2] = 0.0; of[3] = 0.0;
        }
        return;
    }
    const int by = best_c / g.C, bx = best_c - by * g.C;

    // ---- the second peak: the best valid candidate further than excl from the best
    double s2 = MS_NONE;
    for (int c = tid; c < n_cand; c += MS_THREADS) {
        const int cy = c / g.C, cx = c - cy * g.C;
        const int dx = cx > bx ? cx - bx : bx - cx, dy = cy > by ? cy - by : by - cy;
        const double s = sc[c];
        if ((dx > excl || dy > excl) && s > s2) s2 = s;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double s = __shfl_xor(s2, o);
        s2 = s > s2 ? s : s2;
    }
    __syncthreads();                                                 // red_s was read above by every lane
    if (lane == 0) red_s[wave] = s2;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 0; w < MS_WAVES; ++w) s2 = red_s[w] > s2 ? red_s[w] : s2;

    // ---- sub-pixel step per axis: the parabola through the best score and its two neighbours
    double sub[2] = {0.0, 0.0};
    const int pos[2] = {bx, by}, step[2] = {1, g.C};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (pos[k] > 0 && pos[k] < g.C - 1) {
            const double m = sc[best_c - step[k]], p = sc[best_c + step[k]];
            if (m > -1.5 && p > -1.5) {
                const double den = m - 2.0 * best + p;
                if (den < 0.0) {
                    const double t = 0.5 * (m - p) / den;
                    sub[k] = t < -0.5 ? -0.5 : (t > 0.5 ? 0.5 : t);
                }
            }
        }
    }
    const bool border = bx == 0 || bx == g.C - 1 || by == 0 || by == g.C - 1;
    oi[0] = gx + (bx - R); oi[1] = gy + (by - R); oi[2] = border ? 4 : 0; oi[3] = count;
    of[0] = best; of[1] = s2; of[2] = sub[0]; of[3] = sub[1];
}

int match_max_patch() { return MS_MAX_P; }
int match_max_range() { return MS_MAX_R; }

int launch_match_gray(const float* img, int64_t n_pixels, float a_min, uint8_t* gray, uint8_t* valid, hipStream_t st) {
    const int64_t blocks = (n_pixels + MG_THREADS - 1) / MG_THREADS;
    hipLaunchKernelGGL(match_gray_kernel, dim3((unsigned)blocks), dim3(MG_THREADS), 0, st, reinterpret_cast<const float4*>(img), n_pixels,
                       a_min, gray, valid);
    return launch_status();
}

// 0 = every frame index lies in [0, n_frames) (warp: and every affine entry within +-2^19), 1 = one does not; out_i's first word is the
// scratch (the search overwrites it).  warp: the queries have 10 words, else 6.  Waits for the stream.
int match_check_frames(const int32_t* queries, int64_t n, int64_t n_frames, bool warp, int32_t* scratch, hipStream_t st) {
    if (hipMemsetAsync(scratch, 0, sizeof(int32_t), st) != hipSuccess) return DH_ERR_LAUNCH;
    const dim3 grid((unsigned)((n + MG_THREADS - 1) / MG_THREADS)), block(MG_THREADS);
    if (warp) hipLaunchKernelGGL(match_check_kernel<true>, grid, block, 0, st, queries, n, (int)n_frames, scratch);
    else hipLaunchKernelGGL(match_check_kernel<false>, grid, block, 0, st, queries, n, (int)n_frames, scratch);
    if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    int32_t bad = 0;
    if (hipMemcpyAsync(&bad, scratch, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess) return DH_ERR_LAUNCH;
    if (hipStreamSynchronize(st) != hipSuccess) return DH_ERR_LAUNCH;
    return bad != 0 ? 1 : 0;
}

int launch_match_search(const uint8_t* gray, const uint8_t* valid, int H, int W, const int32_t* queries, int64_t n, bool warp, int P,
                        int R, int excl, int64_t min_va, int32_t* out_i, double* out_f, hipStream_t st) {
    const size_t lds = ms_geom(P, R).bytes;
    const dim3 grid((unsigned)n), block(MS_THREADS);
#define DH_MS_CASE(p)                                                                                                                  \
    case p:                                                                                                                            \
        if (warp)                                                                                                                      \
            hipLaunchKernelGGL((match_search_kernel<p, true>), grid, block, lds, st, gray, valid, H, W, queries, R, excl, min_va,      \
                               out_i, out_f);                                                                                          \
        else                                                                                                                           \
            hipLaunchKernelGGL((match_search_kernel<p, false>), grid, block, lds, st, gray, valid, H, W, queries, R, excl, min_va,     \
                               out_i, out_f);                                                                                          \
        break;
    switch (P) {
        DH_MS_CASE(1) DH_MS_CASE(2) DH_MS_CASE(3) DH_MS_CASE(4) DH_MS_CASE(5) DH_MS_CASE(6) DH_MS_CASE(7)
        default: return DH_ERR_BAD_ARG;
    }
#undef DH_MS_CASE
    return launch_status();
}

}  // namespace dh
