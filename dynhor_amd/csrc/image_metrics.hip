// Image metrics (dynhor_amd/image_metrics.py): a masked structural similarity (SSIM) of 8-bit renderings against 8-bit frames, with the
// squared and absolute error sums of the same pixels (include/dynhor_hip.h states the rule in full).
//
// ssim_kernel: grid (tiles of a frame, frames), one workgroup of IM_THREADS lanes per IM_TW x IM_TH output tile, dynamic LDS sized by
// the radius r (HH = IM_TH + 2r rows, HW = IM_TW + 2r columns of halo):
//   stage   seven byte planes [HH][HW]: a and b per channel and u, all 0 where the pixel is unusable or outside the image (so the
//           moments need no second multiply by u).  Read from HBM once.
//   rows    per halo row and output column the row sums over k = -r..r of tap * (u | a | b | a^2 | b^2 | a b) into u32 planes
//           [HH][IM_TW]: u once, then the five moments one channel at a time.  A row sum is at most 65025 * 65536 < 2^32.
//   columns a lane owns the pixels (x, y) and (x, y + 8) of the tile (lane = column: the 32 lanes of a plane row read 32 consecutive
//           words) and adds tap * row sum over the 2r + 1 rows in 64 bits (at most 2^48), then applies the formula in fp64.  The
//           products go through mul_rn (mul_rn.h): nothing is contracted into an fma, so an fp64 restatement gives the same bits.
//   sums    a lane adds its two pixels in ascending y; sum64_block_store (sums64.h) folds the lanes and waves in a fixed order and
//           stores one partial per workgroup; launch_sum64_reduce adds a frame's partials in tile order.
// The filtered planes never leave LDS; no atomics.  The tiles of a frame depend on H and W alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "mul_rn.h"
#include "sums64.h"

#pragma clang fp contract(off)

namespace dh {

namespace {
constexpr int IM_THREADS = SUM64_THREADS;
constexpr int IM_TW = 32, IM_TH = 16;
constexpr int IM_ROWS = IM_THREADS / IM_TW;          // tile rows per pass of the workgroup
constexpr int IM_PER_LANE = IM_TH / IM_ROWS;         // output pixels per lane
constexpr int IM_MAX_R = 16;
constexpr int IM_SUMS = 6;
constexpr int IM_PLANES = 6;                         // u, a, b, a^2, b^2, a b

struct ImTaps {
    int32_t t[2 * IM_MAX_R + 1];
};

__host__ __device__ inline size_t im_stage_bytes(int r) {
    return ((size_t)7 * (IM_TH + 2 * r) * (IM_TW + 2 * r) + 15) & ~(size_t)15;
}
inline size_t im_lds_bytes(int r) { return im_stage_bytes(r) + (size_t)IM_PLANES * (IM_TH + 2 * r) * IM_TW * sizeof(uint32_t); }
inline int64_t im_tiles(int H, int W) { return (int64_t)((H + IM_TH - 1) / IM_TH) * ((W + IM_TW - 1) / IM_TW); }
}  // namespace

// partial [frames, tiles, IM_SUMS] doubles
__global__ __launch_bounds__(IM_THREADS) void ssim_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                           const uint8_t* __restrict__ usable, int H, int W, int tiles_x, ImTaps taps,
                                                           int r, uint64_t w_min, float* __restrict__ map,
                                                           double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int HH = IM_TH + 2 * r, HW = IM_TW + 2 * r, n_halo = HH * HW, n_row = HH * IM_TW, S = 2 * r + 1;
    uint8_t* sa = lds;                                               // [3][HH][HW]
    uint8_t* sb = sa + 3 * n_halo;
    uint8_t* su = sb + 3 * n_halo;                                   // [HH][HW]
    uint32_t* pl = reinterpret_cast<uint32_t*>(lds + im_stage_bytes(r));   // [IM_PLANES][HH][IM_TW]

    const int tid = threadIdx.x;
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int64_t frame = (int64_t)blockIdx.y * H * W;
    const int x0 = tx * IM_TW - r, y0 = ty * IM_TH - r;

    // ---- stage the tile and its halo
    for (int e = tid; e < n_halo; e += IM_THREADS) {
        const int hy = e / HW, hx = e - hy * HW;
        const int x = x0 + hx, y = y0 + hy;
        uint8_t u = 0, av[3] = {0, 0, 0}, bv[3] = {0, 0, 0};
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const int64_t p = frame + (int64_t)y * W + x;
            u = usable ? (usable[p] != 0 ? 1 : 0) : 1;
            if (u) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    av[c] = a[p * 3 + c];
                    bv[c] = b[p * 3 + c];
                }
            }
        }
        su[e] = u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sa[c * n_halo + e] = av[c];
            sb[c * n_halo + e] = bv[c];
        }
    }
    __syncthreads();

    // ---- the lane's pixels: (lx, ly + j IM_ROWS) of the tile
    const int lx = tid & (IM_TW - 1), ly = tid / IM_TW;
    uint64_t wt[IM_PER_LANE];
    double ssum[IM_PER_LANE];
    int64_t se = 0, ae = 0;
#pragma unroll
    for (int j = 0; j < IM_PER_LANE; ++j) ssum[j] = 0.0;

    // C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, each formed as k * k from the rounded k
    constexpr double K1 = 0.01 * 255.0, K2 = 0.03 * 255.0;
    constexpr double C1 = K1 * K1, C2 = K2 * K2;

    for (int c = 0; c < 3; ++c) {
        // ---- rows: tap-weighted sums along x into the u32 planes
        const uint8_t* ca = sa + c * n_halo;
        const uint8_t* cb = sb + c * n_halo;
        for (int e = tid; e < n_row; e += IM_THREADS) {
            const int hy = e / IM_TW, x = e - hy * IM_TW;
            const int o = hy * HW + x;
            uint32_t s_u = 0, s_a = 0, s_b = 0, s_aa = 0, s_bb = 0, s_ab = 0;
            for (int k = 0; k < S; ++k) {
                const uint32_t t = (uint32_t)taps.t[k];
                const uint32_t va = ca[o + k], vb = cb[o + k];
                const uint32_t ta = t * va, tb = t * vb;
                s_a += ta;
                s_b += tb;
                s_aa += ta * va;
                s_bb += tb * vb;
                s_ab += ta * vb;
                if (c == 0) s_u += t * su[o + k];
            }
            if (c == 0) pl[e] = s_u;
            pl[1 * n_row + e] = s_a;
            pl[2 * n_row + e] = s_b;
            pl[3 * n_row + e] = s_aa;
            pl[4 * n_row + e] = s_bb;
            pl[5 * n_row + e] = s_ab;
        }
        __syncthreads();

        // ---- columns, then the formula
#pragma unroll
        for (int j = 0; j < IM_PER_LANE; ++j) {
            const int y = ly + j * IM_ROWS;
            const uint32_t* col = pl + y * IM_TW + lx;
            if (c == 0) {
                uint64_t w = 0;
                for (int k = 0; k < S; ++k) w += (uint64_t)(uint32_t)taps.t[k] * col[k * IM_TW];
                wt[j] = w;
            }
            const int centre = (y + r) * HW + lx + r;
            const int d = (int)ca[centre] - (int)cb[centre];      // both 0 where the pixel is not usable
            se += d * d;
            ae += d < 0 ? -d : d;
            if (su[centre] != 0 && wt[j] >= w_min) {
                uint64_t s_a = 0, s_b = 0, s_aa = 0, s_bb = 0, s_ab = 0;
                for (int k = 0; k < S; ++k) {
                    const uint64_t t = (uint32_t)taps.t[k];
                    const int i = k * IM_TW;
                    s_a += t * col[1 * n_row + i];
                    s_b += t * col[2 * n_row + i];
                    s_aa += t * col[3 * n_row + i];
                    s_bb += t * col[4 * n_row + i];
                    s_ab += t * col[5 * n_row + i];
                }
                const double w = (double)wt[j];
                const double mx = (double)s_a / w, my = (double)s_b / w;
                const double mxx = mul_rn(mx, mx), myy = mul_rn(my, my), mxy = mul_rn(mx, my);
                const double vx = (double)s_aa / w - mxx, vy = (double)s_bb / w - myy, cxy = (double)s_ab / w - mxy;
                const double num = mul_rn(mul_rn(2.0 * mx, my) + C1, 2.0 * cxy + C2);
                const double den = mul_rn((mxx + myy) + C1, (vx + vy) + C2);
                ssum[j] += num / den;                                // (s_0 + s_1) + s_2, from 0.0
            }
        }
        __syncthreads();                                             // the next channel's rows overwrite the planes
    }

    // ---- per-lane sums in ascending y, the map
    double acc[IM_SUMS] = {0.0, 0.0, (double)se, (double)ae, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < IM_PER_LANE; ++j) {
        const int y = ly + j * IM_ROWS;
        const int gx = tx * IM_TW + lx, gy = ty * IM_TH + y;
        const bool inside = gx < W && gy < H;
        const bool use = su[(y + r) * HW + lx + r] != 0;
        const bool counted = use && wt[j] >= w_min;
        const double s = counted ? ssum[j] / 3.0 : 0.0;
        if (counted) {
            acc[0] += s;
            acc[1] += 1.0;
            acc[5] += mul_rn(s, s);
        }
        if (use) acc[4] += 1.0;
        if (map && inside) map[frame + (int64_t)gy * W + gx] = (float)s;
    }
    sum64_block_store<IM_SUMS>(acc, partial + ((int64_t)blockIdx.y * gridDim.x + tile) * IM_SUMS);
}

int ssim_sums() { return IM_SUMS; }
int ssim_max_radius() { return IM_MAX_R; }
int64_t ssim_tiles_per_frame(int H, int W) { return im_tiles(H, W); }

int64_t ssim_workspace(int64_t n_frames, int H, int W) { return n_frames * im_tiles(H, W) * IM_SUMS * (int64_t)sizeof(double); }

int launch_ssim(const uint8_t* a, const uint8_t* b, const uint8_t* usable, int64_t n_frames, int H, int W, const int32_t* taps_host,
                int radius, uint64_t w_min, float* map, double* out, void* ws, hipStream_t st) {
    ImTaps taps = {};
    for (int k = 0; k < 2 * radius + 1; ++k) taps.t[k] = taps_host[k];
    const int64_t tiles = im_tiles(H, W);
    double* partial = static_cast<double*>(ws);
    hipLaunchKernelGGL(ssim_kernel, dim3((unsigned)tiles, (unsigned)n_frames), dim3(IM_THREADS), im_lds_bytes(radius), st, a, b, usable,
                       H, W, (W + IM_TW - 1) / IM_TW, taps, radius, w_min, map, partial);
    if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    return launch_sum64_reduce(partial, n_frames, (int)tiles, IM_SUMS, out, st);
}

}  // namespace dh
