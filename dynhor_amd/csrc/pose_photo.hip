// Photometric pose term (dynhor_amd/pose_photo.py): coloured surface points aligned to blurred frames, the loss and its pose gradient
// reduced to a few numbers per frame (include/dynhor_hip.h states both rules in full).
//
// image_blur_*: a masked, normalised, separable Gaussian.  A pixel's value is v = usable ? (r / 255, g / 255, b / 255, 1) : 0, a tap
// outside the image is 0, and both passes add their taps in ascending order as acc = fma(g_k, v_k, acc) in fp32, so a sum does not
// depend on where a workgroup's run starts.
//   rows:  one workgroup per run of PB_THREADS pixels of an image row; the run and its 2 r neighbours go through LDS once (16 bytes per
//          lane and tap: consecutive lanes read consecutive 16-byte slots), tmp[f,y,x] = sum_k g_k v[f,y,x+k].
//   cols:  one lane per column and PB_ROWS consecutive rows: a row of tmp that several of the lane's outputs need is read once (lanes
//          of a wave read consecutive 16-byte texels), the neighbouring workgroups' rows come from the cache.  s = sum_k g_k tmp[f,y+k,x],
//          out = (s.rgb / s.a, s.a), all 0 where s.a == 0.
// Every frame is worked on alone: bitwise the same from launch to launch and for every split of the frames into calls.
//
// photo_loss_kernel: grid (blocks, frames), one lane per surface point in a grid-stride loop.  The decisions are fp32 and are the
// bake's (mk_project, the nearest pixel, mk_view: mesh_shade.h), then floor(u), floor(w) and the four taps' a >= a_min; a pair that
// passes recomputes x_cam, u, w, cos in fp64 from the fp32 inputs and adds its terms.  Reduction: sums64.h (every lane adds its points
// in ascending order); the workgroups per frame depend on the point count alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "mesh_shade.h"
#include "sums64.h"

namespace dh {

namespace {
constexpr int PB_THREADS = 256;
constexpr int PB_ROWS = 4;                     // output rows per lane of the column pass
constexpr int PB_MAX_RADIUS = 64;              // the row pass keeps PB_THREADS + 2 PB_MAX_RADIUS texels in LDS
constexpr int PH_SUMS = 16;
constexpr int64_t PH_MAX_BLOCKS = 64;          // workgroups per frame of the loss kernel

__device__ __forceinline__ float4 pb_fma(float g, const float4& v, const float4& a) {
    return make_float4(__builtin_fmaf(g, v.x, a.x), __builtin_fmaf(g, v.y, a.y), __builtin_fmaf(g, v.z, a.z), __builtin_fmaf(g, v.w, a.w));
}
}  // namespace

// grid (n_frames * H image rows, column blocks)
__global__ __launch_bounds__(PB_THREADS) void image_blur_rows_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ usable,
                                                                      int W, const float* __restrict__ taps, int r,
                                                                      float4* __restrict__ tmp) {
    __shared__ float4 tile[PB_THREADS + 2 * PB_MAX_RADIUS];
    const int64_t row = (int64_t)blockIdx.x * W;
    const int xb = (int)blockIdx.y * PB_THREADS;
    for (int i = threadIdx.x; i < PB_THREADS + 2 * r; i += PB_THREADS) {
        const int xx = xb - r + i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (xx >= 0 && xx < W && usable[row + xx] != 0) {
            const uint8_t* c = rgb + (row + xx) * 3;
            v = make_float4((float)c[0] / 255.f, (float)c[1] / 255.f, (float)c[2] / 255.f, 1.f);
        }
        tile[i] = v;
    }
    __syncthreads();
    const int x = xb + (int)threadIdx.x;
    if (x >= W) return;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k <= 2 * r; ++k) acc = pb_fma(taps[k], tile[threadIdx.x + k], acc);
    tmp[row + x] = acc;
}

// grid (n_frames * ceil(H / PB_ROWS) row groups, column blocks)
__global__ __launch_bounds__(PB_THREADS) void image_blur_cols_kernel(const float4* __restrict__ tmp, int H, int W, int groups,
                                                                      const float* __restrict__ taps, int r, float4* __restrict__ out) {
    const int x = (int)blockIdx.y * PB_THREADS + threadIdx.x;
    if (x >= W) return;
    const int64_t f = blockIdx.x / (unsigned)groups;
    const int y0 = ((int)blockIdx.x - (int)f * groups) * PB_ROWS;
    const int64_t col = f * (int64_t)H * W + x;                // this frame's row 0, this column
    const int ya = y0 - r > 0 ? y0 - r : 0;
    const int yl = y0 + PB_ROWS - 1 < H - 1 ? y0 + PB_ROWS - 1 : H - 1;
    const int yb = yl < H - 1 - r ? yl + r : H - 1;
    float4 acc[PB_ROWS];
#pragma unroll
    for (int j = 0; j < PB_ROWS; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int yy = ya; yy <= yb; ++yy) {
        const float4 v = tmp[col + (int64_t)yy * W];
#pragma unroll
        for (int j = 0; j < PB_ROWS; ++j) {
            const int k = yy - (y0 + j) + r;                   // ascending in yy: every output adds its taps in ascending order
            if (k >= 0 && k <= 2 * r) acc[j] = pb_fma(taps[k], v, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < PB_ROWS; ++j) {
        if (y0 + j >= H) break;
        const float a = acc[j].w;
        out[col + (int64_t)(y0 + j) * W] = a > 0.f ? make_float4(acc[j].x / a, acc[j].y / a, acc[j].z / a, a)
                                                    : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

namespace {
__device__ __forceinline__ double ph_huber(double e, double delta, double& psi) {
    const double a = fabs(e);
    const bool in = a <= delta;
    psi = in ? e : (e > 0.0 ? delta : -delta);
    return in ? 0.5 * e * e : delta * (a - 0.5 * delta);
}
}  // namespace

// grid (blocks, frames); partial [frames, blocks, PH_SUMS] doubles
static_assert(PB_THREADS == SUM64_THREADS, "sum64_block_store folds a workgroup of SUM64_THREADS");
__global__ __launch_bounds__(PB_THREADS) void photo_loss_kernel(const float* __restrict__ pts, const float* __restrict__ normals,
                                                                 const float* __restrict__ colors, int64_t n,
                                                                 const float4* __restrict__ img, const uint64_t* __restrict__ zbuf,
                                                                 const float* __restrict__ R, const float* __restrict__ T,
                                                                 const float* __restrict__ K, int H, int W, float depth_eps,
                                                                 float min_cos, float a_min, float delta_f,
                                                                 double* __restrict__ partial) {
    const int64_t f = blockIdx.y, HW = (int64_t)H * W;
    const float* Rf = R + f * 9;
    const float* Tf = T + f * 3;
    const float k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5];
    const float fw = (float)W, fh = (float)H;
    const double delta = delta_f;
    double Rd[9], Td[3], Kd[6];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rd[k] = Rf[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) Td[k] = Tf[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) Kd[k] = K[k];
    // the camera centre C = -R^T T in fp64, for the weight
    const double Cx = -(Rd[0] * Td[0] + Rd[3] * Td[1] + Rd[6] * Td[2]);
    const double Cy = -(Rd[1] * Td[0] + Rd[4] * Td[1] + Rd[7] * Td[2]);
    const double Cz = -(Rd[2] * Td[0] + Rd[5] * Td[1] + Rd[8] * Td[2]);
    double acc[PH_SUMS];
#pragma unroll
    for (int k = 0; k < PH_SUMS; ++k) acc[k] = 0.0;
    const float4* imf = img + f * HW;
    const int64_t stride = (int64_t)gridDim.x * PB_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * PB_THREADS + threadIdx.x; i < n; i += stride) {
        const float vx = pts[i * 3 + 0], vy = pts[i * 3 + 1], vz = pts[i * 3 + 2];
        const float nx = normals[i * 3 + 0], ny = normals[i * 3 + 1], nz = normals[i * 3 + 2];
        const Cam c = mk_project(Rf, Tf, k00, k01, k02, k10, k11, k12, vx, vy, vz);
        const float px = floorf(c.u + 0.5f), py = floorf(c.w + 0.5f);
        const bool in = (c.c2 > 1e-3f) & (px >= 0.f) & (px < fw) & (py >= 0.f) & (py < fh);
        const int64_t pix = f * HW + (in ? (int64_t)(int)py * W + (int)px : 0);
        const View v = mk_view(zbuf[pix], c.c2, depth_eps, Rf, Tf, vx, vy, vz, nx, ny, nz);
        const float x0f = floorf(c.u), y0f = floorf(c.w);
        // in bounds the floats are exact integers: x0f + 1 <= W - 1 is the last tap's column
        const bool taps_in = (x0f >= 0.f) & (x0f + 1.f < fw) & (y0f >= 0.f) & (y0f + 1.f < fh);
        if (!(in & v.seen & (v.cos >= min_cos) & taps_in)) continue;
        const int x0 = (int)x0f, y0 = (int)y0f;
        const float4 i00 = imf[(int64_t)y0 * W + x0], i10 = imf[(int64_t)y0 * W + x0 + 1];
        const float4 i01 = imf[(int64_t)(y0 + 1) * W + x0], i11 = imf[(int64_t)(y0 + 1) * W + x0 + 1];
        if (!((i00.w >= a_min) & (i10.w >= a_min) & (i01.w >= a_min) & (i11.w >= a_min))) continue;
        // values in fp64 from the fp32 inputs
        const double x = vx, y = vy, z = vz;
        const double c0 = Rd[0] * x + Rd[1] * y + Rd[2] * z + Td[0];
        const double c1 = Rd[3] * x + Rd[4] * y + Rd[5] * z + Td[1];
        const double c2 = Rd[6] * x + Rd[7] * y + Rd[8] * z + Td[2];
        const double u = (Kd[0] * c0 + Kd[1] * c1 + Kd[2] * c2) / c2;
        const double w = (Kd[3] * c0 + Kd[4] * c1 + Kd[5] * c2) / c2;
        const double fx = u - (double)x0, fy = w - (double)y0;
        const double dx = Cx - x, dy = Cy - y, dz = Cz - z;
        const double om = ((double)nx * dx + (double)ny * dy + (double)nz * dz) / sqrt(dx * dx + dy * dy + dz * dz);
        const float a00[3] = {i00.x, i00.y, i00.z}, a10[3] = {i10.x, i10.y, i10.z};
        const float a01[3] = {i01.x, i01.y, i01.z}, a11[3] = {i11.x, i11.y, i11.z};
        double rho = 0.0, gu = 0.0, gw = 0.0;
        bool inl = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double p00 = a00[k], p10 = a10[k], p01 = a01[k], p11 = a11[k];
            const double I = (1.0 - fy) * ((1.0 - fx) * p00 + fx * p10) + fy * ((1.0 - fx) * p01 + fx * p11);
            const double Iu = (1.0 - fy) * (p10 - p00) + fy * (p11 - p01);
            const double Iw = (1.0 - fx) * (p01 - p00) + fx * (p11 - p10);
            const double e = I - (double)colors[i * 3 + k];
            double psi;
            rho += ph_huber(e, delta, psi);
            inl &= fabs(e) <= delta;
            gu += psi * Iu;
            gw += psi * Iw;
        }
        gu *= om;
        gw *= om;
        const double iz = 1.0 / c2;
        const double g[3] = {(gu * Kd[0] + gw * Kd[3]) * iz, (gu * Kd[1] + gw * Kd[4]) * iz, (gu * (Kd[2] - u) + gw * (Kd[5] - w)) * iz};
        const double p[3] = {x, y, z};
        acc[0] += om * rho;
        acc[1] += om;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[2 + 3 * rr + k] += g[rr] * p[k];
            acc[11 + rr] += g[rr];
        }
        acc[14] += 1.0;
        acc[15] += inl ? 1.0 : 0.0;
    }
    sum64_block_store(acc, partial + (f * gridDim.x + blockIdx.x) * PH_SUMS);
}

int image_blur_max_radius() { return PB_MAX_RADIUS; }

int launch_image_blur(const uint8_t* rgb, const uint8_t* usable, int64_t n_frames, int H, int W, const float* taps, int radius,
                      float* tmp, float* out, hipStream_t st) {
    const unsigned cb = (unsigned)((W + PB_THREADS - 1) / PB_THREADS);
    hipLaunchKernelGGL(image_blur_rows_kernel, dim3((unsigned)(n_frames * H), cb), dim3(PB_THREADS), 0, st, rgb, usable, W, taps, radius,
                       reinterpret_cast<float4*>(tmp));
    if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    const int groups = (H + PB_ROWS - 1) / PB_ROWS;
    hipLaunchKernelGGL(image_blur_cols_kernel, dim3((unsigned)(n_frames * groups), cb), dim3(PB_THREADS), 0, st,
                       reinterpret_cast<const float4*>(tmp), H, W, groups, taps, radius, reinterpret_cast<float4*>(out));
    return launch_status();
}

int photo_loss_sums() { return PH_SUMS; }

int64_t photo_loss_grad_workspace(int64_t n_frames, int64_t n_points) {
    return n_frames * sum64_blocks(n_points, PH_MAX_BLOCKS) * PH_SUMS * (int64_t)sizeof(double);
}

int launch_photo_loss_grad(const float* pts, const float* normals, const float* colors, int64_t n, const float* img,
                           const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                           float depth_eps, float min_cos, float a_min, float delta, double* out, void* ws, hipStream_t st) {
    const int64_t blocks = sum64_blocks(n, PH_MAX_BLOCKS);
    double* partial = static_cast<double*>(ws);
    hipLaunchKernelGGL(photo_loss_kernel, dim3((unsigned)blocks, (unsigned)n_frames), dim3(PB_THREADS), 0, st, pts, normals, colors, n,
                       reinterpret_cast<const float4*>(img), zbuf, R, T, K, H, W, depth_eps, min_cos, a_min, delta, partial);
    if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    return launch_sum64_reduce(partial, n_frames, (int)blocks, PH_SUMS, out, st);
}

}  // namespace dh
