// Signed distance from arbitrary points to a triangle mesh (dynhor_amd/mesh_sdf.py: the template prior of the SDF warm start,
// dynhor_amd/sdf_init.py): per point the squared distance to the closest point of any triangle, the lowest face index that attains
// it, and the generalised winding number (its sign rule: inside where wind >= 0.5).
//
// Brute force, every (point, face) pair, in the layout of nn.hip: each lane holds MS_K points in registers, the workgroup stages the
// face records through LDS in tiles and every lane reads the SAME address (a broadcast: no bank conflict), so three ds_read_b128
// feed MS_K points.  One workgroup size, no atomics, no cross-lane operation at all.
//
// Record (mesh_sdf_prepare_kernel, MS_REC = 12 floats = three float4 per face):
//   [0] corner a.xyz, |e0|^2      [1] e0 = b - a, e0.e1      [2] e1 = c - a, |e1|^2 with the sign bit = "no solid angle"
// The sign bit of the last word (|e1|^2 >= 0 otherwise) marks a face that adds exactly 0 to the winding sum: a zero-area face (the
// fp32 cross product of its edges, products rounded one by one, is exactly zero) or an invalid one (an index outside [0, nv), a
// non-finite corner).  An invalid face has corner +inf and zero edges: every dot product with it is NaN, its distance is NaN, and a
// NaN never passes the strict `<` of the sweep.  A zero-area face is rewritten as (P, Q, Q) with P, Q its two corners farthest apart
// (first pair in the order ab, ac, bc among equals): a segment, or a point, which the region tests below classify without the
// interior case (see `vc`).
//
// Distance (per pair, fp32): the closest point by the seven regions of the triangle (three corners, three edges, the interior),
// computed from ap = p - a, d1 = e0.ap, d2 = e1.ap and the record's edge dot products; every region yields the barycentric pair (v, w)
// of q = a + v e0 + w e1 as numerator / denominator, chosen with selects (no branch: a wave never diverges by region), one reciprocal.
// The squared distance is then formed in the difference form |ap - v e0 - w e1|^2 -- the dot products only classify and
// parametrise, they never enter the distance, so nothing cancels near the surface.
// Winding: with a, b, c = corners - p (b = a + e0, c = a + e1), omega = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|),
// every term fp32, added in fp64 per lane in ascending face order.
//
// Reproducibility: the face range is cut into slabs of MS_SLAB faces (grid.y) -- a constant, so the slab boundaries depend on nf
// alone, never on the point count.  A lane sweeps its slab in ascending order with a strict `<` (the lowest index among ties); with
// more than one slab each writes (sqdist, face, fp64 winding partial) into the caller's workspace and mesh_sdf_merge_kernel takes the
// lexicographic minimum and adds the partials in slab order.  No operation involves two points, so all three outputs are the same
// bits from launch to launch and however the points are chunked over launches.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "launch.h"
#include "mul_rn.h"

namespace dh {

namespace {
constexpr int MS_THREADS = 256;
constexpr int MS_K = 4;                                // points per lane
constexpr int64_t MS_PPB = MS_THREADS * MS_K;          // points per workgroup
constexpr int MS_TILE = 256;                           // faces per LDS tile (12 KB: three float4 each)
constexpr int64_t MS_SLAB = 2 * MS_TILE;               // faces per slab: a constant (see above)
constexpr int MS_REC = 12;

inline int64_t ms_slabs(int64_t nf) { return nf > 0 ? (nf + MS_SLAB - 1) / MS_SLAB : 1; }

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }
}  // namespace

// one thread per face
__global__ __launch_bounds__(256) void mesh_sdf_prepare_kernel(const float* __restrict__ verts, int64_t nv, const int32_t* __restrict__ faces,
                                                               int64_t nf, float4* __restrict__ rec) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int64_t i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    const float inf = INFINITY;
    float4 r0 = make_float4(inf, inf, inf, 0.f), r1 = make_float4(0.f, 0.f, 0.f, 0.f), r2 = make_float4(0.f, 0.f, 0.f, -0.f);
    if (i0 >= 0 && i0 < nv && i1 >= 0 && i1 < nv && i2 >= 0 && i2 < nv) {
        float ax = verts[i0 * 3 + 0], ay = verts[i0 * 3 + 1], az = verts[i0 * 3 + 2];
        float bx = verts[i1 * 3 + 0], by = verts[i1 * 3 + 1], bz = verts[i1 * 3 + 2];
        float cx = verts[i2 * 3 + 0], cy = verts[i2 * 3 + 1], cz = verts[i2 * 3 + 2];
        if (finite3(ax, ay, az) && finite3(bx, by, bz) && finite3(cx, cy, cz)) {
            float ux = bx - ax, uy = by - ay, uz = bz - az;
            float vx = cx - ax, vy = cy - ay, vz = cz - az;
            // edge cross product, every product rounded on its own: a repeated corner gives exactly zero
            const float nx = mul_rn(uy, vz) - mul_rn(uz, vy), ny = mul_rn(uz, vx) - mul_rn(ux, vz), nz = mul_rn(ux, vy) - mul_rn(uy, vx);
            const bool flat = nx == 0.f && ny == 0.f && nz == 0.f;
            if (flat) {
                const float wx = cx - bx, wy = cy - by, wz = cz - bz;
                const float lab = ux * ux + uy * uy + uz * uz, lac = vx * vx + vy * vy + vz * vz, lbc = wx * wx + wy * wy + wz * wz;
                if (lac > lab && lac >= lbc) {                    // P = a, Q = c
                    ux = vx; uy = vy; uz = vz;
                } else if (lbc > lab && lbc > lac) {              // P = b, Q = c
                    ax = bx; ay = by; az = bz;
                    ux = wx; uy = wy; uz = wz;
                }                                                 // else P = a, Q = b
                vx = ux; vy = uy; vz = uz;
            }
            const float d00 = ux * ux + uy * uy + uz * uz, d01 = ux * vx + uy * vy + uz * vz, d11 = vx * vx + vy * vy + vz * vz;
            r0 = make_float4(ax, ay, az, flat ? d01 : d00);       // (flat: e0 == e1, one value for all three -- bit-equal dot products)
            r1 = make_float4(ux, uy, uz, d01);
            r2 = make_float4(vx, vy, vz, flat ? -d01 : d11);
        }
    }
    rec[f * 3 + 0] = r0;
    rec[f * 3 + 1] = r1;
    rec[f * 3 + 2] = r2;
}

// grid (point blocks, slabs).  direct (one slab): sqdist / face / wind are the caller's outputs.  Otherwise slab s writes its
// partials at pd + s * n, pi + s * n, pw + s * n.
__global__ __launch_bounds__(MS_THREADS) void mesh_sdf_query_kernel(const float4* __restrict__ rec, int64_t nf, const float* __restrict__ pts,
                                                                    int64_t n, int direct, float* __restrict__ od, int32_t* __restrict__ oi,
                                                                    float* __restrict__ ow, double* __restrict__ pw) {
    __shared__ float4 tA[MS_TILE], tU[MS_TILE], tV[MS_TILE];
    const int t = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * MS_PPB + t;
    float px[MS_K], py[MS_K], pz[MS_K], best[MS_K];
    int bi[MS_K];
    double wind[MS_K];
#pragma unroll
    for (int k = 0; k < MS_K; ++k) {
        const int64_t i = p0 + (int64_t)k * MS_THREADS;
        const bool in = i < n;
        px[k] = in ? pts[i * 3 + 0] : 0.f;
        py[k] = in ? pts[i * 3 + 1] : 0.f;
        pz[k] = in ? pts[i * 3 + 2] : 0.f;
        best[k] = INFINITY;
        bi[k] = -1;
        wind[k] = 0.0;
    }
    const int64_t f0 = (int64_t)blockIdx.y * MS_SLAB;
    const int64_t f1 = f0 + MS_SLAB < nf ? f0 + MS_SLAB : nf;
    for (int64_t base = f0; base < f1; base += MS_TILE) {
        const int cnt = (int)(f1 - base < MS_TILE ? f1 - base : MS_TILE);
        __syncthreads();                                          // the previous tile has been read by every wave
        if (t < cnt) {                                            // MS_TILE == MS_THREADS: one face per thread
            const int64_t g = base + t;
            tA[t] = rec[g * 3 + 0];
            tU[t] = rec[g * 3 + 1];
            tV[t] = rec[g * 3 + 2];
        }
        __syncthreads();
        const int jb = (int)base;                                 // nf < 2^31 (api.hip)
        for (int j = 0; j < cnt; ++j) {
            const float4 A = tA[j], U = tU[j], V = tV[j];
            const float d00 = A.w, d01 = U.w, d11 = fabsf(V.w);
            const bool solid = __float_as_int(V.w) >= 0;          // the sign bit: no solid angle (zero-area or invalid face)
#pragma unroll
            for (int k = 0; k < MS_K; ++k) {
                const float apx = px[k] - A.x, apy = py[k] - A.y, apz = pz[k] - A.z;
                const float d1 = __builtin_fmaf(U.z, apz, __builtin_fmaf(U.y, apy, U.x * apx));
                const float d2 = __builtin_fmaf(V.z, apz, __builtin_fmaf(V.y, apy, V.x * apx));
                const float d3 = d1 - d00, d4 = d2 - d01;         // e0.(p - b), e1.(p - b)
                const float d5 = d1 - d01, d6 = d2 - d11;         // e0.(p - c), e1.(p - c)
                // products rounded one by one: on a (P, Q, Q) record d1 == d2, d3 == d4, d5 == d6 bit for bit and vc, vb, va are
                // exactly 0, so such a face always ends in a corner or on the edge ab
                const float vc = mul_rn(d1, d4) - mul_rn(d3, d2);
                const float vb = mul_rn(d5, d2) - mul_rn(d1, d6);
                const float va = mul_rn(d3, d6) - mul_rn(d5, d4);
                const float s43 = d4 - d3, s56 = d5 - d6;
                // the interior first, then the regions from the last tested to the first: the first that holds wins
                float vn = vb, wn = vc, den = va + vb + vc;
                const bool rbc = va <= 0.f && s43 >= 0.f && s56 >= 0.f;
                vn = rbc ? s56 : vn; wn = rbc ? s43 : wn; den = rbc ? s43 + s56 : den;
                const bool rac = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
                vn = rac ? 0.f : vn; wn = rac ? d2 : wn; den = rac ? d2 - d6 : den;
                const bool rc = d6 >= 0.f && d5 <= d6;
                vn = rc ? 0.f : vn; wn = rc ? 1.f : wn; den = rc ? 1.f : den;
                const bool rab = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
                vn = rab ? d1 : vn; wn = rab ? 0.f : wn; den = rab ? d1 - d3 : den;
                const bool rb = d3 >= 0.f && d4 <= d3;
                vn = rb ? 1.f : vn; wn = rb ? 0.f : wn; den = rb ? 1.f : den;
                const bool ra = d1 <= 0.f && d2 <= 0.f;
                vn = ra ? 0.f : vn; wn = ra ? 0.f : wn; den = ra ? 1.f : den;
                // (a zero denominator meets a zero numerator only: an edge of length 0, a triangle below fp32's range)
                const float inv = __builtin_amdgcn_rcpf(fmaxf(den, 1.17549435e-38f));
                const float v = fminf(vn * inv, 1.f), w = fminf(wn * inv, 1.f);
                const float rx = __builtin_fmaf(-w, V.x, __builtin_fmaf(-v, U.x, apx));
                const float ry = __builtin_fmaf(-w, V.y, __builtin_fmaf(-v, U.y, apy));
                const float rz = __builtin_fmaf(-w, V.z, __builtin_fmaf(-v, U.z, apz));
                const float d = __builtin_fmaf(rz, rz, __builtin_fmaf(ry, ry, rx * rx));
                if (d < best[k]) {
                    best[k] = d;
                    bi[k] = jb + j;
                }
                // solid angle of the face seen from p (Van Oosterom & Strackee)
                const float ax = -apx, ay = -apy, az = -apz;
                const float bx = ax + U.x, by = ay + U.y, bz = az + U.z;
                const float cx = ax + V.x, cy = ay + V.y, cz = az + V.z;
                const float la = sqrtf(__builtin_fmaf(az, az, __builtin_fmaf(ay, ay, ax * ax)));
                const float lb = sqrtf(__builtin_fmaf(bz, bz, __builtin_fmaf(by, by, bx * bx)));
                const float lc = sqrtf(__builtin_fmaf(cz, cz, __builtin_fmaf(cy, cy, cx * cx)));
                const float ab = __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
                const float bc = __builtin_fmaf(bz, cz, __builtin_fmaf(by, cy, bx * cx));
                const float ca = __builtin_fmaf(cz, az, __builtin_fmaf(cy, ay, cx * ax));
                const float nx = by * cz - bz * cy, ny = bz * cx - bx * cz, nz = bx * cy - by * cx;
                const float det = __builtin_fmaf(az, nz, __builtin_fmaf(ay, ny, ax * nx));
                const float den3 = __builtin_fmaf(ca, lb, __builtin_fmaf(bc, la, __builtin_fmaf(ab, lc, la * lb * lc)));
                const float om = solid ? 2.f * atan2f(det, den3) : 0.f;
                wind[k] += (double)om;
            }
        }
    }
    const int64_t so = direct ? 0 : (int64_t)blockIdx.y * n;
#pragma unroll
    for (int k = 0; k < MS_K; ++k) {
        const int64_t i = p0 + (int64_t)k * MS_THREADS;
        if (i < n) {
            // a non-finite point: every distance was NaN (best = +inf, face = -1 already); its winding sum is dropped
            const double wk = finite3(px[k], py[k], pz[k]) ? wind[k] : 0.0;
            od[so + i] = best[k];
            if (oi) oi[so + i] = bi[k];
            if (direct) {
                if (ow) ow[i] = (float)(wk / (4.0 * M_PI));
            } else {
                pw[so + i] = wk;
            }
        }
    }
}

// lexicographic minimum of the slabs' (sqdist, face) pairs and the sum of their winding partials, both in ascending slab order
__global__ __launch_bounds__(256) void mesh_sdf_merge_kernel(const float* __restrict__ pd, const int32_t* __restrict__ pi,
                                                             const double* __restrict__ pw, int64_t n, int slabs, float* __restrict__ sqdist,
                                                             int32_t* __restrict__ face, float* __restrict__ wind) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float b = pd[i];
    int32_t bi = pi[i];
    double w = pw[i];
    for (int s = 1; s < slabs; ++s) {
        const float d = pd[(int64_t)s * n + i];
        if (d < b) {
            b = d;
            bi = pi[(int64_t)s * n + i];
        }
        w += pw[(int64_t)s * n + i];
    }
    sqdist[i] = b;
    if (face) face[i] = bi;
    if (wind) wind[i] = (float)(w / (4.0 * M_PI));
}

int mesh_sdf_record_floats() { return MS_REC; }

int64_t mesh_sdf_query_workspace(int64_t n, int64_t nf) {
    const int64_t s = ms_slabs(nf);
    return s > 1 ? s * n * (int64_t)(sizeof(double) + sizeof(float) + sizeof(int32_t)) : 0;
}

int64_t mesh_sdf_max_faces() { return 65535 * MS_SLAB; }

int launch_mesh_sdf_prepare(const float* verts, int64_t nv, const int32_t* faces, int64_t nf, float* rec, hipStream_t st) {
    hipLaunchKernelGGL(mesh_sdf_prepare_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, verts, nv, faces, nf,
                       reinterpret_cast<float4*>(rec));
    return launch_status();
}

int launch_mesh_sdf_query(const float* rec, int64_t nf, const float* pts, int64_t n, float* sqdist, int32_t* face, float* wind, void* ws,
                          hipStream_t st) {
    const int64_t pb = (n + MS_PPB - 1) / MS_PPB;
    const int64_t slabs = ms_slabs(nf);
    const float4* r = reinterpret_cast<const float4*>(rec);
    if (slabs == 1) {
        hipLaunchKernelGGL(mesh_sdf_query_kernel, dim3((unsigned)pb, 1), dim3(MS_THREADS), 0, st, r, nf, pts, n, 1, sqdist, face, wind,
                           (double*)nullptr);
        return launch_status();
    }
    // scratch: the slabs' winding partials [slabs, n] doubles, then their distances [slabs, n] floats, then their faces [slabs, n] int32
    double* pw = static_cast<double*>(ws);
    float* pd = reinterpret_cast<float*>(pw + slabs * n);
    int32_t* pi = reinterpret_cast<int32_t*>(pd + slabs * n);
    hipLaunchKernelGGL(mesh_sdf_query_kernel, dim3((unsigned)pb, (unsigned)slabs), dim3(MS_THREADS), 0, st, r, nf, pts, n, 0, pd, pi,
                       (float*)nullptr, pw);
    if (launch_status() != DH_OK) return DH_ERR_LAUNCH;
    hipLaunchKernelGGL(mesh_sdf_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pd, pi, pw, n, (int)slabs, sqdist, face,
                       wind);
    return launch_status();
}

}  // namespace dh
