// extern "C" boundary (include/dynhor_hip.h).  Argument checking + launch dispatch only.
#include "../../include/dynhor_hip.h"
#include "kernels.h"
#include "hash_layout.h"
#include "layout.h"
#include "workspace.h"

using namespace dh;

namespace dh {
// the library's only process-global state (include/dynhor_hip.h "Conventions")
static int g_arith = DH_ARITH_SPLIT_F16;
static int g_hash_scatter = 0;
int hash_scatter_mode() { return __atomic_load_n(&g_hash_scatter, __ATOMIC_RELAXED); }
}  // namespace dh

namespace {
inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
inline bool bad_arith(int a) { return a != DH_ARITH_SPLIT_BF16 && a != DH_ARITH_FP32_MFMA && a != DH_ARITH_SPLIT_F16; }
// stages with a tile-PAIR form (chain_pair.hip) accept DH_CHAIN_FORM_* flags above the arithmetic byte, with DH_ARITH_SPLIT_F16 only
inline bool bad_arith_form(int a) {
    const int form = a & ~0xff;
    return bad_arith(a & 0xff) || (form != 0 && form != DH_CHAIN_FORM_TILE && form != DH_CHAIN_FORM_PAIR) ||
           (form != 0 && (a & 0xff) != DH_ARITH_SPLIT_F16);
}
inline int cur_arith() { return __atomic_load_n(&dh::g_arith, __ATOMIC_RELAXED); }
#ifndef DH_GRID_DIV
#define DH_GRID_DIV 1                    // development macro: 2 = ONE workgroup per CU (what a chain's phases cost without a co-resident partner)
#endif
constexpr int DEFAULT_GRID = 256 * 2 / DH_GRID_DIV;   // persistent workgroups: all that are co-resident (two 64-point tiles per CU)
}  // namespace

extern "C" {

int dh_version(void) { return 3; }

int dh_set_arithmetic(int mode) {
    if (bad_arith(mode)) return DH_ERR_BAD_ARG;
    __atomic_store_n(&dh::g_arith, mode, __ATOMIC_RELAXED);
    return DH_OK;
}
int dh_get_arithmetic(void) { return __atomic_load_n(&dh::g_arith, __ATOMIC_RELAXED); }

int dh_hash_set_scatter_mode(int mode) {
    if (mode < 0 || mode > 2) return DH_ERR_BAD_ARG;
    __atomic_store_n(&dh::g_hash_scatter, mode, __ATOMIC_RELAXED);
    return DH_OK;
}

const char* dh_strerror(int status) {
    switch (status) {
        case DH_OK: return "ok";
        case DH_ERR_BAD_ARG: return "bad argument (null / negative size / misaligned pointer)";
        case DH_ERR_UNSUPPORTED: return "unsupported configuration";
        case DH_ERR_LAUNCH: return "kernel launch failed (hipGetLastError)";
        default: return "unknown dynhor_hip status";
    }
}

int64_t dh_num_params(void) { return N_PARAMS; }
int64_t dh_packed_floats(void) { return PACKH.total; }

int dh_packed_section(int section, int64_t* offset_floats, int64_t* n_floats) {
    if (!offset_floats || !n_floats) return DH_ERR_BAD_ARG;
    switch (section) {
        case 0: *offset_floats = PACKT.stream; *n_floats = PACKT_STREAM_FLOATS; break;
        case 1: *offset_floats = PACKT.bias10; *n_floats = 10 * 256; break;
        case 2: *offset_floats = PACKH.stream; *n_floats = PACKTH_STREAM_FLOATS; break;
        case 3: *offset_floats = PACKH.bias11; *n_floats = 11 * 256; break;
        case 4: *offset_floats = PACKH.wabs; *n_floats = 16; break;
        default: return DH_ERR_BAD_ARG;
    }
    return DH_OK;
}

int dh_param_layout(int net, int layer, int64_t* bias_off, int64_t* g_off, int64_t* v_off, int* out_dim, int* in_dim) {
    if (!bias_off || !g_off || !v_off || !out_dim || !in_dim) return DH_ERR_BAD_ARG;
    if (net == 0) {
        if (layer < 0 || layer >= N_SDF) return DH_ERR_BAD_ARG;
        const LinOff o = sdf_off(layer);
        *bias_off = o.bias; *g_off = o.g; *v_off = o.v; *out_dim = SDF_DIMS[layer].out; *in_dim = SDF_DIMS[layer].in;
    } else if (net == 1) {
        *bias_off = *g_off = *v_off = VARIANCE_OFF; *out_dim = 1; *in_dim = 1;
    } else if (net == 2) {
        if (layer < 0 || layer >= N_COL) return DH_ERR_BAD_ARG;
        const LinOff o = col_off(layer);
        *bias_off = o.bias; *g_off = o.g; *v_off = o.v; *out_dim = COL_DIMS[layer].out; *in_dim = COL_DIMS[layer].in;
    } else {
        return DH_ERR_BAD_ARG;
    }
    return DH_OK;
}

int dh_pack_weights(const float* params, float* packed, void* stream) {
    if (!params || !packed || misaligned16(packed)) return DH_ERR_BAD_ARG;
    return launch_pack_weights(params, packed, 7, static_cast<hipStream_t>(stream));
}
int dh_pack_weights_ex(int arithmetic, const float* params, float* packed, void* stream) {
    if (!params || !packed || misaligned16(packed) || bad_arith(arithmetic)) return DH_ERR_BAD_ARG;
    return launch_pack_weights(params, packed, 1 << arithmetic, static_cast<hipStream_t>(stream));
}

int dh_sdf_nograd_ex(int arithmetic, const float* packed, const float* pts, int64_t npts, float* sdf, void* stream) {
    if (npts < 0 || bad_arith(arithmetic)) return DH_ERR_BAD_ARG;
    if (npts == 0) return DH_OK;
    if (!packed || !pts || !sdf || misaligned16(packed)) return DH_ERR_BAD_ARG;
    return launch_sdf_nograd(packed, pts, npts, sdf, DEFAULT_GRID, arithmetic, static_cast<hipStream_t>(stream));
}

int dh_workspace_floats(int64_t npts, int64_t* infer_floats, int64_t* fwd_floats, int64_t* total_floats) {
    if (npts < 0 || !infer_floats || !fwd_floats || !total_floats) return DH_ERR_BAD_ARG;
    const Workspace w = carve_workspace(nullptr, npts);
    *infer_floats = w.infer_floats;
    *fwd_floats = w.fwd_floats;
    *total_floats = w.total_floats;
    return DH_OK;
}

int dh_range_words(int64_t* act_max_off, int64_t* tag_off, float* limit) {
    if (!act_max_off || !tag_off || !limit) return DH_ERR_BAD_ARG;
    // (absmax is the first block of the workspace: carve_workspace)
    *act_max_off = (int64_t)ABSMAX_ACT * ABSMAX_STRIDE;
    *tag_off = (int64_t)ABSMAX_TAG * ABSMAX_STRIDE;
    *limit = H2_RANGE / H2_XS;
    return DH_OK;
}

int dh_sdf_forward_ex(int arithmetic, const float* packed, const float* pts, int64_t npts, float* ws, float* sdf, void* stream) {
    if (bad_arith(arithmetic)) return DH_ERR_BAD_ARG;
    if (npts <= 0) return npts == 0 ? DH_OK : DH_ERR_BAD_ARG;
    if (!packed || !pts || !ws || !sdf || misaligned16(packed) || misaligned16(ws)) return DH_ERR_BAD_ARG;
    const Workspace w = carve_workspace(ws, npts);
    return launch_sdf_fwd_train(packed, pts, npts, sdf, w.feat, w.act, w.eaux, w.absmax, DEFAULT_GRID, arithmetic, static_cast<hipStream_t>(stream));
}

int dh_sdf_gradient_ex(int arithmetic, const float* packed, const float* pts, int64_t npts, float* ws, float* normals, int save,
                       void* stream) {
    if (bad_arith_form(arithmetic)) return DH_ERR_BAD_ARG;
    if (npts <= 0) return npts == 0 ? DH_OK : DH_ERR_BAD_ARG;
    if (!packed || !pts || !ws || !normals || misaligned16(packed) || misaligned16(ws)) return DH_ERR_BAD_ARG;
    const Workspace w = carve_workspace(ws, npts);
    if (save < 0 || save > 2) return DH_ERR_BAD_ARG;
    return launch_sdf_grad(packed, pts, npts, w.act, w.asave, normals, save, w.gesave, w.absmax, DEFAULT_GRID, arithmetic,
                           static_cast<hipStream_t>(stream));
}

int dh_color_forward_ex(int arithmetic, const float* packed, const float* pts, const float* dirs, int n_per_ray, const float* normals,
                        int64_t npts, float* ws, float* color, int save, void* stream) {
    if (npts < 0 || n_per_ray <= 0 || bad_arith_form(arithmetic)) return DH_ERR_BAD_ARG;
    if (npts == 0) return DH_OK;
    if (!packed || !pts || !dirs || !normals || !ws || !color || misaligned16(packed) || misaligned16(ws)) return DH_ERR_BAD_ARG;
    const Workspace w = carve_workspace(ws, npts);
    return launch_color_fwd(packed, pts, dirs, n_per_ray, normals, w.feat, npts, color, w.cact, w.caux, save, w.absmax, DEFAULT_GRID,
                            arithmetic, static_cast<hipStream_t>(stream));
}

int dh_mlp_forward_ex(int arithmetic, const float* packed, const float* pts, const float* dirs, int n_per_ray, int64_t npts, float* ws,
                      float* sdf, float* normals, float* color, void* stream) {
    int rc = dh_sdf_forward_ex(arithmetic, packed, pts, npts, ws, sdf, stream);
    if (rc) return rc;
    rc = dh_sdf_gradient_ex(arithmetic, packed, pts, npts, ws, normals, 1, stream);
    if (rc) return rc;
    return dh_color_forward_ex(arithmetic, packed, pts, dirs, n_per_ray, normals, npts, ws, color, 1, stream);
}

int dh_color_backward_ex(int arithmetic, const float* packed, const float* colors, const float* d_colors, int64_t npts, float* ws,
                         float* d_normals, void* stream) {
    if (npts <= 0 || bad_arith_form(arithmetic)) return DH_ERR_BAD_ARG;
    if (!packed || !colors || !d_colors || !ws || !d_normals || misaligned16(packed) || misaligned16(ws)) return DH_ERR_BAD_ARG;
    const Workspace w = carve_workspace(ws, npts);
    return launch_color_bwd(packed, colors, d_colors, npts, w.cact, w.czbar, w.featbar, d_normals, w.tpart, w.absmax, DEFAULT_GRID,
                            arithmetic, static_cast<hipStream_t>(stream));
}

int dh_sdf_tangent_ex(int arithmetic, const float* packed, const float* pts, const float* d_normals, int64_t npts, float* ws,
                      void* stream) {
    if (npts <= 0 || bad_arith(arithmetic)) return DH_ERR_BAD_ARG;
    if (!packed || !pts || !d_normals || !ws || misaligned16(packed) || misaligned16(ws)) return DH_ERR_BAD_ARG;
    const Workspace w = carve_workspace(ws, npts);
    return launch_sdf_tangent(packed, pts, d_normals, npts, w.act, w.asave, w.t0aux, w.tsave, w.rsave, w.tpart, w.absmax, DEFAULT_GRID,
                              arithmetic, static_cast<hipStream_t>(stream));
}

int dh_sdf_backward_ex(int arithmetic, const float* packed, const float* d_sdf, int64_t npts, float* ws, void* stream) {
    if (npts <= 0 || bad_arith(arithmetic)) return DH_ERR_BAD_ARG;
    if (!packed || !d_sdf || !ws || misaligned16(packed) || misaligned16(ws)) return DH_ERR_BAD_ARG;
    const Workspace w = carve_workspace(ws, npts);
    return launch_sdf_bwd(packed, d_sdf, npts, w.act, w.rsave, w.featbar, w.zbar, w.tpart, w.absmax, DEFAULT_GRID, arithmetic,
                          static_cast<hipStream_t>(stream));
}

int dh_color_backward_rays_ex(int arithmetic, const float* packed, const float* colors, const float* d_colors, const float* dirs,
                              int n_per_ray, int64_t npts, float* ws, float* d_normals, float* d_pts, float* d_dirs_pts, void* stream) {
    if (npts <= 0 || n_per_ray <= 0 || bad_arith(arithmetic)) return DH_ERR_BAD_ARG;
    if (!packed || !colors || !d_colors || !dirs || !ws || !d_normals || !d_pts || !d_dirs_pts || misaligned16(packed) || misaligned16(ws))
        return DH_ERR_BAD_ARG;
    const Workspace w = carve_workspace(ws, npts);
    return launch_color_bwd_rays(packed, colors, d_colors, dirs, n_per_ray, npts, w.cact, w.czbar, w.featbar, d_normals, w.tpart,
                                 d_pts, d_dirs_pts, w.absmax, DEFAULT_GRID, arithmetic, static_cast<hipStream_t>(stream));
}

int dh_sdf_backward_rays_ex(int arithmetic, const float* packed, const float* d_sdf, const float* pts, const float* d_normals,
                            int64_t npts, float* ws, float* d_pts, void* stream) {
    if (npts <= 0 || bad_arith(arithmetic)) return DH_ERR_BAD_ARG;
    if (!packed || !d_sdf || !pts || !d_normals || !ws || !d_pts || misaligned16(packed) || misaligned16(ws)) return DH_ERR_BAD_ARG;
    const Workspace w = carve_workspace(ws, npts);
    return launch_sdf_bwd_rays(packed, d_sdf, pts, d_normals, npts, w.act, w.rsave, w.featbar, w.gesave, w.zbar, w.tpart, d_pts,
                               w.absmax, DEFAULT_GRID, arithmetic, static_cast<hipStream_t>(stream));
}

int dh_weight_grads_gemm_ex(int arithmetic, int64_t npts, float* ws, void* stream) {
    if (npts <= 0 || bad_arith(arithmetic)) return DH_ERR_BAD_ARG;
    if (!ws || misaligned16(ws)) return DH_ERR_BAD_ARG;
    const Workspace w = carve_workspace(ws, npts);
    return launch_weight_grads_gemm(w, w.slabs, w.tred, DW_G, DW_NS, arithmetic, static_cast<hipStream_t>(stream));
}

int dh_weight_grads_fold(const float* packed, const float* params, int64_t npts, float* ws, float* grad_flat, void* stream) {
    if (npts <= 0) return DH_ERR_BAD_ARG;
    if (!packed || !params || !ws || !grad_flat || misaligned16(packed) || misaligned16(ws)) return DH_ERR_BAD_ARG;
    const Workspace w = carve_workspace(ws, npts);
    return launch_weight_grads_fold(w, w.slabs, w.tred, DW_G, DW_NS, params, packed, grad_flat, static_cast<hipStream_t>(stream));
}

int dh_mlp_backward_ex(int arithmetic, const float* packed, const float* params, const float* pts, int64_t npts, float* ws,
                       const float* colors, const float* d_sdf, float* d_normals, const float* d_colors, float* grad_flat,
                       void* stream) {
    int rc = dh_color_backward_ex(arithmetic, packed, colors, d_colors, npts, ws, d_normals, stream);
    if (rc) return rc;
    rc = dh_sdf_tangent_ex(arithmetic, packed, pts, d_normals, npts, ws, stream);
    if (rc) return rc;
    rc = dh_sdf_backward_ex(arithmetic, packed, d_sdf, npts, ws, stream);
    if (rc) return rc;
    rc = dh_weight_grads_gemm_ex(arithmetic, npts, ws, stream);
    if (rc) return rc;
    return dh_weight_grads_fold(packed, params, npts, ws, grad_flat, stream);
}

// the entry points without an arithmetic argument: the process default (dh_set_arithmetic)
int dh_sdf_nograd(const float* packed, const float* pts, int64_t npts, float* sdf, void* stream) {
    return dh_sdf_nograd_ex(cur_arith(), packed, pts, npts, sdf, stream);
}
int dh_sdf_forward(const float* packed, const float* pts, int64_t npts, float* ws, float* sdf, void* stream) {
    return dh_sdf_forward_ex(cur_arith(), packed, pts, npts, ws, sdf, stream);
}
int dh_sdf_gradient(const float* packed, const float* pts, int64_t npts, float* ws, float* normals, int save, void* stream) {
    return dh_sdf_gradient_ex(cur_arith(), packed, pts, npts, ws, normals, save, stream);
}
int dh_color_forward(const float* packed, const float* pts, const float* dirs, int n_per_ray, const float* normals,
                     int64_t npts, float* ws, float* color, int save, void* stream) {
    return dh_color_forward_ex(cur_arith(), packed, pts, dirs, n_per_ray, normals, npts, ws, color, save, stream);
}
int dh_mlp_forward(const float* packed, const float* pts, const float* dirs, int n_per_ray, int64_t npts, float* ws,
                   float* sdf, float* normals, float* color, void* stream) {
    return dh_mlp_forward_ex(cur_arith(), packed, pts, dirs, n_per_ray, npts, ws, sdf, normals, color, stream);
}
int dh_color_backward(const float* packed, const float* colors, const float* d_colors, int64_t npts, float* ws,
                      float* d_normals, void* stream) {
    return dh_color_backward_ex(cur_arith(), packed, colors, d_colors, npts, ws, d_normals, stream);
}
int dh_sdf_tangent(const float* packed, const float* pts, const float* d_normals, int64_t npts, float* ws, void* stream) {
    return dh_sdf_tangent_ex(cur_arith(), packed, pts, d_normals, npts, ws, stream);
}
int dh_sdf_backward(const float* packed, const float* d_sdf, int64_t npts, float* ws, void* stream) {
    return dh_sdf_backward_ex(cur_arith(), packed, d_sdf, npts, ws, stream);
}
int dh_color_backward_rays(const float* packed, const float* colors, const float* d_colors, const float* dirs, int n_per_ray,
                           int64_t npts, float* ws, float* d_normals, float* d_pts, float* d_dirs_pts, void* stream) {
    return dh_color_backward_rays_ex(cur_arith(), packed, colors, d_colors, dirs, n_per_ray, npts, ws, d_normals, d_pts, d_dirs_pts, stream);
}
int dh_sdf_backward_rays(const float* packed, const float* d_sdf, const float* pts, const float* d_normals, int64_t npts,
                         float* ws, float* d_pts, void* stream) {
    return dh_sdf_backward_rays_ex(cur_arith(), packed, d_sdf, pts, d_normals, npts, ws, d_pts, stream);
}
int dh_weight_grads_gemm(int64_t npts, float* ws, void* stream) { return dh_weight_grads_gemm_ex(cur_arith(), npts, ws, stream); }
int dh_mlp_backward(const float* packed, const float* params, const float* pts, int64_t npts, float* ws,
                    const float* colors, const float* d_sdf, float* d_normals, const float* d_colors, float* grad_flat,
                    void* stream) {
    return dh_mlp_backward_ex(cur_arith(), packed, params, pts, npts, ws, colors, d_sdf, d_normals, d_colors, grad_flat, stream);
}

int dh_gen_rays(const uint8_t* rgb, const int8_t* label, const uint8_t* normal, const float* R, const float* T,
                const float* Kinv, int H, int W, int n_frames, int frame, const int64_t* px, const int64_t* py, int64_t B,
                float* rays, float* near, float* far, void* stream) {
    if (B < 0 || H <= 0 || W <= 0 || frame < 0 || frame >= n_frames) return DH_ERR_BAD_ARG;
    if (B == 0) return DH_OK;
    if (!rgb || !label || !normal || !R || !T || !Kinv || !px || !py || !rays || !near || !far) return DH_ERR_BAD_ARG;
    return launch_gen_rays(rgb, label, normal, R, T, Kinv, H, W, frame, px, py, B, rays, near, far, static_cast<hipStream_t>(stream));
}

int dh_coarse_samples(const float* rays_o, const float* rays_d, const float* near, const float* far, const float* t_rand,
                      int64_t B, int n_samples, float* z, float* pts, void* stream) {
    if (B < 0 || n_samples <= 0) return DH_ERR_BAD_ARG;
    if (B == 0) return DH_OK;
    if (!rays_o || !rays_d || !near || !far || !z || !pts) return DH_ERR_BAD_ARG;
    return launch_coarse_samples(rays_o, rays_d, near, far, t_rand, B, n_samples, z, pts, static_cast<hipStream_t>(stream));
}

int dh_upsample_step(const float* rays_o, const float* rays_d, const float* z, const float* sdf, int64_t B, int n_cur,
                     int n_new, float inv_s, float* z_new, float* pts_new, void* stream) {
    if (B < 0 || n_cur < 2 || n_new <= 0) return DH_ERR_BAD_ARG;
    if (n_cur > 128 || n_new > 64) return DH_ERR_UNSUPPORTED;
    if (B == 0) return DH_OK;
    if (!rays_o || !rays_d || !z || !sdf || !z_new || !pts_new) return DH_ERR_BAD_ARG;
    return launch_upsample(rays_o, rays_d, z, sdf, B, n_cur, n_new, inv_s, z_new, pts_new, static_cast<hipStream_t>(stream));
}

int dh_merge_samples(const float* z, const float* z_new, const float* sdf, const float* sdf_new, int64_t B, int n_cur,
                     int n_new, float* z_out, float* sdf_out, void* stream) {
    if (B < 0 || n_cur <= 0 || n_new <= 0) return DH_ERR_BAD_ARG;
    if (n_cur > 128 || n_new > 64) return DH_ERR_UNSUPPORTED;
    if (B == 0) return DH_OK;
    if (!z || !z_new || !z_out) return DH_ERR_BAD_ARG;
    if (sdf_out && (!sdf || !sdf_new)) return DH_ERR_BAD_ARG;
    return launch_merge(z, z_new, sdf, sdf_new, B, n_cur, n_new, z_out, sdf_out, static_cast<hipStream_t>(stream));
}

int dh_midpoints(const float* rays_o, const float* rays_d, const float* z, int64_t B, int n, float sample_dist, float* pts,
                 void* stream) {
    if (B < 0 || n <= 0) return DH_ERR_BAD_ARG;
    if (B == 0) return DH_OK;
    if (!rays_o || !rays_d || !z || !pts) return DH_ERR_BAD_ARG;
    return launch_midpoints(rays_o, rays_d, z, B, n, sample_dist, pts, static_cast<hipStream_t>(stream));
}

int dh_render_scan_fwd(const float* rays_o, const float* rays_d, const float* z, const float* sdf, const float* normals,
                       const float* colors, const float* inv_s, float cos_anneal_ratio, float sample_dist,
                       const float* background_rgb, int64_t B, int n, float* weights, float* color, float* weight_sum,
                       float* weight_max, float* cdf, float* inside_sphere, float* eik_partial, float* normal_map,
                       void* stream) {
    if (B < 0 || n <= 0) return DH_ERR_BAD_ARG;
    if (n > 128) return DH_ERR_UNSUPPORTED;
    if (B == 0) return DH_OK;
    if (!rays_o || !rays_d || !z || !sdf || !normals || !colors || !inv_s || !weights || !color || !weight_sum ||
        !weight_max || !cdf || !inside_sphere || !eik_partial) return DH_ERR_BAD_ARG;
    return launch_render_fwd(rays_o, rays_d, z, sdf, normals, colors, inv_s, cos_anneal_ratio, sample_dist, background_rgb,
                             B, n, weights, color, weight_sum, weight_max, cdf, inside_sphere, eik_partial, normal_map,
                             nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int dh_render_scan_bwd(const float* rays_o, const float* rays_d, const float* z, const float* sdf, const float* normals,
                       const float* colors, const float* inv_s, float cos_anneal_ratio, float sample_dist,
                       const float* background_rgb, int64_t B, int n, const float* d_color, const float* d_weight_sum,
                       const float* d_weights, const float* d_gradients, const float* d_normal_map, const float* eik_coef,
                       float* d_sdf, float* d_normals, float* d_colors, float* d_inv_s, void* stream) {
    if (B < 0 || n <= 0) return DH_ERR_BAD_ARG;
    if (n > 128) return DH_ERR_UNSUPPORTED;
    if (B == 0) return DH_OK;
    if (!rays_o || !rays_d || !z || !sdf || !normals || !colors || !inv_s || !d_color || !eik_coef || !d_sdf ||
        !d_normals || !d_colors || !d_inv_s) return DH_ERR_BAD_ARG;
    return launch_render_bwd(rays_o, rays_d, z, sdf, normals, colors, inv_s, cos_anneal_ratio, sample_dist, background_rgb,
                             B, n, d_color, d_weight_sum, d_weights, d_gradients, d_normal_map, eik_coef, d_sdf, d_normals, d_colors,
                             d_inv_s, nullptr, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int dh_render_scan_bwd_rays(const float* rays_o, const float* rays_d, const float* z, const float* sdf, const float* normals,
                            const float* colors, const float* inv_s, float cos_anneal_ratio, float sample_dist,
                            const float* background_rgb, int64_t B, int n, const float* d_color, const float* d_weight_sum,
                            const float* d_weights, const float* d_gradients, const float* d_normal_map, const float* eik_coef,
                            float* d_sdf, float* d_normals, float* d_colors, float* d_inv_s, float* d_rays_d, void* stream) {
    if (B < 0 || n <= 0) return DH_ERR_BAD_ARG;
    if (n > 128) return DH_ERR_UNSUPPORTED;
    if (B == 0) return DH_OK;
    if (!rays_o || !rays_d || !z || !sdf || !normals || !colors || !inv_s || !d_color || !eik_coef || !d_sdf ||
        !d_normals || !d_colors || !d_inv_s || !d_rays_d) return DH_ERR_BAD_ARG;
    return launch_render_bwd(rays_o, rays_d, z, sdf, normals, colors, inv_s, cos_anneal_ratio, sample_dist, background_rgb,
                             B, n, d_color, d_weight_sum, d_weights, d_gradients, d_normal_map, eik_coef, d_sdf, d_normals, d_colors,
                             d_inv_s, d_rays_d, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int dh_march_count(const float* rays_o, const float* rays_d, const float* near, const float* far, const float* u,
                   const uint8_t* occupancy, int res, float radius, float step, float half_step, int max_samples, int64_t B,
                   int32_t* cnt, void* stream) {
    if (B < 0 || res <= 0 || !(radius > 0.f) || !(step > 0.f) || max_samples <= 0) return DH_ERR_BAD_ARG;
    if (max_samples > 1024) return DH_ERR_UNSUPPORTED;
    if (B == 0) return DH_OK;
    if (!rays_o || !rays_d || !near || !far || !occupancy || !cnt) return DH_ERR_BAD_ARG;
    return launch_march_count(rays_o, rays_d, near, far, u, occupancy, res, radius, step, half_step, max_samples, B, cnt,
                              static_cast<hipStream_t>(stream));
}

int dh_march_emit(const float* rays_o, const float* rays_d, const float* near, const float* far, const float* u,
                  const uint8_t* occupancy, int res, float radius, float step, float half_step, int max_samples, int64_t B,
                  const int64_t* off, const int32_t* keep, float* t_start, float* pts, float* dirs_pts, int32_t* ray_idx,
                  void* stream) {
    if (B < 0 || res <= 0 || !(radius > 0.f) || !(step > 0.f) || max_samples <= 0) return DH_ERR_BAD_ARG;
    if (max_samples > 1024) return DH_ERR_UNSUPPORTED;
    if (B == 0) return DH_OK;
    if (!rays_o || !rays_d || !near || !far || !occupancy || !off || !t_start || !pts || !dirs_pts || !ray_idx) return DH_ERR_BAD_ARG;
    return launch_march_emit(rays_o, rays_d, near, far, u, occupancy, res, radius, step, half_step, max_samples, B, off, keep,
                             t_start, pts, dirs_pts, ray_idx, static_cast<hipStream_t>(stream));
}

int dh_render_scan_fwd_packed(const float* rays_o, const float* rays_d, const float* t_start, const float* sdf, const float* normals,
                              const float* colors, const float* inv_s, float cos_anneal_ratio, float step,
                              const float* background_rgb, int64_t B, const int64_t* seg_off, const int32_t* seg_cnt,
                              float* weights, float* color, float* weight_sum, float* weight_max, float* cdf,
                              float* inside_sphere, float* eik_partial, float* normal_map, void* stream) {
    if (B < 0) return DH_ERR_BAD_ARG;
    if (B == 0) return DH_OK;
    if (!rays_o || !rays_d || !t_start || !sdf || !normals || !colors || !inv_s || !seg_off || !seg_cnt || !weights || !color ||
        !weight_sum || !weight_max || !cdf || !inside_sphere || !eik_partial) return DH_ERR_BAD_ARG;
    return launch_render_fwd(rays_o, rays_d, t_start, sdf, normals, colors, inv_s, cos_anneal_ratio, step, background_rgb, B, 0,
                             weights, color, weight_sum, weight_max, cdf, inside_sphere, eik_partial, normal_map, seg_off, seg_cnt,
                             static_cast<hipStream_t>(stream));
}

int dh_render_scan_bwd_packed(const float* rays_o, const float* rays_d, const float* t_start, const float* sdf, const float* normals,
                              const float* colors, const float* inv_s, float cos_anneal_ratio, float step,
                              const float* background_rgb, int64_t B, const int64_t* seg_off, const int32_t* seg_cnt,
                              const float* d_color, const float* d_weight_sum, const float* d_weights, const float* d_gradients,
                              const float* d_normal_map, const float* eik_coef, float* d_sdf, float* d_normals, float* d_colors,
                              float* d_inv_s, void* stream) {
    if (B < 0) return DH_ERR_BAD_ARG;
    if (B == 0) return DH_OK;
    if (!rays_o || !rays_d || !t_start || !sdf || !normals || !colors || !inv_s || !seg_off || !seg_cnt || !d_color || !eik_coef ||
        !d_sdf || !d_normals || !d_colors || !d_inv_s) return DH_ERR_BAD_ARG;
    return launch_render_bwd(rays_o, rays_d, t_start, sdf, normals, colors, inv_s, cos_anneal_ratio, step, background_rgb, B, 0,
                             d_color, d_weight_sum, d_weights, d_gradients, d_normal_map, eik_coef, d_sdf, d_normals, d_colors,
                             d_inv_s, nullptr, seg_off, seg_cnt, static_cast<hipStream_t>(stream));
}

int dh_render_scan_bwd_packed_rays(const float* rays_o, const float* rays_d, const float* t_start, const float* sdf, const float* normals,
                                   const float* colors, const float* inv_s, float cos_anneal_ratio, float step,
                                   const float* background_rgb, int64_t B, const int64_t* seg_off, const int32_t* seg_cnt,
                                   const float* d_color, const float* d_weight_sum, const float* d_weights, const float* d_gradients,
                                   const float* d_normal_map, const float* eik_coef, float* d_sdf, float* d_normals, float* d_colors,
                                   float* d_inv_s, float* d_rays_d, void* stream) {
    if (B < 0) return DH_ERR_BAD_ARG;
    if (B == 0) return DH_OK;
    if (!rays_o || !rays_d || !t_start || !sdf || !normals || !colors || !inv_s || !seg_off || !seg_cnt || !d_color || !eik_coef ||
        !d_sdf || !d_normals || !d_colors || !d_inv_s || !d_rays_d) return DH_ERR_BAD_ARG;
    return launch_render_bwd(rays_o, rays_d, t_start, sdf, normals, colors, inv_s, cos_anneal_ratio, step, background_rgb, B, 0,
                             d_color, d_weight_sum, d_weights, d_gradients, d_normal_map, eik_coef, d_sdf, d_normals, d_colors,
                             d_inv_s, d_rays_d, seg_off, seg_cnt, static_cast<hipStream_t>(stream));
}

int dh_ray_adjoint_packed(const float* d_pts, const float* d_dirs_pts, const float* t_start, float step, const int64_t* seg_off,
                          const int32_t* seg_cnt, int64_t B, float* d_rays_o, float* d_rays_d_accum, void* stream) {
    if (B < 0) return DH_ERR_BAD_ARG;
    if (B == 0) return DH_OK;
    if (!d_pts || !d_dirs_pts || !t_start || !seg_off || !seg_cnt || !d_rays_o || !d_rays_d_accum) return DH_ERR_BAD_ARG;
    return launch_ray_adjoint_packed(d_pts, d_dirs_pts, t_start, step, seg_off, seg_cnt, B, d_rays_o, d_rays_d_accum,
                                     static_cast<hipStream_t>(stream));
}

int dh_adam_step(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                 float beta2, float eps, int64_t step, float grad_scale, void* stream) {
    if (n < 0 || step < 1) return DH_ERR_BAD_ARG;
    if (n == 0) return DH_OK;
    if (!params || !grad || !exp_avg || !exp_avg_sq) return DH_ERR_BAD_ARG;
    return launch_adam(params, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, grad_scale,
                       static_cast<hipStream_t>(stream));
}

int dh_neus_loss(const float* color, const float* weight_sum, const float* normal_map, const float* eik_partial,
                 const float* rays, const float* R, int64_t B, float igr_weight, float mask_weight, float normal_weight,
                 float* stats, float* d_color, float* d_weight_sum, float* d_normal_map, float* eik_coef, void* stream) {
    if (B <= 0) return DH_ERR_BAD_ARG;
    if (!color || !weight_sum || !eik_partial || !rays || !stats || !d_color || !d_weight_sum || !eik_coef)
        return DH_ERR_BAD_ARG;
    if (normal_weight > 0.f && (!normal_map || !R || !d_normal_map)) return DH_ERR_BAD_ARG;
    return launch_loss(color, weight_sum, normal_map, eik_partial, rays, R, B, igr_weight, mask_weight, normal_weight, stats,
                       d_color, d_weight_sum, d_normal_map, eik_coef, static_cast<hipStream_t>(stream));
}

int dh_corr_loss(const float* rays_o, const float* rays_d, const float* z, const float* weights, const float* corr,
                 const float* R_all, const float* T_all, int n_frames, const float* K, int64_t B, int n, float sample_dist,
                 float delta_px, float corr_weight, float* stats, float* residual_px, float* d_weights, float* pose_adjoints,
                 void* stream) {
    if (B <= 0 || n <= 0 || n_frames <= 0 || !(delta_px > 0.f)) return DH_ERR_BAD_ARG;
    if (!rays_o || !rays_d || !z || !weights || !corr || !R_all || !T_all || !K || !stats || !residual_px || !d_weights)
        return DH_ERR_BAD_ARG;
    return launch_corr_loss(rays_o, rays_d, z, weights, corr, R_all, T_all, n_frames, K, B, n, sample_dist, delta_px, corr_weight,
                            stats, residual_px, d_weights, pose_adjoints, static_cast<hipStream_t>(stream));
}

int64_t dh_prior_loss_workspace(int64_t B) {
    if (B < 0) return DH_ERR_BAD_ARG;
    return prior_loss_workspace(B);
}

namespace {
// the checks the two forms of dh_prior_loss share; DH_OK + *run = false for the no-op
int prior_args(const float* rays, const float* R, const float* samples, const float* weights, const float* prior, int64_t B,
               float depth_weight, float depth_delta, float normal_weight, const float* stats, const float* d_weights, const void* ws,
               bool* run) {
    *run = false;
    if (B < 0 || !(depth_delta > 0.f) || !(depth_weight >= 0.f) || !(normal_weight >= 0.f)) return DH_ERR_BAD_ARG;   // NaN fails too
    if (B == 0) return DH_OK;
    if (!rays || !R || !stats || !ws || misaligned16(ws)) return DH_ERR_BAD_ARG;
    if (prior && (!samples || !weights || !d_weights)) return DH_ERR_BAD_ARG;
    *run = true;
    return DH_OK;
}
}  // namespace

int dh_prior_loss(const float* rays, const float* R, const float* z, const float* weights, const float* normal_map,
                  const float* prior_depth, int64_t B, int n, float sample_dist, float depth_weight, float depth_delta,
                  float normal_weight, int accumulate, float* stats, float* d_weights, float* d_normal_map, void* ws, void* stream) {
    if (n < 1) return DH_ERR_BAD_ARG;
    bool run;
    const int rc = prior_args(rays, R, z, weights, prior_depth, B, depth_weight, depth_delta, normal_weight, stats, d_weights, ws, &run);
    if (rc != DH_OK || !run) return rc;
    return launch_prior_loss(rays, R, z, weights, normal_map, prior_depth, B, n, nullptr, nullptr, n, sample_dist, depth_weight,
                             depth_delta, normal_weight, accumulate, stats, d_weights, d_normal_map, ws,
                             static_cast<hipStream_t>(stream));
}

int dh_prior_loss_packed(const float* rays, const float* R, const float* t_start, const float* weights, const float* normal_map,
                         const float* prior_depth, int64_t B, const int64_t* seg_off, const int32_t* seg_cnt, int max_samples,
                         float step, float depth_weight, float depth_delta, float normal_weight, int accumulate, float* stats,
                         float* d_weights, float* d_normal_map, void* ws, void* stream) {
    if (max_samples < 0) return DH_ERR_BAD_ARG;
    if (max_samples > 1024) return DH_ERR_UNSUPPORTED;
    bool run;
    const int rc = prior_args(rays, R, t_start, weights, prior_depth, B, depth_weight, depth_delta, normal_weight, stats, d_weights, ws,
                              &run);
    if (rc != DH_OK || !run) return rc;
    if (!seg_off || !seg_cnt) return DH_ERR_BAD_ARG;
    return launch_prior_loss(rays, R, t_start, weights, normal_map, prior_depth, B, 0, seg_off, seg_cnt, max_samples, step, depth_weight,
                             depth_delta, normal_weight, accumulate, stats, d_weights, d_normal_map, ws,
                             static_cast<hipStream_t>(stream));
}

int64_t dh_hashgrid_entries(void) { return hashgrid_entries(); }

int dh_hashgrid_level(int level, float* scale, uint32_t* resolution, uint32_t* offset, uint32_t* dense) {
    if (!scale || !resolution || !offset || !dense) return DH_ERR_BAD_ARG;
    return hashgrid_level(level, scale, resolution, offset, dense) ? DH_ERR_BAD_ARG : DH_OK;
}

int dh_hashgrid_encode(const float* table, const float* x01, int64_t n, float* out, void* stream) {
    if (n < 0) return DH_ERR_BAD_ARG;
    if (n == 0) return DH_OK;
    if (!table || !x01 || !out || (reinterpret_cast<uintptr_t>(table) & 7u) || (reinterpret_cast<uintptr_t>(out) & 7u))
        return DH_ERR_BAD_ARG;
    return launch_hashgrid_fwd(table, x01, n, out, static_cast<hipStream_t>(stream));
}

int dh_hashgrid_encode_backward(const float* x01, const float* d_out, int64_t n, float* d_table, void* stream) {
    if (n < 0) return DH_ERR_BAD_ARG;
    if (n == 0) return DH_OK;
    if (!x01 || !d_out || !d_table || (reinterpret_cast<uintptr_t>(d_out) & 7u)) return DH_ERR_BAD_ARG;
    return launch_hashgrid_bwd(x01, d_out, n, d_table, static_cast<hipStream_t>(stream));
}

int64_t dh_hash_num_params(void) { return hash_num_params(); }
int64_t dh_hash_packed_floats(void) { return HP_TOTAL; }

int dh_hash_param_layout(int net, int layer, int64_t* bias_off, int64_t* g_off, int64_t* v_off, int* out_dim, int* in_dim) {
    if (!bias_off || !g_off || !v_off || !out_dim || !in_dim) return DH_ERR_BAD_ARG;
    const HashParamOff P = make_hash_param_off(hashgrid_entries());
    if (net == 0 && layer == 0) { *bias_off = P.g0_b; *g_off = P.g0_g; *v_off = P.g0_v; *out_dim = 64; *in_dim = HM_GIN; }
    else if (net == 0 && layer == 1) { *bias_off = P.g1_b; *g_off = P.g1_g; *v_off = P.g1_v; *out_dim = HM_GOUT; *in_dim = 64; }
    else if (net == 1 && layer == 0) { *bias_off = *g_off = *v_off = P.variance; *out_dim = 1; *in_dim = 1; }
    else if (net == 2 && layer == 0) { *bias_off = P.c0_b; *g_off = P.c0_g; *v_off = P.c0_v; *out_dim = 64; *in_dim = HM_CIN; }
    else if (net == 2 && layer == 1) { *bias_off = P.c1_b; *g_off = P.c1_g; *v_off = P.c1_v; *out_dim = 64; *in_dim = 64; }
    else if (net == 2 && layer == 2) { *bias_off = P.c2_b; *g_off = P.c2_g; *v_off = P.c2_v; *out_dim = 3; *in_dim = 64; }
    else if (net == 3 && layer == 0) { *bias_off = *g_off = *v_off = P.table; *out_dim = (int)hashgrid_entries(); *in_dim = 2; }
    else return DH_ERR_BAD_ARG;
    return DH_OK;
}

int dh_hash_pack_weights(const float* params, float* packed, void* stream) {
    if (!params || !packed) return DH_ERR_BAD_ARG;
    return launch_hash_pack(params, packed, static_cast<hipStream_t>(stream));
}

int dh_hash_workspace_floats(int64_t npts, int64_t* infer_floats, int64_t* total_floats) {
    if (npts < 0 || !infer_floats || !total_floats) return DH_ERR_BAD_ARG;
    *infer_floats = hash_infer_workspace_floats(npts);
    *total_floats = hash_workspace_floats(npts);
    return DH_OK;
}

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int dh_hash_sdf_nograd(const float* params, const float* packed, const float* pts, int64_t n, float radius, float* sdf,
                       void* stream) {
    if (n < 0 || !(radius > 0.f)) return DH_ERR_BAD_ARG;
    if (n == 0) return DH_OK;
    if (!params || !packed || !pts || !sdf || !al16(params) || !al16(packed)) return DH_ERR_BAD_ARG;
    return launch_hash_sdf_nograd(params, packed, pts, n, radius, sdf, static_cast<hipStream_t>(stream));
}

int dh_hash_geo_forward(const float* params, const float* packed, const float* pts, int64_t n, float radius, float eps,
                        float* ws, int save, float* sdf, float* feature, float* gradient, const int64_t* n_active, void* stream) {
    if (n < 0 || !(radius > 0.f) || !(eps > 0.f) || (n_active && n % 8)) return DH_ERR_BAD_ARG;
    if (n == 0) return DH_OK;
    if (!params || !packed || !pts || !ws || !sdf || !feature || !gradient || !al16(params) || !al16(packed) || !al16(ws))
        return DH_ERR_BAD_ARG;
    return launch_hash_geo_fwd(params, packed, pts, n, radius, eps, ws, save, sdf, feature, gradient, n_active,
                               static_cast<hipStream_t>(stream));
}

int dh_hash_color_forward(const float* packed, const float* feature, const float* normals, const float* dirs,
                          int n_per_ray, int64_t n, float* color, const int64_t* n_active, void* stream) {
    if (n < 0 || n_per_ray <= 0 || n % n_per_ray) return DH_ERR_BAD_ARG;
    if (n == 0) return DH_OK;
    if (!packed || !feature || !normals || !dirs || !color || !al16(packed)) return DH_ERR_BAD_ARG;
    return launch_sh_color_fwd(packed, feature, normals, dirs, n_per_ray, n, color, n_active, static_cast<hipStream_t>(stream));
}

int dh_hash_color_backward(const float* packed, const float* feature, const float* normals, const float* dirs,
                           const float* d_color, int n_per_ray, int64_t n, float* ws, float* d_feature, float* d_normals,
                           const int64_t* n_active, void* stream) {
    if (n <= 0 || n_per_ray <= 0 || n % n_per_ray || (n_active && n % 8)) return DH_ERR_BAD_ARG;
    if (!packed || !feature || !normals || !dirs || !d_color || !ws || !d_feature || !d_normals || !al16(packed) || !al16(ws))
        return DH_ERR_BAD_ARG;
    return launch_sh_color_bwd(packed, feature, normals, dirs, d_color, n_per_ray, n, ws, d_feature, d_normals, nullptr, n_active,
                               static_cast<hipStream_t>(stream));
}

int dh_hash_color_backward_rays(const float* packed, const float* feature, const float* normals, const float* dirs,
                                const float* d_color, int n_per_ray, int64_t n, float* ws, float* d_feature, float* d_normals,
                                const int64_t* n_active, float* d_dirs_pts, void* stream) {
    if (n <= 0 || n_per_ray <= 0 || n % n_per_ray || (n_active && n % 8)) return DH_ERR_BAD_ARG;
    if (!packed || !feature || !normals || !dirs || !d_color || !ws || !d_feature || !d_normals || !d_dirs_pts || !al16(packed) ||
        !al16(ws)) return DH_ERR_BAD_ARG;
    return launch_sh_color_bwd(packed, feature, normals, dirs, d_color, n_per_ray, n, ws, d_feature, d_normals, d_dirs_pts, n_active,
                               static_cast<hipStream_t>(stream));
}

int dh_hash_geo_backward(const float* params, const float* packed, const float* pts, const float* d_sdf,
                         const float* d_feature, const float* d_normals, int64_t n, float radius, float eps, float* ws,
                         const int64_t* n_active, void* stream) {
    if (n <= 0 || !(radius > 0.f) || !(eps > 0.f) || (n_active && n % 8)) return DH_ERR_BAD_ARG;
    if (!params || !packed || !pts || !d_sdf || !d_feature || !d_normals || !ws || !al16(params) || !al16(packed) || !al16(ws))
        return DH_ERR_BAD_ARG;
    return launch_hash_geo_bwd(params, packed, pts, d_sdf, d_feature, d_normals, n, radius, eps, ws, nullptr, n_active,
                               static_cast<hipStream_t>(stream));
}

int dh_hash_geo_backward_rays(const float* params, const float* packed, const float* pts, const float* d_sdf,
                              const float* d_feature, const float* d_normals, int64_t n, float radius, float eps, float* ws,
                              const int64_t* n_active, float* d_pts, void* stream) {
    if (n <= 0 || !(radius > 0.f) || !(eps > 0.f) || (n_active && n % 8)) return DH_ERR_BAD_ARG;
    if (!params || !packed || !pts || !d_sdf || !d_feature || !d_normals || !ws || !d_pts || !al16(params) || !al16(packed) ||
        !al16(ws)) return DH_ERR_BAD_ARG;
    return launch_hash_geo_bwd(params, packed, pts, d_sdf, d_feature, d_normals, n, radius, eps, ws, d_pts, n_active,
                               static_cast<hipStream_t>(stream));
}

int dh_hash_weight_grads(const float* params, const float* packed, int64_t n, float* ws, float* grad, const int64_t* n_active,
                         void* stream) {
    if (n <= 0 || !params || !packed || !ws || !grad || !al16(ws) || (n_active && n % 8)) return DH_ERR_BAD_ARG;
    if (hash_scatter_mode() != 0) return DH_ERR_BAD_ARG;        // the merge ablations exist for the float-atomic form only (header)
    return launch_hash_weight_grads(params, packed, n, ws, grad, n_active, 7, static_cast<hipStream_t>(stream));
}

int dh_hash_weight_grads_parts(const float* params, const float* packed, int64_t n, float* ws, float* grad, const int64_t* n_active,
                               int parts, void* stream) {
    if (n <= 0 || !params || !packed || !ws || !grad || !al16(ws) || (n_active && n % 8) || parts < 1 || parts > 7 || parts == 4 || parts == 6) return DH_ERR_BAD_ARG;
    if ((parts & 4) && hash_scatter_mode() != 0) return DH_ERR_BAD_ARG;      // (as above)
    return launch_hash_weight_grads(params, packed, n, ws, grad, n_active, parts, static_cast<hipStream_t>(stream));
}

int64_t dh_nearest_sqdist_workspace(int64_t nq, int64_t nr) {
    if (nq < 0 || nr < 0) return DH_ERR_BAD_ARG;
    return nearest_sqdist_workspace(nq, nr);
}

int dh_nearest_sqdist(const float* q, int64_t nq, const float* ref, int64_t nr, float* d2, int32_t* idx, void* ws, void* stream) {
    if (nq < 0 || nr < 0) return DH_ERR_BAD_ARG;
    if (nr >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;               // indices are int32
    if (nq == 0) return DH_OK;
    if (!q || !ref || !d2 || nr == 0 || misaligned16(ws)) return DH_ERR_BAD_ARG;
    if (nq > ((int64_t)1 << 40)) return DH_ERR_UNSUPPORTED;                // grid.x = nq / 2048 must fit 2^31
    return launch_nearest_sqdist(q, nq, ref, nr, d2, idx, ws, static_cast<hipStream_t>(stream));
}

int dh_mesh_sdf_record_floats(void) { return mesh_sdf_record_floats(); }

int dh_mesh_sdf_prepare(const float* verts, int64_t nv, const int32_t* faces, int64_t nf, float* rec, void* stream) {
    if (nv < 0 || nf < 0) return DH_ERR_BAD_ARG;
    if (nf >= ((int64_t)1 << 31) || nv >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;     // indices are int32
    if (nf == 0) return DH_OK;
    if (!faces || !rec || (!verts && nv > 0) || misaligned16(rec)) return DH_ERR_BAD_ARG;
    return launch_mesh_sdf_prepare(verts, nv, faces, nf, rec, static_cast<hipStream_t>(stream));
}

int64_t dh_mesh_sdf_query_workspace(int64_t n, int64_t nf) {
    if (n < 0 || nf < 0) return DH_ERR_BAD_ARG;
    if (nf >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;
    return mesh_sdf_query_workspace(n, nf);
}

int dh_mesh_sdf_query(const float* rec, int64_t nf, const float* pts, int64_t n, float* sqdist, int32_t* face, float* wind, void* ws,
                      void* stream) {
    if (n < 0 || nf < 0) return DH_ERR_BAD_ARG;
    if (nf >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;      // face indices are int32; grid.x
    if (n == 0) return DH_OK;
    if (nf == 0 || !rec || !pts || !sqdist || misaligned16(rec) || misaligned16(ws)) return DH_ERR_BAD_ARG;
    if (nf > mesh_sdf_max_faces()) return DH_ERR_UNSUPPORTED;                                 // one slab per grid.y index
    if (!ws && mesh_sdf_query_workspace(n, nf) > 0) return DH_ERR_BAD_ARG;                    // more than one slab needs the scratch
    return launch_mesh_sdf_query(rec, nf, pts, n, sqdist, face, wind, ws, static_cast<hipStream_t>(stream));
}

// shared limits of the ICP entry points: the grid's y / z dimensions carry slabs and hypotheses (65535 each), indices are int32
static int icp_args(int64_t n, int64_t m, int64_t h) {
    if (n < 0 || m < 0 || h < 0) return DH_ERR_BAD_ARG;
    if (m >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31) || h > 65535) return DH_ERR_UNSUPPORTED;
    return DH_OK;
}

int64_t dh_icp_correspond_workspace(int64_t n, int64_t m, int64_t h) {
    const int rc = icp_args(n, m, h);
    if (rc != DH_OK) return rc;
    return icp_correspond_workspace(n, m, h);
}

int dh_icp_correspond(const float* src, int64_t n, const float* tgt, int64_t m, const float* xf, int64_t h, float* d2, int32_t* idx,
                      void* ws, void* stream) {
    const int rc = icp_args(n, m, h);
    if (rc != DH_OK) return rc;
    if (n == 0 || h == 0) return DH_OK;
    if (!src || !tgt || !xf || !d2 || !idx || m == 0 || misaligned16(ws)) return DH_ERR_BAD_ARG;
    return launch_icp_correspond(src, n, tgt, m, xf, h, d2, idx, ws, static_cast<hipStream_t>(stream));
}

int dh_icp_moments_sums(int plane) { return icp_moments_sums(plane != 0); }

int64_t dh_icp_moments_workspace(int64_t n, int64_t h, int plane) {
    const int rc = icp_args(n, 0, h);
    if (rc != DH_OK) return rc;
    return icp_moments_workspace(n, h, plane != 0);
}

int dh_icp_moments(const float* src, const float* tgt, const float* tgt_normals, const float* xf, const int32_t* idx, const float* d2,
                   const float* thr, const float* origin_src, const float* origin_tgt, int64_t n, int64_t m, int64_t h, double* out,
                   void* ws, void* stream) {
    const int rc = icp_args(n, m, h);
    if (rc != DH_OK) return rc;
    if (h == 0) return DH_OK;
    // n == 0 still zeroes out (the sums of no pairs); every pointer is needed either way
    if (!src || !tgt || !xf || !idx || !d2 || !thr || !origin_src || !origin_tgt || !out || !ws || misaligned16(ws)) return DH_ERR_BAD_ARG;
    return launch_icp_moments(src, tgt, tgt_normals, xf, idx, d2, thr, origin_src, origin_tgt, n, m, h, out, ws,
                              static_cast<hipStream_t>(stream));
}

int dh_label_dilate(const int8_t* label, int64_t n_frames, int H, int W, int radius, uint8_t* tmp, uint8_t* keep, void* stream) {
    if (n_frames < 0 || H <= 0 || W <= 0 || radius < 0) return DH_ERR_BAD_ARG;
    if (n_frames == 0) return DH_OK;
    if (!label || !tmp || !keep) return DH_ERR_BAD_ARG;
    if (n_frames * H >= ((int64_t)1 << 31) || W > 65535 * 256) return DH_ERR_UNSUPPORTED;   // grid (rows, column blocks)
    const int r = radius < (H > W ? H : W) ? radius : (H > W ? H : W);                       // a wider window adds nothing
    return launch_label_dilate(label, n_frames, H, W, r, tmp, keep, static_cast<hipStream_t>(stream));
}

int dh_mesh_mask_votes(const float* verts, int64_t nv, const uint8_t* keep, const float* R, const float* T, const float* K,
                       int64_t n_frames, int H, int W, int32_t* bg_votes, int32_t* seen, void* stream) {
    if (nv < 0 || n_frames < 0 || H <= 0 || W <= 0) return DH_ERR_BAD_ARG;
    if (nv == 0) return DH_OK;
    if (!verts || !K || !bg_votes || !seen || (n_frames > 0 && (!keep || !R || !T))) return DH_ERR_BAD_ARG;
    if (nv >= ((int64_t)1 << 40)) return DH_ERR_UNSUPPORTED;
    return launch_mesh_mask_votes(verts, nv, keep, R, T, K, n_frames, H, W, bg_votes, seen, static_cast<hipStream_t>(stream));
}

int dh_hull_accumulate(const float* pts, int64_t n, const float* sd, const float* R, const float* T, const float* K, int64_t n_frames,
                       int H, int W, int frame0, int m, float* topk, int32_t* arg, int32_t* seen, void* stream) {
    if (n < 0 || n_frames < 0 || frame0 < 0 || H < 2 || W < 2 || m < 1 || m > 8) return DH_ERR_BAD_ARG;
    if (H > (1 << 24) || W > (1 << 24) || n >= ((int64_t)1 << 31) * 256) return DH_ERR_UNSUPPORTED;
    if (n_frames > ((int64_t)1 << 31) - 1 - frame0 || n_frames > (((int64_t)1 << 58) / H) / W) return DH_ERR_UNSUPPORTED;
    if (n == 0 || n_frames == 0) return DH_OK;
    if (!pts || !sd || !R || !T || !K || !topk || !arg || !seen) return DH_ERR_BAD_ARG;
    return launch_hull_accumulate(pts, n, sd, R, T, K, (int)n_frames, H, W, frame0, m, topk, arg, seen, static_cast<hipStream_t>(stream));
}

int dh_mesh_components(const int64_t* faces, int64_t nf, int64_t nv, int32_t* labels, void* stream) {
    if (nf < 0 || nv < 0) return DH_ERR_BAD_ARG;
    if (nv >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;               // labels are int32
    if (nv == 0) return DH_OK;
    if (!labels || (nf > 0 && !faces)) return DH_ERR_BAD_ARG;
    return launch_mesh_components(faces, nf, nv, labels, static_cast<hipStream_t>(stream));
}

int dh_mesh_raster_depth(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R, const float* T,
                         const float* K, int64_t n_frames, int H, int W, uint64_t* zbuf, void* stream) {
    if (nv < 0 || nf < 0 || n_frames < 0 || H <= 0 || W <= 0) return DH_ERR_BAD_ARG;
    if (nf >= ((int64_t)1 << 32) || n_frames >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;   // face ids are 32-bit key halves
    if (H > (1 << 24) || W > (1 << 24)) return DH_ERR_UNSUPPORTED;                                // pixel centres exact in fp32
    if (nf == 0 || n_frames == 0) return DH_OK;
    if (!verts || !faces || !R || !T || !K || !zbuf) return DH_ERR_BAD_ARG;
    return launch_mesh_raster_depth(verts, nv, faces, nf, R, T, K, n_frames, H, W, zbuf, static_cast<hipStream_t>(stream));
}

int dh_mesh_bake_colors(const float* verts, const float* normals, int64_t nv, const uint8_t* rgb, const uint8_t* usable,
                        const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                        float depth_eps, float min_cos, float* acc, int32_t* n_views, void* stream) {
    if (nv < 0 || n_frames < 0 || H <= 0 || W <= 0) return DH_ERR_BAD_ARG;
    if (depth_eps != depth_eps || depth_eps < 0.f || min_cos != min_cos) return DH_ERR_BAD_ARG;      // NaN, negative
    if (nv >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;                                        // n_views is int32
    if (H > (1 << 24) || W > (1 << 24)) return DH_ERR_UNSUPPORTED;
    if (nv == 0 || n_frames == 0) return DH_OK;
    if (!verts || !normals || !rgb || !usable || !zbuf || !R || !T || !K || !acc || !n_views) return DH_ERR_BAD_ARG;
    return launch_mesh_bake_colors(verts, normals, nv, rgb, usable, zbuf, R, T, K, n_frames, H, W, depth_eps, min_cos, acc, n_views,
                                   static_cast<hipStream_t>(stream));
}
int dh_mesh_shade(const float* verts, const float* normals, const uint8_t* colors, int64_t nv, const int64_t* faces, int64_t nf,
                  const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                  const uint8_t* rgb, const int8_t* label, float alpha, uint8_t* out, int64_t* counts, void* stream) {
    if (nv < 0 || nf < 0 || n_frames < 0 || H <= 0 || W <= 0) return DH_ERR_BAD_ARG;
    if (alpha != alpha || alpha < 0.f || alpha > 1.f || (label == nullptr) != (counts == nullptr)) return DH_ERR_BAD_ARG;
    if (nf >= ((int64_t)1 << 32) || n_frames >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;   // the z-buffer's limits
    if (H > (1 << 24) || W > (1 << 24)) return DH_ERR_UNSUPPORTED;
    if (n_frames > (((int64_t)1 << 62) / H) / W) return DH_ERR_UNSUPPORTED;                        // pixel indices in int64
    if (n_frames == 0) return DH_OK;
    if (!zbuf || !R || !T || !K || !out || (nf > 0 && (!verts || !normals || !faces))) return DH_ERR_BAD_ARG;
    const int64_t bytes = n_frames * H * W * 3;
    if (rgb && rgb < out + bytes && out < rgb + bytes) return DH_ERR_BAD_ARG;                     // out must not overlap rgb
    return launch_mesh_shade(verts, normals, colors, nv, faces, nf, zbuf, R, T, K, n_frames, H, W, rgb, label, alpha, out, counts,
                             static_cast<hipStream_t>(stream));
}

int dh_texture_bake(const float* verts, const float* normals, int64_t nv, const int64_t* faces, int64_t nf, const float* uv,
                    const int32_t* owner, int S, const uint8_t* rgb, const uint8_t* usable, const uint64_t* zbuf, const float* R,
                    const float* T, const float* K, int64_t n_frames, int H, int W, float depth_eps, float min_cos, int sharpen,
                    float* acc, int32_t* n_views, void* stream) {
    if (nv < 0 || nf < 0 || S < 0 || n_frames < 0 || H <= 0 || W <= 0 || sharpen < 0 || sharpen > 4) return DH_ERR_BAD_ARG;
    if (depth_eps != depth_eps || depth_eps < 0.f || min_cos != min_cos) return DH_ERR_BAD_ARG;      // NaN, negative
    if (nf >= ((int64_t)1 << 31) || S > (1 << 15)) return DH_ERR_UNSUPPORTED;                      // owner is int32; grid (S/16, S/16)
    if (H > (1 << 24) || W > (1 << 24) || n_frames >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;
    if (nf == 0 || S == 0 || n_frames == 0) return DH_OK;
    if (!verts || !normals || !faces || !uv || !owner || !rgb || !usable || !zbuf || !R || !T || !K || !acc || !n_views ||
        misaligned16(acc))
        return DH_ERR_BAD_ARG;
    return launch_texture_bake(verts, normals, nv, faces, nf, uv, owner, S, rgb, usable, zbuf, R, T, K, n_frames, H, W, depth_eps,
                               min_cos, sharpen, acc, n_views, static_cast<hipStream_t>(stream));
}

int dh_mesh_shade_tex(const float* verts, const float* normals, int64_t nv, const int64_t* faces, int64_t nf, const float* uv,
                      const uint8_t* tex, int Sh, int Sw, const uint64_t* zbuf, const float* R, const float* T, const float* K,
                      int64_t n_frames, int H, int W, const uint8_t* rgb, const uint8_t* usable, float alpha, int lit, uint8_t* out,
                      int64_t* sums, void* stream) {
    if (nv < 0 || nf < 0 || n_frames < 0 || H <= 0 || W <= 0 || (lit != 0 && lit != 1)) return DH_ERR_BAD_ARG;
    if (alpha != alpha || alpha < 0.f || alpha > 1.f || (usable == nullptr) != (sums == nullptr) || (sums && !rgb)) return DH_ERR_BAD_ARG;
    if (nf > 0 && (Sh <= 0 || Sw <= 0)) return DH_ERR_BAD_ARG;
    if (nf >= ((int64_t)1 << 32) || n_frames >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;   // the z-buffer's limits
    if (H > (1 << 24) || W > (1 << 24) || Sh > (1 << 24) || Sw > (1 << 24)) return DH_ERR_UNSUPPORTED;
    if (n_frames > (((int64_t)1 << 31) - 1) / shade_tex_blocks_per_frame(H, W)) return DH_ERR_UNSUPPORTED;   // one 1-D grid
    if (n_frames == 0) return DH_OK;
    if (!zbuf || !R || !T || !K || !out || (nf > 0 && (!verts || !normals || !faces || !uv || !tex))) return DH_ERR_BAD_ARG;
    const int64_t bytes = n_frames * H * W * 3;
    if (rgb && rgb < out + bytes && out < rgb + bytes) return DH_ERR_BAD_ARG;                     // out must not overlap rgb
    return launch_mesh_shade_tex(verts, normals, nv, faces, nf, uv, tex, Sh, Sw, zbuf, R, T, K, n_frames, H, W, rgb, usable, alpha, lit,
                                 out, sums, static_cast<hipStream_t>(stream));
}

// shared argument rules of the three dh_mc_* entry points: 2 <= N <= 2^20 grid points per axis, 1 <= B <= 16 cells per block edge,
// fewer than 2^31 blocks per call (one workgroup each)
static int mc_args(int64_t nb, int N, int B) {
    if (nb < 0 || N < 2 || B < 1) return DH_ERR_BAD_ARG;
    if (N > (1 << 20) || B > 16 || nb >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;
    return DH_OK;
}

int dh_mc_block_points(const float* ax, const float* ay, const float* az, int N, const int32_t* blocks, int64_t nb, int B, float* pts,
                       void* stream) {
    const int rc = mc_args(nb, N, B);
    if (rc != DH_OK || nb == 0) return rc;
    if (!ax || !ay || !az || !blocks || !pts) return DH_ERR_BAD_ARG;
    return launch_mc_block_points(ax, ay, az, N, blocks, nb, B, pts, static_cast<hipStream_t>(stream));
}

int dh_mc_count(const float* vals, const int32_t* blocks, int64_t nb, int N, int B, float threshold, const uint8_t* table,
                const int32_t* block_map, int32_t* counts, int32_t* cut_faces, int32_t* nonfinite, void* stream) {
    const int rc = mc_args(nb, N, B);
    if (rc != DH_OK) return rc;
    if (threshold != threshold) return DH_ERR_BAD_ARG;
    if (nb == 0) return DH_OK;
    if (!vals || !blocks || !table || !block_map || !counts || !cut_faces || !nonfinite) return DH_ERR_BAD_ARG;
    return launch_mc_count(vals, blocks, nb, N, B, threshold, table, block_map, counts, cut_faces, nonfinite,
                           static_cast<hipStream_t>(stream));
}

int dh_mc_emit(const float* vals, const int32_t* blocks, int64_t nb, int N, int B, float threshold, const uint8_t* table,
               const int64_t* offsets, int64_t n_tri, int64_t* keys, float* pos, void* stream) {
    const int rc = mc_args(nb, N, B);
    if (rc != DH_OK) return rc;
    if (threshold != threshold || n_tri < 0) return DH_ERR_BAD_ARG;
    if (nb == 0 || n_tri == 0) return DH_OK;
    if (!vals || !blocks || !table || !offsets || !keys || !pos) return DH_ERR_BAD_ARG;
    return launch_mc_emit(vals, blocks, nb, N, B, threshold, table, offsets, n_tri, keys, pos, static_cast<hipStream_t>(stream));
}

// shared argument rules of the silhouette entry points (the z-buffer's limits; grid (rows, column blocks) / (blocks, frames))
static int sil_args(int64_t n_frames, int H, int W) {
    if (n_frames < 0 || H <= 0 || W <= 0) return DH_ERR_BAD_ARG;
    if (H > (1 << 24) || W > (1 << 24) || n_frames >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;
    if (n_frames > (((int64_t)1 << 58) / H) / W) return DH_ERR_UNSUPPORTED;
    return DH_OK;
}

int dh_label_edt(const int8_t* label, int64_t n_frames, int H, int W, int value, int rmax, float* tmp, float* out, void* stream) {
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    if (rmax < 0 || value < -128 || value > 127) return DH_ERR_BAD_ARG;
    if (n_frames == 0) return DH_OK;
    if (!label || !tmp || !out) return DH_ERR_BAD_ARG;
    if (n_frames * H >= ((int64_t)1 << 31) || W > 65535 * 256 || rmax > 2896) return DH_ERR_UNSUPPORTED;   // 2 rmax^2 < 2^24: exact in fp32
    const int r = rmax < (H > W ? H : W) ? rmax : (H > W ? H : W);                                          // a wider window adds nothing
    return launch_label_edt(label, n_frames, H, W, value, r, tmp, out, static_cast<hipStream_t>(stream));
}

int64_t dh_sil_nearest_workspace(int64_t n_frames, int H, int W) {
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    return sil_nearest_workspace(n_frames, H, W);
}

int dh_sil_nearest(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R, const float* T, const float* K,
                   int64_t n_frames, int H, int W, float rmax_px, uint64_t* near, void* ws, void* stream) {
    if (nv < 0 || nf < 0) return DH_ERR_BAD_ARG;
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    if (!(rmax_px >= 0.f) || rmax_px > 4096.f) return DH_ERR_BAD_ARG;                                // NaN, negative, absurd
    if (nf >= ((int64_t)1 << 32)) return DH_ERR_UNSUPPORTED;                                          // face ids are 32-bit key halves
    if (nf == 0 || n_frames == 0) return DH_OK;
    if (!verts || !faces || !R || !T || !K || !near || !ws) return DH_ERR_BAD_ARG;
    return launch_sil_nearest(verts, nv, faces, nf, R, T, K, n_frames, H, W, rmax_px, near, ws, static_cast<hipStream_t>(stream));
}

int dh_sil_loss_sums(void) { return sil_loss_sums(); }

int64_t dh_sil_loss_grad_workspace(int64_t n_frames, int H, int W) {
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    return sil_loss_grad_workspace(n_frames, H, W);
}

int dh_sil_loss_grad(const uint64_t* near, const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R,
                     const float* T, const float* K, const float* d2_obj, const float* d2_hand, const int8_t* label, int64_t n_frames,
                     int H, int W, float sigma, float cut, float edge_offset, double* out, void* ws, void* stream) {
    if (nv < 0 || nf < 0) return DH_ERR_BAD_ARG;
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    if (!(sigma > 0.f) || !(cut > 0.f) || !(edge_offset >= 0.f) || sigma > 4096.f || cut > 16.f || edge_offset > 4096.f)
        return DH_ERR_BAD_ARG;
    if (nf >= ((int64_t)1 << 32) || n_frames > 65535) return DH_ERR_UNSUPPORTED;                     // grid (blocks, frames)
    if (n_frames == 0) return DH_OK;
    if (!near || !R || !T || !K || !d2_obj || !d2_hand || !label || !out || !ws || misaligned16(ws) || (nf > 0 && (!verts || !faces)))
        return DH_ERR_BAD_ARG;
    return launch_sil_loss_grad(near, verts, nv, faces, nf, R, T, K, d2_obj, d2_hand, label, n_frames, H, W, sigma, cut, edge_offset, out,
                                ws, static_cast<hipStream_t>(stream));
}

int dh_image_blur(const uint8_t* rgb, const uint8_t* usable, int64_t n_frames, int H, int W, const float* taps, int radius, float* tmp,
                  float* out, void* stream) {
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    if (radius < 0) return DH_ERR_BAD_ARG;
    if (n_frames == 0) return DH_OK;
    if (!rgb || !usable || !taps || !tmp || !out || misaligned16(tmp) || misaligned16(out)) return DH_ERR_BAD_ARG;
    if (n_frames * H >= ((int64_t)1 << 31) || W > 65535 * 256 || radius > image_blur_max_radius()) return DH_ERR_UNSUPPORTED;
    const int64_t floats = n_frames * H * W * 4;
    if (tmp < out + floats && out < tmp + floats) return DH_ERR_BAD_ARG;                             // the column pass reads tmp's other rows
    return launch_image_blur(rgb, usable, n_frames, H, W, taps, radius, tmp, out, static_cast<hipStream_t>(stream));
}

int dh_photo_loss_sums(void) { return photo_loss_sums(); }

int64_t dh_photo_loss_grad_workspace(int64_t n_frames, int64_t n_points) {
    if (n_frames < 0 || n_points < 0) return DH_ERR_BAD_ARG;
    if (n_frames > 65535 || n_points >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;
    return photo_loss_grad_workspace(n_frames, n_points);
}

int dh_photo_loss_grad(const float* pts, const float* normals, const float* colors, int64_t n_points, const float* img,
                       const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                       float depth_eps, float min_cos, float a_min, float delta, double* out, void* ws, void* stream) {
    if (n_points < 0) return DH_ERR_BAD_ARG;
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    if (!(depth_eps >= 0.f) || min_cos != min_cos || !(a_min >= 0.f) || !(delta > 0.f)) return DH_ERR_BAD_ARG;   // NaN, negative
    if (n_points >= ((int64_t)1 << 31) || n_frames > 65535) return DH_ERR_UNSUPPORTED;               // grid (blocks, frames)
    if (n_frames == 0) return DH_OK;
    if (!R || !T || !K || !out || !ws || misaligned16(ws)) return DH_ERR_BAD_ARG;
    if (n_points > 0 && (!pts || !normals || !colors || !img || !zbuf || misaligned16(img))) return DH_ERR_BAD_ARG;
    return launch_photo_loss_grad(pts, normals, colors, n_points, img, zbuf, R, T, K, n_frames, H, W, depth_eps, min_cos, a_min, delta,
                                  out, ws, static_cast<hipStream_t>(stream));
}

int dh_pose_corr_width(void) { return pose_corr_width(); }

int64_t dh_pose_corr_sums_workspace(int64_t n_pairs, int64_t max_count) {
    if (n_pairs < 0 || max_count < 0) return DH_ERR_BAD_ARG;
    if (n_pairs > 65535 || max_count >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;
    return pose_corr_sums_workspace(n_pairs, max_count);
}

int dh_pose_corr_sums(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R, const float* T, const float* K,
                      int64_t n_frames, const uint64_t* zbuf, int64_t n_z, int H, int W, const float* matches, int64_t n_matches,
                      const int64_t* pairs, int64_t n_pairs, int64_t max_count, float delta_px, float min_cos, double* out, float* resid,
                      void* ws, void* stream) {
    if (nv < 0 || nf < 0 || n_frames < 0 || n_matches < 0 || n_pairs < 0 || max_count < 0) return DH_ERR_BAD_ARG;
    const int rc = sil_args(n_z, H, W);
    if (rc != DH_OK) return rc;
    if (!(delta_px > 0.f) || !(min_cos >= 0.f) || delta_px > 1e6f || min_cos > 1.f) return DH_ERR_BAD_ARG;   // NaN, negative, absurd
    if (nf >= ((int64_t)1 << 32) || n_pairs > 65535 || max_count >= ((int64_t)1 << 31) || n_matches >= ((int64_t)1 << 40)
        || n_frames >= ((int64_t)1 << 31))
        return DH_ERR_UNSUPPORTED;                                                                     // grid (slabs, pairs)
    if (n_pairs == 0) return DH_OK;
    if (!pairs || !out || !ws || misaligned16(ws)) return DH_ERR_BAD_ARG;
    if (max_count > 0 && (!R || !T || !K || !zbuf || !matches || n_z == 0 || (nf > 0 && (!verts || !faces)))) return DH_ERR_BAD_ARG;
    return launch_pose_corr_sums(verts, nv, faces, nf, R, T, K, n_frames, zbuf, n_z, H, W, matches, n_matches, pairs, n_pairs, max_count,
                                 delta_px, min_cos, out, resid, ws, static_cast<hipStream_t>(stream));
}

int dh_pose_corr_frames(const double* rows, const double* scale, int64_t n_pairs, const int64_t* start, const int64_t* entries,
                        int64_t n_entries, int64_t n_frames, double* gR, double* gT, void* stream) {
    if (n_pairs < 0 || n_entries < 0 || n_frames < 0) return DH_ERR_BAD_ARG;
    if (n_frames >= ((int64_t)1 << 31) || n_pairs >= ((int64_t)1 << 31) || n_entries >= ((int64_t)1 << 40)) return DH_ERR_UNSUPPORTED;
    if (n_frames == 0) return DH_OK;
    if (!start || !gR || !gT || (n_entries > 0 && (!rows || !scale || !entries))) return DH_ERR_BAD_ARG;
    return launch_pose_corr_frames(rows, scale, n_pairs, start, entries, n_entries, n_frames, gR, gT, static_cast<hipStream_t>(stream));
}

int dh_match_gray(const float* img, int64_t n_frames, int H, int W, float a_min, uint8_t* gray, uint8_t* valid, void* stream) {
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    if (a_min != a_min) return DH_ERR_BAD_ARG;
    if (n_frames * H * W >= ((int64_t)1 << 38)) return DH_ERR_UNSUPPORTED;                             // one 1-D grid of 256 pixels per workgroup
    if (n_frames == 0) return DH_OK;
    if (!img || !gray || !valid || misaligned16(img)) return DH_ERR_BAD_ARG;
    return launch_match_gray(img, n_frames * H * W, a_min, gray, valid, static_cast<hipStream_t>(stream));
}

// dh_match_search and dh_match_search_warp: the same rules, queries of 6 or 10 words
static int match_search_api(const uint8_t* gray, const uint8_t* valid, int64_t n_frames, int H, int W, const int32_t* queries, int64_t n,
                            bool warp, int P, int R, int excl, int64_t min_va, int32_t* out_i, double* out_f, void* stream) {
    if (n < 0) return DH_ERR_BAD_ARG;
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    if (P < 1 || P > match_max_patch() || R < 0 || R > match_max_range() || excl < 0 || min_va < 1) return DH_ERR_BAD_ARG;
    if (n >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;                                          // one workgroup per query
    if (n == 0) return DH_OK;
    if (!gray || !valid || !queries || !out_i || !out_f || (reinterpret_cast<uintptr_t>(out_f) & 7u) != 0 ||
        (reinterpret_cast<uintptr_t>(out_i) & 3u) != 0 || (reinterpret_cast<uintptr_t>(queries) & 3u) != 0)
        return DH_ERR_BAD_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int bad = match_check_frames(queries, n, n_frames, warp, out_i, st);
    if (bad != 0) return bad < 0 ? bad : DH_ERR_BAD_ARG;
    return launch_match_search(gray, valid, H, W, queries, n, warp, P, R, excl, min_va, out_i, out_f, st);
}

int dh_match_search(const uint8_t* gray, const uint8_t* valid, int64_t n_frames, int H, int W, const int32_t* queries, int64_t n, int P,
                    int R, int excl, int64_t min_va, int32_t* out_i, double* out_f, void* stream) {
    return match_search_api(gray, valid, n_frames, H, W, queries, n, false, P, R, excl, min_va, out_i, out_f, stream);
}

int dh_match_search_warp(const uint8_t* gray, const uint8_t* valid, int64_t n_frames, int H, int W, const int32_t* queries, int64_t n,
                         int P, int R, int excl, int64_t min_va, int32_t* out_i, double* out_f, void* stream) {
    return match_search_api(gray, valid, n_frames, H, W, queries, n, true, P, R, excl, min_va, out_i, out_f, stream);
}

int dh_ssim_sums(void) { return ssim_sums(); }

// the scalar arguments dh_ssim_workspace and dh_ssim share
static int ssim_args(int64_t n_frames, int H, int W) {
    if (n_frames < 0 || H <= 0 || W <= 0) return DH_ERR_BAD_ARG;
    if (H > (1 << 24) || W > (1 << 24) || n_frames > 65535) return DH_ERR_UNSUPPORTED;             // grid (tiles, frames)
    if (ssim_tiles_per_frame(H, W) >= ((int64_t)1 << 22)) return DH_ERR_UNSUPPORTED;
    return DH_OK;
}

int64_t dh_ssim_workspace(int64_t n_frames, int H, int W) {
    const int rc = ssim_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    return ssim_workspace(n_frames, H, W);
}

int dh_ssim(const uint8_t* a, const uint8_t* b, const uint8_t* usable, int64_t n_frames, int H, int W, const int32_t* taps_host,
            int radius, uint64_t w_min, float* map, double* out, void* ws, void* stream) {
    if (n_frames < 0 || H <= 0 || W <= 0 || radius < 0 || w_min == 0 || w_min > ((uint64_t)1 << 32)) return DH_ERR_BAD_ARG;
    const int rc = ssim_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    if (radius > ssim_max_radius()) return DH_ERR_UNSUPPORTED;
    if (n_frames == 0) return DH_OK;
    if (!a || !b || !taps_host || !out || !ws || misaligned16(ws)) return DH_ERR_BAD_ARG;
    int64_t sum = 0;
    for (int k = 0; k < 2 * radius + 1; ++k) {
        if (taps_host[k] < 0) return DH_ERR_BAD_ARG;
        sum += taps_host[k];
    }
    if (sum != 65536) return DH_ERR_BAD_ARG;                                                         // the row sums rest on it
    return launch_ssim(a, b, usable, n_frames, H, W, taps_host, radius, w_min, map, out, ws, static_cast<hipStream_t>(stream));
}

int dh_label_boxes(const int8_t* label, int64_t n, int H, int W, int32_t* boxes, void* stream) {
    const int rc = sil_args(n, H, W);
    if (rc != DH_OK) return rc;
    if (label_boxes_chunks(H, W) >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;                 // grid (chunks, images)
    if (n == 0) return DH_OK;
    if (!label || !boxes) return DH_ERR_BAD_ARG;
    return launch_label_boxes(label, n, H, W, boxes, static_cast<hipStream_t>(stream));
}

int dh_sil_crop_pack(const int8_t* label, int64_t n, int H, int W, const float* sq, int S, uint64_t* obj, uint64_t* keep, void* stream) {
    const int rc = sil_args(n, H, W);
    if (rc != DH_OK) return rc;
    if (S < 8 || S > 128 || (S & 7) != 0) return DH_ERR_BAD_ARG;                                     // S^2 a multiple of 64
    if (n > (((int64_t)1 << 32) - 4) / (S * S / 64)) return DH_ERR_UNSUPPORTED;                       // one 1-D grid, four words per workgroup
    if (n == 0) return DH_OK;
    if (!label || !sq || !obj || !keep) return DH_ERR_BAD_ARG;
    return launch_sil_crop_pack(label, n, H, W, sq, S, obj, keep, static_cast<hipStream_t>(stream));
}

int dh_sil_bank_score(const uint64_t* frame_obj, const uint64_t* frame_keep, int64_t n_frames, const uint64_t* bank_obj, int64_t n_views,
                      int n_words, int32_t* out, void* stream) {
    if (n_frames < 0 || n_views < 0 || n_words < 1) return DH_ERR_BAD_ARG;
    if (n_words > (1 << 20)) return DH_ERR_UNSUPPORTED;                                             // 64 n_words fits an int32 count
    if (sil_bank_score_frame_tiles(n_frames) > 65535 || sil_bank_score_view_tiles(n_views) >= ((int64_t)1 << 31))
        return DH_ERR_UNSUPPORTED;                                                                 // grid (view tiles, frame tiles)
    if (n_frames == 0 || n_views == 0) return DH_OK;
    if (!frame_obj || !frame_keep || !bank_obj || !out || (reinterpret_cast<uintptr_t>(out) & 7u) != 0) return DH_ERR_BAD_ARG;
    return launch_sil_bank_score(frame_obj, frame_keep, n_frames, bank_obj, n_views, n_words, out, static_cast<hipStream_t>(stream));
}

// shared argument rules of the simplification entry points: a grid as dh_simplify_grid returns it
static int simplify_grid_args(const float* lo, float h, const int32_t* dims) {
    if (!lo || !dims || !(h >= 0.f) || !(h <= 3.0e38f)) return DH_ERR_BAD_ARG;
    for (int a = 0; a < 3; ++a) {
        if (!(lo[a] >= -3.4e38f && lo[a] <= 3.4e38f) || dims[a] < 1) return DH_ERR_BAD_ARG;
        if (dims[a] > (1 << 20) + 1) return DH_ERR_UNSUPPORTED;
    }
    return DH_OK;
}

int dh_simplify_grid(const float* lo, const float* hi, int64_t cells, float* h, int32_t* dims) {
    if (!lo || !hi || !h || !dims || cells < 1) return DH_ERR_BAD_ARG;
    if (cells > ((int64_t)1 << 20)) return DH_ERR_UNSUPPORTED;
    for (int a = 0; a < 3; ++a) {
        const float e = hi[a] - lo[a];
        if (!(e >= 0.f && e <= 3.0e38f)) return DH_ERR_BAD_ARG;                                  // NaN, inverted or overflowing box
    }
    simplify_grid(lo, hi, cells, h, dims);
    return DH_OK;
}

int dh_simplify_cells(const float* verts, int64_t nv, const float* lo, float h, const int32_t* dims, int64_t* keys, void* stream) {
    if (nv < 0) return DH_ERR_BAD_ARG;
    const int rc = simplify_grid_args(lo, h, dims);
    if (rc != DH_OK) return rc;
    if (nv >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;
    if (nv == 0) return DH_OK;
    if (!verts || !keys) return DH_ERR_BAD_ARG;
    return launch_simplify_cells(verts, nv, lo, h, dims, keys, static_cast<hipStream_t>(stream));
}

int dh_simplify_sums(void) { return simplify_sums(); }

int dh_simplify_quadrics(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* order,
                         const int64_t* run_start, const int64_t* run_key, int64_t n_runs, const float* lo, float h, const int32_t* dims,
                         double regularization, int placement, float* rep, int32_t* clamped, double* sums, void* stream) {
    if (nv < 0 || nf < 0 || n_runs < 0) return DH_ERR_BAD_ARG;
    const int rc = simplify_grid_args(lo, h, dims);
    if (rc != DH_OK) return rc;
    if (!(regularization > 0.0) || !(regularization <= 1.0e6) || (placement != 0 && placement != 1)) return DH_ERR_BAD_ARG;
    if (nv >= ((int64_t)1 << 31) || nf >= ((int64_t)1 << 31) || n_runs > 3 * nf) return DH_ERR_UNSUPPORTED;
    if (n_runs == 0) return DH_OK;
    if (!verts || !faces || !order || !run_start || !run_key || !rep || !clamped) return DH_ERR_BAD_ARG;
    return launch_simplify_quadrics(verts, nv, faces, nf, order, run_start, run_key, n_runs, lo, h, dims, regularization, placement, rep,
                                    clamped, sums, static_cast<hipStream_t>(stream));
}

int dh_simplify_faces(const int64_t* faces, int64_t nf, const int32_t* vrank, int64_t nv, int64_t n_runs, int64_t* tri, uint8_t* keep,
                      int64_t* key, void* stream) {
    if (nv < 0 || nf < 0 || n_runs < 0) return DH_ERR_BAD_ARG;
    if (nv >= ((int64_t)1 << 31) || nf >= ((int64_t)1 << 31) || n_runs >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;
    if (nf == 0) return DH_OK;
    if (!faces || !vrank || !tri || !keep || !key) return DH_ERR_BAD_ARG;
    return launch_simplify_faces(faces, nf, vrank, nv, n_runs, tri, keep, key, static_cast<hipStream_t>(stream));
}

// ---- sphere tracing of the SDF (trace.hip)
static inline bool trace_dims(int n_views, int H, int W, int level, int64_t& h, int64_t& w, int64_t& N) {
    if (n_views < 0 || H < 1 || W < 1 || level < 1) return false;
    h = ((int64_t)H + level - 1) / level;
    w = ((int64_t)W + level - 1) / level;
    N = (int64_t)n_views * h * w;
    return true;
}

int dh_trace_init(const float* R, const float* T, const float* Kinv, int n_views, int H, int W, int level, float bound, float* o,
                  float* d, float* t, float* t_far, uint8_t* state, void* stream) {
    int64_t h, w, N;
    if (!trace_dims(n_views, H, W, level, h, w, N) || !(bound > 0.f)) return DH_ERR_BAD_ARG;
    if (N >= (1ll << 31)) return DH_ERR_UNSUPPORTED;
    if (N == 0) return DH_OK;
    if (!R || !T || !Kinv || !o || !d || !t || !t_far || !state) return DH_ERR_BAD_ARG;
    return launch_trace_init(R, T, Kinv, (int)h, (int)w, level, bound, N, o, d, t, t_far, state, static_cast<hipStream_t>(stream));
}

int dh_trace_step(const int32_t* idx, const int32_t* count, const float* s, const float* o, const float* d, int64_t rays_per_view,
                  int64_t N, float* t, const float* t_far, float* t_lo, float* s_lo, float* t_hi, float* s_hi, uint8_t* state,
                  uint16_t* nq, uint8_t* nref, uint8_t* flags, float eps, float relax, float min_step, float max_step, int refine_steps,
                  int64_t n_max, float* pts, void* stream) {
    if (N < 0 || n_max < 0 || rays_per_view < 1 || !(eps > 0.f) || !(relax > 0.f) || !(min_step > 0.f) || !(max_step >= min_step) ||
        refine_steps < 1 || refine_steps > 255)
        return DH_ERR_BAD_ARG;
    if (N >= (1ll << 31) || n_max >= (1ll << 31)) return DH_ERR_UNSUPPORTED;
    if (n_max == 0 || N == 0) return DH_OK;
    if (!idx || !s || !o || !d || !t || !t_far || !t_lo || !s_lo || !t_hi || !s_hi || !state || !nq || !nref || !flags || !pts)
        return DH_ERR_BAD_ARG;
    return launch_trace_step(idx, count, s, o, d, rays_per_view, N, t, t_far, t_lo, s_lo, t_hi, s_hi, state, nq, nref, flags, eps, relax,
                             min_step, max_step, refine_steps, n_max, pts, static_cast<hipStream_t>(stream));
}

int dh_trace_points(const int32_t* idx, const float* o, const float* d, const float* t, int64_t rays_per_view, int64_t N, int64_t n,
                    float* pts, void* stream) {
    if (N < 0 || n < 0 || rays_per_view < 1) return DH_ERR_BAD_ARG;
    if (N >= (1ll << 31) || n >= (1ll << 31)) return DH_ERR_UNSUPPORTED;
    if (n == 0 || N == 0) return DH_OK;
    if (!idx || !o || !d || !t || !pts) return DH_ERR_BAD_ARG;
    return launch_trace_points(idx, o, d, t, rays_per_view, N, n, pts, static_cast<hipStream_t>(stream));
}

int dh_trace_compact(const int32_t* idx, const int32_t* count, const uint8_t* state, const float* o, const float* d, const float* t,
                     int64_t rays_per_view, int64_t N, int64_t n_max, int32_t* ws, int32_t* idx_out, int32_t* count_out,
                     float* pts_out, void* stream) {
    if (N < 0 || n_max < 0 || rays_per_view < 1 || !count_out || count_out == count) return DH_ERR_BAD_ARG;
    if (N >= (1ll << 31) || n_max >= (1ll << 31)) return DH_ERR_UNSUPPORTED;
    if (n_max > 0 && (!state || !o || !d || !t || !ws || !idx_out || !pts_out || idx_out == idx)) return DH_ERR_BAD_ARG;
    return launch_trace_compact(idx, count, state, o, d, t, rays_per_view, N, n_max, ws, idx_out, count_out, pts_out,
                                static_cast<hipStream_t>(stream));
}

int dh_trace_compose(const uint8_t* state, const float* t, const float* d, const int32_t* slot, const float* normals,
                     const float* colors, int64_t n_hits, const float* R, int n_views, int H, int W, int level, int background,
                     const uint8_t* frame_rgb, const int32_t* frame_idx, int n_frames, uint8_t* rgb, float* depth, uint8_t* normal,
                     uint8_t* hit, void* stream) {
    int64_t h, w, N;
    if (!trace_dims(n_views, H, W, level, h, w, N) || n_hits < 0 || background < 0 || background > 2 || n_frames < 0)
        return DH_ERR_BAD_ARG;
    if (N >= (1ll << 31) || n_hits >= (1ll << 31)) return DH_ERR_UNSUPPORTED;
    if (N == 0) return DH_OK;
    if (!state || !t || !d || !slot || !R || !rgb || !depth || !normal || !hit) return DH_ERR_BAD_ARG;
    if (n_hits > 0 && (!normals || !colors)) return DH_ERR_BAD_ARG;
    if (background == 2 && (!frame_rgb || !frame_idx || n_frames < 1)) return DH_ERR_BAD_ARG;
    return launch_trace_compose(state, t, d, slot, normals, colors, n_hits, R, (int)h, (int)w, level, H, W, background, frame_rgb,
                                frame_idx, n_frames, N, rgb, depth, normal, hit, static_cast<hipStream_t>(stream));
}

int dh_mvs_sweep(const uint8_t* gray, const uint8_t* valid, int64_t n_frames, int H, int W, const float* R, const float* T, const float* K,
                 const float* Kinv, const int32_t* pix, const float* guide, int64_t n, const int32_t* nbr, int n_nbr, int D, float step,
                 int P, int64_t min_va, float min_vb, int min_views, float min_cos, float* out_f, int32_t* out_i, void* stream) {
    if (n < 0) return DH_ERR_BAD_ARG;
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    if (P < 1 || P > mvs_max_patch() || D < 3 || D > mvs_max_depths() || (D & 1) == 0 || n_nbr < 1 || n_nbr > mvs_max_neighbours() ||
        min_va < 1 || !(min_vb > 0.f) || min_views < 1 || !(step > 0.f) || !std::isfinite(step) || !std::isfinite(min_vb) ||
        !(min_cos >= -1.f && min_cos <= 1.f))
        return DH_ERR_BAD_ARG;
    if (n >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;                                          // at least one pixel per wave
    if (n == 0) return DH_OK;
    if (!gray || !valid || !R || !T || !K || !Kinv || !pix || !guide || !nbr || !out_f || !out_i ||
        ((reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(T) | reinterpret_cast<uintptr_t>(K) |
          reinterpret_cast<uintptr_t>(Kinv) | reinterpret_cast<uintptr_t>(pix) | reinterpret_cast<uintptr_t>(guide) |
          reinterpret_cast<uintptr_t>(nbr) | reinterpret_cast<uintptr_t>(out_f) | reinterpret_cast<uintptr_t>(out_i)) & 3u) != 0)
        return DH_ERR_BAD_ARG;
    return launch_mvs_sweep(gray, valid, (int)n_frames, H, W, R, T, K, Kinv, pix, guide, n, nbr, n_nbr, D, step, P, min_va, min_vb,
                            min_views, min_cos, out_f, out_i, static_cast<hipStream_t>(stream));
}

int dh_mvs_check(const float* depth, int64_t n_frames, int H, int W, const float* R, const float* T, const float* K, const float* Kinv,
                 const int32_t* nbr, int n_nbr, float depth_rel, uint8_t* count, void* stream) {
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    if (n_nbr < 1 || n_nbr > mvs_max_neighbours() || !(depth_rel >= 0.f) || !std::isfinite(depth_rel)) return DH_ERR_BAD_ARG;
    if (n_frames * H * W >= ((int64_t)1 << 38)) return DH_ERR_UNSUPPORTED;                             // one 1-D grid of 256 pixels per workgroup
    if (n_frames == 0) return DH_OK;
    if (!depth || !R || !T || !K || !Kinv || !nbr || !count ||
        ((reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(T) |
          reinterpret_cast<uintptr_t>(K) | reinterpret_cast<uintptr_t>(Kinv) | reinterpret_cast<uintptr_t>(nbr)) & 3u) != 0)
        return DH_ERR_BAD_ARG;
    return launch_mvs_check(depth, (int)n_frames, H, W, R, T, K, Kinv, nbr, n_nbr, depth_rel, count, static_cast<hipStream_t>(stream));
}

namespace {
inline bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// the checks the two forms of dh_ray_depth and dh_ray_depth_bwd share; DH_OK + *run = false for the no-op
int ray_depth_args(const float* rays, const float* R, const float* samples, int64_t B, bool* run) {
    *run = false;
    if (B < 0) return DH_ERR_BAD_ARG;
    if (B == 0) return DH_OK;
    if (!rays || !R || !samples || misaligned4(rays) || misaligned4(R) || misaligned4(samples)) return DH_ERR_BAD_ARG;
    *run = true;
    return DH_OK;
}
}  // namespace

int dh_ray_depth(const float* rays, const float* R, const float* z, const float* weights, int64_t B, int n, float sample_dist, float* t,
                 float* wsum, float* zc, void* stream) {
    if (n < 1 || !std::isfinite(sample_dist)) return DH_ERR_BAD_ARG;
    bool run;
    const int rc = ray_depth_args(rays, R, z, B, &run);
    if (rc != DH_OK || !run) return rc;
    if (!weights || !t || !wsum || !zc || misaligned4(weights) || misaligned4(t) || misaligned4(wsum) || misaligned4(zc)) return DH_ERR_BAD_ARG;
    return launch_ray_depth(rays, R, z, weights, B, n, nullptr, nullptr, n, sample_dist, t, wsum, zc, static_cast<hipStream_t>(stream));
}

int dh_ray_depth_packed(const float* rays, const float* R, const float* t_start, const float* weights, int64_t B, const int64_t* seg_off,
                        const int32_t* seg_cnt, int max_samples, float step, float* t, float* wsum, float* zc, void* stream) {
    if (max_samples < 0 || !std::isfinite(step)) return DH_ERR_BAD_ARG;
    if (max_samples > 1024) return DH_ERR_UNSUPPORTED;
    bool run;
    const int rc = ray_depth_args(rays, R, t_start, B, &run);
    if (rc != DH_OK || !run) return rc;
    if (!weights || !t || !wsum || !zc || !seg_off || !seg_cnt || misaligned4(weights) || misaligned4(t) || misaligned4(wsum) ||
        misaligned4(zc) || (reinterpret_cast<uintptr_t>(seg_off) & 7u) != 0 || misaligned4(seg_cnt))
        return DH_ERR_BAD_ARG;
    return launch_ray_depth(rays, R, t_start, weights, B, 0, seg_off, seg_cnt, max_samples, step, t, wsum, zc,
                            static_cast<hipStream_t>(stream));
}

int dh_ray_depth_bwd(const float* rays, const float* R, const float* z, const float* t, const float* wsum, const float* ray_f,
                     const float* stats, int64_t B, int n, float sample_dist, float warp_weight, int accumulate, float* d_weights,
                     float* d_normal_map, void* stream) {
    if (n < 1 || !std::isfinite(sample_dist) || !(warp_weight >= 0.f) || accumulate < 0 || accumulate > 3) return DH_ERR_BAD_ARG;
    bool run;
    const int rc = ray_depth_args(rays, R, z, B, &run);
    if (rc != DH_OK || !run) return rc;
    if (!t || !wsum || !ray_f || !stats || misaligned4(t) || misaligned4(wsum) || misaligned4(ray_f) || misaligned4(stats) ||
        misaligned4(d_weights) || misaligned4(d_normal_map))
        return DH_ERR_BAD_ARG;
    return launch_ray_depth_bwd(rays, R, z, t, wsum, ray_f, stats, B, n, nullptr, nullptr, n, sample_dist, warp_weight, accumulate,
                                d_weights, d_normal_map, static_cast<hipStream_t>(stream));
}

int dh_ray_depth_bwd_packed(const float* rays, const float* R, const float* t_start, const float* t, const float* wsum, const float* ray_f,
                            const float* stats, int64_t B, const int64_t* seg_off, const int32_t* seg_cnt, int max_samples, float step,
                            float warp_weight, int accumulate, float* d_weights, float* d_normal_map, void* stream) {
    if (max_samples < 0 || !std::isfinite(step) || !(warp_weight >= 0.f) || accumulate < 0 || accumulate > 3) return DH_ERR_BAD_ARG;
    if (max_samples > 1024) return DH_ERR_UNSUPPORTED;
    bool run;
    const int rc = ray_depth_args(rays, R, t_start, B, &run);
    if (rc != DH_OK || !run) return rc;
    if (!t || !wsum || !ray_f || !stats || !seg_off || !seg_cnt || misaligned4(t) || misaligned4(wsum) || misaligned4(ray_f) ||
        misaligned4(stats) || misaligned4(d_weights) || misaligned4(d_normal_map) || (reinterpret_cast<uintptr_t>(seg_off) & 7u) != 0 ||
        misaligned4(seg_cnt))
        return DH_ERR_BAD_ARG;
    return launch_ray_depth_bwd(rays, R, t_start, t, wsum, ray_f, stats, B, 0, seg_off, seg_cnt, max_samples, step, warp_weight, accumulate,
                                d_weights, d_normal_map, static_cast<hipStream_t>(stream));
}

int64_t dh_warp_loss_workspace(int64_t B) {
    if (B < 0) return DH_ERR_BAD_ARG;
    return warp_loss_workspace(B);
}

int dh_warp_loss(const uint8_t* gray, const uint8_t* valid, int64_t n_frames, int H, int W, const float* R, const float* T, const float* K,
                 const float* Kinv, const int32_t* nbr, int n_nbr, int frame, const int32_t* pix, const float* z, const float* wsum,
                 const float* normal, int64_t B, int P, int64_t min_va, float min_vb, int topk, int min_views, float min_cos,
                 float min_wsum, float warp_weight, float* out_f, int32_t* out_i, float* stats, void* ws, void* stream) {
    if (B < 0) return DH_ERR_BAD_ARG;
    const int rc = sil_args(n_frames, H, W);
    if (rc != DH_OK) return rc;
    if (P < 1 || P > warp_max_patch() || n_nbr < 1 || n_nbr > warp_max_neighbours() || topk < 1 || topk > warp_max_neighbours() ||
        min_views < 1 || min_views > warp_max_neighbours() || min_va < 1 || !(min_vb > 0.f) || !std::isfinite(min_vb) ||
        !(min_cos >= -1.f && min_cos <= 1.f) || !std::isfinite(min_wsum) || !(warp_weight >= 0.f) || !std::isfinite(warp_weight))
        return DH_ERR_BAD_ARG;                                                                       // a NaN fails every comparison
    if (B >= ((int64_t)1 << 31)) return DH_ERR_UNSUPPORTED;
    if (B == 0) return DH_OK;
    if (frame < 0 || frame >= n_frames) return DH_ERR_BAD_ARG;
    if (!gray || !valid || !R || !T || !K || !Kinv || !nbr || !pix || !z || !wsum || !normal || !out_f || !out_i || !stats || !ws ||
        misaligned4(R) || misaligned4(T) || misaligned4(K) || misaligned4(Kinv) || misaligned4(nbr) || misaligned4(pix) || misaligned4(z) ||
        misaligned4(wsum) || misaligned4(normal) || misaligned4(out_f) || misaligned4(out_i) || misaligned4(stats) || misaligned16(ws))
        return DH_ERR_BAD_ARG;
    return launch_warp_loss(gray, valid, (int)n_frames, H, W, R, T, K, Kinv, nbr, n_nbr, frame, pix, z, wsum, normal, B, P, min_va, min_vb,
                            topk, min_views, min_cos, min_wsum, warp_weight, out_f, out_i, stats, ws, static_cast<hipStream_t>(stream));
}

int dh_tsdf_integrate(const float* pts, int64_t n, const float* depth, const uint8_t* weight, const float* R, const float* T, const float* K,
                      int64_t n_frames, int H, int W, float trunc, int64_t* num, int32_t* den, int32_t* obs, void* stream) {
    if (n < 0 || n_frames < 0 || H < 1 || W < 1 || !(trunc > 0.f) || !std::isfinite(trunc)) return DH_ERR_BAD_ARG;
    if (H > (1 << 24) || W > (1 << 24) || n >= ((int64_t)1 << 31) * 256) return DH_ERR_UNSUPPORTED;
    if (n_frames > ((int64_t)1 << 31) - 1 || n_frames > (((int64_t)1 << 58) / H) / W) return DH_ERR_UNSUPPORTED;
    if (n == 0 || n_frames == 0) return DH_OK;
    if (!pts || !depth || !weight || !R || !T || !K || !num || !den || !obs) return DH_ERR_BAD_ARG;
    return launch_tsdf_integrate(pts, n, depth, weight, R, T, K, (int)n_frames, H, W, trunc, num, den, obs,
                                 static_cast<hipStream_t>(stream));
}

}  // extern "C"
