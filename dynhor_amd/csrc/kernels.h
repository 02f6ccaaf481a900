// Internal launch-function declarations (one per kernel family).  All enqueue on the caller's stream,
// allocate nothing, and return 0 / negative dh error codes (include/dynhor_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "layout.h"

namespace dh {

// arithmetic of the MLP GEMMs (include/dynhor_hip.h dh_arithmetic): passed to every launch function; the entry points without an
// arithmetic argument pass the process default (dh_set_arithmetic)
enum : int { ARITH_BF16 = 0, ARITH_FP32 = 1, ARITH_F16 = 2 };
int hash_scatter_mode();

int launch_pack_weights(const float* params, float* packed, int arith_mask, hipStream_t stream);

// status of the launches just enqueued: 0, or DH_ERR_LAUNCH (include/dynhor_hip.h) when the runtime reports an error
inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -3; }
// grid of a tile-resident chain launch: one workgroup per TM-point tile, at most `grid` (the workgroups loop over the rest)
inline int grid_for(int64_t npts, int grid) {
    const int64_t ntiles = (npts + TM - 1) / TM;
    return (int)(ntiles < grid ? ntiles : grid);
}

// MLP chains (kernels_mlp.hip).  npts is padded by the caller to a multiple of 128 for saved buffers.
int launch_sdf_nograd(const float* packed, const float* pts, int64_t npts, float* sdf, int grid, int arith, hipStream_t stream);
int launch_sdf_nograd_t(const float* packed, const float* pts, int64_t npts, float* sdf, bool h2, hipStream_t stream);   // chain_t.hip
int launch_sdf_fwd_train_t(const float* packed, const float* pts, int64_t npts, float* sdf, float* feat, float* act, float* eaux,
                           unsigned* absmax, bool h2, hipStream_t stream);

// (absmax: workspace.h -- the two-piece fp16 kernels post the per-launch maxima of their saved-tile classes there)
int launch_sdf_fwd_train(const float* packed, const float* pts, int64_t npts, float* sdf, float* feat, float* act,
                         float* eaux, float* absmax, int grid, int arith, hipStream_t stream);
int launch_sdf_grad(const float* packed, const float* pts, int64_t npts, const float* act, float* asave, float* normals,
                    int save, float* gesave, float* absmax, int grid, int arith, hipStream_t stream);
int launch_color_fwd(const float* packed, const float* pts, const float* dirs, int n_per_ray, const float* normals,
                     const float* feat, int64_t npts, float* color, float* cact, float* caux, int save, float* absmax, int grid,
                     int arith, hipStream_t stream);
// kernels_mlp_h.hip (two-piece fp16)
int launch_sdf_grad_h(const float* packed, const float* pts, int64_t npts, const float* act, float* asave, float* normals,
                      int save, float* gesave, unsigned* absmax, int grid, hipStream_t stream);
int launch_color_fwd_h(const float* packed, const float* pts, const float* dirs, int n_per_ray, const float* normals,
                       const float* feat, int64_t npts, float* color, float* cact, float* caux, int save, unsigned* absmax,
                       int grid, hipStream_t stream);
int launch_color_bwd_h(const float* packed, const float* colors, const float* d_colors, const float* dirs, int n_per_ray,
                       int64_t npts, const float* cact, float* czbar, float* featbar, float* d_normals, float* tpart,
                       float* d_pts, float* d_dirs_pts, unsigned* absmax, unsigned* tmax, int grid, hipStream_t st);
int launch_sdf_tangent_h(const float* packed, const float* pts, const float* d_normals, int64_t npts, const float* act,
                         const float* asave, float* t0aux, float* tsave, float* rsave, float* tpart, unsigned* absmax, unsigned* tmax,
                         int grid, hipStream_t st);
int launch_sdf_bwd_h(const float* packed, const float* d_sdf, const float* pts, const float* d_normals, int64_t npts,
                     const float* act, const float* rsave, const float* featbar, const float* gesave, float* zbar, float* tpart,
                     float* d_pts, unsigned* absmax, unsigned* tmax, int grid, hipStream_t st);

// chain_pair.hip (two-piece fp16, tile-PAIR form: one workgroup per CU, weights held in registers across two tiles; round 6).
// The launchers above pick it for launches of at least 2 x #CUs tiles unless the arithmetic word carries a form flag (CHAIN_FORM_*).
enum : int { CHAIN_FORM_AUTO = 0, CHAIN_FORM_TILE = 1, CHAIN_FORM_PAIR = 2 };
bool pair_form_available();
int pair_form_cus();
// the form a SPLIT_F16 stage launch of npts points takes: forced by the flag; otherwise PAIR where the stage's pair form is the faster one
// on the bench's launch (auto_pair: measured same-process A/Bs, profiles/r06_ab_chain_forms.json -- colour forward yes; input gradient and
// colour backward no: their epilogues load a saved tile, and with one wave per SIMD nothing hides that latency) and every CU gets a pair
inline bool use_pair_form(int form, int64_t npts, bool auto_pair) {
    if (form == CHAIN_FORM_PAIR) return true;
    if (form == CHAIN_FORM_TILE || !auto_pair) return false;
    const int cus = pair_form_cus();
    return cus > 0 && (npts + TM - 1) / TM >= 2 * (int64_t)cus;
}
int launch_color_fwd_p(const float* packed, const float* pts, const float* dirs, int n_per_ray, const float* normals,
                       const float* feat, int64_t npts, float* color, float* cact, float* caux, int save, unsigned* absmax,
                       hipStream_t stream);

int launch_sdf_grad_p(const float* packed, const float* pts, int64_t npts, const float* act, float* asave, float* normals, int save,
                      float* gesave, unsigned* absmax, hipStream_t stream);

int launch_color_bwd_p(const float* packed, const float* colors, const float* d_colors, int64_t npts, const float* cact, float* czbar,
                       float* featbar, float* d_normals, float* tpart, unsigned* absmax, unsigned* tmax, hipStream_t stream);

// per-ray kernels (kernels_ray.hip)
int launch_gen_rays(const uint8_t* rgb, const int8_t* label, const uint8_t* normal, const float* R, const float* T,
                    const float* Kinv, int H, int W, int frame, const int64_t* px, const int64_t* py, int64_t B,
                    float* rays, float* near, float* far, hipStream_t st);
int launch_coarse_samples(const float* o, const float* d, const float* near, const float* far, const float* t_rand,
                          int64_t B, int n, float* z, float* pts, hipStream_t st);
int launch_upsample(const float* o, const float* d, const float* z, const float* sdf, int64_t B, int n, int n_new,
                    float inv_s, float* z_new, float* pts_new, hipStream_t st);
int launch_merge(const float* z, const float* z_new, const float* sdf, const float* sdf_new, int64_t B, int n, int n_new,
                 float* z_out, float* sdf_out, hipStream_t st);
int launch_midpoints(const float* o, const float* d, const float* z, int64_t B, int n, float sample_dist, float* pts,
                     hipStream_t st);
int launch_render_fwd(const float* o, const float* d, const float* z, const float* sdf, const float* normals,
                      const float* colors, const float* inv_s, float car, float sample_dist, const float* bg, int64_t B,
                      int n, float* weights, float* color, float* wsum, float* wmax, float* cdf, float* inside, float* eik,
                      float* nmap, const int64_t* seg_off, const int32_t* seg_cnt, hipStream_t st);
int launch_render_bwd(const float* o, const float* d, const float* z, const float* sdf, const float* normals,
                      const float* colors, const float* inv_s, float car, float sample_dist, const float* bg, int64_t B,
                      int n, const float* d_color, const float* d_wsum, const float* d_weights, const float* d_gradients,
                      const float* d_nmap, const float* eik_coef, float* d_sdf, float* d_normals, float* d_colors,
                      float* d_inv_s, float* d_rays_d, const int64_t* seg_off, const int32_t* seg_cnt, hipStream_t st);
// per-ray fold of the point adjoints over packed rays (pose refinement on the occupancy-grid sampler)
int launch_ray_adjoint_packed(const float* d_pts, const float* d_dirs_pts, const float* t_start, float step, const int64_t* seg_off,
                              const int32_t* seg_cnt, int64_t B, float* d_rays_o, float* d_rays_d, hipStream_t st);
// occupancy-grid marching (march.hip)
int launch_march_count(const float* o, const float* d, const float* near, const float* far, const float* u, const uint8_t* occ,
                       int res, float radius, float step, float half_step, int max_samples, int64_t B, int32_t* cnt,
                       hipStream_t st);
int launch_march_emit(const float* o, const float* d, const float* near, const float* far, const float* u, const uint8_t* occ,
                      int res, float radius, float step, float half_step, int max_samples, int64_t B, const int64_t* off,
                      const int32_t* keep, float* t_start, float* pts, float* dirs_pts, int32_t* ray_idx, hipStream_t st);
// sphere tracing of the SDF (trace.hip): rays of F poses, one state-machine step, order-preserving compaction, image buffers
int launch_trace_init(const float* R, const float* T, const float* Kinv, int h, int w, int level, float bound, int64_t N, float* o,
                      float* d, float* t, float* t_far, uint8_t* state, hipStream_t st);
int launch_trace_step(const int32_t* idx, const int32_t* count, const float* s, const float* o, const float* d, int64_t rays_per_view,
                      int64_t N, float* t, const float* t_far, float* t_lo, float* s_lo, float* t_hi, float* s_hi, uint8_t* state,
                      uint16_t* nq, uint8_t* nref, uint8_t* flags, float eps, float relax, float min_step, float max_step,
                      int refine_steps, int64_t n_max, float* pts, hipStream_t st);
int launch_trace_points(const int32_t* idx, const float* o, const float* d, const float* t, int64_t rays_per_view, int64_t N, int64_t n,
                        float* pts, hipStream_t st);
int launch_trace_compact(const int32_t* idx, const int32_t* count, const uint8_t* state, const float* o, const float* d, const float* t,
                         int64_t rays_per_view, int64_t N, int64_t n_max, int32_t* block_off, int32_t* idx_out, int32_t* count_out,
                         float* pts_out, hipStream_t st);
int launch_trace_compose(const uint8_t* state, const float* t, const float* d, const int32_t* slot, const float* normals,
                         const float* colors, int64_t n_hits, const float* R, int h, int w, int level, int H, int W, int background,
                         const uint8_t* frame_rgb, const int32_t* frame_idx, int n_frames, int64_t N, uint8_t* rgb, float* depth,
                         uint8_t* normal, uint8_t* hit, hipStream_t st);
int launch_loss(const float* color, const float* wsum, const float* nmap, const float* eik, const float* rays,
                const float* R, int64_t B, float igr_w, float mask_w, float normal_w, float* stats, float* d_color,
                float* d_wsum, float* d_nmap, float* eik_coef, hipStream_t st);

int launch_corr_loss(const float* rays_o, const float* rays_d, const float* z, const float* weights, const float* corr,
                     const float* R_all, const float* T_all, int n_frames, const float* K, int64_t B, int n, float sample_dist,
                     float delta_px, float corr_w, float* stats, float* residual_px, float* d_weights, float* pose_adj,
                     hipStream_t st);

// backward chains (kernels_mlp_bwd.hip) and weight gradients (dw.hip)
int launch_color_bwd(const float* packed, const float* colors, const float* d_colors, int64_t npts, const float* cact,
                     float* czbar, float* featbar, float* d_normals, float* tpart, float* absmax, int grid, int arith, hipStream_t st);
// pose-refinement variants (every arithmetic): additionally the adjoints w.r.t. the sample points / view directions
int launch_color_bwd_rays(const float* packed, const float* colors, const float* d_colors, const float* dirs, int n_per_ray,
                          int64_t npts, const float* cact, float* czbar, float* featbar, float* d_normals, float* tpart,
                          float* d_pts, float* d_dirs_pts, float* absmax, int grid, int arith, hipStream_t st);
int launch_sdf_bwd_rays(const float* packed, const float* d_sdf, const float* pts, const float* d_normals, int64_t npts,
                        const float* act, const float* rsave, const float* featbar, const float* gesave, float* zbar,
                        float* tpart, float* d_pts, float* absmax, int grid, int arith, hipStream_t st);
int launch_sdf_tangent(const float* packed, const float* pts, const float* d_normals, int64_t npts, const float* act,
                       const float* asave, float* t0aux, float* tsave, float* rsave, float* tpart, float* absmax, int grid, int arith,
                       hipStream_t st);
int launch_sdf_bwd(const float* packed, const float* d_sdf, int64_t npts, const float* act, const float* rsave,
                   const float* featbar, float* zbar, float* tpart, float* absmax, int grid, int arith, hipStream_t st);
struct Workspace;
int launch_weight_grads_gemm(const Workspace& w, float* slabs, float* tred, int G, int nS, int arith, hipStream_t st);
int launch_weight_grads_fold(const Workspace& w, float* slabs, float* tred, int G, int nS, const float* params,
                             const float* packed, float* grad, hipStream_t st);

int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                int64_t step, float grad_scale, hipStream_t st);

// multiresolution hash-grid encoding (hashgrid.hip)
int64_t hashgrid_entries();
int hashgrid_level(int l, float* scale, uint32_t* res, uint32_t* offset, uint32_t* dense);
int launch_hashgrid_fwd(const float* table, const float* x01, int64_t n, float* out, hipStream_t st);
int launch_hashgrid_bwd(const float* x01, const float* d_out, int64_t n, float* d_table, hipStream_t st);

// hash-grid model family (hash_mlp.hip): fused encoding + small MLPs, forward and backward
int64_t hash_num_params();
int64_t hash_workspace_floats(int64_t n);
int launch_hash_pack(const float* params, float* hp, hipStream_t st);
int launch_hash_sdf_nograd(const float* params, const float* hp, const float* pts, int64_t n, float radius, float* sdf,
                           hipStream_t st);
int64_t hash_infer_workspace_floats(int64_t n);
int launch_hash_geo_fwd(const float* params, const float* hp, const float* pts, int64_t n, float radius, float eps,
                        float* ws, int save, float* sdf, float* feat, float* grad, const int64_t* n_act, hipStream_t st);
int launch_sh_color_fwd(const float* hp, const float* feat, const float* normals, const float* dirs, int n_per_ray,
                        int64_t n, float* color, const int64_t* n_act, hipStream_t st);
// d_dirs_pts / d_pts (pose refinement; null: not formed): the adjoints w.r.t. the view direction and the sample point, [n,3] each
int launch_sh_color_bwd(const float* hp, const float* feat, const float* normals, const float* dirs, const float* d_color,
                        int n_per_ray, int64_t n, float* ws, float* d_feat, float* d_normals, float* d_dirs_pts, const int64_t* n_act,
                        hipStream_t st);
int launch_hash_geo_bwd(const float* params, const float* hp, const float* pts, const float* d_sdf, const float* d_feat,
                        const float* d_grad, int64_t n, float radius, float eps, float* ws, float* d_pts, const int64_t* n_act,
                        hipStream_t st);
int launch_hash_weight_grads(const float* params, const float* hp, int64_t n, float* ws, float* grad, const int64_t* n_act,
                             int parts, hipStream_t st);

// exact nearest-neighbour squared distance (nn.hip): ws = nearest_sqdist_workspace(nq, nr) bytes for the slab-split path, or null
int64_t nearest_sqdist_workspace(int64_t nq, int64_t nr);
int launch_nearest_sqdist(const float* q, int64_t nq, const float* ref, int64_t nr, float* d2, int32_t* idx, void* ws, hipStream_t st);

// signed distance to a triangle mesh (mesh_sdf.hip): one record of mesh_sdf_record_floats() floats per face, then the brute-force query;
// ws = mesh_sdf_query_workspace(n, nf) bytes (0: one slab, ws unused); mesh_sdf_max_faces(): the slabs must fit grid.y
int mesh_sdf_record_floats();
int64_t mesh_sdf_query_workspace(int64_t n, int64_t nf);
int64_t mesh_sdf_max_faces();
int launch_mesh_sdf_prepare(const float* verts, int64_t nv, const int32_t* faces, int64_t nf, float* rec, hipStream_t st);
int launch_mesh_sdf_query(const float* rec, int64_t nf, const float* pts, int64_t n, float* sqdist, int32_t* face, float* wind, void* ws,
                          hipStream_t st);

// similarity ICP (dynhor_amd/mesh_align.py).  Correspondences (nn.hip): the sweep of launch_nearest_sqdist for h hypotheses at once,
// the source transformed on load by xf [h,12]; ws = icp_correspond_workspace(n, m, h) bytes, or null (one slab).  Moment sums of the
// pairs inside the trim threshold (icp.hip): icp_moments_sums(plane) doubles per hypothesis, ws = icp_moments_workspace(n, h, plane) bytes
int64_t icp_correspond_workspace(int64_t n, int64_t m, int64_t h);
int launch_icp_correspond(const float* src, int64_t n, const float* tgt, int64_t m, const float* xf, int64_t h, float* d2, int32_t* idx,
                          void* ws, hipStream_t st);
int icp_moments_sums(int plane);
int64_t icp_moments_workspace(int64_t n, int64_t h, int plane);
int launch_icp_moments(const float* src, const float* tgt, const float* nrm, const float* xf, const int32_t* idx, const float* d2,
                       const float* thr, const float* osrc, const float* otgt, int64_t n, int64_t m, int64_t h, double* out, void* ws,
                       hipStream_t st);

// the last step of a reproducible fp64 sum (sums64.h; the kernel lives in icp.hip): out[g, k] = the `blocks` partials [K] (K <= 64) of
// each of `groups` groups added in block order
// depth / masked normal priors of the training step (prior_loss.hip); seg_off == nullptr: dense rays [B,n]
int64_t prior_loss_workspace(int64_t B);
int launch_prior_loss(const float* rays, const float* R, const float* z, const float* weights, const float* nmap, const float* prior,
                      int64_t B, int n, const int64_t* seg_off, const int32_t* seg_cnt, int max_samples, float sample_dist,
                      float depth_w, float delta, float normal_w, int accumulate, float* stats, float* d_weights, float* d_nmap,
                      void* ws, hipStream_t st);
int launch_sum64_reduce(const double* partial, int64_t groups, int blocks, int K, double* out, hipStream_t st);

// multi-view photometric consistency of the training step (warp_loss.hip); seg_off == nullptr: dense rays [B,n]
int warp_max_patch();
int warp_max_neighbours();
int64_t warp_loss_workspace(int64_t B);
int launch_ray_depth(const float* rays, const float* R, const float* z, const float* weights, int64_t B, int n, const int64_t* seg_off,
                     const int32_t* seg_cnt, int max_samples, float sample_dist, float* t_out, float* w_out, float* z_out, hipStream_t st);
int launch_ray_depth_bwd(const float* rays, const float* R, const float* z, const float* t_in, const float* w_in, const float* ray_f,
                         const float* stats, int64_t B, int n, const int64_t* seg_off, const int32_t* seg_cnt, int max_samples,
                         float sample_dist, float warp_w, int accumulate, float* d_weights, float* d_nmap, hipStream_t st);
int launch_warp_loss(const uint8_t* gray, const uint8_t* valid, int n_frames, int H, int W, const float* R, const float* T, const float* K,
                     const float* Kinv, const int32_t* nbr, int n_nbr, int frame, const int32_t* pix, const float* z, const float* wsum,
                     const float* normal, int64_t B, int P, int64_t min_va, float min_vb, int topk, int min_views, float min_cos,
                     float min_wsum, float warp_w, float* out_f, int32_t* out_i, float* stats, void* ws, hipStream_t st);

// mesh cleaning (mesh_clean.hip): label dilation, silhouette votes per vertex, connected components by union-find
int launch_label_dilate(const int8_t* label, int64_t n_frames, int H, int W, int radius, uint8_t* tmp, uint8_t* keep, hipStream_t st);
int launch_mesh_mask_votes(const float* verts, int64_t nv, const uint8_t* keep, const float* R, const float* T, const float* K,
                           int64_t n_frames, int H, int W, int32_t* bg_votes, int32_t* seen, hipStream_t st);
int launch_mesh_components(const int64_t* faces, int64_t nf, int64_t nv, int32_t* labels, hipStream_t st);

// visual hull (visual_hull.hip): the m largest signed mask distances per point over a chunk of frames (m in 1..8)
int launch_hull_accumulate(const float* pts, int64_t n, const float* sd, const float* R, const float* T, const float* K, int n_frames,
                           int H, int W, int frame0, int m, float* topk, int32_t* arg, int32_t* seen, hipStream_t st);

// mesh colouring (mesh_color.hip): z-buffer of the mesh in every frame, per-vertex colour gathered over the frames
int launch_mesh_raster_depth(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R, const float* T,
                             const float* K, int64_t n_frames, int H, int W, uint64_t* zbuf, hipStream_t st);
int launch_mesh_bake_colors(const float* verts, const float* normals, int64_t nv, const uint8_t* rgb, const uint8_t* usable,
                            const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                            float depth_eps, float min_cos, float* acc, int32_t* n_views, hipStream_t st);
// mesh overlay (mesh_vis.hip): the z-buffer's faces shaded and composited over the frames, silhouette counts against the labels
int launch_mesh_shade(const float* verts, const float* normals, const uint8_t* colors, int64_t nv, const int64_t* faces, int64_t nf,
                      const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                      const uint8_t* rgb, const int8_t* label, float alpha, uint8_t* out, int64_t* counts, hipStream_t st);
// texture atlas (mesh_texture.hip): per-texel colour gathered over the frames; the z-buffer's faces drawn with the texture, squared
// error against the frames (shade_tex_blocks_per_frame: the workgroups one frame takes, for the grid limit)
int launch_texture_bake(const float* verts, const float* normals, int64_t nv, const int64_t* faces, int64_t nf, const float* uv,
                        const int32_t* owner, int S, const uint8_t* rgb, const uint8_t* usable, const uint64_t* zbuf, const float* R,
                        const float* T, const float* K, int64_t n_frames, int H, int W, float depth_eps, float min_cos, int sharpen,
                        float* acc, int32_t* n_views, hipStream_t st);
int64_t shade_tex_blocks_per_frame(int H, int W);
int launch_mesh_shade_tex(const float* verts, const float* normals, int64_t nv, const int64_t* faces, int64_t nf, const float* uv,
                          const uint8_t* tex, int Sh, int Sw, const uint64_t* zbuf, const float* R, const float* T, const float* K,
                          int64_t n_frames, int H, int W, const uint8_t* rgb, const uint8_t* usable, float alpha, int lit, uint8_t* out,
                          int64_t* sums, hipStream_t st);

// silhouette pose refinement (sil.hip): windowed exact distance transform of a label value, nearest face per pixel within rmax_px
// (ws = sil_nearest_workspace bytes), loss / pose-gradient sums per frame (sil_loss_sums() doubles, ws = sil_loss_grad_workspace bytes)
int launch_label_edt(const int8_t* label, int64_t n_frames, int H, int W, int value, int rmax, float* tmp, float* out, hipStream_t st);
int64_t sil_nearest_workspace(int64_t n_frames, int H, int W);
int launch_sil_nearest(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R, const float* T, const float* K,
                       int64_t n_frames, int H, int W, float rmax_px, uint64_t* near, void* ws, hipStream_t st);
int sil_loss_sums();
int64_t sil_loss_grad_workspace(int64_t n_frames, int H, int W);
int launch_sil_loss_grad(const uint64_t* near, const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R,
                         const float* T, const float* K, const float* d2_obj, const float* d2_hand, const int8_t* label, int64_t n_frames,
                         int H, int W, float sigma, float cut, float edge_offset, double* out, void* ws, hipStream_t st);

// photometric pose term (pose_photo.hip): masked separable Gaussian of the frames (radius <= image_blur_max_radius()), loss /
// pose-gradient sums per frame of coloured surface points (photo_loss_sums() doubles, ws = photo_loss_grad_workspace bytes)
int image_blur_max_radius();
int launch_image_blur(const uint8_t* rgb, const uint8_t* usable, int64_t n_frames, int H, int W, const float* taps, int radius,
                      float* tmp, float* out, hipStream_t st);
int photo_loss_sums();
int64_t photo_loss_grad_workspace(int64_t n_frames, int64_t n_points);
int launch_photo_loss_grad(const float* pts, const float* normals, const float* colors, int64_t n, const float* img,
                           const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                           float depth_eps, float min_cos, float a_min, float delta, double* out, void* ws, hipStream_t st);

// correspondence pose term (pose_corr.hip): loss / pose-gradient sums per frame pair of matches lifted to the mesh (pose_corr_width()
// doubles per pair, ws = pose_corr_sums_workspace bytes; max_count = the largest count of the pair table, from the host), and the fold
// of the pairs' rows into per-frame gradients in the order of the host's list
int pose_corr_width();
int64_t pose_corr_sums_workspace(int64_t n_pairs, int64_t max_count);
int launch_pose_corr_sums(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R, const float* T, const float* K,
                          int64_t n_frames, const uint64_t* zbuf, int64_t n_z, int H, int W, const float* matches, int64_t n_matches,
                          const int64_t* pairs, int64_t n_pairs, int64_t max_count, float delta_px, float min_cos, double* out, float* resid,
                          void* ws, hipStream_t st);
int launch_pose_corr_frames(const double* rows, const double* scale, int64_t n_pairs, const int64_t* start, const int64_t* entries,
                            int64_t n_entries, int64_t n_frames, double* gR, double* gT, hipStream_t st);

// dense frame matching (match.hip): 8-bit grey and validity of blurred frames, guided ZNCC block search per query (patch half-size
// <= match_max_patch(), search range <= match_max_range()); match_check_frames waits for the stream: 0 = every query's frames lie in
// [0, n_frames), 1 = one does not.  warp: the queries have 10 words, the last four a 2 x 2 map in Q16 through which the source patch is
// sampled, and the check also answers 1 for an entry beyond +-2^19
int match_max_patch();
int match_max_range();
int launch_match_gray(const float* img, int64_t n_pixels, float a_min, uint8_t* gray, uint8_t* valid, hipStream_t st);
int match_check_frames(const int32_t* queries, int64_t n, int64_t n_frames, bool warp, int32_t* scratch, hipStream_t st);
int launch_match_search(const uint8_t* gray, const uint8_t* valid, int H, int W, const int32_t* queries, int64_t n, bool warp, int P,
                        int R, int excl, int64_t min_va, int32_t* out_i, double* out_f, hipStream_t st);

// image metrics (image_metrics.hip): masked SSIM of u8 images with integer window sums and an fp64 formula, squared / absolute error
// sums of the usable pixels (ssim_sums() doubles per frame, ws = ssim_workspace bytes; radius <= ssim_max_radius(); taps_host is read
// on the host and passed to the kernel by value; ssim_tiles_per_frame: the grid size, for the limit)
int ssim_sums();
int ssim_max_radius();
int64_t ssim_tiles_per_frame(int H, int W);
int64_t ssim_workspace(int64_t n_frames, int H, int W);
int launch_ssim(const uint8_t* a, const uint8_t* b, const uint8_t* usable, int64_t n_frames, int H, int W, const int32_t* taps_host,
                int radius, uint64_t w_min, float* map, double* out, void* ws, hipStream_t st);

// pose initialisation by silhouette retrieval (pose_init.hip): tight box of label == 1 per image, the label resampled on an S x S
// square and packed one bit per sample (obj / keep planes), intersection / union counts of every frame against every bank view
// (label_boxes_chunks / sil_bank_score_*_tiles: the grid sizes, for the limits)
int64_t label_boxes_chunks(int H, int W);
int launch_label_boxes(const int8_t* label, int64_t n, int H, int W, int32_t* boxes, hipStream_t st);
int launch_sil_crop_pack(const int8_t* label, int64_t n, int H, int W, const float* sq, int S, uint64_t* obj, uint64_t* keep,
                         hipStream_t st);
int64_t sil_bank_score_frame_tiles(int64_t F);
int64_t sil_bank_score_view_tiles(int64_t V);
int launch_sil_bank_score(const uint64_t* frame_obj, const uint64_t* frame_keep, int64_t F, const uint64_t* bank_obj, int64_t V, int Wd,
                          int32_t* out, hipStream_t st);

// block-sparse marching cubes (mesh_extract.hip): sample points of the listed blocks, triangles and cut faces per block, triangle emit
int launch_mc_block_points(const float* ax, const float* ay, const float* az, int N, const int32_t* blocks, int64_t nb, int B, float* pts,
                           hipStream_t st);
int launch_mc_count(const float* vals, const int32_t* blocks, int64_t nb, int N, int B, float threshold, const uint8_t* table,
                    const int32_t* block_map, int32_t* counts, int32_t* cut_faces, int32_t* nonfinite, hipStream_t st);
int launch_mc_emit(const float* vals, const int32_t* blocks, int64_t nb, int N, int B, float threshold, const uint8_t* table,
                   const int64_t* offsets, int64_t n_tri, int64_t* keys, float* pos, hipStream_t st);

// mesh simplification by quadric vertex clustering (mesh_simplify.hip): the grid of a bounding box (host only), cell key per vertex,
// per-cell sums / solve / representative over the sorted record runs (simplify_sums() doubles per run), faces remapped to cell ranks
void simplify_grid(const float* lo, const float* hi, int64_t cells, float* h, int32_t* dims);
int launch_simplify_cells(const float* verts, int64_t nv, const float* lo, float h, const int32_t* dims, int64_t* keys, hipStream_t st);
int simplify_sums();
int launch_simplify_quadrics(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* order,
                             const int64_t* run_start, const int64_t* run_key, int64_t n_runs, const float* lo, float h,
                             const int32_t* dims, double lambda, int quadric, float* rep, int32_t* clamped, double* sums,
                             hipStream_t st);
int launch_simplify_faces(const int64_t* faces, int64_t nf, const int32_t* vrank, int64_t nv, int64_t n_runs, int64_t* tri, uint8_t* keep,
                          int64_t* key, hipStream_t st);

// multi-view stereo (mvs.hip): a plane sweep per pixel about a guide depth, scored by fp32 ZNCC over bilinear taps against up to
// mvs_max_neighbours() frames (patch half-size <= mvs_max_patch(), 3 <= D <= mvs_max_depths(), D odd), and the count of neighbours whose
// depth map agrees with a pixel's depth
int mvs_max_patch();
int mvs_max_depths();
int mvs_max_neighbours();
int launch_mvs_sweep(const uint8_t* gray, const uint8_t* valid, int n_frames, int H, int W, const float* R, const float* T, const float* K,
                     const float* Kinv, const int32_t* pix, const float* guide, int64_t n, const int32_t* nbr, int n_nbr, int D, float step,
                     int P, int64_t min_va, float min_vb, int min_views, float min_cos, float* out_f, int32_t* out_i, hipStream_t st);
int launch_mvs_check(const float* depth, int n_frames, int H, int W, const float* R, const float* T, const float* K, const float* Kinv,
                     const int32_t* nbr, int n_nbr, float depth_rel, uint8_t* count, hipStream_t st);

// depth fusion (tsdf.hip): the weighted truncated signed distance of every point to the depth maps of a chunk of frames, in integer sums
int launch_tsdf_integrate(const float* pts, int64_t n, const float* depth, const uint8_t* weight, const float* R, const float* T,
                          const float* K, int n_frames, int H, int W, float trunc, int64_t* num, int32_t* den, int32_t* obs,
                          hipStream_t st);

}  // namespace dh
