/* dynhor_hip.h -- C ABI of libdynhor_hip.so: the MI355X (gfx950) implementation of the NeuS reconstruction
 * hot path named by BASELINE.json.north_star.
 *
 * The reference (EAST-J/Dynhor @ 2025-09-05) exposes NO plugin/FFI surface for this path -- the path itself is
 * unreleased (reference README.md:7-11, 55-58).  Each entry point therefore cites the
 * upstream-NeuS Python method it implements and the reference file:line that constrains
 * its inputs, and INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes; every pointer is a DEVICE pointer unless named host_*; fp32 row-major.
 *   - the caller allocates everything (torch tensors); the library never allocates, frees or retains pointers.
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it, no implicit synchronisation.
 *   - return 0 on success or a negative dh_status; never throws, never exits.  Re-entrant: the library keeps no
 *     pointer and no per-call state.  Its ONLY process-global state is the two DEFAULT words set by dh_set_arithmetic() and
 *     dh_hash_set_scatter_mode() below (plain ints; no environment variable is read anywhere).  Every MLP stage also has
 *     an `_ex` entry point that takes the arithmetic as its first argument and reads no global at all: two host threads
 *     (or two renderers) can run different arithmetics side by side through those.
 *   - arithmetic: every buffer that crosses this boundary is fp32.  Inside, the GEMMs form each fp32 product from
 *     low-precision pieces on the matrix cores with fp32 accumulation, to fp32 accuracy:
 *     DH_ARITH_SPLIT_F16 (default since round 4) two fp16 pieces per operand and three MFMA products, the operands
 *     scaled by powers of two; DH_ARITH_SPLIT_BF16 three bf16 pieces and six products.
 */
#ifndef DYNHOR_HIP_H
#define DYNHOR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    DH_OK = 0,
    DH_ERR_BAD_ARG = -1,        /* null pointer / negative size / misaligned buffer */
    DH_ERR_UNSUPPORTED = -2,    /* configuration outside the fixed NeuS architecture */
    DH_ERR_LAUNCH = -3          /* hipGetLastError() != hipSuccess after enqueue */
} dh_status;

int dh_version(void);
const char* dh_strerror(int status);

/* Arithmetic of the MLP GEMMs.  DH_ARITH_SPLIT_F16 (default): two-piece fp16 split, three products (csrc/tile16h.h).
 * DH_ARITH_SPLIT_BF16: three-piece bf16 split, six products (csrc/tile16.h; the default of rounds 1-3).
 * DH_ARITH_FP32_MFMA: the native v_mfma_f32_32x32x2_f32 twin of every kernel (the independent, exact-fp32 arithmetic that
 * tests/test_gpu_arithmetic_modes.py checks the other two against).  All three read and write the same buffers (packed
 * weights -- dh_pack_weights writes every layout --, workspace, outputs).  dh_set_arithmetic sets the DEFAULT used by the
 * entry points that take no arithmetic argument (for launches enqueued after the call); the `_ex` entry points below
 * ignore it.
 * ONE ARITHMETIC PER STEP: every stage of one training step on one workspace, dh_sdf_forward through dh_weight_grads_gemm, must
 * run in the SAME arithmetic.  The buffers are shared, but the workspace's scale tables (absmax / tmax, csrc/workspace.h) are
 * cleared by dh_sdf_forward and filled by the SPLIT_F16 stages only: a SPLIT_F16 dh_weight_grads_gemm behind a
 * bf16 / fp32 backward (or behind a dh_set_arithmetic between the un-suffixed stage calls of one step) would read stale scale
 * words.  Guard: every training forward clears the table and only the SPLIT_F16 one then writes a tag word into it
 * (csrc/workspace.h ABSMAX_TAG); a SPLIT_F16 dh_weight_grads_gemm that finds no tag writes NaN gradients (loud) instead of
 * gradients scaled by stale words (silently wrong). */
typedef enum { DH_ARITH_SPLIT_BF16 = 0, DH_ARITH_FP32_MFMA = 1, DH_ARITH_SPLIT_F16 = 2 } dh_arithmetic;
/* Chain FORM of a DH_ARITH_SPLIT_F16 stage (round 6; csrc/pair16h.h).  The stages listed below exist in two kernel forms that write
 * bit-identical results: the TILE form (csrc/kernels_mlp_h.hip: one 64-point tile per workgroup, two workgroups per CU, weights
 * streamed from L2 per tile) and the PAIR form (csrc/chain_pair.hip: one workgroup per CU owns two tiles, holds a layer's weight slice
 * in registers across both and runs one tile's epilogue under the other's MFMAs: half the L2 -> CU weight bytes per point).  OR one of
 * these flags into the `arithmetic` argument of the stage's `_ex` entry point to force a form (tests, A/Bs); without a flag the stage
 * takes the form that measured faster on the bench's launch: dh_color_forward_ex the PAIR form for launches of at least 2 x #CUs tiles
 * (32,768 points on MI355X; a pair workgroup occupies a whole CU), dh_sdf_gradient_ex and dh_color_backward_ex the TILE form (their pair
 * forms are 5-20 % slower: DESIGN.md section 3).  The PAIR form returns DH_ERR_UNSUPPORTED on a device without 160 KB of LDS per CU.
 * Stages with a PAIR form: dh_sdf_gradient_ex, dh_color_forward_ex, dh_color_backward_ex (not its pose-refinement form
 * dh_color_backward_rays_ex).  Every other entry point rejects the flags (DH_ERR_BAD_ARG). */
enum { DH_CHAIN_FORM_TILE = 0x100, DH_CHAIN_FORM_PAIR = 0x200 };
int dh_set_arithmetic(int mode);
int dh_get_arithmetic(void);

/* ---- parameter vector / packed weights -----------------------------------------------------------------
 * One flat fp32 vector of dh_num_params() == 802,491 values in state_dict order (SURVEY.md §5 checkpoint row:
 * lin{l}.bias, lin{l}.weight_g, lin{l}.weight_v for sdf_network_fine lin0..8, variance, color_network_fine
 * lin0..4).  dh_param_layout: net 0 = SDFNetwork, 1 = SingleVarianceNetwork (layer ignored; only v_off), 2 =
 * RenderingNetwork. */
int64_t dh_num_params(void);
int64_t dh_packed_floats(void);
int dh_param_layout(int net, int layer, int64_t* bias_off, int64_t* g_off, int64_t* v_off, int* out_dim, int* in_dim);

/* Where a section of the packed buffer lies (float offset, float count) -- for tests and tools that decode it: 0 = the
 * register-resident chains' bf16x3 weight stream (132 stages of 24 KB), 1 = their 10 bias rows, 2 = the two-piece fp16 stream
 * (132 stages of 16 KB), 3 = its 11-row table (16 x bias of lin0..7, lin8 row 0, lin8 bias rows 1..256, 1 / S_w of lin0..8),
 * 4 = max |W| per linear (16 u32: sdf lin0..8, colour lin0..4), from which the fp16 weight scales are derived. */
int dh_packed_section(int section, int64_t* offset_floats, int64_t* n_floats);

/* weight-norm (W = g v/||v||, upstream nn.utils.weight_norm) + MFMA-operand packing; once per optimiser step. */
int dh_pack_weights(const float* params, float* packed, void* stream);

/* SDFNetwork.sdf(pts) under no_grad (upstream NeuSRenderer.render up-sampling loop).
 * pts [npts,3] -> sdf [npts]. */
int dh_sdf_nograd(const float* packed, const float* pts, int64_t npts, float* sdf, void* stream);

/* Workspace size (floats) for a render call over npts fine sample points: infer_floats suffices for a forward-only
 * render (save = 0 below), fwd_floats is what a training forward writes (saved activations), total_floats additionally
 * covers the backward pass. */
int dh_workspace_floats(int64_t npts, int64_t* infer_floats, int64_t* fwd_floats, int64_t* total_floats);

/* Range watch of the DH_ARITH_SPLIT_F16 arithmetic.  Its register-resident SDF forward chain carries the softplus activations at
 * the CONSTANT scale 16 in fp16 (csrc/chain_t.hip): an activation beyond *limit = 65504 / 16 = 4094 overflows the hi piece and the
 * results downstream of it are NaN (every other operand class of the MLPs is scaled dynamically, per tile or per launch, and has no
 * such limit; the embedding input shares the constant scale but is a point of the unit sphere).  dh_sdf_gradient(_ex) -- which reads
 * every activation tile the forward saved -- therefore posts the largest activation of the launch into the workspace: one fp32 word
 * at float offset *act_max_off of ws, valid once dh_sdf_gradient of the step has run; +inf when any activation overflowed (a saved
 * value downstream of an overflowed piece is NaN, and the word never lets a finite survivor stand for it), and then the step's
 * weight-gradient launch writes NaN for every weight the activations feed.  A caller that can afford a device read (the
 * Runner: at report iterations) compares it with *limit and switches to DH_ARITH_SPLIT_BF16 / raises.  *tag_off: the word that holds
 * 0x00F16F16 after a SPLIT_F16 forward (see "ONE ARITHMETIC PER STEP" above).  The no-grad chain has no workspace: beyond the limit
 * its outputs are NaN (never finite garbage). */
int dh_range_words(int64_t* act_max_off, int64_t* tag_off, float* limit);

/* The MLP part of upstream NeuSRenderer.render_core (App. A.7) on npts points (point i belongs to ray
 * i / n_per_ray): sdf_network(pts) -> sdf [npts], feature (kept in ws); sdf_network.gradient(pts) -> normals
 * [npts,3]; color_network(pts, normals, dirs, feature) -> color [npts,3] (post-sigmoid).  Saves what
 * dh_mlp_backward needs into ws. */
int dh_mlp_forward(const float* packed, const float* pts, const float* dirs, int n_per_ray, int64_t npts, float* ws,
                   float* sdf, float* normals, float* color, void* stream);

/* The three stages of dh_mlp_forward as separate single-kernel launches (same ws); save = 0 skips the stores that only
 * the backward pass needs (forward-only rendering: validate_image). */
int dh_sdf_forward(const float* packed, const float* pts, int64_t npts, float* ws, float* sdf, void* stream);
int dh_sdf_gradient(const float* packed, const float* pts, int64_t npts, float* ws, float* normals, int save, void* stream);
int dh_color_forward(const float* packed, const float* pts, const float* dirs, int n_per_ray, const float* normals,
                     int64_t npts, float* ws, float* color, int save, void* stream);

/* Adjoint of dh_mlp_forward (autograd of upstream render_core's network calls, incl. the second-order path through
 * sdf_network.gradient's create_graph=True): given d_sdf [npts], d_normals [npts,3] (updated in place with the colour
 * network's contribution) and d_colors [npts,3] (wrt the post-sigmoid colour), writes the gradient of every network
 * parameter (weight-norm folded: bias, weight_g, weight_v) into grad_flat [dh_num_params()] (the variance entry is
 * left untouched).  ws must be the workspace dh_mlp_forward filled; packed/params the weights it used. */
int dh_mlp_backward(const float* packed, const float* params, const float* pts, int64_t npts, float* ws,
                    const float* colors, const float* d_sdf, float* d_normals, const float* d_colors, float* grad_flat,
                    void* stream);

/* The four stages of dh_mlp_backward as separate launches (same ws, in this order): colour-network backward
 * (adds its d/d normal into d_normals), the forward-mode tangent chain of the second-order path, the SDF backward
 * chain, the split-K weight-gradient GEMMs (one kernel), and their reduction + weight-norm fold into grad_flat. */
int dh_color_backward(const float* packed, const float* colors, const float* d_colors, int64_t npts, float* ws,
                      float* d_normals, void* stream);
int dh_sdf_tangent(const float* packed, const float* pts, const float* d_normals, int64_t npts, float* ws, void* stream);
int dh_sdf_backward(const float* packed, const float* d_sdf, int64_t npts, float* ws, void* stream);
/* Pose refinement (per-frame object poses as trainable cameras; reference precedent for the 6-D
 * rotation + translation parameters and their optimiser: ObjTracker/utils/geometry.py:7-25, jointopt.py:125-141).  The same two
 * stages as above, additionally producing d loss / d sample point (d_pts [npts,3]) and, for the colour network's view embedding,
 * d loss / d ray direction per point (d_dirs_pts [npts,3]).  Call order: dh_sdf_gradient(save = 2) in the forward (keeps the
 * embedding-gradient vector in ws), then dh_color_backward_rays (WRITES d_pts, d_dirs_pts) -> dh_sdf_tangent ->
 * dh_sdf_backward_rays (ACCUMULATES onto d_pts, incl. the second-order path) -> weight-gradient stages as usual.  The caller
 * reduces per ray: d_rays_o = sum_k d_pts, d_rays_d = sum_k (mid_k d_pts + d_dirs_pts) + dh_render_scan_bwd_rays' d_rays_d;
 * sample depths are treated as constants.  Both arithmetic modes (round 3: the fp32-MFMA twins have the same variants). */
int dh_color_backward_rays(const float* packed, const float* colors, const float* d_colors, const float* dirs, int n_per_ray,
                           int64_t npts, float* ws, float* d_normals, float* d_pts, float* d_dirs_pts, void* stream);
int dh_sdf_backward_rays(const float* packed, const float* d_sdf, const float* pts, const float* d_normals, int64_t npts,
                         float* ws, float* d_pts, void* stream);
/* Weight gradients, two launches: _gemm writes the split-K slabs AND the reduced tile partials (bias gradients; its workgroups take
 * that reduction behind their GEMM jobs), _fold reduces the slabs and folds the weight norm.  _fold therefore follows a _gemm on
 * the same workspace with the tile partials unchanged in between. */
int dh_weight_grads_gemm(int64_t npts, float* ws, void* stream);
int dh_weight_grads_fold(const float* packed, const float* params, int64_t npts, float* ws, float* grad_flat, void* stream);

/* The same MLP stages with the arithmetic passed explicitly (a dh_arithmetic value; DH_ERR_BAD_ARG otherwise): no launch
 * depends on process-global state (SURVEY.md section 8b "re-entrant; no global mutable state").  Arguments after the first
 * are those of the entry point of the same name above.  (dh_pack_weights and dh_weight_grads_fold do not depend on the
 * arithmetic.) */
int dh_sdf_nograd_ex(int arithmetic, const float* packed, const float* pts, int64_t npts, float* sdf, void* stream);
int dh_mlp_forward_ex(int arithmetic, const float* packed, const float* pts, const float* dirs, int n_per_ray, int64_t npts, float* ws,
                      float* sdf, float* normals, float* color, void* stream);
int dh_sdf_forward_ex(int arithmetic, const float* packed, const float* pts, int64_t npts, float* ws, float* sdf, void* stream);
int dh_sdf_gradient_ex(int arithmetic, const float* packed, const float* pts, int64_t npts, float* ws, float* normals, int save,
                       void* stream);
int dh_color_forward_ex(int arithmetic, const float* packed, const float* pts, const float* dirs, int n_per_ray, const float* normals,
                        int64_t npts, float* ws, float* color, int save, void* stream);
int dh_mlp_backward_ex(int arithmetic, const float* packed, const float* params, const float* pts, int64_t npts, float* ws,
                       const float* colors, const float* d_sdf, float* d_normals, const float* d_colors, float* grad_flat,
                       void* stream);
int dh_color_backward_ex(int arithmetic, const float* packed, const float* colors, const float* d_colors, int64_t npts, float* ws,
                         float* d_normals, void* stream);
int dh_sdf_tangent_ex(int arithmetic, const float* packed, const float* pts, const float* d_normals, int64_t npts, float* ws,
                      void* stream);
int dh_sdf_backward_ex(int arithmetic, const float* packed, const float* d_sdf, int64_t npts, float* ws, void* stream);
int dh_color_backward_rays_ex(int arithmetic, const float* packed, const float* colors, const float* d_colors, const float* dirs,
                              int n_per_ray, int64_t npts, float* ws, float* d_normals, float* d_pts, float* d_dirs_pts, void* stream);
int dh_sdf_backward_rays_ex(int arithmetic, const float* packed, const float* d_sdf, const float* pts, const float* d_normals,
                            int64_t npts, float* ws, float* d_pts, void* stream);
int dh_weight_grads_gemm_ex(int arithmetic, int64_t npts, float* ws, void* stream);
/* dh_pack_weights for ONE arithmetic: the row scales, biases and small fp32 vectors every arithmetic reads plus that arithmetic's
 * MFMA operands only (a training step then packs one operand set instead of three). */
int dh_pack_weights_ex(int arithmetic, const float* params, float* packed, void* stream);

/* ---- per-ray stages ---------------------------------------------------------------------------------------
 * Mask-conditioned ray generation = upstream Dataset.gen_random_rays_at + near_far_from_sphere (App. A.8) under the
 * reference's hand-off conventions: K per ObjTracker/run.py:119-123 (Kinv = its inverse, row-major [9]); pose
 * x_cam = R x_obj + T per run.py:166 / vis.py:52 (R [F,9] row-major, T [F,3]); label map 1 object / 0 background /
 * -1 hand per run.py:66 and utils/maskutils.py:24-28; obj = label>0, keep = label>=0 per pose_initializtion.py:60-61.
 * Frames stay resident in HBM: rgb u8 [F,H,W,3], label i8 [F,H,W], normal u8 [F,H,W,3] (n = u8/255*2-1, camera frame).
 * rays [B,14] = o(3) d(3) rgb(3) obj(1) keep(1) mono_normal(3); near/far [B]. */
int dh_gen_rays(const uint8_t* rgb, const int8_t* label, const uint8_t* normal, const float* R, const float* T,
                const float* Kinv, int H, int W, int n_frames, int frame, const int64_t* px, const int64_t* py, int64_t B,
                float* rays, float* near, float* far, void* stream);

/* coarse z = near + (far-near) linspace(0,1,n) + (t_rand-0.5)*2/n (t_rand [B] or NULL) and pts = o + d z
 * (upstream NeuSRenderer.render, App. A.5). */
int dh_coarse_samples(const float* rays_o, const float* rays_d, const float* near, const float* far, const float* t_rand,
                      int64_t B, int n_samples, float* z, float* pts, void* stream);

/* upstream NeuSRenderer.up_sample + sample_pdf(det=True) (App. A.6): z,sdf [B,n_cur] -> z_new [B,n_new] and
 * pts_new [B*n_new,3].  n_cur <= 128, n_new <= 64. */
int dh_upsample_step(const float* rays_o, const float* rays_d, const float* z, const float* sdf, int64_t B, int n_cur,
                     int n_new, float inv_s, float* z_new, float* pts_new, void* stream);

/* upstream NeuSRenderer.cat_z_vals (App. A.6): stable sorted merge; sdf gathered alongside unless sdf_out is NULL
 * (the `last` step). */
int dh_merge_samples(const float* z, const float* z_new, const float* sdf, const float* sdf_new, int64_t B, int n_cur,
                     int n_new, float* z_out, float* sdf_out, void* stream);

/* section mid-points of render_core (App. A.7): pts [B*n,3] = o + d (z + dists/2). */
int dh_midpoints(const float* rays_o, const float* rays_d, const float* z, int64_t B, int n, float sample_dist, float* pts,
                 void* stream);

/* render_core tail (App. A.7): alpha from (sdf, normals, inv_s[0], cos_anneal), transmittance scan, compositing.
 * weights/cdf/inside_sphere [B,n]; color [B,3]; weight_sum/weight_max [B]; eik_partial [B,2] = per-ray
 * (sum relax*(|n|-1)^2, sum relax); normal_map [B,3] = sum_j w_j n_j (object frame) or NULL.  n <= 128.
 * background_rgb [3] or NULL. */
int dh_render_scan_fwd(const float* rays_o, const float* rays_d, const float* z, const float* sdf, const float* normals,
                       const float* colors, const float* inv_s, float cos_anneal_ratio, float sample_dist,
                       const float* background_rgb, int64_t B, int n, float* weights, float* color, float* weight_sum,
                       float* weight_max, float* cdf, float* inside_sphere, float* eik_partial, float* normal_map,
                       void* stream);

/* adjoint of dh_render_scan_fwd.  d_weight_sum, d_weights [B,n], d_gradients [B*n,3], d_normal_map [B,3] may be NULL; eik_coef[0] =
 * d(loss)/d(gradient_error) / (sum relax + 1e-5).  d_inv_s [B] holds per-ray partial sums. */
int dh_render_scan_bwd(const float* rays_o, const float* rays_d, const float* z, const float* sdf, const float* normals,
                       const float* colors, const float* inv_s, float cos_anneal_ratio, float sample_dist,
                       const float* background_rgb, int64_t B, int n, const float* d_color, const float* d_weight_sum,
                       const float* d_weights, const float* d_gradients, const float* d_normal_map, const float* eik_coef,
                       float* d_sdf, float* d_normals, float* d_colors, float* d_inv_s, void* stream);
/* The same, additionally d_rays_d [B,3] = d loss / d rays_d through true_cos = d . n (pose refinement). */
int dh_render_scan_bwd_rays(const float* rays_o, const float* rays_d, const float* z, const float* sdf, const float* normals,
                            const float* colors, const float* inv_s, float cos_anneal_ratio, float sample_dist,
                            const float* background_rgb, int64_t B, int n, const float* d_color, const float* d_weight_sum,
                            const float* d_weights, const float* d_gradients, const float* d_normal_map, const float* eik_coef,
                            float* d_sdf, float* d_normals, float* d_colors, float* d_inv_s, float* d_rays_d, void* stream);

/* Loss stack of the training step (upstream Runner.train, App. A.8, with Dynhor's hand gating): rays [B,14] as
 * written by dh_gen_rays; m = obj*keep (the keep-mask gating precedent: reference ObjTracker/utils/losses.py:69-71,
 * pose_initializtion.py:60-65,148-150).
 *   colour L1 over m / (sum m + 1e-5); eikonal = sum eik_partial[:,0] / (sum eik_partial[:,1] + 1e-5);
 *   mask BCE(clip(weight_sum,1e-3,1-1e-3), obj) over keep / (sum keep + 1e-5);
 *   normal (if normal_weight > 0): L1 + (1 - cos) between normalize(R normal_map) and the monocular normal over m.
 * stats[8] = loss, colour, eikonal, mask, normal, psnr, sum m, sum keep.  Also writes the adjoints d_color [B,3],
 * d_weight_sum [B], d_normal_map [B,3] and eik_coef[0] = igr_weight / (sum relax + 1e-5) for dh_render_scan_bwd. */
int dh_neus_loss(const float* color, const float* weight_sum, const float* normal_map, const float* eik_partial,
                 const float* rays, const float* R, int64_t B, float igr_weight, float mask_weight, float normal_weight,
                 float* stats, float* d_color, float* d_weight_sum, float* d_normal_map, float* eik_coef, void* stream);

/* Dense-correspondence reprojection term of the full loss stack (BASELINE.json configs[4]; reference README.md:43 names the
 * input folder `correspondence_infos` "obtained using DKM for reconstruction and outlier-voting" and nothing else, so the form
 * is this build's specification -- oracle/neus_oracle.py:correspondence_loss, DESIGN.md section 9, parity unpinned):
 *   corr [B,4] = (u_j, v_j, certainty, frame_j) per ray, certainty 0 = no match; poses x_cam = R x_obj + T of all n_frames
 *   frames (reference ObjTracker/run.py:166), K [3,3] row-major (run.py:119-123).
 *   t^ = sum_k weights[r,k] m_k (m = mid-point depths of z as in dh_render_scan_fwd), x = o + t^ d, pi = K (R_j x + T_j),
 *   s = |pi - (u_j,v_j)| / fx, rho = Huber(s; delta_px / fx), L = sum c v rho / (sum c v + 1e-5), v = [depth in camera j > 1e-3].
 * stats[4] = L, sum c v, certainty-weighted mean residual in pixels, corr_weight * L.  residual_px [B] feeds the outlier voting
 * (host side): 0 for rays without a match (certainty 0), +inf for a match that cannot be evaluated (partner frame out of range,
 * point behind the partner camera: a gross failure that must vote as an outlier).  d_weights [B,n] = d (corr_weight * L) / d
 * weights, written for EVERY ray (zeros where there is no match): pass it to dh_render_scan_bwd as d_weights.
 * pose_adjoints (may be null; [B,7], pose refinement together with this term): per ray d (corr_weight L) / d x [3] (x = o + t^ d
 * with t^ held fixed: the dependence of t^ on the geometry is what d_weights carries), d (corr_weight L) / d y [3] (y = R_j x +
 * T_j: the partner frame's pose gradient is sum_rays d_y x^T and sum_rays d_y) and t^. */
int dh_corr_loss(const float* rays_o, const float* rays_d, const float* z, const float* weights, const float* corr,
                 const float* R_all, const float* T_all, int n_frames, const float* K, int64_t B, int n, float sample_dist,
                 float delta_px, float corr_weight, float* stats, float* residual_px, float* d_weights, float* pose_adjoints,
                 void* stream);

/* ---- occupancy-grid ray marching, packed variable-length rays (BASELINE.json configs[3]) -------
 * The sampler of the instant-nsr-pl variant the reference names as its direction (README.md:11,13; code on an unmounted
 * branch; it calls nerfacc's OccupancyGrid / ray_marching).  Specification: oracle/occgrid_oracle.py (parity unpinned).
 *   occupancy: res^3 bytes (non-zero = occupied) over the cube [-radius, radius]^3, cell (ix,iy,iz) at (ix*res + iy)*res + iz.
 *   Step k of ray r is [t_k, t_k + step], t_k = near + (k + u[r]) step (u: one stratified offset per ray, null = 0.5); it is a
 *   sample iff t_k + step <= far and the cell of its mid-point is occupied; at most max_samples (<= 1024) per ray, front to back.
 *   half_step = (float)(0.5 * step) as the caller rounds it (kept separate so host and device agree bit for bit).
 * dh_march_count -> cnt [B]; the caller forms off = exclusive prefix sum (int64) and N = sum cnt, then dh_march_emit writes
 * t_start [N], the mid-point positions pts [N,3], the ray direction per sample dirs_pts [N,3] (pass it as `dirs` with
 * n_per_ray = 1 to the colour stages) and ray_idx [N].  No atomics: the packed order is a pure function of the inputs.
 * dh_march_emit's `keep` (device, [B], may be null): ray r emits only its first min(keep[r], max_samples) samples -- the caller
 * may lower the counts on the device (e.g. a per-ray cap chosen so that the total fits a fixed capacity) between the two calls
 * without reading them back. */
int dh_march_count(const float* rays_o, const float* rays_d, const float* near, const float* far, const float* u,
                   const uint8_t* occupancy, int res, float radius, float step, float half_step, int max_samples, int64_t B,
                   int32_t* cnt, void* stream);
int dh_march_emit(const float* rays_o, const float* rays_d, const float* near, const float* far, const float* u,
                  const uint8_t* occupancy, int res, float radius, float step, float half_step, int max_samples, int64_t B,
                  const int64_t* off, const int32_t* keep, float* t_start, float* pts, float* dirs_pts, int32_t* ray_idx,
                  void* stream);
/* dh_render_scan_fwd / _bwd over packed rays: ray r owns samples [seg_off[r], seg_off[r] + seg_cnt[r]) of the packed arrays
 * (seg_cnt <= 1024: the wave takes 128 samples per trip and carries the transmittance), every interval is `step` long and
 * t_start holds the interval starts; per-sample outputs are packed too. */
int dh_render_scan_fwd_packed(const float* rays_o, const float* rays_d, const float* t_start, const float* sdf, const float* normals,
                              const float* colors, const float* inv_s, float cos_anneal_ratio, float step,
                              const float* background_rgb, int64_t B, const int64_t* seg_off, const int32_t* seg_cnt,
                              float* weights, float* color, float* weight_sum, float* weight_max, float* cdf,
                              float* inside_sphere, float* eik_partial, float* normal_map, void* stream);
int dh_render_scan_bwd_packed(const float* rays_o, const float* rays_d, const float* t_start, const float* sdf, const float* normals,
                              const float* colors, const float* inv_s, float cos_anneal_ratio, float step,
                              const float* background_rgb, int64_t B, const int64_t* seg_off, const int32_t* seg_cnt,
                              const float* d_color, const float* d_weight_sum, const float* d_weights, const float* d_gradients,
                              const float* d_normal_map, const float* eik_coef, float* d_sdf, float* d_normals, float* d_colors,
                              float* d_inv_s, void* stream);
/* Pose refinement on packed rays.  dh_render_scan_bwd_packed_rays = dh_render_scan_bwd_packed + d_rays_d [B,3] (written): the adjoint
 * of the ray direction through true_cos = d . n, as dh_render_scan_bwd_rays forms it on dense rays; every shared output is bitwise that
 * of dh_render_scan_bwd_packed.  dh_ray_adjoint_packed folds the per-point adjoints of the network stages into the rays: with
 * t_k = t_start_k + step / 2, the marcher's mid-point x_k = o + t_k d (sample depths are constants),
 *   d_rays_o [B,3] = sum_k d_pts_k (written),   d_rays_d_accum [B,3] += sum_k (t_k d_pts_k + d_dirs_pts_k)
 * over the samples of each ray (seg_cnt read on the device and clamped to 1024 like the scan's).  One wave per ray, fp64 sums in a fixed
 * order, no atomics: bitwise reproducible; a ray without samples gets zeros in d_rays_o and keeps d_rays_d_accum.  B == 0 is a no-op. */
int dh_render_scan_bwd_packed_rays(const float* rays_o, const float* rays_d, const float* t_start, const float* sdf, const float* normals,
                                   const float* colors, const float* inv_s, float cos_anneal_ratio, float step,
                                   const float* background_rgb, int64_t B, const int64_t* seg_off, const int32_t* seg_cnt,
                                   const float* d_color, const float* d_weight_sum, const float* d_weights, const float* d_gradients,
                                   const float* d_normal_map, const float* eik_coef, float* d_sdf, float* d_normals, float* d_colors,
                                   float* d_inv_s, float* d_rays_d, void* stream);
int dh_ray_adjoint_packed(const float* d_pts, const float* d_dirs_pts, const float* t_start, float step, const int64_t* seg_off,
                          const int32_t* seg_cnt, int64_t B, float* d_rays_o, float* d_rays_d_accum, void* stream);

/* Priors that carry a validity, on the training path: a depth term on the expected depth of a ray and the normal term of
 * dh_neus_loss restricted to the rays that have a normal (DESIGN_NEXT_ROWS.md section 27).  dh_prior_loss takes dense rays
 * (z, weights [B,n], sample_dist as dh_corr_loss takes them), dh_prior_loss_packed the occupancy-grid sampler's packed rays
 * (t_start, step, seg_off, seg_cnt as dh_render_scan_bwd_packed takes them; max_samples is the caller's per-ray cap, the one
 * dh_march_count took: a ray's samples past it are not read).  rays [B,14] as dh_gen_rays writes them (3..5 = d, 9 = obj,
 * 10 = keep, 11..13 = the monocular normal), R [9] the frame's object->camera rotation, prior_depth [B] camera z.
 *   depth   m_k = z_k + 0.5 (z_{k+1} - z_k), sample_dist for the last sample (dh_render_scan_fwd, dh_corr_loss); packed:
 *           m_k = t_start_k + 0.5 step, the packed scan's own (m_k is fp32).  t^ = sum_k w_k m_k in fp64 (each lane of a wave adds
 *           its samples lane, lane + 64, .. in ascending k with fma, then the 64 lanes fold in a fixed xor butterfly), c_z = R[6] d_0 +
 *           R[7] d_1 + R[8] d_2, z^ = t^ c_z (dh_trace_compose's t (R d)_z: since R o + T = 0 this is the camera z of o + t^ d); c_z, e,
 *           rho and rho' are fp64 of the fp32 inputs too -- e is what is left of two depths -- and the ray's coefficient rho'(e) c_z is
 *           rounded to fp32.
 *           v = [obj * keep > 0] [1e-3 < prior < inf] (inf, NaN and values <= 1e-3 mean "no prior"); packed: and the ray has a sample.
 *           e = z^ - prior, rho = e^2 / (2 delta) if |e| <= delta else |e| - delta / 2 (dh_corr_loss's Huber form, slope 1 outside),
 *           L_d = sum v rho / (sum v + 1e-5).
 *           d_weights[b,k] = depth_weight v rho'(e) c_z / (sum v + 1e-5) m_k.  accumulate == 0: written for every sample of every
 *           ray, exact zeros where v = 0.  accumulate != 0: added to what the buffer holds (stack it on dh_corr_loss's output);
 *           rays whose coefficient is 0 are not touched, so depth_weight 0 leaves the buffer's bits as they are.
 *   normal  (normal_map not null) dh_neus_loss's L1 + (1 - cos) between normalize(R normal_map) and the monocular normal,
 *           operation by operation, with the weight q = obj keep [mono_0^2 + mono_1^2 + mono_2^2 >= 0.25] (grey 128 decodes to a
 *           squared norm of 4.6e-5, an encoded unit normal to at least (1 - sqrt(3)/255)^2) and the normaliser sum q + 1e-5.
 *           d_normal_map [B,3] (normal_weight > 0 and not null; untouched otherwise) is written for every ray, exact zeros where q = 0.
 * stats[8] = L_d, sum v, sum v |e| / (sum v + 1e-5), depth_weight L_d, the masked normal loss, sum q (its ray count),
 * normal_weight * that loss, 0.  The first three and [4], [5] do not depend on the weights: at weight 0 the call scores a ray set.
 * The batch sums are fp64 sums of the per-ray fp32 values in a fixed order (no atomics): a result is bitwise reproducible.
 * prior_depth null = no ray has a prior (z, weights, d_weights are then not read or written).  ws: dh_prior_loss_workspace(B)
 * bytes, 16-byte aligned.  B == 0 is a no-op; DH_ERR_BAD_ARG for a null pointer, a negative count, n < 1, depth_delta not > 0, a
 * weight that is negative or NaN; DH_ERR_UNSUPPORTED for max_samples > 1024 (seg_cnt lives on the device and is clamped to it).
 * Limits: t^ is NOT divided by sum_k w_k (MonoSDF and dh_corr_loss do the same): a ray whose weights sum to less than 1 reads
 * nearer than its surface. */
int64_t dh_prior_loss_workspace(int64_t B);
int dh_prior_loss(const float* rays, const float* R, const float* z, const float* weights, const float* normal_map,
                  const float* prior_depth, int64_t B, int n, float sample_dist, float depth_weight, float depth_delta,
                  float normal_weight, int accumulate, float* stats, float* d_weights, float* d_normal_map, void* ws, void* stream);
int dh_prior_loss_packed(const float* rays, const float* R, const float* t_start, const float* weights, const float* normal_map,
                         const float* prior_depth, int64_t B, const int64_t* seg_off, const int32_t* seg_cnt, int max_samples,
                         float step, float depth_weight, float depth_delta, float normal_weight, int accumulate, float* stats,
                         float* d_weights, float* d_normal_map, void* ws, void* stream);

/* Multi-view photometric consistency on the training path (DESIGN_NEXT_ROWS.md section 30): the grey patch about a ray's pixel is
 * carried into the neighbouring frames by the homography of the plane through the ray's surface point with the rendered normal and
 * scored by normalised cross-correlation; the mean of the best few 1 - score is the ray's loss, differentiated with respect to the
 * ray's depth and normal.  Pixel centres are integers, x is the column, dot(a, b) = (a0 b0 + a1 b1) + a2 b2 (the conventions of
 * dh_mvs_sweep below).  Poses and intrinsics are constants of the term.
 *
 * dh_ray_depth / dh_ray_depth_packed: the two sample layouts of dh_prior_loss / dh_prior_loss_packed, with its m_k.  Per ray, in
 *   fp64 of the fp32 inputs (each lane of a wave adds its samples lane, lane + 64, .. in ascending k, then a fixed xor butterfly):
 *   W = sum_k w_k, t = sum_k w_k m_k / W (0 when W is not > 0: a packed ray without a sample), z = t c_z with c_z = R[6] d_0 + R[7] d_1 +
 *   R[8] d_2; t [B], wsum [B], zc [B] are those three rounded to fp32.  The depth IS divided by W: a surface point is wanted, not
 *   an expected depth that reads near while the ray is not yet opaque.
 *
 * dh_warp_loss: gray, valid u8 [n_frames,H,W] (dh_match_gray); R f32 [n_frames,9], T f32 [n_frames,3]; K, Kinv f32 [9] in DEVICE
 *   memory; nbr int32 [n_frames,n_nbr] (an entry outside [0, n_frames): none), 1 <= n_nbr <= 8; frame = the frame i of the batch;
 *   pix int32 [B,2] = (px, py); z [B] camera depth, wsum [B], normal [B,3] = the rendered normal in the OBJECT frame (any length);
 *   P in 1..7 (N = (2P+1)^2); min_va >= 1; min_vb > 0; topk, min_views in 1..8; min_cos in [-1, 1].  Per ray:
 *   gate    flag 16 unless wsum >= min_wsum (a NaN fails).
 *   source  the N grey bytes a about (px, py) of frame i; flag 1 when one lies outside the image or is invalid, or when
 *           va = N sum a^2 - (sum a)^2 < min_va (exact integers).
 *   plane   p = (px, py, 1) as floats, e = Kinv p, e_r = (Kinv[r][0] px + Kinv[r][1] py) + Kinv[r][2]; n_c[r] = dot(R_i row r, n);
 *           ne = dot(n_c, e); flag 8 unless z is finite, z > 1e-3, |n_c| = sqrt(dot(n_c, n_c)) > 1e-6 and
 *           -ne / (|n_c| sqrt(dot(e, e))) >= min_cos (a NaN fails); g = z ne.  With any flag nothing more is done.
 *   tap     (c, r), c, r in [-P, P], row-major: x = float(px + c), y = float(py + r); u_r = (Kinv[r][0] x + Kinv[r][1] y) + Kinv[r][2];
 *           sigma = dot(n_c, u) / g.
 *   neighbour j = nbr[i][.]: R_ij[r][c] = dot(R_j row r, R_i row c), t_ij[r] = T_j[r] - dot(R_ij row r, T_i) (dh_mvs_sweep's);
 *           G = K R_ij, A = G Kinv (entry [r][c] = dot(row r, column c)), b_v[r] = dot(K row r, t_ij);
 *           h_r = ((A[r][0] x + A[r][1] y) + A[r][2]) + b_v[r] sigma; the tap needs h_2 > 1e-3; (tx, ty) = (h_0 / h_2, h_1 / h_2).
 *           All of this is fp32, every operation an IEEE operation as written (no contraction): floor tx, floor ty can be restated
 *           bit for bit.  The tap needs 0 <= tx < W - 1, 0 <= ty < H - 1 (a NaN fails) and its four pixels valid; wx, wy, top, bot and
 *           the bilinear value b are dh_mvs_sweep's fp32 operations.  A failing tap makes j invalid for the ray.
 *           sb = sum b, sb2 = sum b b, sab = sum a b are fp64 sums of the fp32 b (a lane adds its taps lane, lane + 64, .. in
 *           ascending order, then a fixed xor butterfly); from here on everything is fp64.  vb = N sb2 - sb sb; j is invalid unless
 *           vb >= min_vb; score_j = (N sab - sum a sb) / sqrt(va vb), l_j = 1 - score_j.
 *   ray     valid = the number of valid neighbours; flag 2 (alone) when valid < min_views.  Else the k = min(topk, valid) smallest
 *           l_j are chosen, the earlier entry of nbr on a tie, and l_r = their sum / k.  The sum (and those of the scores and gradients) runs
 *           over the eight entry slots of nbr, 0 in a slot not chosen, in one fixed tree: ((s0 + s4) + (s2 + s6)) + ((s1 + s5) + (s3 + s7)).
 *   gradient  the exact derivative at fixed floor tx, floor ty and a fixed choice: per tap s_t = d l_j / d b_t (grad b . d q / d sigma),
 *           d l_j / d b_t = score_j (N b_t - sb) / vb - (N a_t - sum a) / sqrt(va vb), grad b = ((g01 - g00) + wy ((g11 - g10) -
 *           (g01 - g00)), (g10 - g00) + wx ((g11 - g10) - (g01 - g00))), d q / d sigma = (b_v[0:2] - (tx, ty) b_v[2]) / h_2;
 *           g_z = -sum_t s_t sigma_t / z, g_nc = sum_t s_t (u_t / g - sigma_t e / ne), both averaged over the chosen,
 *           g_n = R_i^T g_nc (orthogonal to n by construction).  u_t / g - sigma_t e / ne is what is left of two nearly equal vectors:
 *           it is formed as (u_t - rho_t e) / g with rho_t = dot(n_c, u_t) / ne, sigma_t = rho_t / z, and e, n_c, ne, g, u_t in fp64 of the
 *           fp32 inputs; s_t is fp64 of the fp32 b_t, tx, ty, h_2.
 *   out_f f32 [B,8] = (l_r, g_z, g_n[3], the mean score of the chosen, the best score, 0); out_i int32 [B,4] = (valid, chosen count,
 *   flags, bitmask of the chosen entries of nbr).  A ray with a flag: (0, 0, 0, 0, 0, -2, -2, 0) and (valid, 0, flags, 0).
 *   stats f32 [8] = (L = sum l_r / max(count, 1), count, the mean over the counted rays of the chosen's mean score, warp_weight L,
 *   the rays with flag 1, with flag 2, with flag 8, with flag 16): fp64 sums of the per-ray fp32 values in block order, no atomics.
 *   A ray's outputs depend on that ray's inputs alone: bitwise the same from launch to launch and for every split of the batch into
 *   calls.  ws: dh_warp_loss_workspace(B) bytes, 16-byte aligned.  Runs on `stream` and does not wait for it.
 *
 * dh_ray_depth_bwd / dh_ray_depth_bwd_packed: the adjoint of z = t c_z and of the normal into the renderer's two channels, with
 *   s = warp_weight / max(stats[1], 1) read on the device: d_weights[r,k] gets c_r (m_k - t_r), c_r = fp32(s g_z c_z / W_r), and
 *   d_normal_map[r] gets fp32(s g_n); ray_f = dh_warp_loss's out_f, t, wsum = dh_ray_depth's.  accumulate bit 0: add to d_weights
 *   instead of writing it, bit 1: the same for d_normal_map; when adding, a ray whose coefficient is 0 is not touched; when
 *   writing, every sample of every ray is written, exact zeros for a ray that does not count.  Either pointer may be null.
 *
 * B == 0 is a no-op that writes nothing.  DH_ERR_BAD_ARG: a null or misaligned pointer, a negative count, n < 1, frame outside
 * [0, n_frames), P outside 1..7, n_nbr, topk or min_views outside 1..8, min_va < 1, a setting that is NaN or outside its range,
 * accumulate outside 0..3.  DH_ERR_UNSUPPORTED: max_samples > 1024, B or n_frames >= 2^31, H or W > 2^24.
 * Limits: no occlusion test beyond the top-k choice and the validity map; the surface point is the weight-normalised expected
 * depth, not a zero crossing; no pose or intrinsics adjoint. */
int dh_ray_depth(const float* rays, const float* R, const float* z, const float* weights, int64_t B, int n, float sample_dist, float* t,
                 float* wsum, float* zc, void* stream);
int dh_ray_depth_packed(const float* rays, const float* R, const float* t_start, const float* weights, int64_t B, const int64_t* seg_off,
                        const int32_t* seg_cnt, int max_samples, float step, float* t, float* wsum, float* zc, void* stream);
int64_t dh_warp_loss_workspace(int64_t B);
int dh_warp_loss(const uint8_t* gray, const uint8_t* valid, int64_t n_frames, int H, int W, const float* R, const float* T, const float* K,
                 const float* Kinv, const int32_t* nbr, int n_nbr, int frame, const int32_t* pix, const float* z, const float* wsum,
                 const float* normal, int64_t B, int P, int64_t min_va, float min_vb, int topk, int min_views, float min_cos,
                 float min_wsum, float warp_weight, float* out_f, int32_t* out_i, float* stats, void* ws, void* stream);
int dh_ray_depth_bwd(const float* rays, const float* R, const float* z, const float* t, const float* wsum, const float* ray_f,
                     const float* stats, int64_t B, int n, float sample_dist, float warp_weight, int accumulate, float* d_weights,
                     float* d_normal_map, void* stream);
int dh_ray_depth_bwd_packed(const float* rays, const float* R, const float* t_start, const float* t, const float* wsum, const float* ray_f,
                            const float* stats, int64_t B, const int64_t* seg_off, const int32_t* seg_cnt, int max_samples, float step,
                            float warp_weight, int accumulate, float* d_weights, float* d_normal_map, void* stream);

/* ---- optimiser -----------------------------------------------------------------------------------------
 * torch.optim.Adam step (upstream Runner uses Adam, App. A.8; the reference's own optimisers are Adam too:
 * ObjTracker/pose_initializtion.py:346, jointopt.py:135-141) fused over the flat vector; step counts from 1;
 * grad_scale multiplies the gradient first (1/world_size after a sum all-reduce). */
int dh_adam_step(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                 float beta2, float eps, int64_t step, float grad_scale, void* stream);

/* ---- multiresolution hash-grid encoding (BASELINE.json configs[3]) -------------------------
 * The instant-nsr-pl variant the reference names as its direction (README.md:11,13; code on an unmounted branch).
 * Fixed geometry: 16 levels x 2 features, 2^19 entries per hashed level, resolutions 16 .. 2049; dense indexing on the
 * levels whose grid fits the table.  table: [dh_hashgrid_entries(), 2] fp32; x01 [n,3] in [0,1]; out [n,32].
 * Backward ACCUMULATES into d_table with float atomics (caller zeroes it). */
int64_t dh_hashgrid_entries(void);
int dh_hashgrid_level(int level, float* scale, uint32_t* resolution, uint32_t* offset, uint32_t* dense);
int dh_hashgrid_encode(const float* table, const float* x01, int64_t n, float* out, void* stream);
int dh_hashgrid_encode_backward(const float* x01, const float* d_out, int64_t n, float* d_table, void* stream);

/* ---- hash-grid model family: fused encoding + small MLPs (BASELINE.json configs[3]) ---------
 * geometry: [2 x01 - 1 (3), hash encoding (32)] -> 64 softplus(100) -> 13 (out[0] = sdf, all 13 = feature), x01 =
 * (x + radius) / (2 radius); normals by central finite differences with step eps (instant-nsr-pl 'finite_difference').
 * colour: [feature(13), SH degree-4 of the view dir (16), normal(3)] -> 64 relu -> 64 relu -> 3 sigmoid.
 * All five linears are weight-normed.  Flat parameter vector: the table first, then per linear bias | g | v (see
 * dh_hash_param_layout), `variance` between the two networks.  `packed` (dh_hash_packed_floats) holds the effective
 * weights; refresh it with dh_hash_pack_weights whenever params change.
 * dh_hash_param_layout: net 0 = geometry (layers 0..1), 1 = variance, 2 = colour (layers 0..2), 3 = table
 * (v_off = offset, out_dim = entries, in_dim = 2). */
int64_t dh_hash_num_params(void);
int64_t dh_hash_packed_floats(void);
int dh_hash_param_layout(int net, int layer, int64_t* bias_off, int64_t* g_off, int64_t* v_off, int* out_dim, int* in_dim);
int dh_hash_pack_weights(const float* params, float* packed, void* stream);
/* workspace sizes (floats): *infer for dh_hash_geo_forward(save = 0), *total for a forward that a backward follows */
int dh_hash_workspace_floats(int64_t npts, int64_t* infer_floats, int64_t* total_floats);
/* sdf only (hierarchical up-sampling): pts [n,3] -> sdf [n] */
int dh_hash_sdf_nograd(const float* params, const float* packed, const float* pts, int64_t n, float radius, float* sdf,
                       void* stream);
/* sdf [n], feature [n,13], finite-difference gradient [n,3].  ws: caller-owned workspace (save = 0: *infer floats; save =
 * 1: *total floats, and the encodings of the 7 evaluations stay in it for the three backward calls below).
 * n_active (every stage of this family that takes it; device pointer to ONE int64, may be null): packed rays know their sample
 * count only on the device.  The caller then sizes buffers, workspace and n for a CAPACITY (a multiple of 8) and passes the
 * device-resident count: rows >= *n_active are neither read nor written and contribute nothing to any gradient, and no
 * device -> host read is needed.  All stages of one forward / backward must be given the same n and n_active. */
int dh_hash_geo_forward(const float* params, const float* packed, const float* pts, int64_t n, float radius, float eps,
                        float* ws, int save, float* sdf, float* feature, float* gradient, const int64_t* n_active, void* stream);
/* colour [n,3]; dirs [n / n_per_ray, 3] */
int dh_hash_color_forward(const float* packed, const float* feature, const float* normals, const float* dirs,
                          int n_per_ray, int64_t n, float* color, const int64_t* n_active, void* stream);
/* Adjoint, three calls in this order on the workspace dh_hash_geo_forward(save = 1) filled:
 *   colour   : d_color [n,3] -> d_feature [n,13] (written) and d_normals [n,3] (ACCUMULATED onto the caller's values)
 *   geometry : d_sdf [n], d_feature, d_normals (= cotangent of the finite-difference gradient)
 *   weights  : every parameter gradient -> grad [dh_hash_num_params()] (table part zeroed then scattered with float
 *              atomics: order-dependent in the last bits, unlike the NeuS fp32 path); the variance slot is left untouched */
int dh_hash_color_backward(const float* packed, const float* feature, const float* normals, const float* dirs,
                           const float* d_color, int n_per_ray, int64_t n, float* ws, float* d_feature, float* d_normals,
                           const int64_t* n_active, void* stream);
int dh_hash_geo_backward(const float* params, const float* packed, const float* pts, const float* d_sdf,
                         const float* d_feature, const float* d_normals, int64_t n, float radius, float eps, float* ws,
                         const int64_t* n_active, void* stream);
int dh_hash_weight_grads(const float* params, const float* packed, int64_t n, float* ws, float* grad, const int64_t* n_active,
                         void* stream);
/* Pose refinement: the same two calls, which also leave the adjoints w.r.t. the view direction and the sample point.  Every other
 * output and every workspace row is bitwise what dh_hash_color_backward / dh_hash_geo_backward write, so dh_hash_weight_grads follows
 * unchanged.  No float atomics: both results are bitwise the same from launch to launch.  Rows >= *n_active are not touched.
 *   dh_hash_color_backward_rays: d_dirs_pts [n,3], one row PER POINT (written): the first layer's input adjoint of the 16 SH columns
 *       chained through the analytic gradient of the SH-4 polynomials (plain polynomials of an unnormalised direction).  The caller sums
 *       the n_per_ray rows of a ray; with n_per_ray = 1 a row is the sample's own direction.
 *   dh_hash_geo_backward_rays: d_pts [n,3] (written) = d loss / d x of the sample point x through the E = 7 evaluations x_e (centre,
 *       +-eps per axis; d x_e / d x = I) with din_e the adjoint of evaluation e's 35 inputs:
 *         the xyz inputs   in[c] = x_c / radius:            (1 / radius) sum_e din_e[0..2]
 *         the 16 levels    pos = x01 scale_l + 0.5:         sum_e sum_l (scale_l / (2 radius)) sum_corners (d w_corner / d pos) <table[corner], din_e[l]>
 *       -- the derivative of the trilinear blend inside the cell; floor has derivative 0, so the result jumps at cell faces (the value
 *       does not).  ONE call launches two kernels: the geometry adjoint, which also adds up the xyz share, and a gather of one
 *       thread per point that walks the 16 levels in ascending order (per level the gathers of the forward's encoder: the centre cell's 8
 *       corners once, a shifted evaluation re-using them or the shared face) and adds them on top.  It needs no workspace of its own. */
int dh_hash_color_backward_rays(const float* packed, const float* feature, const float* normals, const float* dirs,
                                const float* d_color, int n_per_ray, int64_t n, float* ws, float* d_feature, float* d_normals,
                                const int64_t* n_active, float* d_dirs_pts, void* stream);
int dh_hash_geo_backward_rays(const float* params, const float* packed, const float* pts, const float* d_sdf,
                              const float* d_feature, const float* d_normals, int64_t n, float radius, float eps, float* ws,
                              const int64_t* n_active, float* d_pts, void* stream);
/* The same in two parts, for data-parallel callers: parts & 1 writes the table gradient (the leading dh_hashgrid_entries() x 2 floats
 * of grad: 49 MB), parts & 2 the five small linears.  Calling the table part, starting its all-reduce on a side stream, then the
 * linears, hides the large collective behind the small weight-gradient GEMMs (dynhor_amd/hash_fields.py).
 * parts & 4 selects how the table scatter adds.  Set (5, 7; dh_hash_weight_grads = 7): every contribution is converted to 2^-48 fixed
 * point and added by an INTEGER atomic to an int64 accumulator in the workspace (dh_hash_workspace_floats counts it), converted to
 * float once -- integer addition is associative, so the result is bit-identical from launch to launch; resolution 3.6e-15.  Range: one
 * contribution below 64, a sum exact up to +-16,384 (256 same-signed contributions at the limit).  A non-finite contribution or one
 * beyond 64 turns the WHOLE table gradient into NaN; an entry whose accumulator ends at |sum| >= 16,384 is NaN itself (the guard band
 * covers every true sum up to 3 x that; a finite wrong value would need more than 768 same-signed contributions at the
 * limit on one entry).  Same speed as the float form on MI355X (both are bound by the memory side's atomic request rate).  Clear (1,
 * 3): float atomics, whose sums depend on the order in which the memory side sees the requests (last-bit differences from launch to
 * launch: the only such sums in the library; kept for comparison).  The merge ablations of dh_hash_set_scatter_mode apply to the float
 * form only: with bit 4 set and a scatter mode other than 0 selected the call returns DH_ERR_BAD_ARG instead of ignoring the mode. */
int dh_hash_weight_grads_parts(const float* params, const float* packed, int64_t n, float* ws, float* grad, const int64_t* n_active,
                               int parts, void* stream);
/* Diagnosis only (scripts/psnr_parity.py ablations): how the FLOAT-atomic table scatter (dh_hash_weight_grads_parts with parts 1 or
 * 3) merges table-gradient adds before they reach memory.  0 (default, shipping) = 7-evaluation blending + ray-run merging + quad-lane
 * packing; 1 = no ray-run merging; 2 = neither (one atomic per evaluation corner, tcnn's scheme).  Same sums up to float-atomic
 * ordering.  The fixed-point form (parts bit 4, dh_hash_weight_grads) always merges: it refuses to run while a mode other than 0 is
 * selected (DH_ERR_BAD_ARG). */
int dh_hash_set_scatter_mode(int mode);

/* ---- nearest-neighbour squared distance (mesh evaluation: dynhor_amd/metrics.py, Chamfer distance / F-score) -------------------
 * For each of nq query points q[i] (float3, row-major [nq,3]): d2[i] = min_j |q[i] - ref[j]|^2 over the nr reference points and,
 * if idx != NULL, idx[i] = the smallest j that attains it.  Exact fp32 difference form, one operation order for every pair:
 * dx = q.x - r.x (dy, dz alike), d = fma(dz, dz, fma(dy, dy, dx * dx)) -- never the expanded |q|^2 - 2 q.r + |r|^2, which cancels.
 * Bitwise reproducible (ascending sweep with a strict <, no atomics).  A query whose every distance is +inf or NaN gets d2 = +inf and
 * idx = -1.  nq == 0: no-op.
 * ws: caller-owned scratch of dh_nearest_sqdist_workspace(nq, nr) bytes (16-byte aligned) for the slab-split path, which fills the
 * GPU when nq is small by cutting the reference range into slabs and merging their (d2, idx) pairs deterministically -- the result
 * is bit-identical to the one-slab sweep; NULL = one slab.  dh_nearest_sqdist_workspace returns 0 where one slab is used anyway,
 * DH_ERR_BAD_ARG for a negative count.
 * DH_ERR_BAD_ARG: null pointer, negative count, nr == 0 with nq > 0.  DH_ERR_UNSUPPORTED: nr >= 2^31. */
int64_t dh_nearest_sqdist_workspace(int64_t nq, int64_t nr);
int dh_nearest_sqdist(const float* q, int64_t nq, const float* ref, int64_t nr, float* d2, int32_t* idx, void* ws, void* stream);

/* ---- signed distance to a triangle mesh (dynhor_amd/mesh_sdf.py: the template prior of the SDF warm start, sdf_init.py) -----------
 * dh_mesh_sdf_prepare: verts [nv,3] fp32, faces [nf,3] int32 -> rec, one record of dh_mesh_sdf_record_floats() (12) floats per face
 * (caller-owned, 16-byte aligned): corner a and |e0|^2, e0 = b - a and e0.e1, e1 = c - a and |e1|^2, whose sign bit marks a face that
 * adds exactly 0 to the winding sum.  A face with an index outside [0, nv) or a non-finite corner becomes a record that is never the
 * nearest face and adds 0 to the winding sum.  A zero-area face (the fp32 cross product of its edges is exactly zero: a repeated
 * corner always is) is kept as the segment, or point, between its two corners farthest apart: it counts for the distance and adds
 * exactly 0 to the winding sum; it never yields a NaN.  nf == 0: no-op.
 * dh_mesh_sdf_query: for each of n points pts [n,3] fp32:
 *   sqdist[i] = the squared distance to the closest point of any triangle (closest point by the corner / edge / interior regions,
 *               chosen with selects; the distance itself in the difference form |(p - a) - v e0 - w e1|^2, never an expanded one);
 *   face[i]   = the lowest face index that attains it (face may be NULL);
 *   wind[i]   = the generalised winding number sum_f omega_f(p) / 4 pi, omega = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| +
 *               (c.a)|b|) with a, b, c = corners - p in fp32, added in fp64 in ascending face order (wind may be NULL).
 * A non-finite point gets sqdist = +inf, face = -1, wind = 0.  n == 0: no-op.
 * The face range is swept in slabs of a fixed number of faces, so the slab boundaries depend on nf alone: all three outputs are the
 * same bits from launch to launch and however the points are chunked over launches (no atomics, no cross-lane operation).
 * ws: caller-owned scratch of dh_mesh_sdf_query_workspace(n, nf) bytes (16-byte aligned), required when that is not 0 (more than one
 * slab); the slabs' (sqdist, face) pairs merge lexicographically and their fp64 winding partials add, both in slab order.
 * DH_ERR_BAD_ARG: null pointer, negative count, misaligned rec / ws, nf == 0 with n > 0, ws NULL where scratch is needed.
 * DH_ERR_UNSUPPORTED: nf >= 2^31, nv >= 2^31 or n >= 2^31; more than 65535 slabs (nf > 33,553,920).  The cost is n x nf pairs: simplify a
 * template beyond about 10^5 faces first (dynhor_amd/mesh_simplify.py). */
int dh_mesh_sdf_record_floats(void);
int dh_mesh_sdf_prepare(const float* verts, int64_t nv, const int32_t* faces, int64_t nf, float* rec, void* stream);
int64_t dh_mesh_sdf_query_workspace(int64_t n, int64_t nf);
int dh_mesh_sdf_query(const float* rec, int64_t nf, const float* pts, int64_t n, float* sqdist, int32_t* face, float* wind, void* ws,
                      void* stream);

/* ---- similarity ICP (dynhor_amd/mesh_align.py: the ground-truth mesh registered to the reconstruction before it is scored) -------
 * dh_icp_correspond: dh_nearest_sqdist for H hypotheses at once, the query transformed on load.  xf [H,12] fp32: A row-major (9), then
 * t (3).  For source point p = src[i] and hypothesis h the query is, for every row r, x_r = fma(A_r2, p.z, fma(A_r1, p.y,
 * fma(A_r0, p.x, t_r))) in fp32; d2[h,i] and idx[h,i] ([H,N], both required) are then exactly what dh_nearest_sqdist returns for the
 * query x against tgt [M,3]: the same direct-form distance, the same smallest index among ties, the same -1 / +inf for a query without
 * a finite distance, bit for bit, with or without the slab split.  ws: dh_icp_correspond_workspace(N, M, H) bytes (16-byte aligned),
 * or NULL = one slab.  N == 0 or H == 0: no-op.
 * DH_ERR_BAD_ARG: null pointer, negative count, M == 0 with work to do.  DH_ERR_UNSUPPORTED: N or M >= 2^31, H > 65535.
 *
 * dh_icp_moments: for every hypothesis the fp64 sums of the closed-form update over the pairs with d2[h,i] <= thr[h] (thr [H] fp32 on
 * the device; a NaN distance or an index outside [0, M) is no pair).  origin_src, origin_tgt: [3] fp32 on the device (the clouds'
 * centroids: the products stay small).  tgt_normals == NULL, point-to-point, out [H,19] with p = src[i] - origin_src (NOT transformed)
 * and q = tgt[idx] - origin_tgt:  [0] count, [1..3] sum p, [4..6] sum q, [7..15] sum q p^T row-major, [16] sum |p|^2, [17] sum |q|^2,
 * [18] sum sqrt(d2).  tgt_normals [M,3] given, point-to-plane, out [H,36]: y = A_h p + t_h - origin_tgt (fp64 arithmetic on the fp32
 * xf), n the normal of target sample idx, J = (y x n, n, n . y), b = -n . (y - q):  [0..27] upper triangle of sum J^T J row by row,
 * [28..34] sum J^T b, [35] count.  dh_icp_moments_sums(plane) returns 19 / 36.  ws: dh_icp_moments_workspace(N, H, plane) bytes, always
 * required: every workgroup stores its partial there and a second kernel adds the partials in block order (no atomics: bitwise
 * reproducible).  H == 0: no-op; N == 0: out is zeroed.
 * DH_ERR_BAD_ARG: null pointer (ws included), negative count.  DH_ERR_UNSUPPORTED: as above. */
int64_t dh_icp_correspond_workspace(int64_t n, int64_t m, int64_t h);
int dh_icp_correspond(const float* src, int64_t n, const float* tgt, int64_t m, const float* xf, int64_t h, float* d2, int32_t* idx,
                      void* ws, void* stream);
int dh_icp_moments_sums(int plane);
int64_t dh_icp_moments_workspace(int64_t n, int64_t h, int plane);
int dh_icp_moments(const float* src, const float* tgt, const float* tgt_normals, const float* xf, const int32_t* idx, const float* d2,
                   const float* thr, const float* origin_src, const float* origin_tgt, int64_t n, int64_t m, int64_t h, double* out,
                   void* ws, void* stream);

/* ---- mesh cleaning (dynhor_amd/mesh_clean.py: silhouette culling with the object masks of every view, connected components) ----
 * dh_label_dilate: label i8 [n_frames,H,W] (1 object / 0 background / -1 hand, Dataset.label) -> keep u8 [n_frames,H,W]:
 * keep[f,y,x] = 1 if any pixel of the square window of half-width `radius` about (x,y), clipped to the image, has label != 0 (object
 * and hand both count as "not background": a hand pixel hides what lies behind it), else 0.  radius 0 = a copy of label != 0.
 * Two separable passes through the caller's tmp u8 [n_frames,H,W].  n_frames == 0: no-op.
 * DH_ERR_BAD_ARG: null pointer, negative n_frames or radius, H or W < 1.  DH_ERR_UNSUPPORTED: n_frames * H >= 2^31, W > 65535 * 256.
 *
 * dh_mesh_mask_votes: for each vertex v of verts [nv,3] and each frame f, x_cam = R_f v + T_f (R [n_frames,9] row-major, T
 * [n_frames,3]: Dataset.R / Dataset.T), u = (K0 . x_cam) / z, w = (K1 . x_cam) / z with K [3,3] row-major, one for the sequence
 * (z = x_cam[2]; the inverse of dh_gen_rays, whose ray of pixel (x,y) passes through K^-1 [x,y,1]).  v is SEEN in f when z > 0 and the
 * pixel (floor(u + 0.5), floor(w + 0.5)) lies inside the image (range-checked in fp32 before any integer conversion); a seen vertex
 * whose pixel has keep == 0 is a background vote.  seen[v] and bg_votes[v] (int32) count the frames: bitwise reproducible.
 * Dataset.T of a sequence read from disk is already T / obj_scale; a pinhole camera does not see that factor, so the pixels are those
 * of the on-disk poses.  fp32 in the order: c_r = fma(R_r2, z, fma(R_r1, y, R_r0 x)) + T_r; u = fma(K02, c2, fma(K01, c1, K00 c0)) / c2.
 * nv == 0: no-op.  DH_ERR_BAD_ARG: null pointer, negative count, H or W < 1.
 *
 * dh_mesh_components: connected components of the graph on nv vertices whose edges are the three edges of every face of faces
 * int64 [nf,3]: labels[v] (int32) = the smallest vertex index of v's component (independent of scheduling: bitwise reproducible);
 * a vertex in no face is its own component; a face with an index outside [0, nv) is ignored.  Lock-free union-find (agent-scope
 * atomics only while hooking) and then ceil(log2 nv) pointer-jumping launches: a bounded number of launches whatever the depth.
 * DH_ERR_BAD_ARG: null pointer, negative count.  DH_ERR_UNSUPPORTED: nv >= 2^31. */
int dh_label_dilate(const int8_t* label, int64_t n_frames, int H, int W, int radius, uint8_t* tmp, uint8_t* keep, void* stream);
int dh_mesh_mask_votes(const float* verts, int64_t nv, const uint8_t* keep, const float* R, const float* T, const float* K,
                       int64_t n_frames, int H, int W, int32_t* bg_votes, int32_t* seen, void* stream);
int dh_mesh_components(const int64_t* faces, int64_t nf, int64_t nv, int32_t* labels, void* stream);

/* ---- visual hull (dynhor_amd/visual_hull.py: the object's shape carved from the masks at the current poses; csrc/visual_hull.hip) ----
 * dh_hull_accumulate: pts f32 [n,3]; sd f32 [n_frames,H,W], the signed pixel distance of each frame of the chunk (negative on object
 * and hand pixels, clamped to a band); R [n_frames,9] row-major, T [n_frames,3], K [9] as for dh_mesh_mask_votes; frame0 = the global
 * index of the chunk's first frame.  Per point p and frame f, in fp32: c = R_f p + T_f and (u, w) in dh_mesh_mask_votes' fma order;
 * p is seen when c_2 > 1e-6 and 0 <= u <= W - 1 and 0 <= w <= H - 1 (false for a NaN); x0 = min(floor(u), W - 2), y0 = min(floor(w),
 * H - 2), fx = u - x0, fy = w - y0; top = fma(fx, s01 - s00, s00), bot = fma(fx, s11 - s10, s10), val = fma(fy, bot - top, top) over
 * the taps s00 = sd[f, y0, x0], s01 = sd[f, y0, x0 + 1], s10 = sd[f, y0 + 1, x0], s11 = sd[f, y0 + 1, x0 + 1]; g = ((val c_2) / K00) + 0.
 * State per point, carried from call to call: topk f32 [n,m] = the m largest g of the frames that see p, descending (the caller
 * starts it at -inf); arg int32 [n] = frame0 + f of the largest value, the lower frame on exactly equal values (starts at -1);
 * seen int32 [n] = the frames that see p (starts at 0).  All three depend on the multiset of frames alone: every split of the
 * frames into calls, in any order, gives the same bits.  No atomics; the library allocates nothing and keeps no state.
 * n == 0 or n_frames == 0: no-op.  DH_ERR_BAD_ARG: null pointer, negative count, negative frame0, H or W < 2, m outside 1..8.
 * DH_ERR_UNSUPPORTED: H or W > 2^24, n >= 2^31 * 256, frame0 + n_frames > 2^31 - 1, n_frames H W > 2^58. */
int dh_hull_accumulate(const float* pts, int64_t n, const float* sd, const float* R, const float* T, const float* K, int64_t n_frames,
                       int H, int W, int frame0, int m, float* topk, int32_t* arg, int32_t* seen, void* stream);

/* ---- mesh colouring (dynhor_amd/mesh_color.py: vertex colours from the frames that see each vertex) ----
 * Both entry points project as dh_mesh_mask_votes does: x_cam = R_f v + T_f (R [n_frames,9] row-major, T [n_frames,3]), then
 * u = (K0 . x_cam) / z, w = (K1 . x_cam) / z with K [3,3] row-major, in fp32 in the order c_r = fma(R_r2, z, fma(R_r1, y, R_r0 x)) + T_r;
 * u = fma(K02, c2, fma(K01, c1, K00 c0)) / c2.  Pixel centres sit at integer (u, w).
 *
 * dh_mesh_raster_depth: z-buffer zbuf u64 [n_frames,H,W] of the mesh verts [nv,3] / faces int64 [nf,3].  The caller fills zbuf with
 * UINT64_MAX ("empty") before the call; each covered pixel centre is combined by a 64-bit atomic minimum with the key
 * (float_bits(z) << 32) | face, z the perspective-correct camera depth z = 1 / sum_i(b_i / z_i), b_i the screen-space barycentrics.
 * Coverage is double-sided and inclusive: the three fp32 edge functions edge(a, b, p) = fma(b.u - a.u, p.w - a.w, -((b.w - a.w) *
 * (p.u - a.u))) of (v1,v2), (v2,v0), (v0,v1) all >= 0 or all <= 0; the depth is computed as (e0 + e1 + e2) / fma(e2, 1/z2, fma(e1,
 * 1/z1, e0 / z0)).  A face is skipped when a vertex has z <= 1e-3, when its screen area edge(v0, v1, v2) is 0, or when an index lies
 * outside [0, nv).  The minimum does not depend on scheduling: the buffer is bitwise reproducible, and a depth tie goes to the smaller
 * face index.  Faces whose clipped pixel box exceeds 32 px in width or height are rasterised by a whole wave.  nf == 0 or
 * n_frames == 0: no-op.  DH_ERR_BAD_ARG: null pointer, negative count, H or W < 1.  DH_ERR_UNSUPPORTED: nf >= 2^32,
 * n_frames >= 2^31, H or W > 2^24.
 *
 * dh_mesh_bake_colors: for each vertex v (unit normal n, normals [nv,3]) and frame f in ascending order, the frame contributes when
 * z > 1e-3, the nearest pixel (floor(u + 0.5), floor(w + 0.5)) lies in the image (range-checked in fp32), usable u8 [n_frames,H,W] is
 * set there, zbuf is not empty there and z <= depth(zbuf) + depth_eps, and c = <n, normalize(C_f - v)> >= min_cos with C_f = -R_f^T
 * T_f the camera centre.  A contributing frame ADDS acc[v] += (c rgb / 255, c) (acc f32 [nv,4], rgb u8 [n_frames,H,W,3]) and
 * n_views[v] += 1 (int32): the caller zeroes both once and issues frame chunks in order on one stream, so every vertex's sum is a fixed
 * sequential fp32 sum (rgb terms as fma(c, rgb / 255, acc)), bitwise reproducible whatever the chunking.  nv == 0 or n_frames == 0:
 * no-op.  DH_ERR_BAD_ARG: null pointer, negative count, H or W < 1, depth_eps negative or NaN, min_cos NaN.  DH_ERR_UNSUPPORTED:
 * nv >= 2^31, H or W > 2^24. */
int dh_mesh_raster_depth(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R, const float* T,
                         const float* K, int64_t n_frames, int H, int W, uint64_t* zbuf, void* stream);
int dh_mesh_bake_colors(const float* verts, const float* normals, int64_t nv, const uint8_t* rgb, const uint8_t* usable,
                        const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                        float depth_eps, float min_cos, float* acc, int32_t* n_views, void* stream);

/* ---- mesh overlay (dynhor_amd/mesh_vis.py: the mesh drawn over every frame, silhouette agreement with the object labels) ----
 * dh_mesh_shade: for each pixel of n_frames frames of H x W, out u8 [n_frames,H,W,3].  zbuf u64 [n_frames,H,W] is the buffer
 * dh_mesh_raster_depth left for the same mesh, cameras and image size.  A pixel is covered when its key is not UINT64_MAX, its face
 * i = key & 0xffffffff is < nf and the three vertex indices of faces[i] lie in [0, nv); only then is the face read.  A covered pixel
 * centre (x, y) of frame f: the face's vertices are projected as above and the three edge functions of dh_mesh_raster_depth give
 * e0, e1, e2 at (x, y) (the rasteriser's own fp32 code: coverage and barycentrics agree with the z-buffer bit for bit); the weights are
 * l_j = (e_j / z_j) / sum_m (e_m / z_m), the normal n = sum_j l_j normals_j (normals [nv,3], unit, object frame) and the shading term
 * s = |(R_f n).z| / |n| (0 when |n| is 0).  base = colors ? sum_j l_j colors_j / 255 (colors u8 [nv,3]) : (0.8, 0.46, 0.51);
 * c = min(1, base (0.3 + 0.7 s)) -- a double-sided headlight along the optical axis; o = alpha c + (1 - alpha) bg with bg = rgb / 255
 * (rgb u8 [n_frames,H,W,3]; 1 when rgb is null); out = floor(255 o + 0.5).  An uncovered pixel copies rgb byte for byte (255 without
 * rgb).  The mesh is drawn over hand pixels too.  label i8 [n_frames,H,W] (1 object, 0 background, -1 hand) and counts int64
 * [n_frames,3] go together: over the pixels with label >= 0 the call ADDS to counts[f] (tp, fp, fn) = (covered and label 1, covered and
 * label 0, uncovered and label 1); the caller zeroes counts.  Integer atomics after a per-wave reduction: output and counts are bitwise
 * reproducible.  out must not overlap rgb.  With nf == 0 every pixel is uncovered and verts, normals, faces may be null; n_frames == 0:
 * no-op.  DH_ERR_BAD_ARG: null required pointer, negative count, H or W < 1, alpha NaN or outside [0, 1], exactly one of label / counts
 * null, out overlapping rgb.  DH_ERR_UNSUPPORTED: nf >= 2^32, n_frames >= 2^31, H or W > 2^24, n_frames H W >= 2^62. */
int dh_mesh_shade(const float* verts, const float* normals, const uint8_t* colors, int64_t nv, const int64_t* faces, int64_t nf,
                  const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                  const uint8_t* rgb, const int8_t* label, float alpha, uint8_t* out, int64_t* counts, void* stream);

/* ---- texture atlas (dynhor_amd/mesh_texture.py: one UV triangle per face, baked from the frames; the mesh drawn with its texture) ----
 * uv f32 [nf,3,2]: the texture coordinates of every face corner in continuous texel units (texel (i, j), i the column, has its
 * centre at (i + 0.5, j + 0.5)); projection, pixel centres and the edge function are dh_mesh_raster_depth's.
 *
 * dh_texture_bake: one lane per texel of the S x S atlas; owner int32 [S,S] names the face a texel belongs to (< 0: none).  A texel
 * (x, y) is worked on when o = owner[y,x] lies in [0, nf), the vertex indices of faces[o] lie in [0, nv) and area = edge(uv0, uv1, uv2)
 * is not 0; every other texel is left untouched.  b_i = max(edge_i(x + 0.5, y + 0.5) / area, 0), renormalised to sum 1 (a texel outside
 * its UV triangle repeats the nearest edge); p = sum_i b_i v_i, n = sum_i b_i normals_i.  For each frame f in ascending order the frame
 * contributes when z > 1e-3, 0 <= u <= W - 1 and 0 <= w <= H - 1, usable u8 [n_frames,H,W] is set at the nearest pixel (floor(u + 0.5),
 * floor(w + 0.5)), zbuf (dh_mesh_raster_depth for the same mesh and cameras) is not empty there and z <= depth(zbuf) + depth_eps, and
 * c = <n, normalize(C_f - p)> / |n| >= min_cos.  Its weight is c squared `sharpen` times (0: c, the vertex rule; 2: c^4); its colour the
 * bilinear fetch of rgb / 255 at (u, w).  A contributing frame ADDS acc[y,x] += (weight colour, weight) (acc f32 [S,S,4], 16-byte
 * aligned) and n_views[y,x] += 1 (int32 [S,S]): the caller zeroes both once and issues frame chunks in order on one stream, so every
 * texel's sum is a fixed sequential fp32 sum (colour terms as fma(weight, colour, acc)), bitwise reproducible whatever the chunking.
 * nf == 0, S == 0 or n_frames == 0: no-op.  DH_ERR_BAD_ARG: null pointer, misaligned acc, negative count, H or W < 1, depth_eps
 * negative or NaN, min_cos NaN, sharpen outside [0, 4].  DH_ERR_UNSUPPORTED: nf >= 2^31, S > 2^15, n_frames >= 2^31, H or W > 2^24.
 *
 * dh_mesh_shade_tex: dh_mesh_shade with a texture in place of vertex colours.  Coverage, the weights l_j and the shading term s are
 * dh_mesh_shade's; (s_t, t_t) = sum_j l_j uv[face][j]; base = the bilinear fetch of tex u8 [Sh,Sw,3] / 255: taps at floor(s_t - 0.5)
 * and + 1 (likewise t_t), indices clamped to the image, weights from the fractional parts.  lit 0: c = base; lit 1: c = min(1, base
 * (0.3 + 0.7 s)).  o = alpha c + (1 - alpha) bg as in dh_mesh_shade; an uncovered pixel copies rgb (255 without rgb).  usable u8
 * [n_frames,H,W] and sums int64 [n_frames,2] go together and need rgb: over the covered pixels with usable set the call ADDS to
 * sums[f] (sum over the three channels of (out - rgb)^2, 1); the caller zeroes sums.  Integer atomics after a per-wave reduction:
 * output and sums are bitwise reproducible.  out must not overlap rgb.  With nf == 0 every pixel is uncovered and verts, normals,
 * faces, uv, tex may be null; n_frames == 0: no-op.  DH_ERR_BAD_ARG: null required pointer, negative count, H or W < 1, Sh or Sw < 1
 * with nf > 0, alpha NaN or outside [0, 1], lit not 0 or 1, exactly one of usable / sums null, sums without rgb, out overlapping rgb.
 * DH_ERR_UNSUPPORTED: nf >= 2^32, n_frames >= 2^31, H, W, Sh or Sw > 2^24, n_frames ceil(H W / 1024) >= 2^31. */
int dh_texture_bake(const float* verts, const float* normals, int64_t nv, const int64_t* faces, int64_t nf, const float* uv,
                    const int32_t* owner, int S, const uint8_t* rgb, const uint8_t* usable, const uint64_t* zbuf, const float* R,
                    const float* T, const float* K, int64_t n_frames, int H, int W, float depth_eps, float min_cos, int sharpen,
                    float* acc, int32_t* n_views, void* stream);
int dh_mesh_shade_tex(const float* verts, const float* normals, int64_t nv, const int64_t* faces, int64_t nf, const float* uv,
                      const uint8_t* tex, int Sh, int Sw, const uint64_t* zbuf, const float* R, const float* T, const float* K,
                      int64_t n_frames, int H, int W, const uint8_t* rgb, const uint8_t* usable, float alpha, int lit, uint8_t* out,
                      int64_t* sums, void* stream);

/* ---- silhouette pose refinement (dynhor_amd/pose_sil.py: per-frame poses fitted to the object masks through a soft silhouette) ----
 * Projection, pixel centres, edge function, coverage and the rule by which a face is skipped are dh_mesh_raster_depth's (the same
 * fp32 code), so a pixel is "covered" here exactly where that z-buffer is not empty.
 *
 * dh_label_edt: label i8 [n_frames,H,W] -> out f32 [n_frames,H,W]: the exact squared Euclidean distance, in pixels, to the nearest pixel
 * whose label == value, searched over the window |dx|, |dy| <= rmax clipped to the image; +inf where the window holds none.  Every
 * result <= rmax^2 is the image's exact distance transform; a larger one only says "farther than rmax".  Two separable passes through
 * the caller's tmp f32 [n_frames,H,W]; every value is an integer <= 2 rmax^2 < 2^24 (rmax <= 2896), exact in fp32.  n_frames == 0: no-op.
 * DH_ERR_BAD_ARG: null pointer, negative n_frames or rmax, H or W < 1, value outside [-128, 127].  DH_ERR_UNSUPPORTED:
 * n_frames * H >= 2^31, W > 65535 * 256, rmax > 2896, H or W > 2^24.
 *
 * dh_sil_nearest: near u64 [n_frames,H,W], filled with UINT64_MAX ("empty") by the caller, is combined by a 64-bit atomic minimum with
 * (float_bits(d2) << 32) | face for every face and every pixel centre p with d2 <= rmax_px^2: d2 = 0 when the face covers p, else the
 * squared distance from p to the nearest of the face's three edge segments, in fp32: for a segment a b, t = clamp(<p - a, b - a> /
 * |b - a|^2, 0, 1), r = (p - a) - t (b - a), d2 = fma(r.w, r.w, r.u r.u); never below FLT_MIN for an uncovered p, so d2 == 0 marks
 * exactly the covered pixels.  The minimum does not depend on scheduling: the buffer is bitwise reproducible and a tie goes to the
 * smaller face.  A pixel farther than rmax_px from every face stays empty.  ws: dh_sil_nearest_workspace(n_frames, H, W) bytes (one
 * byte per 16 x 16 pixel tile: whether it still holds an uncovered pixel after the covering pass; faces whose grown box touches no
 * such tile are skipped).  nf == 0 or n_frames == 0: no-op.
 * DH_ERR_BAD_ARG: null pointer (ws included), negative count, H or W < 1, rmax_px NaN, negative or > 4096.  DH_ERR_UNSUPPORTED:
 * nf >= 2^32, n_frames >= 2^31, H or W > 2^24.
 *
 * dh_sil_loss_grad: out f64 [n_frames, dh_sil_loss_sums() = 17].  Per frame over its pixels, in fp64 from the fp32 inputs:
 * cs2 = (cut sigma)^2 formed in fp32; halo(x) = x <= cs2 ? max(0, exp(-x / sigma^2) - exp(-cut^2)) / (1 - exp(-cut^2)) : 0;
 * w = label >= 0 and not (d2_hand <= cs2); M = halo(max(0, sqrt(d2_obj) - edge_offset)^2); S = 1 where near's d2 bits are 0, 0 where near
 * is empty (or names no face of this mesh), else halo(d2) with d2 recomputed in fp64 from near's face (its vertices projected in fp64;
 * the nearest of the segments v0 v1, v1 v2, v2 v0, the first on a tie).  d2_obj, d2_hand f32 [n_frames,H,W]: dh_label_edt of the values
 * 1 and -1 with rmax >= cut sigma + edge_offset.
 *   [0] sum w (S - M)^2   [1] sum w   [2..10] d[0] / dR_f row-major   [11..13] d[0] / dT_f   [14..16] tp, fp, fn
 * The gradient goes through the closest point q = a + t (b - a) of the winning segment: d d2 / da = -2 (1 - t)(p - q), d d2 / db =
 * -2 t (p - q), then u = (K0 . x_cam) / z, x_cam = R_f v + T_f.  (tp, fp, fn) over label >= 0 = (covered and label 1, covered and
 * label 0, uncovered and label 1): dh_mesh_shade's counts.  ws: dh_sil_loss_grad_workspace(n_frames, H, W) bytes, 16-byte aligned:
 * every workgroup stores its partial and a second kernel adds them in block order (no float atomics); the workgroups of a frame
 * depend on H W alone, so out is bitwise reproducible from launch to launch and for every split of the frames into calls.
 * n_frames == 0: no-op.  DH_ERR_BAD_ARG: null pointer (ws included; verts, faces may be null with nf == 0), negative count, H or
 * W < 1, sigma or cut not > 0, edge_offset negative, NaN.  DH_ERR_UNSUPPORTED: nf >= 2^32, n_frames > 65535, H or W > 2^24. */
int dh_label_edt(const int8_t* label, int64_t n_frames, int H, int W, int value, int rmax, float* tmp, float* out, void* stream);
int64_t dh_sil_nearest_workspace(int64_t n_frames, int H, int W);
int dh_sil_nearest(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R, const float* T, const float* K,
                   int64_t n_frames, int H, int W, float rmax_px, uint64_t* near, void* ws, void* stream);
int dh_sil_loss_sums(void);
int64_t dh_sil_loss_grad_workspace(int64_t n_frames, int H, int W);
int dh_sil_loss_grad(const uint64_t* near, const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R,
                     const float* T, const float* K, const float* d2_obj, const float* d2_hand, const int8_t* label, int64_t n_frames,
                     int H, int W, float sigma, float cut, float edge_offset, double* out, void* ws, void* stream);

/* ---- photometric pose term (dynhor_amd/pose_photo.py: coloured surface points aligned to blurred frames, next to the silhouette) ----
 * Projection and pixel centres are dh_mesh_raster_depth's; the view test is dh_mesh_bake_colors's (the same fp32 code).
 *
 * dh_image_blur: a masked, normalised, separable Gaussian.  rgb u8 [n_frames,H,W,3], usable u8 [n_frames,H,W] (object pixels, eroded:
 * mesh_color.usable_map), taps f32 [2 radius + 1] (the host forms exp(-k^2 / 2 sigma^2) / sum in fp64 and rounds once; the kernel
 * evaluates no exponential) -> out f32 [n_frames,H,W,4].  With v = usable ? (r / 255, g / 255, b / 255, 1) : 0 and 0 outside the image:
 * rows tmp[f,y,x] = sum_k taps[k + radius] v[f,y,x+k], columns s = sum_k taps[k + radius] tmp[f,y+k,x], both over k = -radius..radius
 * in ascending order as acc = fma(tap, value, acc) in fp32; out = (s.rgb / s.a, s.a), all four 0 where s.a == 0.  radius 0 with the tap
 * 1 is the identity (usable ? rgb / 255 : 0, usable).  tmp f32 [n_frames,H,W,4] is the caller's and must not overlap out; both 16-byte
 * aligned.  Every frame is worked on alone: bitwise the same from launch to launch and for every split of the frames into calls.
 * n_frames == 0: no-op.  DH_ERR_BAD_ARG: null pointer, misaligned or overlapping tmp / out, negative n_frames or radius, H or W < 1.
 * DH_ERR_UNSUPPORTED: radius > 64, n_frames * H >= 2^31, W > 65535 * 256, H or W > 2^24.
 *
 * dh_photo_loss_grad: out f64 [n_frames, dh_photo_loss_sums() = 16] for the surface points pts f32 [n_points,3] with unit normals
 * [n_points,3] and colours [n_points,3] in 0..1 (object frame), img f32 [n_frames,H,W,4] from dh_image_blur (16-byte aligned) and zbuf
 * u64 [n_frames,H,W] from dh_mesh_raster_depth for the same mesh, poses and image size.  A (point, frame) pair contributes when, in
 * fp32 and by dh_mesh_bake_colors's code: z > 1e-3; the nearest pixel (floor(u + 0.5), floor(w + 0.5)) lies in the image; zbuf is not
 * empty there and z <= depth(zbuf) + depth_eps; cos = <n, normalize(C_f - p)> >= min_cos; with x0 = floor(u), y0 = floor(w) the taps
 * (x0..x0+1, y0..y0+1) lie in the image; and every tap has a >= a_min.  A contributing pair recomputes x_cam, u, w, fx = u - x0,
 * fy = w - y0 and cos in fp64 from the fp32 inputs:
 *   I = (1-fy)((1-fx) I00 + fx I10) + fy((1-fx) I01 + fx I11) per channel,  e = I - colour,
 *   rho = sum_channels huber(e), huber(x) = x^2 / 2 for |x| <= delta, else delta (|x| - delta / 2);  weight om = cos, constant in the gradient;
 *   dI/du = (1-fy)(I10 - I00) + fy(I11 - I01), dI/dw = (1-fx)(I01 - I00) + fx(I11 - I10); g = om sum_channels huber'(e) (dI/du, dI/dw),
 *   then through du/dx_cam = (K00, K01, K02 - u) / z (dw alike) to G = d/dx_cam.
 *   [0] sum om rho   [1] sum om   [2..10] sum G p^T row-major (d/dR_f)   [11..13] sum G (d/dT_f)   [14] pairs   [15] pairs with every |e| <= delta
 * ws: dh_photo_loss_grad_workspace(n_frames, n_points) bytes, 16-byte aligned: every workgroup stores its partial and a second kernel
 * adds them in block order (no float atomics); the workgroups of a frame depend on n_points alone, so out is bitwise reproducible from
 * launch to launch and for every split of the frames into calls.  n_frames == 0: no-op; n_points == 0: out is zeroed.
 * DH_ERR_BAD_ARG: null pointer (ws included; pts, normals, colors, img, zbuf may be null with n_points == 0), misaligned img or ws,
 * negative count, H or W < 1, depth_eps or a_min negative, delta not > 0, NaN.  DH_ERR_UNSUPPORTED: n_points >= 2^31, n_frames > 65535,
 * H or W > 2^24. */
int dh_image_blur(const uint8_t* rgb, const uint8_t* usable, int64_t n_frames, int H, int W, const float* taps, int radius, float* tmp,
                  float* out, void* stream);
int dh_photo_loss_sums(void);
int64_t dh_photo_loss_grad_workspace(int64_t n_frames, int64_t n_points);
int dh_photo_loss_grad(const float* pts, const float* normals, const float* colors, int64_t n_points, const float* img,
                       const uint64_t* zbuf, const float* R, const float* T, const float* K, int64_t n_frames, int H, int W,
                       float depth_eps, float min_cos, float a_min, float delta, double* out, void* ws, void* stream);

/* ---- correspondence pose term (dynhor_amd/pose_corr.py: dense matches between frames, next to the silhouette) ----
 * All arithmetic is fp64 from fp32 inputs.  Pixel centres are integers, x is the column, K is upper triangular with K22 = 1.
 *
 * dh_pose_corr_sums: out f64 [n_pairs, dh_pose_corr_width() = 28] for the mesh verts f32 [nv,3], faces i64 [nf,3]; the poses R f32
 * [n_frames,3,3], T f32 [n_frames,3] (object -> camera) of ALL frames and K f32 [3,3]; zbuf u64 [n_z,H,W] = dh_mesh_raster_depth of
 * that mesh at the current poses of a chunk of source frames (only the face index in the low 32 bits is read); matches f32
 * [n_matches,5] = (p_x, p_y, q_x, q_y, c): p the integer pixel in frame i, q the sub-pixel position in frame j, c the confidence;
 * pairs i64 [n_pairs,5] = (z-buffer slot of frame i, i, j, first match, count): a pair's matches are consecutive.  max_count: a bound
 * on the counts from the host (it sizes the grid and ws; it does not change a result).  Per match:
 *   d = K^-1 (p_x, p_y, 1): d_y = (p_y - K12) / K11, d_x = (p_x - K02 - K01 d_y) / K00, d_z = 1;
 *   f = the face of zbuf[slot] at the pixel (floor(p_x + 0.5), floor(p_y + 0.5));  a = v0(f), n = (v1 - v0) x (v2 - v0);
 *   o = -R_i^T T_i, e = R_i^T d, s = n.(a - o) / (n.e), X = o + s e   (this form is the contract: the derivative below is entrywise
 *   in R_i and belongs to it; R_i^T stands for the inverse);
 *   Y = R_j X + T_j, u = (K00 Y_x + K01 Y_y + K02 Y_z) / Y_z, w = (K11 Y_y + K12 Y_z) / Y_z, r = (u, w) - q,
 *   rho = huber(|r|), huber(x) = x^2 / 2 for x <= delta_px, else delta_px (x - delta_px / 2); the weight c is constant in the gradient.
 * A match counts when the pixel lies in the image, zbuf is not empty there and f < nf (and the face's vertices < nv), |n|^2 > 0,
 * |n.e| >= min_cos |n| |e|, s > 1e-3, Y_z > 1e-3, c > 0 and every input (the match, both poses, K, the face's vertices) and |r| is finite.
 * With g = huber'(|r|) r / |r| (0 at r = 0) and G = c (g_u du/dY + g_w dw/dY), du/dY = (K00, K01, K02 - u) / Y_z, dw/dY = (0, K11,
 * K12 - w) / Y_z:   frame j: d/dR_j = G X^T, d/dT_j = G;   frame i: om = R_j^T G, om' = om - n (om.e) / (n.e), d/dR_i = (s d - T_i) om'^T,
 * d/dT_i = -R_i om'.
 *   [0] sum c rho  [1] sum c  [2..10] d/dR_i row-major  [11..13] d/dT_i  [14..22] d/dR_j  [23..25] d/dT_j  [26] counted matches
 *   [27] counted matches with |r| <= delta_px
 * resid f32 [n_matches] or null: |r| of every match of a usable pair, -1 where the match does not count (a match of no pair, or of an
 * unusable one, is left as it is).  One lane per match, workgroups over slabs of 256 matches of one pair; every workgroup stores its
 * partial (ws: dh_pose_corr_sums_workspace(n_pairs, max_count) bytes, 16-byte aligned) and a second kernel adds a pair's partials in
 * slab order: no atomics, a pair's row is bitwise the same from launch to launch, for every order of the pairs and every split of them
 * into calls.  i == j is allowed.  A pair whose slot lies outside [0, n_z), whose i or j lies outside [0, n_frames), whose matches do
 * not lie in [0, n_matches) or whose count exceeds max_count gets a row of zeros.  n_pairs == 0: no-op; count == 0: a row of zeros.
 * DH_ERR_BAD_ARG: null pointer (ws included; resid may be null; with max_count == 0 only pairs, out, ws are read), misaligned ws,
 * negative count, H or W < 1, delta_px not > 0, min_cos outside [0, 1], NaN.  DH_ERR_UNSUPPORTED: n_pairs > 65535, max_count >= 2^31,
 * nf >= 2^32, n_matches >= 2^40, H or W > 2^24.
 *
 * dh_pose_corr_frames: the rows f64 [n_pairs,28] of every pair of a step folded into gR f64 [n_frames,9], gT f64 [n_frames,3]:
 * frame f adds, for k = start[f] .. start[f+1] - 1 in this order, scale[pair] * rows[pair, 2..13] where entries[k] = 2 pair + 0
 * (f is the pair's i) or scale[pair] * rows[pair, 14..25] where entries[k] = 2 pair + 1 (f is its j); start i64 [n_frames + 1],
 * entries i64 [n_entries], scale f64 [n_pairs].  A frame with no entry gets zeros; an entry that names no pair is skipped.  The order
 * of the additions is the list's: bitwise the same from launch to launch.  n_frames == 0: no-op.  DH_ERR_BAD_ARG: null pointer (rows,
 * scale, entries may be null with n_entries == 0), negative count.  DH_ERR_UNSUPPORTED: n_frames or n_pairs >= 2^31, n_entries >= 2^40. */
int dh_pose_corr_width(void);
int64_t dh_pose_corr_sums_workspace(int64_t n_pairs, int64_t max_count);
int dh_pose_corr_sums(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* R, const float* T, const float* K,
                      int64_t n_frames, const uint64_t* zbuf, int64_t n_z, int H, int W, const float* matches, int64_t n_matches,
                      const int64_t* pairs, int64_t n_pairs, int64_t max_count, float delta_px, float min_cos, double* out, float* resid,
                      void* ws, void* stream);
int dh_pose_corr_frames(const double* rows, const double* scale, int64_t n_pairs, const int64_t* start, const int64_t* entries,
                        int64_t n_entries, int64_t n_frames, double* gR, double* gT, void* stream);

/* ---- dense frame matching (dynhor_amd/match.py: guided block matching by zero-mean normalised cross-correlation, ZNCC) ----
 * Integer sums, fp64 scores, no atomics in the search: every output is bitwise the same from launch to launch, for every order of the
 * queries and for every split of them into calls.  Pixel centres are integers; x is the column.
 *
 * dh_match_gray: img f32 [n_frames,H,W,4] = (r, g, b, a) from dh_image_blur (16-byte aligned) -> gray u8 [n_frames,H,W] and valid u8
 * [n_frames,H,W]:  valid = a >= a_min;  gray = valid ? min(max(floor(fma(255, fma(0.114f, b, fma(0.587f, g, 0.299f * r)), 0.5f)), 0),
 * 255) : 0, every operation an fp32 IEEE operation as written.  n_frames == 0: no-op.  DH_ERR_BAD_ARG: null pointer, misaligned img,
 * negative n_frames, H or W < 1, NaN a_min.  DH_ERR_UNSUPPORTED: H or W > 2^24, n_frames H W >= 2^38.
 *
 * dh_match_search: queries int32 [n,6] = (fi, fj, px, py, gx, gy): the patch about (px, py) of frame fi is searched for in frame fj
 * about the guess (gx, gy).  P in 1..7 is the patch half-size (N = (2P+1)^2 pixels), R in 0..32 the search range, excl >= 0, min_va >= 1.
 * A pixel outside the image is invalid; the guess is not clamped; fi == fj is allowed.  With a the source patch and b a candidate's:
 *   source: usable when all N pixels are valid and va = N sum a^2 - (sum a)^2 >= min_va; otherwise flags = 1 and nothing is searched.
 *   candidate (dx, dy), |dx|, |dy| <= R: the patch about (gx + dx, gy + dy); valid when all N pixels are valid and
 *     vb = N sum b^2 - (sum b)^2 >= min_va.  num = N sum ab - sum a sum b; the sums are exact integers (sum ab in 32 bits; num, va, vb
 *     in 64), score = (double)num / sqrt((double)va * (double)vb): one multiply, one square root, one divide, each rounded once.
 *   selection: the best score wins, a tie goes to the smallest c = (dy + R)(2R + 1) + (dx + R).  s2 = the best score among the valid
 *     candidates with max(|dx - dx*|, |dy - dy*|) > excl, -2 when there is none.  No valid candidate: flags = 2.  The best on the
 *     border of the window (|dx*| == R or |dy*| == R): flags = 4.
 *   sub-pixel step per axis from the scores m, p of the best's two neighbours along it and its own c: den = m - 2 c + p,
 *     sub = min(max(0.5 (m - p) / den, -0.5), 0.5) when den < 0 and both neighbours are valid candidates inside the window, else 0.
 * out_i int32 [n,4] = (qx, qy, flags, valid candidates), (qx, qy) = (gx + dx*, gy + dy*); out_f f64 [n,4] (8-byte aligned) =
 * (s1, s2, sub_x, sub_y).  With flags 1 or 2: (gx, gy, flags, 0) and (-2, -2, 0, 0).
 * The frame indices are checked on the device before the search and the verdict is read back: the call waits for the stream once
 * (out_i's first word is the scratch).  n == 0: no-op.
 * DH_ERR_BAD_ARG: null pointer, misaligned queries / out_i / out_f, negative count, H or W < 1, P outside 1..7, R outside 0..32,
 * excl < 0, min_va < 1, a frame index outside [0, n_frames).  DH_ERR_UNSUPPORTED: n or n_frames >= 2^31, H or W > 2^24.
 *
 * dh_match_search_warp: dh_match_search with queries int32 [n,10] = (fi, fj, px, py, gx, gy, a00, a01, a10, a11); A = a / 65536 (Q16)
 * maps an offset in the target patch to an offset in the source image, and the source patch is sampled through it.  Only the source
 * patch differs from dh_match_search; va, the flags, the window, the scores, the selection and the sub-pixel step are the same.  Cell
 * (c, r), c, r in [-P, P], of the source patch, in int64:
 *   X = px 65536 + a00 c + a01 r, Y = py 65536 + a10 c + a11 r;  x0 = X >> 16, y0 = Y >> 16 (arithmetic shifts: floors, also below 0);
 *   fx = (X & 0xFFFF) >> 8, fy = (Y & 0xFFFF) >> 8, each in 0..255; the taps (x0 + i, y0 + j), i, j in {0, 1}, weigh
 *   (256 - fx, fx)[i] (256 - fy, fy)[j] (sum 65536).  A tap of weight 0 is not needed and not read.  The cell is valid iff every
 *   needed tap lies in the image and has valid != 0; value = (sum w gray + 32768) >> 16 (below 2^32).
 * With a = (65536, 0, 0, 65536) every cell needs the one tap (px + c, py + r) with weight 65536: every output equals
 * dh_match_search's bit for bit.  All of it is integer arithmetic: the outputs stay bitwise independent of launch, order and split.
 * The argument rules are dh_match_search's; the device check of the frame indices also answers DH_ERR_BAD_ARG for a query with an
 * |a_kl| > 2^19 (a scale of 8). */
int dh_match_gray(const float* img, int64_t n_frames, int H, int W, float a_min, uint8_t* gray, uint8_t* valid, void* stream);
int dh_match_search(const uint8_t* gray, const uint8_t* valid, int64_t n_frames, int H, int W, const int32_t* queries, int64_t n, int P,
                    int R, int excl, int64_t min_va, int32_t* out_i, double* out_f, void* stream);
int dh_match_search_warp(const uint8_t* gray, const uint8_t* valid, int64_t n_frames, int H, int W, const int32_t* queries, int64_t n,
                         int P, int R, int excl, int64_t min_va, int32_t* out_i, double* out_f, void* stream);

/* ---- image metrics (dynhor_amd/image_metrics.py: renderings scored against the frames, Runner.evaluate_views) ----
 * Integer window sums, a short fp64 formula, no atomics: map and out are bitwise the same from launch to launch and for every split
 * of the frames into calls.
 *
 * dh_ssim: a, b u8 [n_frames,H,W,3] (the rendering and the frame), usable u8 [n_frames,H,W] (non-zero = usable; null: every pixel is),
 * taps_host int32 [2 radius + 1] in HOST memory: a Gaussian in Q16, every tap >= 0 and their sum exactly 65536 (validated on the host
 * and passed to the kernel by value; the kernel evaluates no exponential).  With u = usable ? 1 : 0 (0 outside the image) and
 * w(dx, dy) = taps[dx + radius] taps[dy + radius], every pixel has the integer sums over |dx|, |dy| <= radius
 *   Wt = sum w u;  per channel  Sx = sum w u a,  Sy = sum w u b,  Sxx = sum w u a^2,  Syy = sum w u b^2,  Sxy = sum w u a b,
 * formed separably (rows, then columns) and exactly: a per-pixel quantity is at most 255^2 = 65025 and the taps sum to 2^16, so a
 * ROW SUM IS BELOW 2^32 (65025 * 65536 = 0xFE010000; the row pass keeps 32-bit registers and LDS words on the strength of this) and
 * a COLUMN SUM IS BELOW 2^48 (exact in 64-bit integers and as a double).  Wt <= 2^32.
 * A pixel is counted when it is usable and Wt >= w_min.  For a counted pixel, in fp64 from the integers, every operation rounded once
 * as written and nothing contracted into an fma:
 *   mx = Sx / Wt,  my = Sy / Wt,  vx = Sxx / Wt - mx mx,  vy = Syy / Wt - my my,  cxy = Sxy / Wt - mx my,
 *   s_c = ((2 mx my + C1)(2 cxy + C2)) / ((mx mx + my my + C1)(vx + vy + C2)),  2 mx my = (2 mx) my, sums from the left,
 *   C1 = k1 k1 with k1 = 0.01 * 255,  C2 = k2 k2 with k2 = 0.03 * 255 (doubles),   s = ((s_0 + s_1) + s_2) / 3.
 * map f32 [n_frames,H,W] (may be null) = (float)s for a counted pixel, 0 for any other.  out f64 [n_frames, dh_ssim_sums() = 6]:
 *   [0] sum s over the counted pixels   [1] counted pixels   [2] sum over usable pixels and channels of (a - b)^2
 *   [3] sum |a - b| over the same       [4] usable pixels    [5] sum s^2 over the counted pixels
 * [1]..[4] are integers below 2^53, hence exact.  ws: dh_ssim_workspace(n_frames, H, W) bytes, 16-byte aligned: every workgroup (one
 * per 32 x 16 pixel tile) stores its partial and a second kernel adds a frame's partials in tile order (no float atomics); the tiles
 * depend on H and W alone.  The filtered planes are never written to memory.  n_frames == 0: no-op.
 * DH_ERR_BAD_ARG: null a, b, taps_host, out or ws, misaligned ws, negative n_frames or radius, H or W < 1, a negative tap, taps that
 * do not sum to 65536, w_min == 0 or > 2^32.  DH_ERR_UNSUPPORTED: radius > 16, n_frames > 65535, H or W > 2^24, 2^22 or more tiles
 * in a frame. */
int dh_ssim_sums(void);
int64_t dh_ssim_workspace(int64_t n_frames, int H, int W);
int dh_ssim(const uint8_t* a, const uint8_t* b, const uint8_t* usable, int64_t n_frames, int H, int W, const int32_t* taps_host,
            int radius, uint64_t w_min, float* map, double* out, void* ws, void* stream);

/* ---- pose initialisation by silhouette retrieval (dynhor_amd/pose_init.py: a bank of views of a template, retrieval per frame) ----
 * Integer kernels without float atomics: every output is bitwise the same from launch to launch and for every split of the images,
 * frames or views into calls.  Pixel centres are integers, as for dh_mesh_raster_depth.
 *
 * dh_label_boxes: label i8 [n,H,W] -> boxes int32 [n,4] = (xmin, ymin, xmax, ymax) over the pixels with label == 1, (W, H, -1, -1) for
 * an image without one (32-bit integer atomic min / max after a reduction per workgroup).  n == 0: no-op.
 * DH_ERR_BAD_ARG: null pointer, negative n, H or W < 1.  DH_ERR_UNSUPPORTED: n >= 2^31, H or W > 2^24, H W >= 2^44.
 *
 * dh_sil_crop_pack: sq f32 [n,3] = (x0, y0, step) of a square sampling grid per image, S a multiple of 8 in [8, 128].  Sample (r, c),
 * r the row, reads the pixel px = floorf(fmaf(c + 0.5f, step, x0) + 0.5f), py = floorf(fmaf(r + 0.5f, step, y0) + 0.5f) in fp32; inside
 * the image obj = (label == 1), keep = (label >= 0), outside both are 0.  Sample s = r S + c is bit (s & 63) of word (s >> 6) of
 * obj / keep u64 [n, S^2 / 64] (one wave's ballot is one word).  An image whose step is not > 0 (0: the caller's mark of an empty box;
 * NaN) gets all-zero words.  n == 0: no-op.  DH_ERR_BAD_ARG: null pointer, negative n, H or W < 1, S not a multiple of 8 in [8, 128].
 * DH_ERR_UNSUPPORTED: n >= 2^31, H or W > 2^24, n S^2 / 64 >= 2^32 - 4.
 *
 * dh_sil_bank_score: frame_obj, frame_keep u64 [n_frames,n_words], bank_obj u64 [n_views,n_words] -> out int32 [n_frames,n_views,2]
 * (8-byte aligned) = (sum over the words of popc(fo & bo & fk), of popc((fo | bo) & fk)): intersection and union of the frame's and
 * the view's object samples over the frame's keep samples.  n_frames == 0 or n_views == 0: no-op.  DH_ERR_BAD_ARG: null pointer,
 * misaligned out, negative count, n_words < 1.  DH_ERR_UNSUPPORTED: n_words > 2^20, n_frames > 16 * 65535, n_views >= 2^37. */
int dh_label_boxes(const int8_t* label, int64_t n, int H, int W, int32_t* boxes, void* stream);
int dh_sil_crop_pack(const int8_t* label, int64_t n, int H, int W, const float* sq, int S, uint64_t* obj, uint64_t* keep, void* stream);
int dh_sil_bank_score(const uint64_t* frame_obj, const uint64_t* frame_keep, int64_t n_frames, const uint64_t* bank_obj, int64_t n_views,
                      int n_words, int32_t* out, void* stream);

/* ---- block-sparse marching cubes (dynhor_amd/mesh_extract.py: the iso-surface from the blocks near it only) ----
 * The grid has N points per axis, cut into nbk = ceil((N - 1) / B) blocks of B cells per axis; block (bx, by, bz) of blocks int32 [nb,3]
 * covers the grid indices [b B, min(b B + B, N - 1)] and carries P^3 samples, P = B + 1, sample (i, j, k) of block n at row n P^3 +
 * (i P + j) P + k; samples of a clipped end block beyond N - 1 are padding.  table u8 [256,16]: row = case (bit n = corner n above the
 * threshold, corners (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1)), bytes 0..14 the edge ids of up to five
 * triangles (edge e joins the corners 01 12 23 30 45 56 67 74 04 15 26 37), byte 15 their number.  No state is kept.
 * dh_mc_block_points: pts f32 [nb P^3,3] = (ax[gx], ay[gy], az[gz]), READ from the axis arrays f32 [N] (the bits of a dense grid meshed
 * from them); padding repeats index N - 1.
 * dh_mc_count: vals f32 [nb P^3] = the field at those samples.  counts[n] (int32) = the triangles of block n: over its cells (indices
 * < N - 1) the table's count for the case of u - threshold > 0.  *cut_faces (int32, zeroed by the caller, integer atomic) gains the
 * cell faces on a block's boundary whose four corners disagree and whose neighbour block lies inside the grid with block_map < 0
 * (block_map int32 [nbk,nbk,nbk], >= 0 for every listed block).  *nonfinite (int32, zeroed by the caller) becomes 1 when a value is NaN
 * or infinite.  A block outside [0, nbk)^3 counts nothing.
 * dh_mc_emit: offsets int64 [nb] = the exclusive prefix sum of counts, n_tri their total.  Triangle offsets[n] + m of block n is the
 * m-th in (cell (i, j, k) lexicographic, table) order; row r = 3 (offsets[n] + m) + c of its corner c receives keys[r] (int64) =
 * lin(g) 3 + a and pos f32 [r,3]: the corner lies on the grid edge from g (the end with the smaller lin = (gx N + gy) N + gz) along
 * z / y / x for a = 0 / 1 / 2; v0 = u(g) - threshold, v1 the other end's, t = min(max(v0 / (v0 - v1), 0), 1) in fp32 with IEEE
 * division, pos = g in grid units with t added along the edge.  No atomics: bitwise reproducible.  Rows >= 3 n_tri are never written.
 * nb == 0 (or n_tri == 0): no-op.  DH_ERR_BAD_ARG: null pointer, negative count, N < 2, B < 1, NaN threshold.  DH_ERR_UNSUPPORTED:
 * N > 2^20, B > 16, nb >= 2^31. */
int dh_mc_block_points(const float* ax, const float* ay, const float* az, int N, const int32_t* blocks, int64_t nb, int B, float* pts,
                       void* stream);
int dh_mc_count(const float* vals, const int32_t* blocks, int64_t nb, int N, int B, float threshold, const uint8_t* table,
                const int32_t* block_map, int32_t* counts, int32_t* cut_faces, int32_t* nonfinite, void* stream);
int dh_mc_emit(const float* vals, const int32_t* blocks, int64_t nb, int N, int B, float threshold, const uint8_t* table,
               const int64_t* offsets, int64_t n_tri, int64_t* keys, float* pos, void* stream);

/* ---- mesh simplification (dynhor_amd/mesh_simplify.py: vertex clustering with per-cell quadrics) ----
 * dh_simplify_grid (host only, no GPU): the grid of the bounding box lo, hi (float[3] each, host memory) cut into `cells` cells along
 * its longest axis, in fp32 IEEE operations: ext_a = hi_a - lo_a, *h = max_a ext_a / (float)cells, dims[a] = max(1, (int)ceil(ext_a /
 * h)); a box of extent 0 gives h = 0 and dims 1, 1, 1.  DH_ERR_BAD_ARG: null pointer, cells < 1, a NaN, inverted or overflowing box.
 * DH_ERR_UNSUPPORTED: cells > 2^20.
 * The three device entry points take that grid by value (lo float[3] and dims int32[3] in HOST memory, h); they keep no state and need
 * no workspace.
 * dh_simplify_cells: keys[v] (int64) = i_x + dims_x (i_y + dims_y i_z) with i_a = min(dims_a - 1, (int)floor((v_a - lo_a) / h)) in
 * fp32 (subtraction, IEEE division, floor; compared as a float before the conversion); h == 0: every key is 0.  Correct beyond 2^31.
 * The vertices must be finite and inside the box.  nv == 0: no-op.
 * dh_simplify_quadrics: record 3 f + k is corner k of face f (faces int64 [nf,3]) and belongs to the cell of its vertex.  order int64
 * [3 nf]: the records sorted stably by cell key; run r = order[run_start[r] .. run_start[r + 1]) (run_start int64 [n_runs + 1]) holds the
 * records of the cell run_key[r] in ascending order.  Per run, one wave: every lane adds its records (l, l + 64, ...) in ascending order,
 * the lanes fold by a fixed xor butterfly -- no atomics, bitwise reproducible -- into dh_simplify_sums() = 17 fp64 sums, all relative
 * to the cell centre c_a = lo_a + (i_a + 0.5) h, with n the face's unit normal, a its area (a zero-area face: a = 0, n = 0),
 * d = n . (c - P_0), q = corner - c:  [0..5] sum a n n^T (xx xy xz yy yz zz)  [6..8] sum a d n  [9] sum a  [10..12] sum a q
 * [13..15] sum q  [16] the corner count (csrc/mesh_simplify.hip gives the order of every operation).  sums f64 [n_runs,17] receives
 * them when it is not null.  rep f32 [n_runs,3]: xbar = [10..12] / [9] ([13..15] / [16] when [9] == 0); placement 1 (quadric), when [9]
 * > 0 and w = trace / 3 > 0: (A + regularization w I) y = -(A xbar + b) by Cholesky, xbar + y clamped per axis to [-h/2, h/2]
 * (clamped[r] int32 = 1 when an axis moved, else 0); placement 0 (mean) or a cell without area: xbar.  rep = (float)(c + x).  A record
 * whose face has an index outside [0, nv) is skipped.  n_runs == 0: no-op.
 * dh_simplify_faces: vrank int32 [nv] = the run of each vertex's cell (any value for a vertex no face uses).  Per face: tri int64
 * [nf,3] = the three ranks rotated so that the smallest comes first (orientation kept), keep u8 [nf] = 1 when the three differ (else 0
 * and tri = 0), key int64 [nf] = tri_0 n_runs + tri_1.  A face with an index outside [0, nv) or a rank outside [0, n_runs) gets
 * keep 0.  nf == 0: no-op.
 * DH_ERR_BAD_ARG: null pointer, negative count, a grid dh_simplify_grid cannot have returned, regularization not in (0, 1e6],
 * placement not 0 / 1.  DH_ERR_UNSUPPORTED: nv, nf or n_runs >= 2^31, dims > 2^20 + 1, n_runs > 3 nf. */
int dh_simplify_grid(const float* lo, const float* hi, int64_t cells, float* h, int32_t* dims);
int dh_simplify_cells(const float* verts, int64_t nv, const float* lo, float h, const int32_t* dims, int64_t* keys, void* stream);
int dh_simplify_sums(void);
int dh_simplify_quadrics(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* order,
                         const int64_t* run_start, const int64_t* run_key, int64_t n_runs, const float* lo, float h, const int32_t* dims,
                         double regularization, int placement, float* rep, int32_t* clamped, double* sums, void* stream);
int dh_simplify_faces(const int64_t* faces, int64_t nf, const int32_t* vrank, int64_t nv, int64_t n_runs, int64_t* tri, uint8_t* keep,
                      int64_t* key, void* stream);

/* ---- sphere tracing of the SDF: novel views, depth and normal maps (dynhor_amd/surface_render.py; csrc/trace.hip) --------------
 * The network query is the caller's (dh_sdf_nograd / dh_hash_sdf_nograd, or any field); these entry points are the per-ray work
 * around it.  All are stateless: the per-ray state lives in caller-owned arrays over the N = F h w rays of F views (ray index
 * (view h + row) w + column; h = ceil(H / level), w = ceil(W / level), pixel (row level, column level) as Dataset.gen_rays_at):
 *   o [F,3] (one origin per view), d [N,3], t [N] (the next query is o + t d), t_far [N], t_lo / s_lo / t_hi / s_hi [N] (the bracket:
 *   last positive and first negative sample), state u8 [N] (dh_trace_state), nq u16 [N] (queries made), nref u8 [N] (REFINE steps
 *   counted), flags u8 [N] (dh_trace_flag bits).  No float atomics anywhere: the same inputs give the same bits.
 * dh_trace_init: rays of the poses R [F,9], T [F,3] (x_cam = R x_obj + T) with Kinv [9]; o and d are dh_gen_rays' expressions term for
 *   term (bitwise equal at a dataset pose).  With b = o.d, disc = b^2 - (|o|^2 - bound^2), near, far = -b -+ sqrt(disc) (fp64 from the
 *   fp32 o, d): t = max(near, 0), t_far = far, state MARCH; disc <= 0 or far <= 0: state MISS (t = t_far = 0 when disc <= 0).  The
 *   other per-ray arrays are the caller's to zero.
 * dh_trace_step: one step for the rays idx[0 .. min(*count, n_max)) (count: device, null = n_max), s[k] = sdf(o + t d) of ray idx[k].
 *   A ray in state MARCH or REFINE:  s not finite -> FAIL;  |s| <= eps -> HIT at t;  MARCH, s < 0: nq == 0 -> HIT at t with flag
 *   INSIDE, else t_hi = t, s_hi = s, REFINE, first secant point in the same step;  MARCH, s > eps: t_lo = t, s_lo = s, t' = t +
 *   clamp(relax s, min_step, max_step), t' > t_far -> MISS else t = t';  REFINE: (t, s) replaces the bracket end of its sign, nref += 1,
 *   nref >= refine_steps -> HIT at t with flag CAPPED, else t_hi - t_lo <= eps -> HIT at t, else the secant point.  Secant point:
 *   t_lo + w s_lo / (s_lo - s_hi), w = t_hi - t_lo, clamped to [t_lo + 0.1 w, t_hi - 0.1 w].  nq += 1 (saturating).  Every product is
 *   rounded on its own (no fma).  A listed ray in any other state is left as it is.  pts [n_max,3]: pts[k] = fma(t, d, o) of ray idx[k]
 *   after the step (the next query point, in list order).  List entries outside [0, N) are skipped.
 * dh_trace_points: pts[k] = fma(t, d, o) of ray idx[k], k < n, whatever the ray's state: the point the tracer queried last (at a hit:
 *   where it saw |s| <= eps), bit for bit.  List entries outside [0, N) are skipped.
 * dh_trace_compact: the listed rays (idx null: 0 .. n_max-1) that are MARCH or REFINE, densely and in list order: idx_out, their
 *   points pts_out = o + t d, *count_out (device) their number.  Per-block counts, one scan, emit; ws: int32 [ceil(n_max / 256)].
 *   idx_out must not be idx, count_out not count (the emit reads both again).  n_max == 0 writes *count_out = 0.
 * dh_trace_compose: the image buffers of the N rays.  A ray is drawn as a hit iff state == HIT and 0 <= slot[ray] < n_hits; normals /
 *   colors [n_hits,3] are the network's at the hit points (object frame; colour in [0, 1]).  rgb u8 [N,3] = round(255 clamp(colour)) over
 *   the background: 0 white, 1 black, 2 the pixel of frame frame_idx[view] of frame_rgb u8 [n_frames,H,W,3] (black for an index outside it);  depth f32 [N] = t (R d)_z,
 *   the camera z of the hit, +inf elsewhere;  normal u8 [N,3] = trunc(255 clamp(0.5 n_cam / (|n_cam| + 1e-6) + 0.5)), n_cam = R n (127
 *   elsewhere);  hit u8 [N].
 * N == 0 / n_max == 0: no-op (dh_trace_compact still writes the count).  DH_ERR_BAD_ARG: null pointer, negative count, H, W, h, w or
 * level < 1, bound, eps, min_step not > 0, max_step < min_step, relax not > 0, refine_steps outside [1, 255], background outside
 * 0 .. 2 (or 2 without frames), idx_out == idx, count_out == count.  DH_ERR_UNSUPPORTED: N or n_max >= 2^31. */
enum dh_trace_state { DH_TRACE_MARCH = 0, DH_TRACE_REFINE = 1, DH_TRACE_HIT = 2, DH_TRACE_MISS = 3, DH_TRACE_FAIL = 4 };
enum dh_trace_flag { DH_TRACE_INSIDE = 1, DH_TRACE_CAPPED = 2, DH_TRACE_SCANNED = 4 /* set by the caller's chord scan */ };
int dh_trace_init(const float* R, const float* T, const float* Kinv, int n_views, int H, int W, int level, float bound, float* o,
                  float* d, float* t, float* t_far, uint8_t* state, void* stream);
int dh_trace_step(const int32_t* idx, const int32_t* count, const float* s, const float* o, const float* d, int64_t rays_per_view,
                  int64_t N, float* t, const float* t_far, float* t_lo, float* s_lo, float* t_hi, float* s_hi, uint8_t* state,
                  uint16_t* nq, uint8_t* nref, uint8_t* flags, float eps, float relax, float min_step, float max_step, int refine_steps,
                  int64_t n_max, float* pts, void* stream);
int dh_trace_points(const int32_t* idx, const float* o, const float* d, const float* t, int64_t rays_per_view, int64_t N, int64_t n,
                    float* pts, void* stream);
int dh_trace_compact(const int32_t* idx, const int32_t* count, const uint8_t* state, const float* o, const float* d, const float* t,
                     int64_t rays_per_view, int64_t N, int64_t n_max, int32_t* ws, int32_t* idx_out, int32_t* count_out,
                     float* pts_out, void* stream);
int dh_trace_compose(const uint8_t* state, const float* t, const float* d, const int32_t* slot, const float* normals,
                     const float* colors, int64_t n_hits, const float* R, int n_views, int H, int W, int level, int background,
                     const uint8_t* frame_rgb, const int32_t* frame_idx, int n_frames, uint8_t* rgb, float* depth, uint8_t* normal,
                     uint8_t* hit, void* stream);

/* ---- multi-view stereo (dynhor_amd/mvs.py: a mesh-guided plane sweep and a consistency count between depth maps) ----
 * fp32 throughout, every operation an IEEE operation as written (no contraction), every sum in a fixed order, no atomics: a pixel's
 * outputs depend on that pixel's inputs alone and are bitwise the same for every order of the pixels and every split into calls.
 * Pixel centres are integers; x is the column.  dot(a, b) below is (a0 b0 + a1 b1) + a2 b2; a 3 x 3 product uses it per entry.
 *
 * dh_mvs_sweep: gray, valid u8 [n_frames,H,W] (dh_match_gray); R f32 [n_frames,9], T f32 [n_frames,3]; K, Kinv f32 [9] in DEVICE memory
 * (Kinv inverted on the host in fp64); pix int32 [n,3] = (fi, px, py); guide f32 [n,4] = (z0, nx, ny, nz): the guide's camera z at the
 * pixel and the unit plane normal in frame fi's camera frame; nbr int32 [n_frames,n_nbr]: the neighbour frames of every frame, an entry
 * outside [0, n_frames) (-1) means none; 1 <= n_nbr <= 8; D odd in 3..63; step > 0; P in 1..7 (N = (2P+1)^2); min_va >= 1; min_vb > 0;
 * min_views >= 1; min_cos in [-1, 1].  Per pixel, with p = (px, py, 1) as floats:
 *   source: the patch a about (px, py) of frame fi; flag 1 when a pixel of it lies outside the image or is invalid, fi lies outside
 *     [0, n_frames), or va = N sum a^2 - (sum a)^2 < min_va (exact integers, as dh_match_search).
 *   guide: e = Kinv p, e_r = (Kinv[r][0] px + Kinv[r][1] py) + Kinv[r][2]; flag 8 unless z0 is finite, z0 > 1e-3 and
 *     -dot(n, e) / sqrt(dot(e, e)) >= min_cos (a NaN fails).  With flag 1 or 8 nothing is swept.
 *   hypothesis k in [0, D): z_k = z0 + float(k - (D-1)/2) * step, X_k = z_k e; invalid unless z_k > 1e-3.  d = dot(n, X_k), s = n / d.
 *   neighbour j = nbr[fi][.]: R_ij[r][c] = dot(R_j row r, R_i row c), t_ij[r] = T_j[r] - dot(R_ij row r, T_i),
 *     M[r][c] = R_ij[r][c] + t_ij[r] s[c], G = K M, Hm = G Kinv (entry [r][c] = dot(row r, column c)), h = Hm p with
 *     h_r = (Hm[r][0] px + Hm[r][1] py) + Hm[r][2]; invalid for j unless h_2 > 1e-3.  q = (h_0 / h_2, h_1 / h_2),
 *     A = [[(Hm00 - q_x Hm20) / h_2, (Hm01 - q_x Hm21) / h_2], [(Hm10 - q_y Hm20) / h_2, (Hm11 - q_y Hm21) / h_2]].
 *   tap (c, r), c, r in [-P, P], row-major: (tx, ty) = (q_x + (A00 c + A01 r), q_y + (A10 c + A11 r)); it needs the four pixels
 *     (floor tx + {0, 1}, floor ty + {0, 1}) whatever the fractions: j is invalid for this hypothesis unless 0 <= tx < W - 1,
 *     0 <= ty < H - 1 (a NaN fails) and all four are valid.  wx = tx - floor tx, wy = ty - floor ty, top = g00 + wx (g01 - g00),
 *     bot = g10 + wx (g11 - g10), b = top + wy (bot - top); sb += b, sb2 += b b, sab += a b in this order from 0.
 *   score: vb = N sb2 - sb sb; j is invalid unless vb >= min_vb; score = (N sab - float(sum a) sb) / sqrt(float(va) vb).
 *     c_k = (the scores of the valid neighbours added in nbr's order) / their number when that is >= min_views, else NONE = -2.
 *   result: k* = the largest c_k, the lowest k on a tie; c_second = the largest c_k with |k - k*| > 1, else -2; flag 2: no valid
 *     hypothesis; flag 4: k* is 0 or D - 1; sub = min(max((0.5 (c_{k*-1} - c_{k*+1})) / den, -0.5), 0.5) with
 *     den = (c_{k*-1} - 2 c_{k*}) + c_{k*+1} when den < 0, neither neighbour is NONE and flag 4 is not set, else 0;
 *     z = z0 + (float(k* - (D-1)/2) + sub) * step.
 * out_f f32 [n,4] = (z, c_best, c_second, sub); out_i int32 [n,4] = (k*, valid neighbours at k*, flags, valid hypotheses).  With flag
 * 1, 2 or 8: (0, -2, -2, 0) and (0, 0, flags, 0).  Runs on `stream` and does not wait for it.  n == 0: no-op.
 * DH_ERR_BAD_ARG: null or misaligned pointer, negative count, H or W < 1, a setting outside the ranges above, NaN.
 * DH_ERR_UNSUPPORTED: n or n_frames >= 2^31, H or W > 2^24.
 *
 * dh_mvs_check: depth f32 [n_frames,H,W] (NaN or inf: none) -> count u8 [n_frames,H,W].  A pixel (px, py) of frame i with depth z:
 * c = z (Kinv p) - T_i per component, X = R_i^T c, and for every neighbour j of nbr (as above): y = R_j X + T_j; j is skipped unless
 * y_2 > 1e-3; (u, w) = (floor(dot(K row 0, y) / y_2 + 0.5), floor(dot(K row 1, y) / y_2 + 0.5)); skipped unless 0 <= u < W,
 * 0 <= w < H and z_j = depth[j][w][u] is finite; j agrees when |y_2 - z_j| <= depth_rel z_j.  count = the number of agreeing
 * neighbours (0 without a depth).  depth_rel >= 0.  n_frames == 0: no-op.  DH_ERR_BAD_ARG: null or misaligned pointer, negative
 * n_frames, H or W < 1, n_nbr outside 1..8, depth_rel negative or not finite.  DH_ERR_UNSUPPORTED: H or W > 2^24, n_frames H W >= 2^38. */
int dh_mvs_sweep(const uint8_t* gray, const uint8_t* valid, int64_t n_frames, int H, int W, const float* R, const float* T, const float* K,
                 const float* Kinv, const int32_t* pix, const float* guide, int64_t n, const int32_t* nbr, int n_nbr, int D, float step,
                 int P, int64_t min_va, float min_vb, int min_views, float min_cos, float* out_f, int32_t* out_i, void* stream);
int dh_mvs_check(const float* depth, int64_t n_frames, int H, int W, const float* R, const float* T, const float* K, const float* Kinv,
                 const int32_t* nbr, int n_nbr, float depth_rel, uint8_t* count, void* stream);

/* ---- depth fusion (dynhor_amd/depth_fuse.py: the depth maps of all frames integrated into a truncated signed distance field; csrc/tsdf.hip) ----
 * dh_tsdf_integrate: pts f32 [n,3]; depth f32 [n_frames,H,W], camera z; weight u8 [n_frames,H,W]; R [n_frames,9] row-major,
 * T [n_frames,3], K [9] = the K of the depth image, as for dh_mesh_mask_votes; trunc > 0 in object units.  State per point, updated in
 * place and carried from call to call (the caller starts all three at 0): num int64 [n], den int32 [n], obs int32 [n].
 * Per point p and frame f, in fp32:
 *   1. c = R_f p + T_f and (u, w) in dh_mesh_mask_votes' fma order (mk_project); skipped unless c_2 > 1e-3.
 *   2. The nearest pixel, as dh_mvs_check: xf = floor(u + 0.5), yf = floor(w + 0.5); skipped unless 0 <= xf <= W - 1 and
 *      0 <= yf <= H - 1, compared as floats before any conversion (a NaN or a huge value skips).
 *   3. zd = depth[f, yf, xf], wt = weight[f, yf, xf]; skipped when wt == 0, when zd is not finite, or when zd <= 1e-3.
 *   4. d = zd - c_2; skipped when d < -trunc (the point is hidden behind the surface).
 *   5. t = min(d / trunc, 1) with one division; q = rint(t * 65536) (round to nearest even) as int32, in [-65536, 65536].
 *   6. num += (int64) wt * q; den += wt; obs += 1.
 * The sums are integers, so the state after any set of frames is the same bits for every order of the frames and every split of them
 * into calls.  |num| <= 255 * 2^16 * frames; den <= 255 * frames fits in int32 up to 8.4e6 frames (the caller's bound: it is not
 * checked).  No atomics; the library allocates nothing and keeps no state.  Runs on `stream` and does not wait for it.
 * n == 0 or n_frames == 0: no-op.  DH_ERR_BAD_ARG: negative count, H or W < 1, trunc not finite and positive, a null pointer with
 * n > 0 and n_frames > 0.  DH_ERR_UNSUPPORTED: H or W > 2^24, n >= 2^31 * 256, n_frames >= 2^31, n_frames H W > 2^58. */
int dh_tsdf_integrate(const float* pts, int64_t n, const float* depth, const uint8_t* weight, const float* R, const float* T, const float* K,
                      int64_t n_frames, int H, int W, float trunc, int64_t* num, int32_t* den, int32_t* obs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DYNHOR_HIP_H */
