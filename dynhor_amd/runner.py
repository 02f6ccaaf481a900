"""Runner -- mirror of upstream ``exp_runner.py:Runner`` in the reference's config style
(flat yaml.safe_load dict, ObjTracker/configs/custom_shoes.yaml:1-18; experiment directory exps/<seq>/<exp>/ with the
config copied in, ObjTracker/run.py:125-128; one scalar per loss key per step as jointopt.py:151-153 logs them).

Data-parallel: one process per GPU (torch.distributed, backend nccl == RCCL over xGMI).  Rank r takes frame
perm[(iter*world + r) % n_images]; the only exchange is ONE all-reduce of the flat 802,491-float gradient per
iteration, then every rank applies the same fused Adam step.
"""
from __future__ import annotations

import json
import math
import os
import shutil

import numpy as np
import torch
import torch.distributed as dist
import yaml

from . import dist as dh_dist
from . import schedules
from .dataset import Dataset
from .fields import ParamStore, RenderingNetwork, SDFNetwork, SingleVarianceNetwork
from .match import DEFAULTS as MATCH_DEFAULTS
from .mesh_extract import DEFAULT_LIPSCHITZ
from .mvs import DEFAULTS as MVS_DEFAULTS
from .pose_init import DEFAULTS as POSE_INIT_DEFAULTS
from .pose_corr import DEFAULTS as POSE_CORR_DEFAULTS
from .pose_photo import DEFAULTS as POSE_PHOTO_DEFAULTS
from .pose_sil import DEFAULTS as POSE_SIL_DEFAULTS
from .renderer import NeuSRenderer
from .sdf_init import SDF_INIT_DEFAULTS
from .settings import PRIOR_DEFAULTS, int_in, is_int, merge, one_of, prior_settings, warp_settings
from .warp_loss import DEFAULTS as WARP_DEFAULTS

DEFAULT_CONF = {
    "seq_name": "synthetic", "exp_name": "neus",
    "data_info": {"dataroot": None, "synthetic": {"n_frames": 64, "H": 512, "W": 512, "seed": 4321}},
    "train": {"learning_rate": 5e-4, "learning_rate_alpha": 0.05, "end_iter": 300000, "batch_size": 2048,
              "warm_up_end": 5000, "anneal_end": 50000, "igr_weight": 0.1, "mask_weight": 0.1, "normal_weight": 0.0,
              "save_freq": 10000, "val_freq": 2500, "report_freq": 100, "use_white_bkgd": False, "keep_only": False,
              "seed": 1234, "ray_seed": 4321,
              # frames kept out of training, to score renderings on (--mode evaluate_views): none | every:K[:offset] | a list of stems;
              # a held-out frame keeps its input pose
              "holdout": "none",
              # roctx: put every C-ABI stage call into a ROCm marker range (rocprofv3 --marker-trace); off by default
              "roctx": False,
              # full loss stack (BASELINE.json configs[4]): dense-correspondence reprojection term, DESIGN.md section 9
              "corr_weight": 0.0, "corr_fraction": 0.25, "corr_delta_px": 4.0, "corr_vote_freq": 0, "corr_vote_tau_px": 8.0,
              # priors with a validity (dh_prior_loss, DESIGN_NEXT_ROWS.md section 27; settings.PRIOR_DEFAULTS): the depth term reads
              # data_info.depth; normal_skip_missing takes the normal term over the pixels that have a normal.  First settings, not tuned
              **PRIOR_DEFAULTS,
              # multi-view photometric consistency (dh_warp_loss, DESIGN_NEXT_ROWS.md section 30; warp_loss.DEFAULTS): warp_weight 0 = off;
              # the grey tables are built at the first iteration >= warp_start_iter.  First settings, not tuned.  Not with refine_poses
              "warp_weight": 0.0, **{"warp_" + k: (list(v) if isinstance(v, tuple) else v) for k, v in WARP_DEFAULTS.items()},
              # per-frame pose refinement: 6-D rotation + translation per frame, rotation at 10x lr
              "refine_poses": False, "pose_lr": 1e-4, "pose_rot_lr_mult": 10.0, "pose_start_iter": 0},
    # family "neus": the 8x256 / 4x256 fp32 MLPs (BASELINE.json configs[1]); "hash": hash-grid + shallow MLPs (configs[3])
    # arithmetic: null (the library's default: split_f16), "split_f16" (two fp16 pieces / three products, shipping), "split_bf16"
    # (three bf16 pieces / six products) or "fp32_mfma" (the native fp32-MFMA twins) for THIS Runner's renderer -- passed with every
    # launch, so Runners of one process (also on different host threads) may differ
    "model": {"family": "neus", "arithmetic": None, "sdf_network": {}, "variance_network": {"init_val": 0.3}, "rendering_network": {},
              "hash_sdf_network": {}, "sh_rendering_network": {},
              # hash family only: sampler "hierarchical" (NeuS 64+64) or "occgrid" (instant-nsr-pl occupancy-grid marching);
              # reproducible_table_grad: the table scatter through fixed-point integer atomics (bitwise reproducible training; False:
              # float atomics)
              "hash_renderer": {"sampler": "hierarchical", "march_samples_per_ray": 512, "grid_res": 128, "grid_update_every": 16,
                                "max_samples": 128, "reproducible_table_grad": True},
              "neus_renderer": {"n_samples": 64, "n_importance": 64, "n_outside": 0, "up_sample_steps": 4, "perturb": 1.0}},
    # silhouette pose refinement (--mode refine_poses): dynhor_amd/pose_sil.py says what each number is, DESIGN_NEXT_ROWS.md section 13
    # where it comes from; resolution = the marching-cubes grid of the reconstruction the poses are fitted to
    "pose_sil": dict(POSE_SIL_DEFAULTS),
    # the optional photometric term of refine_poses (--pose_photo): dynhor_amd/pose_photo.py says what each number is,
    # DESIGN_NEXT_ROWS.md section 19 where it comes from; mode none | views | mesh
    "pose_photo": dict(POSE_PHOTO_DEFAULTS),
    # the optional correspondence term of refine_poses (--pose_corr): dynhor_amd/pose_corr.py says what each number is,
    # DESIGN_NEXT_ROWS.md section 24 where it comes from; mode none | dataset | match
    "pose_corr": dict(POSE_CORR_DEFAULTS),
    # pose initialisation from a template mesh (--mode init_poses): dynhor_amd/pose_init.py says what each number is,
    # DESIGN_NEXT_ROWS.md section 16 where it comes from; its final joint refinement takes the pose_sil: block
    "pose_init": dict(POSE_INIT_DEFAULTS),
    # SDF warm start from a template mesh (--mode init_sdf): dynhor_amd/sdf_init.py says what each number is, DESIGN_NEXT_ROWS.md
    # section 18 where it comes from
    "sdf_init": dict(SDF_INIT_DEFAULTS),
    # dense frame matching (--mode match_frames): dynhor_amd/match.py says what each number is, DESIGN_NEXT_ROWS.md section 20 where it
    # comes from; guide none | mesh
    "match": dict(MATCH_DEFAULTS),
}


# the optional mesh_clean: block of the YAML (validate_mesh / evaluate_mesh; dynhor_amd/mesh_clean.py).  dilate_px 2 = the smallest
# safe dilation plus one pixel of margin: on the synthetic scene (64 frames of 512 x 512, hand on) meshed at resolution 512, mask culling
# removes 176,562 of the 395,896 object vertices at 0 px (silhouette vertices whose pixel centre misses the object in some frame) and
# none at 1, 2 or 3 px (MI355X; tests/test_gpu_mesh_clean.py::test_default_dilation_culls_no_object_vertex prints the sweep)
MESH_CLEAN_DEFAULTS = {"mode": "none", "dilate_px": 2, "min_bg_votes": 1, "min_area_frac": None}

# the optional mesh_color: block of the YAML (validate_mesh; dynhor_amd/mesh_color.py)
MESH_COLOR_DEFAULTS = {"mode": "none", "erode_px": 1, "min_cos": 0.1, "depth_eps": 0.01}

# the optional surface_render: block of the YAML (render_views; dynhor_amd/surface_render.py): method surface | volume, level = the
# pixel stride, background white | black | frame, and the tracer's parameters (surface_render.TRACE_DEFAULTS; compact_every stays 1
# until the two settings have been timed on a GPU: DESIGN_NEXT_ROWS.md section 17)
SURFACE_RENDER_DEFAULTS = {"method": "surface", "level": 1, "background": "white", "eps": 2e-4, "relax": 0.8, "min_step": 1e-3,
                           "max_step": 0.1, "refine_steps": 8, "max_steps": 48, "scan_step": 0.01, "compact_every": 1}

# the optional image_eval: block of the YAML (evaluate_views; dynhor_amd/image_metrics.py): frames auto (the held-out frames if there are
# any, else all) | all | train | holdout | every:K[:offset] | stems; sigma / radius = the SSIM window (the usual 11 x 11 Gaussian);
# min_weight = the share of the window's weight that must lie on usable pixels for a pixel to count; erode_px as in mesh_color; maps:
# also write <name>_ssim.png
IMAGE_EVAL_DEFAULTS = {"frames": "auto", "sigma": 1.5, "radius": 5, "min_weight": 0.5, "erode_px": 0, "maps": False}

# the optional mesh_texture: block of the YAML (validate_mesh; dynhor_amd/mesh_texture.py): mode none | views | views+network, size = the
# atlas edge in texels; erode_px / min_cos / depth_eps as in mesh_color; sharpen: the weight is cos^(2^sharpen); image: png | jpg
MESH_TEXTURE_DEFAULTS = {"mode": "none", "size": 1024, "erode_px": 1, "min_cos": 0.1, "depth_eps": 0.01, "sharpen": 2, "image": "png"}

# the optional mesh_extract: block of the YAML (validate_mesh / evaluate_mesh / visualize_mesh; dynhor_amd/mesh_extract.py): mode "dense"
# queries the whole grid; "sparse" only the blocks of `block`^3 cells whose centre value lies within lipschitz x the block radius of the
# threshold (the same mesh, no resolution limit).  lipschitz: mesh_extract.DEFAULT_LIPSCHITZ says where the number comes from
MESH_EXTRACT_DEFAULTS = {"mode": "dense", "block": 8, "lipschitz": DEFAULT_LIPSCHITZ}

# the optional mesh_simplify: block of the YAML (validate_mesh / evaluate_mesh / visualize_mesh / refine_poses; dynhor_amd/mesh_simplify.py):
# mode none | cells:N (N cells along the bounding box's longest axis) | faces:T (the finest grid of at most cells_max cells that leaves at
# most T faces); regularization = the Tikhonov pull of the quadric placement towards the cell's centroid
MESH_SIMPLIFY_DEFAULTS = {"mode": "none", "regularization": 1e-3, "cells_max": 1024}

# the optional mesh_vis: block of the YAML (visualize_mesh; dynhor_amd/mesh_vis.py): mesh None = the reconstruction at `resolution`;
# normalize "none" | "reference" for a mesh file; turntable = frames of the orbit GIF (0: none)
MESH_VIS_DEFAULTS = {"mesh": None, "normalize": "none", "resolution": 512, "alpha": 0.6, "turntable": 0}
# the optional eval: block of the YAML (evaluate_mesh; dynhor_amd/metrics.py); a key at null counts as not set
EVAL_DEFAULTS = {"gt_mesh": None, "gt_normalize": "none", "resolution": 512, "gt_resolution": 512, "n_samples": 1_000_000,
                 "taus": (0.005, 0.01, 0.02), "gt_align": "none", "gt_align_init": "identity", "align_opts": None}
VIS_WRITERS = 8                  # JPEG writer threads of visualize_mesh (a fixed pool: JPEG encoding is host work)


def _merge(base, over):
    out = dict(base)
    for k, v in (over or {}).items():
        out[k] = _merge(base[k], v) if isinstance(v, dict) and isinstance(base.get(k), dict) else v
    return out


def _newest_mvs_dir(base_exp_dir, who):
    """The newest <exp>/mvs/*/ that holds a depth/ folder (fuse_depth's default, --prior_dir auto)."""
    root = os.path.join(base_exp_dir, "mvs")
    runs = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d, "depth"))) if os.path.isdir(root) else []
    if not runs:
        raise ValueError(f"{who}: no depth maps under {root}: run --mode mvs_depth first, or give --mvs_dir")
    return os.path.join(root, runs[-1])


class Runner:
    def __init__(self, conf_path=None, mode="train", case=None, is_continue=False, conf: dict | None = None,
                 dataset: Dataset | None = None, device=None, exp_root="exps", prior_dir=None):
        """prior_dir: a folder in mvs_depth's layout -- sets data_info.depth to <prior_dir>/depth and data_info.monocular_normal to
        <prior_dir>/monocular_normal; "auto": the newest <exp>/mvs/*/, as fuse_depth finds it."""
        if conf is None:
            with open(conf_path, "r") as f:
                conf = yaml.safe_load(f)
        self.conf = _merge(DEFAULT_CONF, conf)
        if case is not None:
            self.conf["seq_name"] = case
        self.mode = mode
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        self.device = torch.device(device if device is not None else f"cuda:{int(os.environ.get('LOCAL_RANK', 0))}")
        self.base_exp_dir = os.path.join(exp_root, self.conf["seq_name"], self.conf["exp_name"])
        if self.rank == 0:
            os.makedirs(self.base_exp_dir, exist_ok=True)
            if conf_path is not None:
                shutil.copy(conf_path, os.path.join(self.base_exp_dir, "config.yaml"))
            else:
                with open(os.path.join(self.base_exp_dir, "config.yaml"), "w") as f:
                    yaml.safe_dump(self.conf, f)
        tr = self.conf["train"]
        self.end_iter = tr["end_iter"]; self.batch_size = tr["batch_size"]
        self.learning_rate = tr["learning_rate"]; self.learning_rate_alpha = tr["learning_rate_alpha"]
        self.warm_up_end = tr["warm_up_end"]; self.anneal_end = tr["anneal_end"]
        self.igr_weight = tr["igr_weight"]; self.mask_weight = tr["mask_weight"]; self.normal_weight = tr["normal_weight"]
        self.save_freq = tr["save_freq"]; self.val_freq = tr["val_freq"]; self.report_freq = tr["report_freq"]
        self.use_white_bkgd = tr["use_white_bkgd"]; self.keep_only = tr["keep_only"]
        self.corr_weight = tr["corr_weight"]; self.corr_fraction = tr["corr_fraction"]; self.corr_delta_px = tr["corr_delta_px"]
        self.corr_vote_freq = tr["corr_vote_freq"]; self.corr_vote_tau_px = tr["corr_vote_tau_px"]
        pr = prior_settings(tr)
        self.depth_weight, self.depth_delta, self.depth_start_iter = pr["depth_weight"], pr["depth_delta"], pr["depth_start_iter"]
        self.normal_skip_missing = pr["normal_skip_missing"]
        self.warp_conf = warp_settings(tr)
        self.warp_weight = self.warp_conf.pop("weight")
        self.warp_tables = None          # warp_loss.frames_for's tables, built at the first iteration with the term
        if self.warp_weight > 0.0 and tr["refine_poses"]:
            raise ValueError("train.warp_weight > 0 with train.refine_poses is not supported: the multi-view photometric term has no "
                             "pose adjoint and its grey tables and homographies would go stale as the poses move")
        self.iter_step = 0
        if prior_dir is not None:
            d = _newest_mvs_dir(self.base_exp_dir, "--prior_dir auto") if prior_dir == "auto" else str(prior_dir)
            if not os.path.isdir(os.path.join(d, "depth")):
                raise ValueError(f"--prior_dir: {d} holds no depth/ folder: run --mode mvs_depth first, or give its folder")
            self.conf["data_info"] = dict(self.conf["data_info"], depth=os.path.join(d, "depth"),
                                          monocular_normal=os.path.join(d, "monocular_normal"))

        if dataset is None:
            di = self.conf["data_info"]
            if di.get("dataroot"):
                # init_poses alone starts without pose files (it writes them); every other mode keeps the loader's error
                dataset = Dataset(di, device=self.device, poses=mode != "init_poses")
            else:
                dataset = Dataset.from_synthetic(device=self.device, **di["synthetic"])
        self.dataset = dataset
        if self.depth_weight > 0.0 and self.dataset.depth is None:
            raise ValueError("train.depth_weight > 0 needs depth maps: point data_info.depth at a folder of <stem>.npy (mvs_depth "
                             "writes one: --prior_dir), or put them under <dataroot>/depth")

        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(tr["seed"])          # identical initial weights on every rank
            family = self.conf["model"]["family"]
            if family == "neus":
                self.sdf_network = SDFNetwork(**self.conf["model"]["sdf_network"])
                self.color_network = RenderingNetwork(**self.conf["model"]["rendering_network"])
                store_cls, renderer_cls = ParamStore, NeuSRenderer
            elif family == "hash":
                from .hash_fields import HashNeuSRenderer, HashParamStore, HashSDFNetwork, SHRenderingNetwork
                self.sdf_network = HashSDFNetwork(**self.conf["model"]["hash_sdf_network"])
                self.color_network = SHRenderingNetwork(**self.conf["model"]["sh_rendering_network"])
                store_cls, renderer_cls = HashParamStore, HashNeuSRenderer
            else:
                raise ValueError(f"model.family must be 'neus' or 'hash', got {family!r}")
            self.deviation_network = SingleVarianceNetwork(**self.conf["model"]["variance_network"])
        self.nerf_outside = None
        self.store = store_cls(self.sdf_network, self.deviation_network, self.color_network, self.device)
        extra = dict(self.conf["model"]["hash_renderer"]) if family == "hash" else {}
        if family == "hash" and tr["refine_poses"]:
            if self.corr_weight > 0.0 and extra.get("sampler") == "occgrid":
                raise ValueError("train.corr_weight > 0 with model.family 'hash', model.hash_renderer.sampler 'occgrid' and "
                                 "train.refine_poses is not supported: the correspondence term runs on the hierarchical sampler")
            extra["ray_grads"] = True        # the packed path's adjoint buffers (hash_fields.HashNeuSRenderer)
        ar = self.conf["model"].get("arithmetic")
        if ar is not None:
            from . import _lib
            extra["arithmetic"] = _lib.ARITH_NAMES[ar]
        self.renderer = renderer_cls(self.nerf_outside, self.sdf_network, self.deviation_network, self.color_network,
                                     store=self.store, device=self.device, **self.conf["model"]["neus_renderer"], **extra)
        if tr.get("roctx"):
            self.renderer.timer.set_markers(True)
        # hash family, data-parallel: the 49 MB table gradient is reduced by a collective of its own, started the moment the table
        # scatter has been enqueued and overlapped with the small weight-gradient GEMMs (hash_fields.HashNeuSRenderer._weight_grads);
        # train.overlap_table_reduce = False keeps the one serial all-reduce of the whole bucket (the two are bitwise identical at
        # two ranks; at more ranks a ring may add the same numbers in a different order)
        self.overlap_table_reduce = bool(tr.get("overlap_table_reduce", True)) and hasattr(self.store, "table_floats") \
            and dist.is_available() and dist.is_initialized()
        if self.overlap_table_reduce:
            self.renderer.table_grad_hook = lambda t: dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=True)
        self.pose_refiner = None
        if tr["refine_poses"]:
            from .pose import PoseRefiner
            self.pose_refiner = PoseRefiner(self.dataset.R, self.dataset.T, lr=tr["pose_lr"], rot_lr_mult=tr["pose_rot_lr_mult"]).to(self.device)
            self.pose_start_iter = tr["pose_start_iter"]
        self.ray_gen = torch.Generator(device=self.device)
        self.ray_gen.manual_seed(tr["ray_seed"] * 1000003 + self.rank)
        self.train_frames, self.holdout_frames = schedules.split_holdout(tr["holdout"], self.dataset.n_images, self.dataset.stems)
        if self.holdout_frames and self.corr_weight > 0.0:
            raise ValueError("train.holdout with train.corr_weight > 0 is not supported: a correspondence pair would pull rays from a "
                             "held-out frame into the loss")
        self.frame_perm = schedules.FramePermutation(self.dataset.n_images, tr["ray_seed"],    # same on every rank
                                                     frames=self.train_frames if self.holdout_frames else None)
        self.scalars = []
        self._board = None
        self.last_clean_stats = None     # validate_mesh / evaluate_mesh with cleaning: mesh_clean.clean_mesh's counts
        self.last_mesh_colors = None     # validate_mesh with colouring: mesh_color.color_mesh's u8 [V,3] colours and its stats
        self.last_color_stats = None
        self.last_texture = None         # validate_mesh with a texture: (tex u8 [S,S,3], uv [M,3,2], owner [S,S]) of mesh_texture.bake_texture
        self.last_texture_stats = None   # ... and its stats with the re-render PSNR (what <iter>_texture.json holds)
        self.last_simplify_stats = None  # validate_mesh / evaluate_mesh / _select_mesh with simplification: mesh_simplify's counts
        self.last_extract_stats = None   # validate_mesh / evaluate_mesh / visualize_mesh with sparse extraction: its counts
        self.last_vis_dir = None         # visualize_mesh: the render_res/<iter> directory it wrote
        self.last_pose_dir = None        # refine_poses_silhouette / export_poses: the directory the .npz files went to
        self.last_view_dir = None        # render_views: the novel_views/<iter> directory it wrote
        self.last_match_dir = None       # match_frames: the correspondences directory it wrote
        self.last_eval_dir = None        # evaluate_views: the image_eval/<iter> directory it wrote
        self.last_hull = None            # visual_hull: (verts, faces) of the hull it meshed
        self.last_mvs_dir = None         # mvs_depth: the mvs/<iter> directory it wrote
        self.last_fuse_dir = None        # fuse_depth: the fuse/<iter> directory it wrote
        if is_continue:
            ck_dir = os.path.join(self.base_exp_dir, "checkpoints")
            ck = sorted(f for f in os.listdir(ck_dir) if f.endswith(".pth")) if os.path.isdir(ck_dir) else []
            if ck:
                self.load_checkpoint(ck[-1])

    # ------------------------------------------------------------------ schedules (App. A.8)
    @property
    def image_perm(self):
        """Upstream name of the current epoch's frame permutation (with train.holdout: of the positions in train_frames)."""
        return self.frame_perm.perm

    def get_cos_anneal_ratio(self):
        return schedules.cos_anneal_ratio(self.iter_step, self.anneal_end)

    def current_lr(self):
        return self.learning_rate * schedules.lr_factor(self.iter_step, self.warm_up_end, self.end_iter,
                                                        self.learning_rate_alpha)

    def update_learning_rate(self):
        self.lr = self.current_lr()
        return self.lr

    def frame_for_slot(self, slot: int) -> int:
        """Frame of permutation slot `slot`: the permutation is re-drawn once per epoch (upstream re-permutes when
        iter_step % n_images == 0) from the SHARED perm_gen, so every rank holds the same e-th permutation for epoch e
        whatever the world size.  Never a frame of train.holdout."""
        return self.frame_perm.frame(slot)

    # ------------------------------------------------------------------ one iteration (the hot loop)
    def train_iteration(self):
        frame = self.frame_for_slot(schedules.frame_slot(self.iter_step, self.rank, self.world))
        refine = self.pose_refiner is not None and self.iter_step >= self.pose_start_iter
        corr = None
        if self.corr_weight > 0.0 and self.dataset.corr is not None:
            if self.corr_vote_freq and self.iter_step > 0 and self.iter_step % self.corr_vote_freq == 0:
                self.vote_correspondences()
            rays, corr, _ = self.dataset.gen_corr_rays_at(frame, self.batch_size, int(self.batch_size * self.corr_fraction),
                                                         generator=self.ray_gen)
        else:
            rays = self.dataset.gen_random_rays_at(frame, self.batch_size, keep_only=self.keep_only, generator=self.ray_gen)
        near, far = self.dataset._last_near_far
        self._last_rays = rays
        bg = torch.ones(3, device=self.device) if self.use_white_bkgd else None
        # the per-ray perturbation of the coarse samples comes from the SAME checkpointed stream as the pixels
        t_rand = torch.rand([rays.shape[0], 1], device=self.device, generator=self.ray_gen) if self.renderer.perturb > 0 else None
        prior = {}
        if self.depth_weight > 0.0 and self.iter_step >= self.depth_start_iter:
            prior.update(prior_depth=self.dataset.prior_depth_at(frame, *self.dataset._last_pixels), depth_weight=self.depth_weight,
                         depth_delta=self.depth_delta)
        if self.normal_skip_missing:
            prior["normal_skip_missing"] = True
        if self.warp_weight > 0.0 and self.iter_step >= self.warp_conf["start_iter"]:
            from . import warp_loss
            if self.warp_tables is None:
                self.warp_tables = warp_loss.frames_for(self.dataset, self.train_frames, **self.warp_conf)
            prior["warp"] = warp_loss.step_input(self.warp_tables, self.dataset, frame, self.warp_weight)
        self._warp_on = "warp" in prior
        stats = self.renderer.train_step_core(rays, near, far, self.dataset.R[frame], self.get_cos_anneal_ratio(),
                                              self.igr_weight, self.mask_weight, self.normal_weight, background_rgb=bg,
                                              t_rand=t_rand, corr=corr, corr_weight=self.corr_weight,
                                              corr_frames=self.dataset.corr_frames() if corr is not None else None,
                                              corr_delta_px=self.corr_delta_px, ray_grads=refine, **prior)
        self._prior_on = any(k != "warp" for k in prior)
        if refine:
            # chain the per-ray adjoints into this frame's 9 pose numbers (torch autograd over the ray formula), step, and
            # write the refined pose back into the resident frame table the HIP ray gather reads
            px, py = self.dataset._last_pixels
            o, d, Rf = self.pose_refiner.rays(frame, px, py, self.dataset.Kinv)
            d_o, d_d, d_R = self.renderer.last_ray_grads
            self.pose_refiner.step(o, d, Rf, d_o, d_d, d_R, grad_scale=1.0 / self.world,
                                   allreduce=dh_dist.allreduce_sum_ if self.world > 1 else None,
                                   partner=getattr(self.renderer, "last_partner_pose_grads", None))
            with torch.no_grad():
                Rn, Tn = self.pose_refiner.poses()
                self.dataset.R.copy_(Rn); self.dataset.T.copy_(Tn)
        grad = self.store.grad_flat
        pending = getattr(self.renderer, "pending_table_reduce", None)
        if pending is not None:
            # hash family: the table slice is already on its way (started behind the table scatter); reduce the small rest, then join
            dh_dist.allreduce_sum_(grad[self.store.table_floats:])
            pending.wait()
            self.renderer.pending_table_reduce = None
        else:
            dh_dist.allreduce_sum_(grad)                         # RCCL over xGMI: one 3.2 MB bucket
        lr = self.current_lr()          # 0 at iter_step 0, as upstream (update_learning_rate() runs before the loop)
        self.store.adam_step(lr, grad=grad, grad_scale=1.0 / self.world)
        self.iter_step += 1
        return stats

    def train(self, n_iters=None):
        end = self.end_iter if n_iters is None else min(self.end_iter, self.iter_step + n_iters)
        while self.iter_step < end:
            stats = self.train_iteration()
            if self.iter_step % self.report_freq == 0:
                self.report(stats)
            if self.rank == 0 and self.iter_step % self.save_freq == 0:
                self.save_checkpoint()
            if self.rank == 0 and self.val_freq and self.iter_step % self.val_freq == 0:
                self.validate_image()
        self.close()
        return self

    def close(self):
        """Flush and close the scalar writer (train() calls it; safe to call twice)."""
        if self._board is not None:
            self._board.flush()
            self._board.close()
            self._board = None

    def report(self, stats):
        v = dh_dist.mean_stats(stats).tolist()
        # loud, never silent: the two-piece fp16 arithmetic's range watch (one device read, report iterations
        # only) and a finite-loss check
        # (reduced with MAX over the ranks first -- ADVICE r5: a rank that raised alone left the others in the next all-reduce)
        if hasattr(self.renderer, "check_range"):
            self.renderer.check_range(max_over_ranks=lambda x: dh_dist.max_over_ranks(x, self.device))
        if not math.isfinite(v[0]):
            from ._lib import DynhorHipError
            raise DynhorHipError(f"non-finite loss at iteration {self.iter_step}: {v[0]}")
        rec = {"iter": self.iter_step, "Loss/loss": v[0], "Loss/color_loss": v[1], "Loss/eikonal_loss": v[2],
               "Loss/mask_loss": v[3], "Loss/normal_loss": v[4], "Statistics/psnr": v[5],
               **({"Loss/corr_loss": float(self.renderer.last_corr_stats[0]), "Statistics/corr_residual_px": float(self.renderer.last_corr_stats[2])}
                  if self.corr_weight > 0.0 and getattr(self.renderer, "last_corr_stats", None) is not None else {}),
               "Statistics/s_val": float(1.0 / self.store.inv_s().item()), "lr": self.current_lr()}
        if getattr(self, "_prior_on", False) and getattr(self.renderer, "last_prior_stats", None) is not None:
            ps = self.renderer.last_prior_stats.tolist()       # this rank's batch, as the correspondence scalars are
            rec.update({"Loss/depth_loss": ps[0], "Statistics/depth_abs": ps[2], "Statistics/depth_rays": ps[1],
                        "Statistics/normal_rays": ps[5]})
        if getattr(self, "_warp_on", False) and getattr(self.renderer, "last_warp_stats", None) is not None:
            ws = self.renderer.last_warp_stats.tolist()        # this rank's batch
            rec.update({"Loss/warp_loss": ws[0], "Statistics/warp_score": ws[2], "Statistics/warp_rays": ws[1]})
        st = getattr(self.renderer, "last_state", None)
        if st is not None and getattr(self, "_last_rays", None) is not None:
            # upstream Statistics/cdf and Statistics/weight_max (App. A.8), masked by obj*keep like the colour loss
            m = (self._last_rays[:, 9:10] * self._last_rays[:, 10:11])
            msum = float(m.sum()) + 1e-5
            rec["Statistics/cdf"] = float((self.renderer.first_cdf(st) * m).sum()) / msum
            rec["Statistics/weight_max"] = float((st.wmax * m).sum()) / msum
        if self.rank == 0:
            self.scalars.append(rec)
            with open(os.path.join(self.base_exp_dir, "scalars.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")
            # the reference's logger: one scalar per key per step to a SummaryWriter under <exp>/board
            # (ObjTracker/run.py:125-127, jointopt.py:151-153)
            if self._board is None:
                from .tb_events import make_writer
                self._board = make_writer(os.path.join(self.base_exp_dir, "board"))
            for k, v in rec.items():
                if k != "iter":
                    self._board.add_scalar(k, v, self.iter_step)
            self._board.flush()
        return rec

    @torch.no_grad()
    def vote_correspondences(self, chunk=8192):
        """Outlier voting over ALL matches with the current geometry (forward-only render of every matched ray, residuals from
        dh_corr_loss, then Dataset.vote_correspondences).  Every rank evaluates the same matches with the same weights, so
        the certainties stay identical across ranks without a collective."""
        from .renderer import corr_loss
        ds, ren = self.dataset, self.renderer
        res = torch.full((ds.corr.shape[0],), float("nan"), device=self.device)
        for f, (lo, hi) in ds._corr_range.items():
            for s0 in range(lo, hi, chunk):
                m = ds.corr[s0:min(s0 + chunk, hi)]
                B = m.shape[0]
                rays = ds.gen_rays_at_pixels(f, m[:, 0].long(), m[:, 1].long())
                near, far = ds._last_near_far
                o, d = rays[:, :3].contiguous(), rays[:, 3:6].contiguous()
                z = ren.sample_z(o, d, near, far, perturb_overwrite=0)
                st = ren._forward_core(o, d, z, self.get_cos_anneal_ratio(), None, want_nmap=False, infer_only=True)
                corr = torch.cat([m[:, 2:4], torch.ones(B, 1, device=self.device), m[:, 5:6]], -1).contiguous()
                _, r = corr_loss(o, d, z, st.weights, corr, ds.corr_frames(), st.sample_dist, self.corr_delta_px, 1.0,
                                 torch.empty(B, st.n, device=self.device))
                # rays that render (almost) nothing have no surface estimate yet: leave them un-voted (NaN); a match whose point
                # lands behind the partner camera comes back +inf and votes as an outlier
                res[s0:s0 + B] = torch.where(st.wsum.view(-1) > 0.5, r, torch.full_like(r, float("nan")))
        self.last_vote = ds.vote_correspondences(res, tau_px=self.corr_vote_tau_px)
        return self.last_vote

    # ------------------------------------------------------------------ checkpoints (App. A.8 layout)
    def save_checkpoint(self):
        ck = {"nerf": {}, "sdf_network_fine": self.sdf_network.state_dict(),
              "variance_network_fine": self.deviation_network.state_dict(),
              "color_network_fine": self.color_network.state_dict(),
              "optimizer": self.store.optimizer_state_dict(self.current_lr()), "iter_step": self.iter_step,
              # extra keys (upstream loaders ignore them): the ray / permutation RNG streams, so that a resumed run draws
              # the pixels and frames an uninterrupted one would have drawn
              "dynhor_rng": {"ray_gen": self.ray_gen.get_state(), "frame_perm": self.frame_perm.state_dict(),
                             "rank": self.rank, "world": self.world}}
        if self.pose_refiner is not None:
            ck["pose_refiner"] = {"model": self.pose_refiner.state_dict(), "optimizer": self.pose_refiner.opt.state_dict()}
        occ = getattr(self.renderer, "sampler_state_dict", lambda: None)()
        if occ is not None:
            ck["dynhor_occgrid"] = occ
        d = os.path.join(self.base_exp_dir, "checkpoints")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "ckpt_{:0>6d}.pth".format(self.iter_step))
        torch.save({k: (v if not isinstance(v, dict) else _to_cpu(v)) for k, v in ck.items()}, path)
        return path

    def load_checkpoint(self, checkpoint_name):
        path = checkpoint_name if os.path.isabs(checkpoint_name) or os.path.exists(checkpoint_name) else \
            os.path.join(self.base_exp_dir, "checkpoints", checkpoint_name)
        ck = torch.load(path, map_location=self.device, weights_only=False)
        if ck.get("dynhor_rng") is not None:
            self.frame_perm.check_state(ck["dynhor_rng"]["frame_perm"])   # another train.holdout: raise before anything is loaded
        self.sdf_network.load_state_dict(ck["sdf_network_fine"])
        self.deviation_network.load_state_dict(ck["variance_network_fine"])
        self.color_network.load_state_dict(ck["color_network_fine"])
        opt = ck.get("optimizer")
        if opt:
            st = opt.get("state", {})
            extra = len(st) - len(self.store.slices)
            if extra > 0:   # upstream checkpoints list the (unused here) NeRF++ background parameters first
                opt = {"state": {i - extra: v for i, v in st.items() if i >= extra}, "param_groups": opt["param_groups"]}
            self.store.load_optimizer_state_dict(opt)
        self.iter_step = ck["iter_step"]
        if self.pose_refiner is not None and "pose_refiner" in ck:
            self.pose_refiner.load_state_dict(ck["pose_refiner"]["model"])
            self.pose_refiner.opt.load_state_dict(ck["pose_refiner"]["optimizer"])
            with torch.no_grad():
                Rn, Tn = self.pose_refiner.poses()
                self.dataset.R.copy_(Rn); self.dataset.T.copy_(Tn)
        if "dynhor_occgrid" in ck and hasattr(self.renderer, "load_sampler_state_dict"):
            self.renderer.load_sampler_state_dict(ck["dynhor_occgrid"])
        rng = ck.get("dynhor_rng")
        if rng is not None:
            self.frame_perm.load_state_dict(rng["frame_perm"])
            if rng.get("rank", 0) == self.rank and rng.get("world", 1) == self.world:
                self.ray_gen.set_state(rng["ray_gen"].cpu())
            else:   # only rank 0 writes checkpoints: the other ranks restart their own stream at a point no earlier
                    # iteration used (not bit-equal to an uninterrupted run, but no pixel draw is replayed)
                self.ray_gen.manual_seed((self.conf["train"]["ray_seed"] * 1000003 + self.rank) ^ (self.iter_step * 2654435761 % (1 << 31)))
        self.store.bump()

    # ------------------------------------------------------------------ what the opt-in modes share: settings, mesh, compute, write
    def _board_writer(self):
        """The scalar writer under <exp>/board, made at first use."""
        if self._board is None:
            from .tb_events import make_writer
            self._board = make_writer(os.path.join(self.base_exp_dir, "board"))
        return self._board

    def _write_json(self, d, name, res):
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name), "w") as f:
            json.dump(res, f, indent=1)

    def _reseed_pose_refiner(self):
        """With train.refine_poses on: a new PoseRefiner from the dataset's current poses (its Adam state starts afresh).  Returns
        whether there is one."""
        if self.pose_refiner is not None:
            from .pose import PoseRefiner
            tr = self.conf["train"]
            self.pose_refiner = PoseRefiner(self.dataset.R, self.dataset.T, lr=tr["pose_lr"], rot_lr_mult=tr["pose_rot_lr_mult"]).to(self.device)
        return self.pose_refiner is not None

    def _guide_mesh(self, fn, mesh, normalize, resolution, clean, extract, simplify):
        """(verts f32, faces int64, name, clean mode, simplify mode) of the mesh refine_poses_silhouette fits and match_frames /
        mvs_depth take as their guide: _select_mesh with `mesh` / `normalize` left at None taken from the config's mesh_vis: block and
        `resolution` from its pose_sil: block.  A mesh without faces raises."""
        vc = merge("mesh_vis", MESH_VIS_DEFAULTS, self.conf.get("mesh_vis"), {"mesh": mesh, "normalize": normalize})
        resolution = int(resolution if resolution is not None else
                         merge("pose_sil", POSE_SIL_DEFAULTS, self.conf.get("pose_sil"))["resolution"])
        verts, faces, name, cmode = self._select_mesh(fn, vc["mesh"], vc["normalize"], resolution, clean, extract, simplify)
        if faces.shape[0] == 0:
            raise ValueError(f"{fn}: the mesh {name} has no faces")
        return verts.to(torch.float32).contiguous(), faces.to(torch.int64).contiguous(), name, cmode, self._simplify_conf(simplify)["mode"]

    def _template_mesh(self, fn, mesh, normalize):
        """(verts f32, faces int64, mesh, normalize) of the template init_poses and init_sdf start from: the .ply / .obj file `mesh` with
        normalize "none" | "reference"; left at None it is the config's data_info.obj_path, normalised as the reference normalises
        its prior when data_info.normalize_mesh is true."""
        from . import metrics
        di = self.conf["data_info"]
        if mesh is None:
            mesh = di.get("obj_path")
            if normalize is None:
                normalize = "reference" if di.get("normalize_mesh") else "none"
        normalize = normalize if normalize is not None else "none"
        if mesh is None:
            raise ValueError(f"{fn}: no template mesh: give --vis_mesh (with --vis_normalize) or data_info.obj_path (with "
                             "normalize_mesh) in the config")
        if normalize not in ("none", "reference"):
            raise ValueError(f"{fn}: normalize must be 'none' or 'reference', got {normalize!r}")
        verts, faces = metrics.load_mesh(str(mesh))
        if normalize == "reference":
            verts = metrics.normalize_like_reference(verts)[0]
        verts, faces = verts.to(self.device, torch.float32).contiguous(), faces.to(self.device, torch.int64).contiguous()
        if faces.shape[0] == 0:
            raise ValueError(f"{fn}: the template {mesh} has no faces")
        return verts, faces, mesh, normalize

    # ------------------------------------------------------------------ validation
    @torch.no_grad()
    def render_image(self, idx, resolution_level=4, chunk=4096):
        rays, h, w = self.dataset.gen_rays_at(idx, resolution_level)
        near, far = self.dataset._last_near_far
        cols, nrms = [], []
        bg = torch.ones(3, device=self.device) if self.use_white_bkgd else None
        for s in range(0, rays.shape[0], chunk):
            r = rays[s:s + chunk]
            o, d = r[:, :3].contiguous(), r[:, 3:6].contiguous()
            c, nm = self.renderer.render_rays(o, d, near[s:s + chunk], far[s:s + chunk], self.get_cos_anneal_ratio(), bg)
            cols.append(c); nrms.append(nm)
        return torch.cat(cols).view(h, w, 3), torch.cat(nrms).view(h, w, 3), rays.view(h, w, 14)

    @torch.no_grad()
    def validate_image(self, idx=-1, resolution_level=4):
        if idx < 0:
            idx = int(np.random.randint(self.dataset.n_images))
        img, nrm, rays = self.render_image(idx, resolution_level)
        m = (rays[..., 9:10] * rays[..., 10:11])
        mse = (((img - rays[..., 6:9]) ** 2) * m).sum() / (m.sum() * 3.0 + 1e-5)
        psnr = float(20.0 * torch.log10(1.0 / mse.sqrt()))
        if self.rank == 0:
            from PIL import Image
            d = os.path.join(self.base_exp_dir, "validations_fine")
            dn = os.path.join(self.base_exp_dir, "normals")
            os.makedirs(d, exist_ok=True); os.makedirs(dn, exist_ok=True)
            gt = (rays[..., 6:9].clamp(0, 1) * 255).byte().cpu().numpy()
            pr = (img.clamp(0, 1) * 255).byte().cpu().numpy()
            # upstream writes prediction and ground truth side by side
            Image.fromarray(np.concatenate([pr, gt], axis=1)).save(os.path.join(d, "{:0>8d}_{}.png".format(self.iter_step, idx)))
            n_cam = nrm @ self.dataset.R[idx].T                      # object -> camera frame (x_cam = R x_obj)
            nimg = ((n_cam / (n_cam.norm(dim=-1, keepdim=True) + 1e-6)) * 0.5 + 0.5).clamp(0, 1)
            Image.fromarray((nimg * 255).byte().cpu().numpy()).save(os.path.join(dn, "{:0>8d}_{}.png".format(self.iter_step, idx)))
        return psnr

    @torch.no_grad()
    def validate_mesh(self, resolution=64, threshold=0.0, world_space=False, save=True, clean=None, color=None, extract=None,
                      simplify=None, texture=None, texture_size=None):
        """Upstream Runner.validate_mesh / NeuSRenderer.extract_geometry: -sdf on a regular grid over
        the object bounding box (HIP no-grad SDF kernel, 64^3-point chunks), iso-surface by marching cubes (model.mesh_method: 'cubes' | 'tetrahedra')
        (dynhor_amd/mesh.py; mcubes is not available), written as meshes/<iter>.ply.  Returns (vertices, triangles).
        clean: a mesh_clean.clean_mesh mode (None: the config's mesh_clean.mode, default "none").  With a mode other than "none" the raw
        mesh is still written as <iter>.ply, the cleaned one as <iter>_clean.ply, and the cleaned mesh is returned (its counts in
        self.last_clean_stats).
        color: a mesh_color.color_mesh mode (None: the config's mesh_color.mode, default "none").  With a mode other than "none" the
        returned mesh is coloured and additionally written as <iter>_color.ply (colours and stats in self.last_mesh_colors /
        self.last_color_stats); <iter>.ply and <iter>_clean.ply are unchanged.
        extract: "dense" | "sparse" (None: the config's mesh_extract.mode, default "dense"): how the grid is queried
        (NeuSRenderer.extract_geometry's mode; block and lipschitz from the config's mesh_extract: block).  Sparse gives the same mesh
        from far fewer SDF queries and leaves its counts in self.last_extract_stats.
        simplify: none | cells:N | faces:T (None: the config's mesh_simplify.mode, default "none"; mesh_simplify.simplify_mesh).  With a
        mode other than "none" the (cleaned) mesh is simplified before it is coloured, written as <iter>_simple.ply and returned (its
        counts in self.last_simplify_stats); <iter>.ply and <iter>_clean.ply are unchanged and <iter>_color.ply is the simplified mesh.
        texture: none | views | views+network (None: the config's mesh_texture.mode, default "none"; mesh_texture.bake_texture), on an
        atlas of texture_size texels per side (None: the config's mesh_texture.size, default 1024).  With a mode other than "none" the
        mesh that would be coloured (after clean and simplify) gets a texture atlas baked from the frames, written as
        <iter>_textured.obj + <iter>_textured.obj.mtl + <iter>_textured_texture_kd.png, and <iter>_texture.json holds the bake's stats
        and the re-render PSNR per frame (mesh_texture.texture_psnr); texture, coordinates and stats stay in self.last_texture /
        self.last_texture_stats.  Every other file is unchanged."""
        from .mesh import write_ply
        bmin, bmax = self.dataset.object_bbox_min, self.dataset.object_bbox_max
        ec = self._extract_conf(extract)
        verts, faces = self.renderer.extract_geometry(bmin, bmax, resolution=resolution, threshold=threshold,
                                                      method=self.conf.get("model", {}).get("mesh_method", "cubes"),
                                                      mode=ec["mode"], block=int(ec["block"]), lipschitz=float(ec["lipschitz"]))
        self.last_extract_stats = dict(self.renderer.last_extract_stats, mode="sparse", block=int(ec["block"]),
                                       lipschitz=float(ec["lipschitz"])) if ec["mode"] == "sparse" else None
        d = os.path.join(self.base_exp_dir, "meshes")
        if save and self.rank == 0:
            os.makedirs(d, exist_ok=True)
            write_ply(os.path.join(d, "{:0>8d}.ply".format(self.iter_step)), verts, faces)
        mode = self._clean_conf(clean)["mode"]
        if mode != "none":
            verts, faces = self._clean_mesh(verts, faces, clean)
            if save and self.rank == 0:
                write_ply(os.path.join(d, "{:0>8d}_clean.ply".format(self.iter_step)), verts, faces)
        self.last_simplify_stats = None
        if self._simplify_conf(simplify)["mode"] != "none":
            verts, faces = self._simplify_mesh(verts, faces, simplify)
            if save and self.rank == 0:
                os.makedirs(d, exist_ok=True)
                write_ply(os.path.join(d, "{:0>8d}_simple.ply".format(self.iter_step)), verts, faces)
        cc = self._color_conf(color)
        if cc["mode"] != "none":
            from .mesh_color import color_mesh
            self.last_mesh_colors, self.last_color_stats = color_mesh(
                verts, faces, cc["mode"], dataset=self.dataset, renderer=self.renderer, erode_px=int(cc["erode_px"]),
                min_cos=float(cc["min_cos"]), depth_eps=float(cc["depth_eps"]))
            if save and self.rank == 0:
                os.makedirs(d, exist_ok=True)
                write_ply(os.path.join(d, "{:0>8d}_color.ply".format(self.iter_step)), verts, faces, colors=self.last_mesh_colors)
        tc = self._texture_conf(texture, texture_size)
        self.last_texture = self.last_texture_stats = None
        if tc["mode"] != "none":
            from .mesh_texture import bake_texture, texture_psnr, write_textured_obj
            tex, uv, owner, st = bake_texture(verts, faces, self.dataset, size=int(tc["size"]), mode=tc["mode"], renderer=self.renderer,
                                              erode_px=int(tc["erode_px"]), min_cos=float(tc["min_cos"]),
                                              depth_eps=float(tc["depth_eps"]), sharpen=int(tc["sharpen"]))
            ps = texture_psnr(verts, faces, self.dataset, uv, tex, erode_px=int(tc["erode_px"]))
            ds = self.dataset
            stems = list(ds.stems) if ds.stems is not None else ["{:04d}".format(i) for i in range(ds.n_images)]
            fin = lambda x: x if x is None or math.isfinite(x) else None           # an exact match has no finite PSNR
            st = dict(st, iter=self.iter_step, verts=int(verts.shape[0]), psnr=fin(ps["pooled"]), psnr_pixels=ps["count"],
                      frames=[{"stem": s_, "psnr": fin(p_)} for s_, p_ in zip(stems, ps["frames"])])
            self.last_texture, self.last_texture_stats = (tex, uv, owner), st
            if save and self.rank == 0:
                os.makedirs(d, exist_ok=True)
                write_textured_obj(os.path.join(d, "{:0>8d}_textured.obj".format(self.iter_step)), verts, faces, uv, tex,
                                   image=tc["image"])
                self._write_json(d, "{:0>8d}_texture.json".format(self.iter_step), st)
        return verts, faces

    def _texture_conf(self, mode=None, size=None):
        """The YAML's optional mesh_texture: block over MESH_TEXTURE_DEFAULTS; `mode` / `size` (when not None) override its mode / size."""
        from .mesh_texture import IMAGES, MODES
        c = merge("mesh_texture", MESH_TEXTURE_DEFAULTS, self.conf.get("mesh_texture"), {"mode": mode, "size": size})
        one_of("mesh_texture", "mode", c["mode"], MODES)
        int_in("mesh_texture", "size", c["size"], 8, 32768)
        int_in("mesh_texture", "sharpen", c["sharpen"], 0, 4)
        one_of("mesh_texture", "image", c["image"], IMAGES)
        return c

    def _color_conf(self, mode=None):
        """The YAML's optional mesh_color: block over MESH_COLOR_DEFAULTS; `mode` (when not None) overrides its mode."""
        from .mesh_color import MODES
        c = merge("mesh_color", MESH_COLOR_DEFAULTS, self.conf.get("mesh_color"), {"mode": mode})
        one_of("mesh_color", "mode", c["mode"], MODES)
        return c

    def _extract_conf(self, mode=None):
        """The YAML's optional mesh_extract: block over MESH_EXTRACT_DEFAULTS; `mode` (when not None) overrides its mode."""
        from .mesh_extract import MAX_BLOCK, MODES
        c = merge("mesh_extract", MESH_EXTRACT_DEFAULTS, self.conf.get("mesh_extract"), {"mode": mode})
        one_of("mesh_extract", "mode", c["mode"], MODES)
        int_in("mesh_extract", "block", c["block"], 1, MAX_BLOCK)
        if isinstance(c["lipschitz"], bool) or not isinstance(c["lipschitz"], (int, float)) or not c["lipschitz"] > 0:
            raise ValueError(f"mesh_extract lipschitz must be a number > 0, got {c['lipschitz']!r}")
        return c

    def _simplify_conf(self, mode=None):
        """The YAML's optional mesh_simplify: block over MESH_SIMPLIFY_DEFAULTS; `mode` (when not None) overrides its mode."""
        from .mesh_simplify import MAX_CELLS, parse_mode
        c = merge("mesh_simplify", MESH_SIMPLIFY_DEFAULTS, self.conf.get("mesh_simplify"), {"mode": mode})
        c["mode"] = "none" if c["mode"] is None else c["mode"]
        parse_mode(c["mode"])
        if isinstance(c["regularization"], bool) or not isinstance(c["regularization"], (int, float)) or not 0 < c["regularization"] <= 1e6:
            raise ValueError(f"mesh_simplify regularization must be a number in (0, 1e6], got {c['regularization']!r}")
        int_in("mesh_simplify", "cells_max", c["cells_max"], 1, MAX_CELLS)
        return c

    def _simplify_mesh(self, verts, faces, mode=None):
        """mesh_simplify.simplify_by_mode with the config's parameters; the counts go to self.last_simplify_stats."""
        from .mesh_simplify import simplify_by_mode
        c = self._simplify_conf(mode)
        verts, faces, self.last_simplify_stats = simplify_by_mode(
            verts.to(self.device, torch.float32).contiguous(), faces.to(self.device, torch.int64).contiguous(), c["mode"],
            regularization=float(c["regularization"]), cells_max=int(c["cells_max"]))
        self.last_simplify_stats["mode"] = c["mode"]
        return verts, faces

    def _clean_conf(self, mode=None):
        """The YAML's optional mesh_clean: block over MESH_CLEAN_DEFAULTS; `mode` (when not None) overrides its mode."""
        from .mesh_clean import MODES
        c = merge("mesh_clean", MESH_CLEAN_DEFAULTS, self.conf.get("mesh_clean"), {"mode": mode})
        one_of("mesh_clean", "mode", c["mode"], MODES)
        return c

    def _clean_mesh(self, verts, faces, mode=None):
        """mesh_clean.clean_mesh with the config's parameters, the dataset's labels and its current (refined) poses."""
        from .mesh_clean import clean_mesh
        c = self._clean_conf(mode)
        verts, faces, self.last_clean_stats = clean_mesh(verts, faces, self.dataset, c["mode"], dilate_px=int(c["dilate_px"]),
                                                         min_bg_votes=int(c["min_bg_votes"]), min_area_frac=c["min_area_frac"])
        return verts, faces

    @torch.no_grad()
    def evaluate_mesh(self, gt_mesh=None, gt_normalize=None, resolution=None, n_samples=None, taus=None, seed=0, save=True,
                      gt_resolution=None, clean=None, extract=None, gt_align=None, gt_align_init=None, align_opts=None, simplify=None):
        """Geometry metrics of the current reconstruction against a ground-truth surface (dynhor_amd/metrics.py: Chamfer distance,
        F-score, normal consistency; definitions in its docstring).  The mesh is extracted as validate_mesh does (renderer
        extract_geometry over the object bounding box, model.mesh_method) at `resolution`, then scored by metrics.mesh_metrics.

        Ground truth: the mesh file `gt_mesh` (.obj / .ply), in the canonical frame (gt_normalize "none") or brought into it as the
        reference normalises its shape prior (gt_normalize "reference": metrics.normalize_like_reference; the result then carries
        gt_scale).  Without one, a synthetic dataset's true surface is the zero level set of scene.scene_sdf, extracted by marching
        cubes at gt_resolution over [-0.55, 0.55]^3; any other dataset raises ValueError.  Arguments left at None take the YAML's
        optional `eval:` block (gt_mesh, gt_normalize, resolution, gt_resolution, n_samples, taus), else 512 / 1,000,000 /
        (0.005, 0.01, 0.02).  data_info.obj_path is NOT ground truth (the reference's stage-1 shape prior) and is never used.
        clean: a mesh_clean.clean_mesh mode (None: the config's mesh_clean.mode, default "none"); with a mode other than "none" the
        cleaned mesh is scored and the dict gains clean, clean_removed_verts, clean_removed_faces and clean_components.
        extract: validate_mesh's extraction mode (None: the config's mesh_extract.mode).  With "sparse" the reconstruction AND the
        analytic ground truth are extracted sparsely (the ground truth at lipschitz 1, exact for that field) and the dict gains
        extract, extract_block, extract_lipschitz, extract_blocks, extract_active_blocks, extract_samples and extract_dense_samples.
        gt_align: "none" | "rigid" | "similarity" (None: eval.gt_align, default "none"), gt_align_init: "identity" | "global" (None:
        eval.gt_align_init, default "identity"), align_opts: options over mesh_align.ALIGN_DEFAULTS (None: eval.align_opts).  With a mode
        other than "none" the ground truth (after gt_normalize) is registered to the mesh that is scored -- the cleaned one when cleaning
        is on -- by trimmed ICP before the metrics are taken (metrics.mesh_metrics says what the dict gains); rank 0 then also writes
        meshes/<iter:08d>_gt_aligned.ply, the ground truth in the canonical frame: load it next to <iter>.ply to see the registration.
        The analytic ground truth of a synthetic dataset accepts the flags too (it is aligned already: a self-check).
        simplify: validate_mesh's simplification mode (None: the config's mesh_simplify.mode).  With a mode other than "none" the
        (cleaned) mesh is simplified before it is scored and the dict gains `simplify`: the mode and mesh_simplify.simplify_mesh's stats.
        Rank 0 writes meshes/<iter:08d>_eval.json and logs every number as eval/<key> to <exp>/board.  Returns the dict."""
        from . import metrics
        ec = merge("eval", EVAL_DEFAULTS, {k: v for k, v in (self.conf.get("eval") or {}).items() if v is not None},
                   dict(gt_mesh=gt_mesh, gt_normalize=gt_normalize, resolution=resolution, gt_resolution=gt_resolution, n_samples=n_samples,
                        taus=taus, gt_align=gt_align, gt_align_init=gt_align_init, align_opts=align_opts))
        gt_mesh, gt_normalize, gt_align, gt_align_init, align_opts = (ec[k] for k in ("gt_mesh", "gt_normalize", "gt_align", "gt_align_init",
                                                                                      "align_opts"))
        resolution, gt_resolution, n_samples = int(ec["resolution"]), int(ec["gt_resolution"]), int(ec["n_samples"])
        taus = tuple(float(t) for t in ec["taus"])
        metrics.check_align_args("evaluate_mesh", gt_align, gt_align_init)
        if gt_mesh is not None:
            gt_v, gt_f = metrics.load_mesh(gt_mesh)
            gt_name = str(gt_mesh)
        elif getattr(self.dataset, "synthetic", False):
            gt_v, gt_f = self._scene_gt_mesh(gt_resolution, mode=self._extract_conf(extract)["mode"])
            gt_name = f"scene_sdf@{gt_resolution}"
            gt_normalize = "none"                      # the analytic scene is defined in the canonical frame
        else:
            raise ValueError("evaluate_mesh: no ground truth -- pass gt_mesh (or set eval.gt_mesh in the config); only a synthetic "
                             "dataset has one built in")
        verts, faces = self.validate_mesh(resolution=resolution, save=False, clean="none", extract=extract, simplify="none",
                                          texture="none")
        mode = self._clean_conf(clean)["mode"]
        if mode != "none":
            verts, faces = self._clean_mesh(verts, faces, clean)
        smode = self._simplify_conf(simplify)["mode"]
        if smode != "none":
            verts, faces = self._simplify_mesh(verts, faces, simplify)
        res = metrics.mesh_metrics(verts, faces, gt_v, gt_f, n_samples=n_samples, taus=taus, seed=seed, gt_normalize=gt_normalize,
                                   device=self.device, gt_align=gt_align, gt_align_init=gt_align_init, align_opts=align_opts)
        res.update(iter=self.iter_step, resolution=resolution, gt=gt_name)
        if mode != "none":
            st = self.last_clean_stats
            res.update(clean=mode, clean_removed_verts=st["removed_verts"], clean_removed_faces=st["removed_faces"],
                       clean_components=st["components"])
        if smode != "none":
            res.update(simplify=dict(self.last_simplify_stats))
        es = self.last_extract_stats
        if es is not None:
            res.update(extract="sparse", extract_block=es["block"], extract_lipschitz=es["lipschitz"], extract_blocks=es["blocks"],
                       extract_active_blocks=es["active_blocks"], extract_samples=es["samples"],
                       extract_dense_samples=es["dense_samples"])
        if save and self.rank == 0:
            d = os.path.join(self.base_exp_dir, "meshes")
            self._write_json(d, "{:0>8d}_eval.json".format(self.iter_step), res)
            if gt_align != "none":
                from .mesh import write_ply
                write_ply(os.path.join(d, "{:0>8d}_gt_aligned.ply".format(self.iter_step)),
                          metrics.aligned_ground_truth(gt_v, res, gt_normalize), gt_f)
            board = self._board_writer()
            for k, v in res.items():
                if k != "iter" and isinstance(v, (int, float)):
                    board.add_scalar("eval/" + k, float(v), self.iter_step)
            board.flush()
        return res

    @torch.no_grad()
    def _select_mesh(self, fn, mesh, normalize, resolution, clean, extract, simplify=None):
        """(verts, faces, name, clean mode) of the mesh visualize_mesh draws and refine_poses_silhouette fits: the .ply / .obj file `mesh`
        (metrics.load_mesh; normalize "none" | "reference"), else the reconstruction extracted as validate_mesh extracts it at
        `resolution` (no .ply written); cleaned when `clean` (None: the config's mesh_clean.mode) says so, then simplified when
        `simplify` (None: the config's mesh_simplify.mode) says so -- a mesh from a file too."""
        from . import metrics
        if normalize not in ("none", "reference"):
            raise ValueError(f"{fn}: normalize must be 'none' or 'reference', got {normalize!r}")
        if mesh is None:
            verts, faces = self.validate_mesh(resolution=resolution, save=False, clean="none", color="none", extract=extract,
                                              simplify="none", texture="none")
            name = f"reconstruction@{resolution}"
        else:
            verts, faces = metrics.load_mesh(str(mesh))
            if normalize == "reference":
                verts = metrics.normalize_like_reference(verts)[0]
            verts, faces = verts.to(self.device).contiguous(), faces.to(self.device).contiguous()
            name = str(mesh)
        cmode = self._clean_conf(clean)["mode"]
        if cmode != "none":
            verts, faces = self._clean_mesh(verts, faces, clean)
        if self._simplify_conf(simplify)["mode"] != "none":
            verts, faces = self._simplify_mesh(verts, faces, simplify)
        return verts, faces, name, cmode

    @torch.no_grad()
    def visualize_mesh(self, mesh=None, normalize=None, resolution=None, clean=None, color=None, alpha=None, turntable=None, save=True,
                       extract=None, simplify=None):
        """The mesh drawn over every frame at the dataset's current poses (refined ones included) and its silhouette IoU against the
        object labels, hand pixels excluded (dynhor_amd/mesh_vis.py).  The mesh: the reconstruction, extracted as validate_mesh
        extracts it at `resolution` (no .ply written), or the .ply / .obj file `mesh` (metrics.load_mesh), taken as in the canonical
        frame (normalize "none") or normalised as the reference normalises its prior (normalize "reference").  clean / color: the
        mesh_clean / mesh_color modes of validate_mesh (None: the config's blocks), applied to whichever mesh is drawn; with a colour
        mode the shading uses the vertex colours.  A textured .obj (`vt` lines and a `map_Kd` image, mesh_texture.load_textured_obj) that
        is neither cleaned, simplified nor coloured is drawn with its texture, lit (silhouette.json then carries `textured`: true); a
        mesh without a texture is drawn exactly as before.  extract: validate_mesh's extraction mode for the reconstruction.  simplify:
        validate_mesh's simplification mode, applied after cleaning (silhouette.json then carries `simplify`).  Arguments left at
        None take the YAML's optional mesh_vis: block over MESH_VIS_DEFAULTS.  Rank 0 writes render_res/<iter:08d>/<stem>.jpg for every frame (quality 95), silhouette.json (the summary
        plus iter, mesh, clean, color, alpha), turntable.gif when turntable > 0 (orbit_cameras, 100 ms per frame, looping), and logs
        vis/iou_mean, vis/iou_median, vis/iou_min to <exp>/board.  Returns the mesh_vis.silhouette_summary dict with those keys (the
        other ranks return None)."""
        from .mesh_vis import orbit_cameras, overlay_frames, silhouette_summary, turntable as render_turntable
        if self.rank != 0:
            return None
        vc = merge("mesh_vis", MESH_VIS_DEFAULTS, self.conf.get("mesh_vis"),
                   {"mesh": mesh, "normalize": normalize, "resolution": resolution, "alpha": alpha, "turntable": turntable})
        mesh, normalize = vc["mesh"], vc["normalize"]
        resolution, alpha, n_turn = int(vc["resolution"]), float(vc["alpha"]), int(vc["turntable"])
        verts, faces, name, cmode = self._select_mesh("visualize_mesh", mesh, normalize, resolution, clean, extract, simplify)
        smode = self._simplify_conf(simplify)["mode"]
        cc = self._color_conf(color)
        colors = None
        if cc["mode"] != "none":
            from .mesh_color import color_mesh
            colors, self.last_color_stats = color_mesh(verts, faces, cc["mode"], dataset=self.dataset, renderer=self.renderer,
                                                       erode_px=int(cc["erode_px"]), min_cos=float(cc["min_cos"]),
                                                       depth_eps=float(cc["depth_eps"]))
        textured = None                                          # (uv, tex) of a mesh file that brings its own texture
        if mesh is not None and str(mesh).lower().endswith(".obj") and cmode == "none" and smode == "none" and cc["mode"] == "none":
            from .mesh_texture import load_textured_obj
            _, tfaces, tuv, ttex = load_textured_obj(str(mesh))
            if tuv is not None and torch.equal(tfaces, faces.cpu()):
                textured = (tuv.to(self.device).contiguous(), ttex.to(self.device).contiguous())
        ds = self.dataset
        stems = list(ds.stems) if ds.stems is not None else ["{:04d}".format(i) for i in range(ds.n_images)]
        d = os.path.join(self.base_exp_dir, "render_res", "{:0>8d}".format(self.iter_step))
        sink, pool, pending = None, None, []
        if save:
            from concurrent.futures import ThreadPoolExecutor
            from PIL import Image
            os.makedirs(d, exist_ok=True)
            pool = ThreadPoolExecutor(max_workers=VIS_WRITERS)

            def write(path, img):
                Image.fromarray(img).save(path, quality=95)

            def sink(f0, out):
                host = out.cpu().numpy()
                pending.extend(pool.submit(write, os.path.join(d, stems[f0 + k] + ".jpg"), host[k]) for k in range(host.shape[0]))
        try:
            counts = overlay_frames(verts, faces, ds, colors=colors, alpha=alpha, sink=sink, texture=textured)
            res = silhouette_summary(counts.cpu(), stems)
            res.update(iter=self.iter_step, mesh=name, clean=cmode, color=cc["mode"], alpha=alpha)
            if textured is not None:
                res.update(textured=True)
            if smode != "none":
                res.update(simplify=smode, faces=int(faces.shape[0]))
            if save and n_turn > 0:
                Ro, To = orbit_cameras(ds.R, ds.T, n_turn)
                imgs = render_turntable(verts, faces, ds.K, ds.H, ds.W, Ro, To, colors=colors, texture=textured).cpu().numpy()
                frames = [Image.fromarray(im) for im in imgs]
                frames[0].save(os.path.join(d, "turntable.gif"), save_all=True, append_images=frames[1:], duration=100, loop=0)
        finally:
            for fut in pending:
                fut.result()
            if pool is not None:
                pool.shutdown()
        if save:
            self._write_json(d, "silhouette.json", res)
            self.last_vis_dir = d
            board = self._board_writer()
            for k in ("iou_mean", "iou_median", "iou_min"):
                if res[k] is not None:
                    board.add_scalar("vis/" + k, float(res[k]), self.iter_step)
            board.flush()
        return res

    # ------------------------------------------------------------------ novel views, depth and normal maps (surface_render.py)
    def _surface_conf(self, method=None, level=None, background=None):
        """The YAML's optional surface_render: block over SURFACE_RENDER_DEFAULTS; arguments that are not None override it."""
        from .surface_render import BACKGROUNDS
        c = merge("surface_render", SURFACE_RENDER_DEFAULTS, self.conf.get("surface_render"),
                  {"method": method, "level": level, "background": background})
        unknown = set(c) - set(SURFACE_RENDER_DEFAULTS)
        if unknown:
            raise ValueError(f"surface_render: unknown keys {sorted(unknown)}")
        if c["method"] not in ("surface", "volume"):
            raise ValueError(f"surface_render method must be 'surface' or 'volume', got {c['method']!r}")
        one_of("surface_render", "background", c["background"], BACKGROUNDS)
        if not is_int(c["level"]) or c["level"] < 1:
            raise ValueError(f"surface_render level must be an integer >= 1, got {c['level']!r}")
        if c["method"] == "volume" and c["background"] == "frame":
            raise ValueError("surface_render: method 'volume' has no hit mask to lay over a frame; use background 'white' or 'black'")
        return c

    @torch.no_grad()
    def _render_views_volume(self, R, T, level, background, chunk=4096):
        """The views by renderer.render_rays on surface_render.volume_rays: (rgb u8 [V,h,w,3], normal u8 [V,h,w,3])."""
        from .surface_render import volume_rays
        ds = self.dataset
        bg = torch.ones(3, device=self.device) if background == "white" else None
        rgbs, nrms = [], []
        for v in range(R.shape[0]):
            o, d, near, far, h, w = volume_rays(R[v:v + 1], T[v:v + 1], ds.K, ds.H, ds.W, level)
            cols, ns = [], []
            for s in range(0, o.shape[0], chunk):
                c, nm = self.renderer.render_rays(o[s:s + chunk].contiguous(), d[s:s + chunk].contiguous(), near[s:s + chunk],
                                                  far[s:s + chunk], self.get_cos_anneal_ratio(), bg)
                cols.append(c); ns.append(nm)
            img, nrm = torch.cat(cols).view(h, w, 3), torch.cat(ns).view(h, w, 3)
            n_cam = nrm @ R[v].T
            nimg = ((n_cam / (n_cam.norm(dim=-1, keepdim=True) + 1e-6)) * 0.5 + 0.5).clamp(0, 1)
            rgbs.append((img.clamp(0, 1) * 255.0).round().to(torch.uint8)); nrms.append((nimg * 255).byte())
        return torch.stack(rgbs), torch.stack(nrms)

    @torch.no_grad()
    def _draw_views(self, c, R, T, frame_of):
        """One chunk of views (R [V,3,3], T [V,3] float32 on the device) drawn as the surface_render settings `c` say: render_surface's
        dict, or {"rgb", "normal"} for method volume.  frame_of: the views' frames (background frame), or None."""
        from . import surface_render as sr
        ds = self.dataset
        if c["method"] == "surface":
            targs = {k: c[k] for k in sr.TRACE_DEFAULTS}
            return sr.render_surface(self.renderer, R, T, ds.K, ds.H, ds.W, level=int(c["level"]), background=c["background"],
                                     frames=frame_of, frame_rgb=ds.rgb if c["background"] == "frame" else None, **targs)
        rgb, normal = self._render_views_volume(R, T, int(c["level"]), c["background"])
        return {"rgb": rgb, "normal": normal}

    @torch.no_grad()
    def render_views(self, views="frames", level=None, method=None, background=None, save=True):
        """Pictures of the networks themselves from any pose (dynhor_amd/surface_render.py): views "frames" (every training frame at its
        current pose), "interpolate:i:j:n" (n poses from frame i to frame j and back, upstream's interpolate_<i>_<j> video) or "orbit:n"
        (frame 0's pose with the object turned about its z axis).  method "surface" sphere-traces the SDF (render_surface: colour, depth
        and normal maps, hit mask); "volume" draws the same views with render_rays (no depth map, no hit mask; the yardstick of the
        timing).  level = pixel stride; background white | black | frame (the view's own frame behind the object: "frames" only).
        Arguments left at None take the YAML's optional surface_render: block over SURFACE_RENDER_DEFAULTS.
        Rank 0 writes novel_views/<iter:08d>/<name>.png, <name>_normal.png, <name>_depth.npy (surface only), views.gif (100 ms per
        view, looping) and views.json, and returns its content plus `dir` and the images on the host: `rgb` u8 [V,h,w,3], `normal`
        and, for method surface, `depth` and `hit` (the other ranks return None).  Views are drawn, scored and written in chunks of at
        most surface_render.MAX_RAYS rays, so the device never holds more than a chunk's images and ground truth.  For "frames" views.json holds per-frame PSNR (validate_image's mask and formula) and, for method surface, the IoU of the
        hit mask against label > 0 with hand pixels excluded (the rule of vis/iou_*), their means and the five worst frames; view/psnr
        and view/iou are logged to <exp>/board."""
        from . import surface_render as sr
        if self.rank != 0:
            return None
        ds = self.dataset
        c = self._surface_conf(method, level, background)
        spec = sr.parse_views(views, ds.n_images)
        if c["background"] == "frame" and spec[0] != "frames":
            raise ValueError("render_views: background 'frame' needs views 'frames' (another pose has no frame of its own)")
        names, R64, T64, frame_of = sr.view_poses(spec, ds.R, ds.T)
        if spec[0] == "frames" and ds.stems is not None:
            names = list(ds.stems)
        R = R64.to(self.device, torch.float32).contiguous()
        T = T64.to(self.device, torch.float32).contiguous()
        L = int(c["level"])
        res = {"iter": self.iter_step, "views": views, "method": c["method"], "level": L, "background": c["background"], "names": names}
        surface = c["method"] == "surface"
        score = spec[0] == "frames"
        d = os.path.join(self.base_exp_dir, "novel_views", "{:0>8d}".format(self.iter_step))
        if save:
            from PIL import Image
            os.makedirs(d, exist_ok=True)
        h, w = sr.image_size(ds.H, ds.W, L)
        per = max(1, sr.MAX_RAYS // (h * w))                   # views per chunk: images, ground truth and scores never hold more
        keys = ("rgb", "normal", "depth", "hit") if surface else ("rgb", "normal")
        host = {k: [] for k in keys}
        stats, psnr, iou = None, [], []
        for v0 in range(0, R.shape[0], per):
            v1 = min(R.shape[0], v0 + per)
            out = self._draw_views(c, R[v0:v1], T[v0:v1], frame_of[v0:v1] if frame_of is not None else None)
            if surface:
                stats = sr.merge_stats(stats, out["stats"])
            if score:
                gt = ds.rgb[v0:v1, ::L, ::L].float() / 255.0
                lab = ds.label[v0:v1, ::L, ::L]
                m = (lab > 0).float()[..., None]
                mse = (((out["rgb"].float() / 255.0 - gt) ** 2) * m).sum(dim=(1, 2, 3)) / (m.sum(dim=(1, 2, 3)) * 3.0 + 1e-5)
                psnr += [float(p) for p in (20.0 * torch.log10(1.0 / mse.sqrt())).tolist()]
                if surface:
                    keep, obj, hb = lab >= 0, lab > 0, out["hit"] > 0
                    inter = (hb & obj & keep).sum(dim=(1, 2)).double()
                    union = ((hb | obj) & keep).sum(dim=(1, 2)).double()
                    iou += [float(x) for x in torch.where(union > 0, inter / union.clamp(min=1), torch.ones_like(union)).tolist()]
            chunk = {k: out[k].cpu() for k in keys}
            for k in keys:
                host[k].append(chunk[k])
            if save:
                for n in range(v1 - v0):
                    name = names[v0 + n]
                    Image.fromarray(chunk["rgb"][n].numpy()).save(os.path.join(d, name + ".png"))
                    Image.fromarray(chunk["normal"][n].numpy()).save(os.path.join(d, name + "_normal.png"))
                    if surface:
                        np.save(os.path.join(d, name + "_depth.npy"), chunk["depth"][n].numpy())
        host = {k: torch.cat(v) for k, v in host.items()}
        if surface:
            res["stats"] = stats
        if score:
            res["psnr"] = psnr
            finite = [p for p in psnr if math.isfinite(p)]
            res["psnr_mean"] = float(np.mean(finite)) if finite else None
            order = sorted(range(len(psnr)), key=lambda k: psnr[k])
            res["worst_psnr"] = [{"frame": names[k], "psnr": psnr[k]} for k in order[:5]]
            if surface:
                res["iou"] = iou
                res["iou_mean"] = float(np.mean(iou))
                order = sorted(range(len(iou)), key=lambda k: iou[k])
                res["worst_iou"] = [{"frame": names[k], "iou": iou[k]} for k in order[:5]]
        if save:
            frames = [Image.fromarray(im) for im in host["rgb"].numpy()]
            frames[0].save(os.path.join(d, "views.gif"), save_all=True, append_images=frames[1:], duration=100, loop=0)
            self._write_json(d, "views.json", res)
            if score:
                board = self._board_writer()
                for k in ("psnr", "iou"):
                    if res.get(k + "_mean") is not None:
                        board.add_scalar("view/" + k, float(res[k + "_mean"]), self.iter_step)
                board.flush()
        self.last_view_dir = d if save else None
        return dict(res, dir=self.last_view_dir, **host)

    # ------------------------------------------------------------------ renderings scored against the frames (image_metrics.py)
    def _image_eval_conf(self, frames=None, maps=None):
        """The YAML's optional image_eval: block over IMAGE_EVAL_DEFAULTS; arguments that are not None override it."""
        c = merge("image_eval", IMAGE_EVAL_DEFAULTS, self.conf.get("image_eval"),
                  {"frames": frames, "maps": None if maps is None else bool(maps)}, check_block="keys")
        if not is_int(c["erode_px"]) or c["erode_px"] < 0:
            raise ValueError(f"image_eval erode_px must be an integer >= 0, got {c['erode_px']!r}")
        return c

    def eval_frame_indices(self, spec="auto"):
        """Sorted frame indices of an image_eval.frames value: auto (the held-out frames if there are any, else all), all, train,
        holdout, every:K[:offset] or frame names.  An empty selection raises."""
        n = self.dataset.n_images
        if spec == "auto":
            idx = list(self.holdout_frames) if self.holdout_frames else list(range(n))
        elif spec == "train":
            idx = list(self.train_frames)
        elif spec == "holdout":
            idx = list(self.holdout_frames)
        else:
            idx = schedules.select_frames(spec, n, self.dataset.stems, "image_eval.frames")
        if not idx:
            raise ValueError(f"image_eval.frames {spec!r} selects no frame (train.holdout is {self.conf['train']['holdout']!r})")
        return idx

    @torch.no_grad()
    def evaluate_views(self, frames=None, maps=None, level=None, method=None, background=None, save=True):
        """Image metrics of the networks' renderings against the frames (dynhor_amd/image_metrics.py): the chosen frames are drawn at
        their current poses as render_views draws them (surface_render: block or the arguments; chunks of at most
        surface_render.MAX_RAYS rays) and scored against the frames' pixels 0, level, 2 level, ... over usable =
        mesh_color.usable_map(label, erode_px) subsampled the same way: masked SSIM over the counted pixels, PSNR and L1 over the
        usable ones (image_metrics.ssim_frames).  frames / maps: None takes the YAML's optional image_eval: block over
        IMAGE_EVAL_DEFAULTS (eval_frame_indices says what `frames` may be).  A held-out frame (train.holdout) is scored at its input
        pose.  Rank 0 writes image_eval/<iter:08d>/eval.json (settings, method, per frame name / split / psnr / ssim / ssim_std / l1 /
        counted / usable, the means per split and overall, the five worst frames by SSIM) and, with maps, <name>_ssim.png (grey
        clamp(s, 0, 1), black where the pixel is not counted), logs eval_img/{psnr,ssim}_{train,holdout} to <exp>/board and returns
        the JSON's content plus `dir` and, with maps, `map` float32 [n,h,w] on the host (the other ranks return None)."""
        from . import image_metrics as im
        from . import surface_render as sr
        from .mesh_color import usable_map
        if self.rank != 0:
            return None
        ds = self.dataset
        c = self._surface_conf(method, level, background)
        ec = self._image_eval_conf(frames, maps)
        idx = self.eval_frame_indices(ec["frames"])
        names = schedules.frame_names(ds.n_images, ds.stems)
        held = set(self.holdout_frames)
        _, R64, T64, _ = sr.view_poses(("frames",), ds.R, ds.T)
        R = R64.to(self.device, torch.float32).contiguous()
        T = T64.to(self.device, torch.float32).contiguous()
        L = int(c["level"])
        h, w = sr.image_size(ds.H, ds.W, L)
        per = max(1, sr.MAX_RAYS // (h * w))
        d = os.path.join(self.base_exp_dir, "image_eval", "{:0>8d}".format(self.iter_step))
        if save:
            os.makedirs(d, exist_ok=True)
        rows, host_maps = [], []
        for v0 in range(0, len(idx), per):
            sel = idx[v0:v0 + per]
            st = torch.tensor(sel, dtype=torch.long, device=self.device)
            out = self._draw_views(c, R[st].contiguous(), T[st].contiguous(), sel)
            gt = ds.rgb[st][:, ::L, ::L].contiguous()
            usable = usable_map(ds.label[st].contiguous(), ec["erode_px"])[:, ::L, ::L].contiguous()
            r = im.ssim_frames(out["rgb"].contiguous(), gt, usable, sigma=ec["sigma"], radius=ec["radius"],
                               min_weight=ec["min_weight"], want_map=ec["maps"], chunk=per)
            for k, f in enumerate(sel):
                rows.append({"frame": names[f], "index": f, "split": "holdout" if f in held else "train", "psnr": r["psnr"][k],
                             "ssim": r["ssim"][k], "ssim_std": r["ssim_std"][k], "l1": r["l1"][k], "counted": r["counted"][k],
                             "usable": r["usable"][k]})
            if ec["maps"]:
                m = r["map"].cpu()
                host_maps.append(m)
                if save:
                    from PIL import Image
                    grey = (m.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).numpy()
                    for k, f in enumerate(sel):
                        Image.fromarray(grey[k]).save(os.path.join(d, names[f] + "_ssim.png"))

        def mean(split, key):
            v = [x[key] for x in rows if (split is None or x["split"] == split) and x[key] is not None and math.isfinite(x[key])]
            return float(np.mean(v)) if v else None

        res = {"iter": self.iter_step, "method": c["method"], "level": L, "background": c["background"], "settings": dict(ec),
               "frames": rows, "n_train": sum(x["split"] == "train" for x in rows),
               "n_holdout": sum(x["split"] == "holdout" for x in rows)}
        for key in ("psnr", "ssim", "l1"):
            res[key + "_mean"] = mean(None, key)
            for split in ("train", "holdout"):
                res[f"{key}_{split}"] = mean(split, key)
        scored = sorted((x for x in rows if x["ssim"] is not None), key=lambda x: x["ssim"])
        res["worst_ssim"] = [{"frame": x["frame"], "ssim": x["ssim"], "psnr": x["psnr"]} for x in scored[:5]]
        if save:
            self._write_json(d, "eval.json", res)
            board = self._board_writer()
            for key in ("psnr", "ssim"):
                for split in ("train", "holdout"):
                    if res[f"{key}_{split}"] is not None:
                        board.add_scalar(f"eval_img/{key}_{split}", res[f"{key}_{split}"], self.iter_step)
            board.flush()
        self.last_eval_dir = d if save else None
        res = dict(res, dir=self.last_eval_dir)
        if ec["maps"]:
            res["map"] = torch.cat(host_maps)
        return res

    # ------------------------------------------------------------------ poses out (the reference's hand-off format)
    def export_poses(self, dir=None):
        """The dataset's CURRENT poses (photometrically or silhouette-refined ones included) as <dir>/<stem>.npz with R [3,3], T [1,3],
        K [3,3] float32: the layout ObjTracker/run.py:172-179 writes and Dataset reads through data_info.obj_infos.  A frame that was
        loaded with an obj_scale s != 1 gets T * s and obj_scale written back, so the file round-trips through Dataset._load_from_disk.
        dir None: <exp>/poses/<iter:08d>/obj_infos.  Rank 0 writes; returns the directory."""
        ds = self.dataset
        d = dir if dir is not None else os.path.join(self.base_exp_dir, "poses", "{:0>8d}".format(self.iter_step), "obj_infos")
        if self.rank == 0:
            os.makedirs(d, exist_ok=True)
            stems = list(ds.stems) if ds.stems is not None else ["{:04d}".format(i) for i in range(ds.n_images)]
            R = ds.R.detach().cpu().numpy().astype(np.float32)
            T = ds.T.detach().cpu().numpy().astype(np.float32)
            K = ds.K.detach().cpu().numpy().astype(np.float32)
            scale = ds.obj_scale.cpu().numpy().astype(np.float32) if ds.obj_scale is not None else None
            for k, stem in enumerate(stems):
                if scale is None or scale[k] == 1.0:
                    np.savez(os.path.join(d, stem + ".npz"), R=R[k], T=T[k].reshape(1, 3), K=K)
                else:
                    np.savez(os.path.join(d, stem + ".npz"), R=R[k], T=(T[k] * scale[k]).reshape(1, 3), K=K, obj_scale=scale[k])
        self.last_pose_dir = d
        return d

    def _photo_term(self, mode, pp, verts, faces, mesh, cmode, smode):
        """The pose_photo.PhotometricTerm of refine_poses_silhouette: `pp` the merged pose_photo: block.  "views": the mesh being fitted
        coloured from the frames at the current poses (mesh_color, mode "views": unseen vertices grey); "mesh": the vertex colours of the
        .ply file `mesh`, or the texture of the .obj file `mesh` (mesh_texture.load_textured_obj), which must reach the fit neither
        cleaned nor simplified."""
        from .pose_photo import make_term
        fn = "refine_poses_silhouette"
        kw = dict(n_points=int(pp["points"]), seed=int(pp["seed"]), erode_px=int(pp["erode_px"]), levels=tuple(pp["levels"]),
                  delta=float(pp["delta"]), a_min=float(pp["a_min"]), min_cos=float(pp["min_cos"]), depth_eps=float(pp["depth_eps"]))
        if mode == "views":
            from .mesh_color import color_mesh
            colors, _ = color_mesh(verts, faces, "views", dataset=self.dataset, erode_px=int(pp["erode_px"]),
                                   min_cos=MESH_COLOR_DEFAULTS["min_cos"], depth_eps=float(pp["depth_eps"]))
            return make_term(verts, faces, self.dataset, vertex_colors=colors, **kw)
        if mesh is None or cmode != "none" or smode != "none":
            raise ValueError(f"{fn}: pose_photo 'mesh' takes the colours of a mesh file (--vis_mesh) that is neither cleaned nor simplified")
        if str(mesh).lower().endswith(".obj"):
            from .mesh_texture import load_textured_obj
            _, tfaces, uv, tex = load_textured_obj(str(mesh))
            if uv is None or not torch.equal(tfaces, faces.cpu()):
                raise ValueError(f"{fn}: pose_photo 'mesh' needs a textured .obj (vt lines and a map_Kd image); {mesh} has none")
            return make_term(verts, faces, self.dataset, uv=uv.to(self.device), texture=tex.to(self.device), **kw)
        from .metrics import load_ply_colors
        colors = load_ply_colors(str(mesh))
        if colors is None or colors.shape[0] != verts.shape[0]:
            raise ValueError(f"{fn}: pose_photo 'mesh' needs a .ply with red / green / blue vertex properties; {mesh} has none")
        return make_term(verts, faces, self.dataset, vertex_colors=colors.to(self.device), **kw)

    def refine_poses_silhouette(self, mesh=None, normalize=None, resolution=None, clean=None, extract=None, frames=None, save=True,
                                simplify=None, photo=None, corr=None, **overrides):
        """Every frame's pose refined against a mesh by silhouette matching (dynhor_amd/pose_sil.py) and written into Dataset.R /
        Dataset.T.  The mesh is chosen as visualize_mesh chooses it (_select_mesh; `mesh` and `normalize` left at None take the config's
        mesh_vis: block): the .ply / .obj file `mesh` (normalize "none" | "reference"), else the reconstruction extracted at
        `resolution` (default pose_sil.resolution, 128: a silhouette at pixel precision does not need the 512^3 mesh), cleaned when
        mesh_clean says so and simplified when `simplify` / mesh_simplify says so (a fine extraction reduced to a few thousand faces
        keeps the detail a coarse extraction rounds off; refine.json then carries `simplify`).  frames: None / "all", "worst:N" (the N lowest silhouette IoUs before the
        refinement) or stems "a,b,c": the frames that move; the others stay fixed.  overrides: any key of the config's pose_sil: block.
        Rank 0 writes poses/<iter:08d>/obj_infos/<stem>.npz (export_poses) and poses/<iter:08d>/refine.json (settings, per-frame IoU
        before / after, loss curve, mesh name), and logs pose_sil/* to <exp>/board.  With train.refine_poses on, the PoseRefiner is
        re-seeded from the new poses (its Adam state starts afresh) and, when save is on, checkpoints/ckpt_<iter>.pth is written again
        with it: load_checkpoint copies a checkpoint's PoseRefiner poses over Dataset.R / T, so that is what a later --is_continue run
        starts from.  Without train.refine_poses, point data_info.obj_infos at the written folder.  Returns the dict of refine.json
        plus dir (single process: run it on one rank).
        photo: None (the config's pose_photo.mode) | "none" | "views" | "mesh": add the photometric term of dynhor_amd/pose_photo.py
        (_photo_term says where the colours come from; the other keys of the pose_photo: block are its settings).  refine.json then
        carries `photo`, the loss_photo curve and the contributing pairs per refined frame (photo_pairs), and pose/loss_photo goes to
        the board.  With "none" everything is exactly what it is without the term.
        corr: None (the config's pose_corr.mode) | "none" | "dataset" | "match": add the correspondence term of dynhor_amd/pose_corr.py
        over the matches the dataset holds ("dataset": data_info.correspondence_infos, or an earlier match_frames of this process) or
        over matches made first by match_frames guided by the very mesh being fitted ("match"; they are not refreshed while the poses
        move).  The other keys of the pose_corr: block are its settings.  refine.json then carries `corr`, settings["corr"], the
        loss_corr curve, corr_resid_before / corr_resid_after and corr_worst, and pose/loss_corr goes to the board.  With "none"
        everything is exactly what it is without the term."""
        from .pose_corr import MODES as CORR_MODES
        from .pose_photo import MODES as PHOTO_MODES
        from .pose_sil import refine_poses
        if self.world > 1:
            raise ValueError("refine_poses_silhouette runs on one rank (the poses of all frames are optimised jointly)")
        fn = "refine_poses_silhouette"
        pc = merge("pose_sil", POSE_SIL_DEFAULTS, self.conf.get("pose_sil"), overrides, who=fn, check_overrides=True)

        def term(name, defaults, mode, known):                      # an optional term's block with its mode; both are checked
            c = merge(name, defaults, self.conf.get(name), {"mode": mode})
            unknown = sorted(set(c) - set(defaults))
            if unknown or c["mode"] not in known:
                raise ValueError(f"{fn}: {name} mode {c['mode']!r} (one of {known}), unknown setting(s) {unknown}; known: {sorted(defaults)}")
            return c

        pp = term("pose_photo", POSE_PHOTO_DEFAULTS, photo, PHOTO_MODES)
        cc = term("pose_corr", POSE_CORR_DEFAULTS, corr, CORR_MODES)
        pmode, kmode = pp["mode"], cc["mode"]
        verts, faces, name, cmode, smode = self._guide_mesh(fn, mesh, normalize, resolution, clean, extract, simplify)
        mesh_file = merge("mesh_vis", MESH_VIS_DEFAULTS, self.conf.get("mesh_vis"), {"mesh": mesh})["mesh"]     # None: the reconstruction
        corr_term = None
        if kmode != "none":
            from .pose_corr import make_term as make_corr_term
            if kmode == "match":
                self.match_frames(guide="mesh", mesh=mesh, normalize=normalize, resolution=resolution, clean=clean, extract=extract,
                                  simplify=simplify, save=save)
            if self.dataset.corr is None:
                raise ValueError("refine_poses_silhouette: pose_corr 'dataset' needs correspondences and the dataset holds none: point "
                                 "data_info.correspondence_infos at a folder of matches, run --mode match_frames first, or use "
                                 "--pose_corr match")
            corr_term = lambda active: make_corr_term(self.dataset, active=active, delta_px=float(cc["delta_px"]),
                                                      min_cos=float(cc["min_cos"]), min_conf=float(cc["min_conf"]),
                                                      frame_chunk=int(pc["frame_chunk"]))
        res = refine_poses(verts, faces, self.dataset, iters=pc["iters"], lr=pc["lr"], rot_lr_mult=pc["rot_lr_mult"],
                           sigma_px=pc["sigma_px"], sigma_end_px=pc["sigma_end_px"], cut=pc["cut"], edge_offset_px=pc["edge_offset_px"],
                           lw_sil=pc["lw_sil"], lw_smooth=pc["lw_smooth"], frame_chunk=pc["frame_chunk"], report_freq=pc["report_freq"],
                           frames=frames, lw_photo=float(pp["lw_photo"]), corr=corr_term, lw_corr=float(cc["lw_corr"]),
                           photo=None if pmode == "none" else self._photo_term(pmode, pp, verts, faces, mesh_file, cmode, smode))
        res.pop("R"); res.pop("T")
        res.update(iter=self.iter_step, mesh=name, clean=cmode, faces=int(faces.shape[0]))
        if pmode != "none":
            res.update(photo=pmode)
        if kmode != "none":
            res.update(corr=kmode)
        if smode != "none":
            res.update(simplify=smode)
        if self._reseed_pose_refiner() and save:
            # load_checkpoint copies the checkpoint's PoseRefiner poses over Dataset.R / T: without a checkpoint of the re-seeded
            # refiner a later --is_continue run would bring the old poses back
            res["checkpoint"] = self.save_checkpoint()
        if save:
            d = os.path.join(self.base_exp_dir, "poses", "{:0>8d}".format(self.iter_step))
            self.export_poses(os.path.join(d, "obj_infos"))
            self._write_json(d, "refine.json", res)
            res["dir"] = d
            self.last_pose_dir = d
            board = self._board_writer()
            for st in res["curve"]:
                for k in ("loss", "loss_sil", "loss_smooth", "iou_mean", "iou_min", "sigma"):
                    board.add_scalar("pose_sil/" + k, float(st[k]), int(st["iter"]))
                for k in st:                                        # the optional terms' losses, in the order they were added
                    if k.startswith("loss_") and k not in ("loss_sil", "loss_smooth"):
                        board.add_scalar("pose/" + k, float(st[k]), int(st["iter"]))
            for k in ("iou_mean_before", "iou_mean_after"):
                if res[k] is not None:
                    board.add_scalar("pose_sil/" + k, float(res[k]), self.iter_step)
            board.flush()
        return res

    def init_poses(self, mesh=None, normalize=None, save=True, **overrides):
        """Every frame's pose initialised from its mask and a template mesh alone (dynhor_amd/pose_init.py: a bank of random views,
        retrieval per frame, depth from the box, a short fit per candidate, one candidate per frame, the joint silhouette refinement)
        and written into Dataset.R / Dataset.T.  The template: the .ply / .obj file `mesh` with normalize "none" | "reference"; left at
        None it is the config's data_info.obj_path, normalised as the reference normalises its prior when data_info.normalize_mesh
        is true (ObjTracker/run.py:106-114).  overrides: any key of the config's pose_init: block; the final refinement takes the
        pose_sil: block.  Rank 0 writes poses/init/obj_infos/<stem>.npz (export_poses) and poses/init/init.json (per frame: view, rank,
        iou_bank, iou_fit, iou_final, angle_prev_deg; the settings) and logs init/* to <exp>/board.  With train.refine_poses on, the
        PoseRefiner is re-seeded from the new poses.  Returns the dict of init.json plus dir (single process: run it on one rank)."""
        from .pose_init import init_poses
        if self.world > 1:
            raise ValueError("init_poses runs on one rank (the final refinement optimises the poses of all frames jointly)")
        ic = merge("pose_init", POSE_INIT_DEFAULTS, self.conf.get("pose_init"), overrides, who="init_poses", check_overrides=True)
        pc = merge("pose_sil", POSE_SIL_DEFAULTS, self.conf.get("pose_sil"))
        verts, faces, mesh, normalize = self._template_mesh("init_poses", mesh, normalize)
        res = init_poses(verts, faces, self.dataset,
                         pose_sil={k: pc[k] for k in ("iters", "lr", "rot_lr_mult", "sigma_px", "sigma_end_px", "cut", "edge_offset_px",
                                                      "lw_sil", "lw_smooth", "frame_chunk", "report_freq")}, **ic)
        res.pop("R"); res.pop("T")
        res.update(iter=self.iter_step, mesh=str(mesh), normalize=normalize, faces=int(faces.shape[0]))
        self._reseed_pose_refiner()
        if save:
            d = os.path.join(self.base_exp_dir, "poses", "init")
            self.export_poses(os.path.join(d, "obj_infos"))
            self._write_json(d, "init.json", res)
            res["dir"] = d
            self.last_pose_dir = d
            board = self._board_writer()
            for k, fr in enumerate(res["frames"]):
                for key in ("iou_bank", "iou_fit", "iou_final", "angle_prev_deg"):
                    if fr[key] is not None:
                        board.add_scalar("init/" + key, float(fr[key]), k)
            for key in ("iou_fit_mean", "iou_final_mean"):
                if res[key] is not None:
                    board.add_scalar("init/" + key, float(res[key]), self.iter_step)
            board.flush()
        return res

    @torch.no_grad()
    def match_frames(self, guide=None, offsets=None, mesh=None, normalize=None, resolution=None, clean=None, extract=None, simplify=None,
                     save=True, warp=None, **overrides):
        """Dense correspondences between the frames by guided block matching (dynhor_amd/match.py), set on the dataset
        (Dataset.set_correspondences), so that a run in the same process can train on them (train.corr_weight).  guide: None (the
        config's match.guide) | "none" (the guess is the displacement of the object's box) | "mesh" (the guess comes from a mesh at the
        dataset's current poses, chosen as refine_poses_silhouette chooses it: _select_mesh with `mesh`, `normalize`, `resolution`
        (default pose_sil.resolution), `clean`, `extract`, `simplify`).  offsets: a list or "1,2,5"; warp: None (the config's
        match.warp) | "none" | "affine" (with the mesh guide: source patches sampled through the affine map of the face plane, for wide
        baselines); overrides: any key of the config's match: block.  Rank 0 writes <exp>/correspondences/correspondence_infos/<stem_i>_<stem_j>.npz
        (scene.write_correspondences_to_disk with the dataset's stems; point data_info.correspondence_infos at that folder) and
        <exp>/correspondences/match.json (settings, per pair queries / searched / kept and the count lost to each gate, mean s1, with a
        mesh the median distance of the kept matches from the guide, totals, seconds), and logs match/kept and match/kept_share to
        <exp>/board.  Returns the dict of match.json plus dir (single process: run it on one rank)."""
        from .match import match_frames
        from .scene import write_correspondences_to_disk
        if self.world > 1:
            raise ValueError("match_frames runs on one rank")
        mc = merge("match", MATCH_DEFAULTS, self.conf.get("match"), dict(overrides, guide=guide, offsets=offsets, warp=warp),
                   who="match_frames", check_overrides=True)
        verts = faces = name = None
        if (mc["guide"] or MATCH_DEFAULTS["guide"]) == "mesh":
            verts, faces, name, _, _ = self._guide_mesh("match_frames", mesh, normalize, resolution, clean, extract, simplify)
        matches, res = match_frames(self.dataset, verts, faces, **mc)
        res.update(iter=self.iter_step, mesh=name)
        self.dataset.set_correspondences(matches)
        if save and self.rank == 0:
            d = os.path.join(self.base_exp_dir, "correspondences")
            cdir = os.path.join(d, "correspondence_infos")
            if os.path.isdir(cdir):                        # a pair that kept nothing this time must not leave an older file behind
                for f in os.listdir(cdir):
                    if f.endswith(".npz"):
                        os.remove(os.path.join(cdir, f))
            write_correspondences_to_disk(matches, d, self.dataset.stems)
            self._write_json(d, "match.json", res)
            res["dir"] = d
            self.last_match_dir = d
            board = self._board_writer()
            board.add_scalar("match/kept", float(res["totals"]["kept"]), self.iter_step)
            board.add_scalar("match/kept_share", float(res["totals"]["kept_share"]), self.iter_step)
            board.flush()
        return res

    @torch.no_grad()
    def mvs_depth(self, mesh=None, normalize=None, resolution=None, clean=None, extract=None, simplify=None, frames=None, save=True,
                  **overrides):
        """Per-frame depth and normal maps and a fused point cloud from the frames' texture, by a plane sweep about a guide mesh at the
        dataset's current poses (dynhor_amd/mvs.py).  The guide is chosen as match_frames with guide "mesh" chooses it: _select_mesh
        with `mesh`, `normalize`, `resolution` (default pose_sil.resolution), `clean`, `extract`, `simplify` -- the reconstruction, the
        template, the hull or a scan.  frames: None (all) or a list of frame indices; overrides: any key of the config's optional mvs:
        block (mvs.DEFAULTS: first settings, not tuned); an unknown key raises.  Rank 0 writes under <exp>/mvs/<iter:08d>/:
        depth/<stem>.npy (camera z, f32, inf where not kept: render_views' _depth.npy convention), monocular_normal/<stem>.png (the
        loader's encoding round((n 0.5 + 0.5) 255) in the camera frame, 128 where there is no normal), cloud.ply (points, normals,
        colours; thinned to one point per mvs.voxel cell when the override `voxel` is given) and mvs.json (settings, per frame the pixels
        swept, the count lost to each gate, the kept share, the mean c_best, the median and 95th percentile of |z - z_guide|; totals,
        seconds per phase, the five frames with the lowest kept share), and logs mvs/kept_share and mvs/guide_dev_median to
        <exp>/board.  Pointing data_info's monocular_normal/ at that folder is the user's step.  Returns the dict of mvs.json plus dir
        (single process: run it on one rank)."""
        from . import mvs
        if self.world > 1:
            raise ValueError("mvs_depth runs on one rank")
        # voxel is this mode's own key of the block (mvs.fuse takes it, mvs.depth_maps does not)
        mc = merge("mvs", dict(MVS_DEFAULTS, voxel=None), self.conf.get("mvs"), overrides, who="mvs_depth", check_block=True,
                   check_overrides=True)
        voxel = mc.pop("voxel")
        mvs.check_settings(mc)
        verts, faces, name, _, _ = self._guide_mesh("mvs_depth", mesh, normalize, resolution, clean, extract, simplify)
        ds = self.dataset
        out = mvs.depth_maps(ds, verts, faces, frames=frames, **mc)
        res = out["stats"]
        res.update(iter=self.iter_step, mesh=name, voxel=voxel)
        if save and self.rank == 0:
            import time
            from PIL import Image
            t0 = time.time()
            d = os.path.join(self.base_exp_dir, "mvs", f"{self.iter_step:08d}")
            os.makedirs(os.path.join(d, "depth"), exist_ok=True)
            os.makedirs(os.path.join(d, "monocular_normal"), exist_ok=True)
            stems = ds.stems if ds.stems is not None else ["%04d" % f for f in range(ds.n_images)]
            todo = [r["frame"] for r in res["per_frame"]]
            for f in todo:
                z = torch.where(out["kept"][f], out["depth"][f], torch.full_like(out["depth"][f], float("inf")))
                np.save(os.path.join(d, "depth", stems[f] + ".npy"), z.cpu().numpy())
                enc = mvs.encode_normals(out["normal"][f], out["normal_ok"][f])
                Image.fromarray(enc.cpu().numpy()).save(os.path.join(d, "monocular_normal", stems[f] + ".png"))
            pts, nrm, col, _ = mvs.fuse(out["depth"], out["kept"], out["normal"], out["normal_ok"], ds.rgb, ds.R, ds.T, ds.K, voxel)
            mvs.write_cloud_ply(os.path.join(d, "cloud.ply"), pts, nrm, col)
            res["cloud_points"] = int(pts.shape[0])
            res["seconds"]["write"] = time.time() - t0
            self._write_json(d, "mvs.json", res)
            res["dir"] = d
            self.last_mvs_dir = d
            board = self._board_writer()
            board.add_scalar("mvs/kept_share", float(res["totals"]["kept_share"]), self.iter_step)
            if res["totals"]["guide_dev_median"] is not None:
                board.add_scalar("mvs/guide_dev_median", float(res["totals"]["guide_dev_median"]), self.iter_step)
            board.flush()
        return res

    def _sdf_init_conf(self, **overrides):
        """The YAML's optional sdf_init: block over SDF_INIT_DEFAULTS, then the overrides that are not None; an unknown key raises."""
        from .sdf_init import check_settings
        c = merge("sdf_init", SDF_INIT_DEFAULTS, self.conf.get("sdf_init"), overrides, who="init_sdf", check_block=True, check_overrides=True)
        check_settings(c)
        return c

    def init_sdf(self, mesh=None, normalize=None, save=True, simplify_mode=None, **overrides):
        """The SDF network warm-started from a template mesh (dynhor_amd/sdf_init.py: an Adam fit of the network of either family to
        the template's signed distance, dynhor_amd/mesh_sdf.py), before any training: it runs only at iteration 0.  The template is
        chosen exactly as init_poses chooses it: the .ply / .obj file `mesh` with normalize "none" | "reference"; left at None it is
        the config's data_info.obj_path, normalised as the reference normalises its prior when data_info.normalize_mesh is true -- the
        canonical frame the poses of init_poses refer to.  simplify_mode: a mesh_simplify mode for the template (None: the config's
        mesh_simplify.mode; the cost of the fit is points x faces per iteration).  overrides: any key of the config's sdf_init:
        block.  The colour network and the variance are left bit for bit as they were, and the optimiser moments are reset, so the
        training that follows (--mode train --is_continue) starts its own Adam.  Rank 0 writes checkpoints/ckpt_000000.pth,
        sdf_init/init.json (template, faces, settings, loss curve, held-out error before and after, seconds) and
        sdf_init/<template>_fit.ply (the fitted network's zero level set at `resolution`), and logs sdf_init/* to <exp>/board.
        Returns the dict of init.json plus dir and checkpoint.  The template is a category-level prior: training moves away from
        it."""
        from .sdf_init import fit_sdf_to_mesh
        if self.world > 1:
            raise ValueError("init_sdf runs on one rank (the fit is a single-process loop; start training on several afterwards)")
        sc = self._sdf_init_conf(**overrides)
        if self.iter_step != 0:
            raise ValueError(f"init_sdf: this run has already trained to iteration {self.iter_step}; the warm start replaces the "
                             "network's initialisation and runs only at iteration 0 (use a fresh exp_name)")
        verts, faces, mesh, normalize = self._template_mesh("init_sdf", mesh, normalize)
        faces_in = int(faces.shape[0])
        self.last_simplify_stats = None
        if self._simplify_conf(simplify_mode)["mode"] != "none":
            verts, faces = self._simplify_mesh(verts, faces, simplify_mode)
        st = self.store
        st.exp_avg.zero_(); st.exp_avg_sq.zero_(); st.step_count = 0
        board = self._board_writer() if save else None
        res = fit_sdf_to_mesh(self.renderer, verts, faces,
                              report=(lambda it, loss: board.add_scalar("sdf_init/loss", loss, it)) if board is not None else None, **sc)
        # fresh optimiser moments: the checkpoint, and a training that goes on in this process, start their own Adam
        st.exp_avg.zero_(); st.exp_avg_sq.zero_(); st.step_count = 0
        res.update(iter=self.iter_step, mesh=str(mesh), normalize=normalize, faces_in=faces_in,
                   simplify=self._simplify_conf(simplify_mode)["mode"], family=self.conf["model"]["family"])
        if save:
            from .mesh import write_ply
            d = os.path.join(self.base_exp_dir, "sdf_init")
            os.makedirs(d, exist_ok=True)
            fv, ff = self.renderer.extract_geometry(self.dataset.object_bbox_min, self.dataset.object_bbox_max,
                                                    resolution=int(sc["resolution"]), threshold=0.0)
            stem = os.path.splitext(os.path.basename(str(mesh)))[0]
            res["fit_mesh"] = os.path.join(d, stem + "_fit.ply")
            res["fit_mesh_faces"] = int(ff.shape[0])
            write_ply(res["fit_mesh"], fv, ff)
            res["checkpoint"] = self.save_checkpoint()
            self._write_json(d, "init.json", res)
            res["dir"] = d
            for k in ("heldout_before", "heldout_after", "seconds"):
                board.add_scalar("sdf_init/" + k, float(res[k]), self.iter_step)
            board.flush()
        return res

    def _visual_hull_conf(self, **overrides):
        """The YAML's optional visual_hull: block over VISUAL_HULL_DEFAULTS, then the overrides that are not None; an unknown or bad
        key raises."""
        from .visual_hull import hull_settings
        return hull_settings(self.conf.get("visual_hull"), **overrides)

    @torch.no_grad()
    def visual_hull(self, save=True, simplify=None, **overrides):
        """The visual hull of the object masks at the dataset's current poses (dynhor_amd/visual_hull.py): a mesh of the object's own
        shape, up to its concavities, from the label maps and the poses alone -- no checkpoint, no template.  It uses every frame:
        train.holdout does not apply (the hull is geometry from masks, not a rendering that is scored).  overrides: any key of the
        config's visual_hull: block; simplify: a mesh_simplify mode (None: the config's mesh_simplify.mode).  Rank 0 writes
        <exp>/hull/hull.ply, with simplification also hull_simple.ply, and hull.json (settings, stats -- grid, cell, volume,
        radius_max, touches_bound, sole_carved: per frame the cells that frame alone carves, the frames to distrust first --,
        silhouette: mesh_vis.silhouette_summary of the hull drawn over the frames, seconds per phase), and logs hull/iou_mean,
        hull/volume and hull/sole_carved_max to <exp>/board.  Returns the dict of hull.json plus dir (single process: run it on one
        rank)."""
        import time
        from .mesh_vis import overlay_frames, silhouette_summary
        from .visual_hull import visual_hull
        if self.world > 1:
            raise ValueError("visual_hull runs on one rank")
        hc = self._visual_hull_conf(**overrides)
        seconds = {}
        verts, faces, stats = visual_hull(self.dataset, timer=seconds, **hc)
        smode = self._simplify_conf(simplify)["mode"]
        sv = sf = None
        self.last_simplify_stats = None
        if smode != "none":
            t0 = time.perf_counter()
            sv, sf = self._simplify_mesh(verts, faces, simplify)
            torch.cuda.synchronize(self.device)
            seconds["simplify"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        names = schedules.frame_names(self.dataset.n_images, self.dataset.stems)
        sil = silhouette_summary(overlay_frames(verts, faces, self.dataset, frame_chunk=hc["frame_chunk"]).cpu(), names)
        seconds["silhouette"] = time.perf_counter() - t0
        res = {"iter": self.iter_step, "settings": hc, "stats": stats, "silhouette": sil, "seconds": seconds, "simplify": smode,
               "simplify_stats": self.last_simplify_stats}
        self.last_hull = (verts, faces)
        if save and self.rank == 0:
            from .mesh import write_ply
            d = os.path.join(self.base_exp_dir, "hull")
            os.makedirs(d, exist_ok=True)
            res["mesh"] = os.path.join(d, "hull.ply")
            write_ply(res["mesh"], verts, faces)
            if sv is not None:
                res["mesh_simple"] = os.path.join(d, "hull_simple.ply")
                write_ply(res["mesh_simple"], sv, sf)
            self._write_json(d, "hull.json", res)
            res["dir"] = d
            board = self._board_writer()
            if sil["iou_mean"] is not None:
                board.add_scalar("hull/iou_mean", float(sil["iou_mean"]), self.iter_step)
            board.add_scalar("hull/volume", float(stats["volume"]), self.iter_step)
            board.add_scalar("hull/sole_carved_max", float(stats["sole_carved"]["share_max"]), self.iter_step)
            board.flush()
        return res

    @torch.no_grad()
    def fuse_depth(self, mvs_dir=None, save=True, **overrides):
        """The depth maps of mvs_depth fused into a mesh (dynhor_amd/depth_fuse.py): a truncated signed distance field on the visual
        hull's grid with the hull as a weak prior, at the dataset's current poses -- no checkpoint, no template.  mvs_dir: the folder
        mvs_depth wrote (None: the one this runner wrote last, else the newest <exp>/mvs/*/; none: an error that names --mode
        mvs_depth).  It reads depth/<stem>.npy (inf: no depth; a frame without a file contributes nothing; a map of another shape than
        the frames' raises), monocular_normal/<stem>.png (128 in all three channels: no normal) and settings.step_px of mvs.json.  It
        uses the frames that have depth files: train.holdout does not apply (as for the hull).  overrides: any key of the config's
        optional depth_fuse: block (depth_fuse.DEPTH_FUSE_DEFAULTS: first settings, not tuned); the hull pass takes the config's
        visual_hull: block.  Rank 0 writes <exp>/fuse/<iter:08d>/fused.ply and fuse.json (settings, stats, mvs_dir, step_px, silhouette:
        mesh_vis.silhouette_summary of the mesh drawn over the frames, residual_median per frame and residual_worst: the frames that
        disagree most with the fusion of all, seconds per phase) and logs fuse/volume, fuse/carved_cells and fuse/residual_median to
        <exp>/board.  Returns the dict of fuse.json plus dir (single process: run it on one rank)."""
        import time
        from . import depth_fuse
        from .mesh_vis import overlay_frames, silhouette_summary
        if self.world > 1:
            raise ValueError("fuse_depth runs on one rank")
        fz = depth_fuse.fuse_settings(self.conf.get("depth_fuse"), **overrides)
        hc = self._visual_hull_conf()
        if mvs_dir is None:
            mvs_dir = self.last_mvs_dir
        if mvs_dir is None:
            mvs_dir = _newest_mvs_dir(self.base_exp_dir, "fuse_depth")
        if not os.path.isdir(os.path.join(str(mvs_dir), "depth")):
            raise ValueError(f"fuse_depth: {mvs_dir} holds no depth/ folder: run --mode mvs_depth first, or give its folder as --mvs_dir")
        mvs_dir = str(mvs_dir)
        ds = self.dataset
        seconds = {}
        t0 = time.perf_counter()
        names = schedules.frame_names(ds.n_images, ds.stems)
        stems = ds.stems if ds.stems is not None else ["%04d" % f for f in range(ds.n_images)]
        step_px = 1
        if os.path.exists(os.path.join(mvs_dir, "mvs.json")):
            with open(os.path.join(mvs_dir, "mvs.json")) as f:
                step_px = int((json.load(f).get("settings") or {}).get("step_px", 1))
        depth, normal, present = depth_fuse.read_maps(mvs_dir, stems, ds.H, ds.W)
        if not any(present):
            raise ValueError(f"fuse_depth: {mvs_dir}/depth holds no map of this sequence's frames: run --mode mvs_depth first")
        depth = depth.to(self.device)
        weight = depth_fuse.map_weights(depth, normal.to(self.device), ds.Kinv, fz["weight"], fz["floor_weight"])
        del normal
        seconds["read"] = time.perf_counter() - t0
        kept = {}
        verts, faces, stats = depth_fuse.fused_mesh(ds, depth, weight, step_px=step_px, hull=hc, timer=seconds, keep=kept, **fz)
        t0 = time.perf_counter()
        d_s, w_s, K_s = depth_fuse._step_maps(depth, weight, ds.K, step_px)
        rs = depth_fuse.frame_residuals(kept["field"], kept["lo"], kept["hi"], kept["trunc"], d_s, w_s, ds.R, ds.T, K_s, names)
        torch.cuda.synchronize(self.device)
        seconds["residuals"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        sil = silhouette_summary(overlay_frames(verts, faces, ds, frame_chunk=fz["frame_chunk"]).cpu(), names)
        seconds["silhouette"] = time.perf_counter() - t0
        have = [m for m in rs["median"] if m is not None]
        res = {"iter": self.iter_step, "settings": fz, "hull_settings": hc, "stats": stats, "mvs_dir": mvs_dir, "step_px": step_px,
               "frames_with_depth": int(sum(present)), "silhouette": sil, "residual_median": rs["median"], "residual_count": rs["count"],
               "residual_worst": rs["worst"], "residual_median_all": float(np.median(have)) if have else None, "seconds": seconds}
        if save and self.rank == 0:
            from .mesh import write_ply
            d = os.path.join(self.base_exp_dir, "fuse", f"{self.iter_step:08d}")
            os.makedirs(d, exist_ok=True)
            res["mesh"] = os.path.join(d, "fused.ply")
            write_ply(res["mesh"], verts, faces)
            self._write_json(d, "fuse.json", res)
            res["dir"] = d
            self.last_fuse_dir = d
            board = self._board_writer()
            board.add_scalar("fuse/volume", float(stats["volume"]), self.iter_step)
            board.add_scalar("fuse/carved_cells", float(stats["carved_cells"]), self.iter_step)
            if res["residual_median_all"] is not None:
                board.add_scalar("fuse/residual_median", float(res["residual_median_all"]), self.iter_step)
            board.flush()
        return res

    def _scene_gt_mesh(self, resolution, chunk=1 << 22, mode="dense"):
        """Zero level set of the synthetic scene's analytic SDF (scene.scene_sdf) by mesh.marching_cubes over [-0.55, 0.55]^3
        (the object lies inside the radius-0.5 ball), the SDF evaluated on the device in chunks.  mode "sparse": by
        mesh_extract.sparse_marching_cubes at lipschitz 1 (a distance field's exact constant), block 8.  Cached per resolution and mode."""
        from .mesh import marching_cubes
        from .scene import scene_sdf
        cache = self.__dict__.setdefault("_gt_meshes", {})
        if mode == "sparse":
            if (resolution, mode) not in cache:
                from .mesh_extract import sparse_marching_cubes
                cache[(resolution, mode)] = sparse_marching_cubes(lambda p: -scene_sdf(p), int(resolution), [-0.55] * 3, [0.55] * 3,
                                                                  lipschitz=1.0, device=self.device)[:2]
            return cache[(resolution, mode)]
        if resolution not in cache:
            N = int(resolution)
            ax = torch.linspace(-0.55, 0.55, N, device=self.device)
            u = torch.empty(N * N * N, device=self.device)
            for s in range(0, N * N * N, chunk):
                i = torch.arange(s, min(s + chunk, N * N * N), device=self.device)
                p = torch.stack([ax[i // (N * N)], ax[(i // N) % N], ax[i % N]], dim=-1)
                u[s:s + i.shape[0]] = -scene_sdf(p)
            cache[resolution] = marching_cubes(u.view(N, N, N), 0.0, [-0.55] * 3, [0.55] * 3)
        return cache[resolution]


def _to_cpu(d):
    return {k: (_to_cpu(v) if isinstance(v, dict) else (v.detach().cpu() if torch.is_tensor(v) else v)) for k, v in d.items()}
