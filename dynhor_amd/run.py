"""CLI in the reference's style (ObjTracker/run.py:90-95): python -m dynhor_amd.run --config_path X.yaml [--mode train].

    python -m dynhor_amd.run --config_path configs/synthetic.yaml                 # one GPU
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --gpus 8        # frames shard 8-way data-parallel (RCCL)
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode evaluate_mesh --is_continue   # Chamfer / F-score, one JSON line
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode evaluate_mesh --is_continue --mesh_clean mask+largest
    python -m dynhor_amd.run --config_path X.yaml --mode evaluate_mesh --is_continue --gt_mesh scan.ply --gt_align similarity --gt_align_init global
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode validate_mesh --is_continue --mesh_color views+network
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode validate_mesh --is_continue --mesh_extract sparse --mesh_resolution 1024
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode validate_mesh --is_continue --mesh_resolution 512 --mesh_simplify faces:12000
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode validate_mesh --is_continue --mesh_resolution 512 --mesh_simplify faces:5000 --mesh_texture views
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode visualize_mesh --is_continue --turntable 36   # overlays, IoU
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode refine_poses --is_continue --pose_frames worst:5   # silhouette fit
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode refine_poses --is_continue --pose_photo views   # plus a colour term
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode refine_poses --is_continue --pose_corr match    # plus dense matches
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode export_poses --is_continue    # obj_infos/<stem>.npz of the poses
    python -m dynhor_amd.run --config_path X.yaml --mode init_poses --vis_mesh template.obj --vis_normalize reference   # poses from masks
    python -m dynhor_amd.run --config_path X.yaml --mode init_sdf --vis_mesh template.obj --vis_normalize reference     # SDF warm start
    python -m dynhor_amd.run --config_path X.yaml --mode init_sdf --mesh_simplify faces:5000   # template: data_info.obj_path, simplified
    python -m dynhor_amd.run --config_path X.yaml --mode visual_hull   # <exp>/hull/hull.ply from masks and poses alone; no template
    python -m dynhor_amd.run --config_path X.yaml --mode visual_hull --hull_resolution 256 --hull_votes 2   # simplified too when the config's mesh_simplify.mode says so
    python -m dynhor_amd.run --config_path X.yaml --mode refine_poses --vis_mesh exps/<seq>/<exp>/hull/hull.ply   # poses fitted to the hull
    python -m dynhor_amd.run --config_path X.yaml --mode match_frames --match_offsets 1,2,5   # correspondence_infos from the frames
    python -m dynhor_amd.run --config_path X.yaml --mode match_frames --is_continue --match_guide mesh   # guided by the reconstruction
    python -m dynhor_amd.run --config_path X.yaml --mode mvs_depth --vis_mesh hull.ply   # depth and normal maps by plane-sweep stereo
    python -m dynhor_amd.run --config_path X.yaml --mode fuse_depth   # <exp>/fuse/<iter>/fused.ply: the newest mvs_depth maps fused on the hull's grid
    python -m dynhor_amd.run --config_path X.yaml --mode fuse_depth --mvs_dir exps/<seq>/<exp>/mvs/00000000 --fuse_resolution 256 --fuse_trunc_cells 3
    python -m dynhor_amd.run --config_path X.yaml --mode mvs_depth --vis_mesh exps/<seq>/<exp>/fuse/00000000/fused.ply   # the fused mesh as the next guide
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode render_views --is_continue   # every frame sphere-traced: png, normal, depth, PSNR, IoU
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode render_views --is_continue --views orbit:36 --view_level 2
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode evaluate_views --is_continue   # masked SSIM, PSNR, L1 of the held-out frames
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode evaluate_views --is_continue --eval_frames all --eval_maps
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode interpolate_0_38 --is_continue   # upstream's video: volume rendering, level 2
    python -m dynhor_amd.run --config_path configs/synthetic.yaml --mode interpolate_0_38 --is_continue --view_method surface

With --gpus N > 1 this process starts N ranks (one per GPU) through dynhor_amd.launch before it touches the GPU and exits
with their code; under an external `torch.distributed.run` (WORLD_SIZE set) it is one of the ranks.
"""
import argparse
import os
import sys


MODES = ("train", "validate_image", "validate_mesh", "evaluate_mesh", "visualize_mesh", "refine_poses", "export_poses", "init_poses",
         "init_sdf", "render_views", "match_frames", "evaluate_views", "visual_hull", "mvs_depth", "fuse_depth")


def mode_arg(value: str) -> str:
    """--mode: one of MODES, or upstream's interpolate_<i>_<j> (two frame indices)."""
    import re
    if value in MODES or re.fullmatch(r"interpolate_\d+_\d+", value):
        return value
    raise argparse.ArgumentTypeError(f"invalid choice: {value!r} (choose from {', '.join(MODES)}, interpolate_<i>_<j>)")


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config_path", type=str, required=True)
    ap.add_argument("--mode", type=mode_arg, default="train", metavar="{" + ",".join(MODES) + ",interpolate_<i>_<j>}")
    ap.add_argument("--is_continue", action="store_true")
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--gpus", type=int, default=1, help="data-parallel ranks on this node (one process per GPU)")
    ap.add_argument("--backend", type=str, default="nccl", help="torch.distributed backend (nccl == RCCL; gloo for tests)")
    ap.add_argument("--share-gpu", action="store_true", help="TEST ONLY: every rank uses cuda:0 (with --backend gloo)")
    ap.add_argument("--exp_root", type=str, default="exps")
    # evaluate_mesh only (defaults: the config's eval: block, else the analytic scene of a synthetic sequence, resolution 512)
    ap.add_argument("--gt_mesh", type=str, default=None, help="evaluate_mesh: ground-truth mesh (.obj / .ply)")
    ap.add_argument("--gt_normalize", type=str, default=None, choices=["none", "reference"],
                    help="evaluate_mesh: 'reference' = bring the ground truth into the canonical frame (mean 0, max vertex norm 0.5)")
    ap.add_argument("--gt_align", type=str, default=None, choices=["none", "rigid", "similarity"],
                    help="evaluate_mesh: register the ground truth (after --gt_normalize) to the reconstruction by trimmed ICP before "
                         "scoring it; also writes meshes/<iter>_gt_aligned.ply (default: the config's eval.gt_align, else none)")
    ap.add_argument("--gt_align_init", type=str, default=None, choices=["identity", "global"],
                    help="evaluate_mesh: start the registration where --gt_normalize leaves the ground truth, or search the rotations "
                         "(default: the config's eval.gt_align_init, else identity)")
    ap.add_argument("--mesh_resolution", type=int, default=None,
                    help="validate_mesh / evaluate_mesh / visualize_mesh: marching-cubes grid of the reconstruction (validate_mesh: 64 "
                         "when unset)")
    ap.add_argument("--mesh_extract", type=str, default=None, choices=["dense", "sparse"],
                    help="validate_mesh / evaluate_mesh / visualize_mesh: query the whole grid, or only the blocks near the surface "
                         "(the same mesh; default: the config's mesh_extract.mode, else dense)")
    ap.add_argument("--mesh_clean", type=str, default=None, choices=["none", "mask", "largest", "mask+largest"],
                    help="validate_mesh / evaluate_mesh / visualize_mesh: clean the mesh (default: the config's mesh_clean.mode, "
                         "else none)")
    ap.add_argument("--mesh_color", type=str, default=None, choices=["none", "views", "network", "views+network"],
                    help="validate_mesh: colour the mesh and also write <iter>_color.ply; visualize_mesh: shade with the vertex colours "
                         "(default: the config's mesh_color.mode, else none)")
    ap.add_argument("--mesh_simplify", type=str, default=None,
                    help="validate_mesh / evaluate_mesh / visualize_mesh / refine_poses / init_sdf: none | cells:N | faces:T -- simplify "
                         "the (cleaned) mesh, or init_sdf's template, by quadric vertex clustering on N cells along its longest axis, or to at most T faces; "
                         "validate_mesh also writes <iter>_simple.ply (default: the config's mesh_simplify.mode, else none)")
    ap.add_argument("--mesh_texture", type=str, default=None, choices=["none", "views", "views+network"],
                    help="validate_mesh: bake a texture atlas for the (cleaned, simplified) mesh from the frames and also write "
                         "<iter>_textured.obj, .obj.mtl, _texture_kd.png and <iter>_texture.json (default: the config's "
                         "mesh_texture.mode, else none)")
    ap.add_argument("--texture_size", type=int, default=None,
                    help="validate_mesh: texels per side of the atlas; two faces share a square cell of at least 8 texels, so size S "
                         "holds 2 (S // 8)^2 faces (default: the config's mesh_texture.size, else 1024)")
    # visualize_mesh only (defaults: the config's mesh_vis: block, else the reconstruction at --mesh_resolution, no turntable)
    ap.add_argument("--vis_mesh", type=str, default=None,
                    help="visualize_mesh: draw this mesh (.ply / .obj; an .obj with a texture is drawn with it) instead of the "
                         "reconstruction; refine_poses: fit the poses to it; match_frames --match_guide mesh: the guide; init_poses / init_sdf: "
                         "the template (default: the config's "
                         "data_info.obj_path with normalize_mesh)")
    ap.add_argument("--vis_normalize", type=str, default=None, choices=["none", "reference"],
                    help="visualize_mesh: 'reference' = bring --vis_mesh into the canonical frame (mean 0, max vertex norm 0.5)")
    ap.add_argument("--turntable", type=int, default=None, help="visualize_mesh: frames of render_res/<iter>/turntable.gif (0: none)")
    # refine_poses only (defaults: the config's pose_sil: block; the mesh is chosen by --vis_mesh / --vis_normalize / --mesh_resolution)
    ap.add_argument("--pose_frames", type=str, default=None,
                    help="refine_poses: the frames that move: all (default), worst:N (the N lowest silhouette IoUs) or stems a,b,c")
    ap.add_argument("--pose_photo", type=str, default=None, choices=["none", "views", "mesh"],
                    help="refine_poses: add a photometric term next to the silhouette: 'views' colours the mesh being fitted from the "
                         "frames at the current poses, 'mesh' takes the vertex colours (.ply) or the texture (.obj) of --vis_mesh "
                         "(default: the config's pose_photo.mode, else none)")
    ap.add_argument("--pose_corr", type=str, default=None, choices=["none", "dataset", "match"],
                    help="refine_poses: add a correspondence term next to the silhouette: 'dataset' uses the matches the dataset holds "
                         "(data_info.correspondence_infos), 'match' first runs match_frames guided by the mesh being fitted "
                         "(default: the config's pose_corr.mode, else none)")
    ap.add_argument("--pose_dir", type=str, default=None, help="export_poses: write the .npz files here (default <exp>/poses/<iter>/obj_infos)")
    # render_views / interpolate_<i>_<j> (defaults: the config's surface_render: block)
    ap.add_argument("--views", type=str, default="frames", help="render_views: frames | interpolate:i:j:n | orbit:n")
    ap.add_argument("--view_level", type=int, default=None, help="render_views: pixel stride of the pictures")
    ap.add_argument("--view_method", type=str, default=None, choices=["surface", "volume"],
                    help="render_views: sphere-trace the SDF (colour, depth and normal maps) or volume-render (interpolate_<i>_<j>: "
                         "volume unless given)")
    ap.add_argument("--view_background", type=str, default=None, choices=["white", "black", "frame"])
    # evaluate_views only (defaults: the config's image_eval: block; the pictures are drawn as --view_level / --view_method /
    # --view_background and the surface_render: block say)
    ap.add_argument("--eval_frames", type=str, default=None,
                    help="evaluate_views: the frames that are scored: auto (the frames of train.holdout if there are any, else all), "
                         "all, train, holdout, every:K[:offset] or stems a,b,c (default: the config's image_eval.frames, else auto)")
    ap.add_argument("--eval_maps", action="store_true", default=None,
                    help="evaluate_views: also write <name>_ssim.png, the per-pixel SSIM in grey (black: not counted)")
    # match_frames only (defaults: the config's match: block; with --match_guide mesh the mesh is chosen by --vis_mesh / --vis_normalize /
    # --mesh_resolution as for refine_poses, cleaned, extracted and simplified as the config's mesh_* blocks say)
    ap.add_argument("--match_guide", type=str, default=None, choices=["none", "mesh"],
                    help="match_frames: where a query's guess comes from: 'none' = the displacement of the object's box between the two "
                         "frames, 'mesh' = the mesh at the current poses (default: the config's match.guide, else none)")
    ap.add_argument("--match_offsets", type=str, default=None,
                    help="match_frames: frame i is matched to i + every offset of this comma-separated list (default: the config's "
                         "match.offsets, else 1,2,5)")
    ap.add_argument("--match_warp", type=str, default=None, choices=["none", "affine"],
                    help="match_frames: 'affine' = with --match_guide mesh, sample every source patch through the affine map that the "
                         "plane of the mesh face seen there induces between the two frames (wide baselines, in-plane rotation); 'none' = "
                         "patches as they lie in the image (default: the config's match.warp, else none)")
    # visual_hull only (defaults: the config's visual_hull: block; with the config's mesh_simplify.mode it also writes hull_simple.ply)
    ap.add_argument("--hull_resolution", type=int, default=None,
                    help="visual_hull: grid points per axis of the fine grid, at most 512 (default: the config's visual_hull.resolution, "
                         "else 128)")
    ap.add_argument("--hull_votes", type=int, default=None,
                    help="visual_hull: a point is outside the hull when this many frames say so; K > 1 tolerates K - 1 frames with a "
                         "wrong pose or mask (default: the config's visual_hull.min_carve_votes, else 1)")
    # mvs_depth only (defaults: the config's optional mvs: block, else mvs.DEFAULTS -- first settings, not tuned; the guide mesh is chosen
    # by --vis_mesh / --vis_normalize / --mesh_resolution as for match_frames --match_guide mesh, cleaned, extracted and simplified as
    # the config's mesh_* blocks say)
    ap.add_argument("--mvs_offsets", type=str, default=None,
                    help="mvs_depth: the neighbours of frame i are i - o and i + o for every offset o of this comma-separated list, at "
                         "most four (default: the config's mvs.offsets, else 1,2)")
    ap.add_argument("--mvs_range", type=float, default=None,
                    help="mvs_depth: the sweep covers this many object units either side of the guide mesh (default: the config's "
                         "mvs.range, else 0.04)")
    ap.add_argument("--mvs_step_px", type=int, default=None,
                    help="mvs_depth: sweep the pixels of a grid of this step (default: the config's mvs.step_px, else 1)")
    # fuse_depth only (defaults: the config's optional depth_fuse: block, else depth_fuse.DEPTH_FUSE_DEFAULTS -- first settings, not tuned;
    # the hull pass takes the config's visual_hull: block)
    ap.add_argument("--mvs_dir", type=str, default=None,
                    help="fuse_depth: the folder mvs_depth wrote (default: the newest <exp>/mvs/*/)")
    ap.add_argument("--fuse_resolution", type=int, default=None,
                    help="fuse_depth: grid points per axis, at most 512 (default: the config's depth_fuse.resolution, else 128)")
    ap.add_argument("--fuse_trunc_cells", type=float, default=None,
                    help="fuse_depth: the truncation distance in cells of the grid (default: the config's depth_fuse.trunc_cells, else 4)")
    ap.add_argument("--prior_dir", type=str, default=None,
                    help="train: a folder in mvs_depth's layout; sets data_info.depth to its depth/ and data_info.monocular_normal to its "
                         "monocular_normal/ (auto: the newest <exp>/mvs/*/).  The terms themselves are train.depth_weight and "
                         "train.normal_weight with train.normal_skip_missing")
    return ap


def main():
    args = build_parser().parse_args()

    from . import launch
    if args.gpus > 1 and not launch.launched_by_torchrun():
        sys.exit(launch.spawn_ranks("dynhor_amd.run", sys.argv[1:], args.gpus, module=True))

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print(f"dynhor_amd.run: --gpus {args.gpus} but the launcher set WORLD_SIZE={world}", file=sys.stderr, flush=True)
        sys.exit(2)
    local_rank = 0 if args.share_gpu else int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local_rank)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
        else:
            dist.init_process_group(args.backend)

    from .runner import Runner
    runner = Runner(conf_path=args.config_path, mode=args.mode, is_continue=args.is_continue,
                    device=f"cuda:{local_rank}", exp_root=args.exp_root, prior_dir=args.prior_dir)
    if args.mode == "train":
        runner.train(args.iters)
        if runner.rank == 0:
            print(f"trained to iteration {runner.iter_step} on {world} rank(s)", flush=True)
    elif args.mode == "validate_image":
        print("psnr", runner.validate_image())
    elif args.mode == "evaluate_mesh":
        res = runner.evaluate_mesh(gt_mesh=args.gt_mesh, gt_normalize=args.gt_normalize, resolution=args.mesh_resolution,
                                   clean=args.mesh_clean, extract=args.mesh_extract, gt_align=args.gt_align,
                                   gt_align_init=args.gt_align_init, simplify=args.mesh_simplify)
        if runner.rank == 0:
            import json
            print(json.dumps(res), flush=True)
    elif args.mode == "visualize_mesh":
        res = runner.visualize_mesh(mesh=args.vis_mesh, normalize=args.vis_normalize, resolution=args.mesh_resolution,
                                    clean=args.mesh_clean, color=args.mesh_color, turntable=args.turntable,
                                    extract=args.mesh_extract, simplify=args.mesh_simplify)
        if runner.rank == 0:
            import json
            res = {k: v for k, v in res.items() if k != "frames"}
            res["dir"] = runner.last_vis_dir
            print(json.dumps(res), flush=True)
    elif args.mode == "refine_poses":
        res = runner.refine_poses_silhouette(mesh=args.vis_mesh, normalize=args.vis_normalize, resolution=args.mesh_resolution,
                                             clean=args.mesh_clean, extract=args.mesh_extract, frames=args.pose_frames,
                                             simplify=args.mesh_simplify, photo=args.pose_photo, corr=args.pose_corr)
        runner.close()
        if runner.rank == 0:
            import json
            print(json.dumps({k: v for k, v in res.items() if k not in ("stems", "curve")}), flush=True)
    elif args.mode == "init_poses":
        res = runner.init_poses(mesh=args.vis_mesh, normalize=args.vis_normalize)
        runner.close()
        if runner.rank == 0:
            import json
            print(json.dumps({k: v for k, v in res.items() if k not in ("frames", "refine")}), flush=True)
    elif args.mode == "init_sdf":
        res = runner.init_sdf(mesh=args.vis_mesh, normalize=args.vis_normalize, simplify_mode=args.mesh_simplify)
        runner.close()
        if runner.rank == 0:
            import json
            print(json.dumps({k: v for k, v in res.items() if k != "loss"}), flush=True)
    elif args.mode == "visual_hull":
        res = runner.visual_hull(resolution=args.hull_resolution, min_carve_votes=args.hull_votes)
        runner.close()
        if runner.rank == 0:
            import json
            res["silhouette"] = {k: v for k, v in res["silhouette"].items() if k != "frames"}
            res["stats"] = dict(res["stats"], sole_carved={k: v for k, v in res["stats"]["sole_carved"].items()
                                                           if k not in ("cells", "share")})
            print(json.dumps(res), flush=True)
    elif args.mode == "match_frames":
        res = runner.match_frames(guide=args.match_guide, offsets=args.match_offsets, mesh=args.vis_mesh, normalize=args.vis_normalize,
                                  resolution=args.mesh_resolution, warp=args.match_warp)
        runner.close()
        if runner.rank == 0:
            import json
            print(json.dumps({k: v for k, v in res.items() if k not in ("pairs", "steps")}), flush=True)
    elif args.mode == "mvs_depth":
        res = runner.mvs_depth(mesh=args.vis_mesh, normalize=args.vis_normalize, resolution=args.mesh_resolution,
                               offsets=args.mvs_offsets, range=args.mvs_range, step_px=args.mvs_step_px)
        runner.close()
        if runner.rank == 0:
            import json
            print(json.dumps({k: v for k, v in res.items() if k != "per_frame"}), flush=True)
    elif args.mode == "fuse_depth":
        res = runner.fuse_depth(mvs_dir=args.mvs_dir, resolution=args.fuse_resolution, trunc_cells=args.fuse_trunc_cells)
        runner.close()
        if runner.rank == 0:
            import json
            res["silhouette"] = {k: v for k, v in res["silhouette"].items() if k != "frames"}
            res["stats"] = {k: v for k, v in res["stats"].items() if k != "pixels"}
            print(json.dumps({k: v for k, v in res.items() if k not in ("residual_median", "residual_count")}), flush=True)
    elif args.mode == "render_views" or args.mode.startswith("interpolate_"):
        if args.mode == "render_views":
            views, level, method = args.views, args.view_level, args.view_method
        else:       # upstream's spelling: 60 poses there and back at half resolution, volume-rendered unless --view_method says otherwise
            _, i, j = args.mode.split("_")
            views = f"interpolate:{int(i)}:{int(j)}:60"
            level = 2 if args.view_level is None else args.view_level
            method = "volume" if args.view_method is None else args.view_method
        res = runner.render_views(views=views, level=level, method=method, background=args.view_background)
        if runner.rank == 0:
            import json
            print(json.dumps({k: v for k, v in res.items() if k not in ("rgb", "depth", "normal", "hit", "names", "psnr", "iou")}),
                  flush=True)
    elif args.mode == "evaluate_views":
        res = runner.evaluate_views(frames=args.eval_frames, maps=args.eval_maps, level=args.view_level, method=args.view_method,
                                    background=args.view_background)
        if runner.rank == 0:
            import json
            print(json.dumps({k: v for k, v in res.items() if k not in ("frames", "map")}), flush=True)
    elif args.mode == "export_poses":
        d = runner.export_poses(args.pose_dir)
        if runner.rank == 0:
            import json
            print(json.dumps({"dir": d, "frames": runner.dataset.n_images, "iter": runner.iter_step}), flush=True)
    else:
        res = 64 if args.mesh_resolution is None else args.mesh_resolution
        print("surface crossings", runner.validate_mesh(resolution=res, clean=args.mesh_clean, color=args.mesh_color,
                                                        extract=args.mesh_extract, simplify=args.mesh_simplify,
                                                        texture=args.mesh_texture, texture_size=args.texture_size)[1])
        xs = runner.last_extract_stats
        if xs is not None and runner.rank == 0:
            print(f"mesh_extract sparse: {xs['active_blocks']} of {xs['blocks']} blocks of {xs['block']}^3 cells active at lipschitz "
                  f"{xs['lipschitz']:g}, {xs['samples']} SDF queries against {xs['dense_samples']} dense "
                  f"({xs['dense_samples'] / xs['samples']:.1f}x fewer), {xs['verts']} vertices, {xs['faces']} faces", flush=True)
        st = runner.last_clean_stats
        if st is not None:
            print(f"mesh_clean {st['mode']}: removed {st['removed_verts']} of {st['verts_in']} vertices, {st['removed_faces']} of "
                  f"{st['faces_in']} faces ({st['components']} components)", flush=True)
        ss = runner.last_simplify_stats
        if ss is not None and runner.rank == 0:
            print(f"mesh_simplify {ss['mode']}: {ss['cells']} cells of edge {ss['cell_size']:.6g}, {ss['n_verts_in']} -> "
                  f"{ss['n_verts_out']} vertices, {ss['n_faces_in']} -> {ss['n_faces_out']} faces ({ss['n_collapsed']} collapsed, "
                  f"{ss['n_duplicate']} duplicate, {ss['n_clamped']} cells clamped, {ss['n_boundary_edges']} boundary and "
                  f"{ss['n_nonmanifold_edges']} non-manifold edges)", flush=True)
        cs = runner.last_color_stats
        if cs is not None and runner.rank == 0:
            print(f"mesh_color {cs['mode']}: {cs['verts_in']} vertices, {cs['unseen_verts']} seen by no view, "
                  f"{cs['mean_views']:.2f} views per seen vertex", flush=True)
        ts = runner.last_texture_stats
        if ts is not None and runner.rank == 0:
            print(f"mesh_texture {ts['mode']}: {ts['faces']} faces on a {ts['size']} x {ts['size']} atlas (cells of {ts['cell']} texels, "
                  f"{100 * ts['owned_frac']:.1f} % owned), {ts['unseen_texels']} owned texels seen by no view, {ts['mean_views']:.2f} "
                  f"views per seen texel, re-render PSNR {ts['psnr'] if ts['psnr'] is None else round(ts['psnr'], 2)} dB", flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
