"""Record tests/golden/runner_settings.json: what every settings block of the Runner and of the feature modules makes of a fixed list
of cases -- the merged dict, or the exception's type and full message.  tests/test_cpu_settings.py replays the file.

    python tests/golden/make_golden_runner_settings.py [--out path]

It needs no GPU and calls only entry points that outlive a reorganisation of the settings code: the Runner's _x_conf methods on
Runner.__new__(Runner) with .conf set, the modules' merge_settings / check_settings, and the Runner's modes themselves on such a bare
Runner with world = 1, whose inline merges raise on a bad key before any device work (a good key gets as far as _select_mesh, which is
replaced by a recorder, so the case holds the arguments the merge led to).  Run it at the commit BEFORE a change that must not move a
setting or a message; a difference in the test is a finding to explain, never a reason to run this again.

The cases of a block: an empty config, a partial block, every override alone, overrides that are None, an unknown key in the config,
an unknown key in the overrides, and for every bounded key the values at its bounds, the first ones outside them, a bool, a string and a
NaN."""
import argparse
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

NAN, INF = float("nan"), float("inf")
UNKNOWN = "no_such_key"


class Selected(Exception):
    """Raised by the recorder that stands in for Runner._select_mesh."""


def bare(conf):
    """A Runner with nothing but what the settings code reads."""
    from dynhor_amd.runner import Runner
    r = Runner.__new__(Runner)
    r.conf, r.world, r.rank, r.iter_step, r.pose_refiner = dict(conf), 1, 0, 0, None
    r.conf.setdefault("data_info", {})

    def select(*args, **kw):
        raise Selected(json.dumps({"args": list(args), "kw": kw}, sort_keys=True))
    r._select_mesh = select
    return r


def record(fn):
    try:
        return {"ok": json.loads(json.dumps(fn()))}
    except Selected as e:
        return {"select_mesh": json.loads(str(e))}
    except Exception as e:  # noqa: BLE001 -- the type and the message are what is recorded
        return {"error": type(e).__name__, "message": str(e)}


def ints(lo, hi=None):
    return [lo, lo - 1, True, "x", NAN, 2.0] + ([hi, hi + 1] if hi is not None else [])


def nums(lo, hi=None):
    out = [lo, math.nextafter(lo, -INF), math.nextafter(lo, INF), True, "x", NAN, INF]
    return out + ([hi, math.nextafter(hi, -INF), math.nextafter(hi, INF)] if hi is not None else [])


def block_cases(name, call, partial, overrides, bounded, unknown_override=True):
    """The standard cases of one block: call(conf, **overrides) -> the merged dict."""
    out = {"empty": (lambda: call({})), "partial": (lambda: call({name: partial})), "null_block": (lambda: call({name: None})),
           "none_overrides": (lambda: call({name: partial}, **{k: None for k in overrides})),
           "unknown_config": (lambda: call({name: {UNKNOWN: 1}}))}
    if unknown_override:
        out["unknown_override"] = lambda: call({}, **{UNKNOWN: 1})
        out["unknown_override_none"] = lambda: call({}, **{UNKNOWN: None})
    for k, v in overrides.items():
        out[f"override:{k}"] = lambda k=k, v=v: call({name: partial}, **{k: v})
    for k, values in bounded.items():
        for v in values:
            out[f"config:{k}={v!r}"] = lambda k=k, v=v: call({name: {k: v}})
    return out


def all_cases():
    from dynhor_amd import depth_fuse as df
    from dynhor_amd import match, mvs, pose_init, sdf_init
    from dynhor_amd import visual_hull as vh
    from dynhor_amd.mesh_extract import MAX_BLOCK
    from dynhor_amd.mesh_simplify import MAX_CELLS
    from dynhor_amd.pose_sil import DEFAULTS as POSE_SIL
    C = {}
    C["mesh_clean"] = block_cases("mesh_clean", lambda c, **o: bare(c)._clean_conf(**o), {"dilate_px": 3}, {"mode": "largest"},
                                  {"mode": ["none", "mask", "mask+largest", "bogus", 3, None], "dilate_px": [NAN, "x", -1]})
    C["mesh_color"] = block_cases("mesh_color", lambda c, **o: bare(c)._color_conf(**o), {"erode_px": 3}, {"mode": "network"},
                                  {"mode": ["views", "views+network", "texture", True], "min_cos": [NAN, "x"]})
    C["mesh_texture"] = block_cases("mesh_texture", lambda c, **o: bare(c)._texture_conf(**o), {"mode": "views", "size": 2048},
                                    {"mode": "views+network", "size": 512},
                                    {"size": ints(8, 32768), "sharpen": ints(0, 4), "mode": ["views", "network", None],
                                     "image": ["jpg", "bmp", None]})
    C["mesh_extract"] = block_cases("mesh_extract", lambda c, **o: bare(c)._extract_conf(**o), {"mode": "sparse", "lipschitz": 4},
                                    {"mode": "dense"}, {"block": ints(1, MAX_BLOCK), "lipschitz": nums(0.0), "mode": ["sparse", "blocks"]})
    C["mesh_simplify"] = block_cases("mesh_simplify", lambda c, **o: bare(c)._simplify_conf(**o), {"cells_max": 256}, {"mode": "faces:500"},
                                     {"mode": ["cells:32", "cells:0", "faces:x", "bogus", None, 3], "regularization": nums(0.0, 1e6),
                                      "cells_max": ints(1, MAX_CELLS)})
    C["surface_render"] = block_cases("surface_render", lambda c, **o: bare(c)._surface_conf(**o), {"level": 2, "max_steps": 64},
                                      {"method": "volume", "level": 4, "background": "black"},
                                      {"level": ints(1), "method": ["volume", "mesh"], "background": ["frame", "grey"], "eps": [NAN, "x"]})
    C["surface_render"]["volume_over_frame"] = lambda: bare({"surface_render": {"method": "volume"}})._surface_conf(background="frame")
    C["image_eval"] = block_cases("image_eval", lambda c, **o: bare(c)._image_eval_conf(**o), {"radius": 3}, {"frames": "all", "maps": True},
                                  {"erode_px": ints(0), "sigma": [NAN, "x"]})
    D = sdf_init.SDF_INIT_DEFAULTS
    sdf_over = {"iters": 0, "points": 2048, "ray_points": 4, "lr": 1e-2, "eik_weight": 0.0, "seed": -7, "share_near": 0.25, "share_far": 0.75,
                "sigma_near": 0.01, "sigma_far": 0.1, "heldout_points": 1, "heldout_seed": 5, "report_freq": 1, "resolution": 64}
    assert set(sdf_over) == set(D)
    sdf_bound = {k: ints(0 if k == "iters" else 1) for k in ("iters", "points", "ray_points", "heldout_points", "report_freq", "resolution")}
    sdf_bound.update({k: [-1, True, "x", NAN, 1.5] for k in ("seed", "heldout_seed")})
    sdf_bound.update({k: nums(0.0) for k in ("lr", "sigma_near", "sigma_far", "eik_weight", "share_near", "share_far")})
    C["sdf_init"] = block_cases("sdf_init", lambda c, **o: bare(c)._sdf_init_conf(**o), {"points": 4096, "lr": 2e-3}, sdf_over, sdf_bound)
    C["sdf_init"]["shares_over_one"] = lambda: bare({"sdf_init": {"share_near": 0.8, "share_far": 0.3}})._sdf_init_conf()
    C["sdf_init"]["points_not_a_multiple"] = lambda: bare({})._sdf_init_conf(points=10, ray_points=4)
    C["sdf_init"]["check_settings:defaults"] = lambda: sdf_init.check_settings(dict(D))
    C["sdf_init"]["check_settings:bad"] = lambda: sdf_init.check_settings(dict(D, iters=-1))
    C["sdf_init"]["init_sdf:unknown_override"] = lambda: bare({}).init_sdf(**{UNKNOWN: 1})
    C["sdf_init"]["init_sdf:no_template"] = lambda: bare({}).init_sdf()
    C["sdf_init"]["init_sdf:bad_normalize"] = lambda: bare({"data_info": {"obj_path": "t.ply"}}).init_sdf(normalize="unit")
    C["sdf_init"]["init_sdf:trained"] = lambda: setattr(r := bare({}), "iter_step", 5) or r.init_sdf(mesh="t.ply")
    V = vh.VISUAL_HULL_DEFAULTS
    vh_over = {"resolution": 64, "bound": 0.6, "coarse_resolution": 32, "band_px": 8, "min_carve_votes": 2, "min_seen": 0.25,
               "outside_value": 2.0, "frame_chunk": 4, "point_chunk": 1024}
    assert set(vh_over) == set(V)
    vh_bound = {"resolution": ints(2, vh.MAX_RESOLUTION), "coarse_resolution": ints(2, vh.MAX_RESOLUTION), "bound": nums(0.0) + ["auto", "box"],
                "band_px": nums(1, 2048), "min_carve_votes": ints(1, 8), "min_seen": nums(0, 1), "outside_value": nums(0.0),
                "frame_chunk": ints(1), "point_chunk": ints(1)}
    C["visual_hull"] = block_cases("visual_hull", lambda c, **o: bare(c)._visual_hull_conf(**o), {"resolution": 96, "min_carve_votes": 2},
                                   vh_over, vh_bound)
    C["visual_hull"].update({"merge_settings:" + k: f for k, f in block_cases(
        "visual_hull", lambda c, **o: vh.merge_settings(c.get("visual_hull"), **o), {"resolution": 96}, {"band_px": 8}, {}).items()})
    C["visual_hull"]["check_settings:defaults"] = lambda: vh.check_settings(dict(V))
    C["visual_hull"]["check_settings:unknown"] = lambda: vh.check_settings(dict(V, **{UNKNOWN: 1}))
    C["visual_hull"]["check_settings:missing"] = lambda: vh.check_settings({k: v for k, v in V.items() if k != "band_px"})
    C["visual_hull"]["visual_hull:unknown_override"] = lambda: bare({}).visual_hull(**{UNKNOWN: 1})
    Z = df.DEPTH_FUSE_DEFAULTS
    df_over = {"resolution": 96, "trunc_cells": 2.5, "prior_weight": 510, "weight": "uniform", "floor_weight": 1, "frame_chunk": 4,
               "point_chunk": 1024}
    assert set(df_over) == set(Z)
    df_bound = {"resolution": ints(2, vh.MAX_RESOLUTION), "trunc_cells": nums(0.0, 64), "prior_weight": nums(0.0, 1e9),
                "weight": ["cos", "sin", None], "floor_weight": ints(1, 255), "frame_chunk": ints(1), "point_chunk": ints(1)}
    C["depth_fuse"] = block_cases("depth_fuse", lambda c, **o: df.merge_settings(c.get("depth_fuse"), **o),
                                  {"resolution": 96, "prior_weight": 510}, df_over, df_bound)
    C["depth_fuse"]["check_settings:defaults"] = lambda: df.check_settings(dict(Z))
    C["depth_fuse"]["check_settings:unknown"] = lambda: df.check_settings(dict(Z, **{UNKNOWN: 1}))
    C["depth_fuse"]["check_settings:missing"] = lambda: df.check_settings({k: v for k, v in Z.items() if k != "prior_weight"})
    C["depth_fuse"]["fuse_depth:unknown_override"] = lambda: bare({}).fuse_depth(**{UNKNOWN: 1})
    C["depth_fuse"]["fuse_depth:unknown_config"] = lambda: bare({"depth_fuse": {UNKNOWN: 1}}).fuse_depth()
    C["depth_fuse"]["fuse_depth:bad_hull_block"] = lambda: bare({"visual_hull": {"min_seen": 2.0}}).fuse_depth()
    # mvs and match: the module's check_settings takes the settings as one dict (a key at None keeps its default); the Runner's mode
    # layers the block and the overrides first
    M = mvs.DEFAULTS
    mvs_over = {"offsets": "1,3", "sigma": 0.0, "a_min": 0.25, "erode_px": 0, "patch": 2, "range": 0.1, "depths": 17, "fine_depths": 5,
                "step_px": 2, "min_va": 100, "min_vb": 50.0, "min_views": 1, "min_cos": -1.0, "score_min": 0.5, "peak_margin": 0.0,
                "depth_rel": 0.0, "min_consistent": 0, "frame_chunk": 1}
    assert set(mvs_over) == set(M)
    mvs_bound = {"patch": ints(1, mvs.MAX_PATCH), "depths": ints(3, mvs.MAX_DEPTHS) + [4], "fine_depths": ints(3, mvs.MAX_DEPTHS) + [4],
                 "offsets": [(1, 2, 3, 4), (1, 2, 3, 4, 5), (0,), (), "", "a", True], "range": nums(0.0), "step_px": ints(1),
                 "min_views": ints(1, 4), "min_consistent": ints(0, 4), "min_va": ints(1), "min_vb": nums(0.0), "min_cos": nums(-1, 1),
                 "depth_rel": nums(0.0), "sigma": nums(0.0), "erode_px": ints(0), "frame_chunk": ints(1)}
    C["mvs"] = block_cases("mvs", lambda c, **o: mvs.check_settings(dict(c.get("mvs") or {}, **o)), {"patch": 3, "range": None}, mvs_over,
                           mvs_bound)
    run_mvs = lambda c, **o: bare(c).mvs_depth(**o)
    C["mvs"].update({"mvs_depth:" + k: f for k, f in block_cases("mvs", run_mvs, {"patch": 3, "voxel": 0.01}, {"step_px": 2, "voxel": 0.02},
                                                                 {"patch": [0, "x"], "voxel": [NAN]}).items()})
    C["mvs"]["mvs_depth:many_ranks"] = lambda: setattr(r := bare({}), "world", 2) or r.mvs_depth()
    A = match.DEFAULTS
    match_over = {"guide": "mesh", "offsets": "1,2", "sigma": 0.0, "a_min": 0.25, "erode_px": 0, "patch": 2, "range": 5, "excl": 0, "min_va": 100,
                  "zncc_min": 0.5, "peak_margin": 0.0, "peak_full": 0.5, "fb_px": 0, "step": 2, "max_per_pair": 16, "depth_eps": 0.0,
                  "min_cos": 0.0, "frame_chunk": 1, "warp": "none", "warp_max": 1}
    assert set(match_over) == set(A)
    match_bound = {"guide": ["mesh", "hull", None], "patch": ints(1, 7), "range": ints(0, 32), "excl": ints(0), "min_va": ints(1),
                   "peak_full": nums(0.0), "fb_px": nums(0.0), "sigma": nums(0.0), "erode_px": ints(0),
                   "offsets": [(1,), (0,), (), "", "a", True], "warp": ["affine", "bogus"], "warp_max": nums(1.0, match.WARP_MAX_LIMIT)}
    C["match"] = block_cases("match", lambda c, **o: match.check_settings(dict(c.get("match") or {}, **o)), {"patch": 3, "range": None},
                             match_over, match_bound)
    C["match"]["affine_with_mesh"] = lambda: match.check_settings({"guide": "mesh", "warp": "affine", "warp_max": 2})
    run_match = lambda c, **o: bare(dict(c, match=dict({"guide": "mesh"}, **(c.get("match") or {})))).match_frames(**o)
    C["match"].update({"match_frames:" + k: f for k, f in block_cases(
        "match", run_match, {"patch": 3}, {"guide": "mesh", "offsets": "1,2", "warp": "affine", "step": 2, "resolution": 64, "mesh": "m.ply",
                                           "normalize": "reference", "clean": "mask", "extract": "sparse", "simplify": "cells:32"},
        {"patch": [0, "x"]}).items()})
    C["match"]["match_frames:config_guide"] = lambda: bare({"match": {"guide": "mesh"}, "pose_sil": {"resolution": 64}}).match_frames()
    C["match"]["match_frames:many_ranks"] = lambda: setattr(r := bare({}), "world", 2) or r.match_frames()
    # the four blocks refine_poses_silhouette merges inline, the two of init_poses, and mesh_vis
    refine = lambda c, **o: bare(c).refine_poses_silhouette(**o)
    sil_over = {k: (v * 2 if not isinstance(v, bool) else v) for k, v in POSE_SIL.items()}
    C["pose_sil"] = block_cases("pose_sil", refine, {"resolution": 64, "iters": 10}, sil_over, {"resolution": [2, True, "x", NAN, 64.5]})
    C["pose_sil"]["many_ranks"] = lambda: setattr(r := bare({}), "world", 2) or r.refine_poses_silhouette()
    C["pose_photo"] = block_cases("pose_photo", refine, {"points": 1000}, {"photo": "views"},
                                  {"mode": ["none", "views", "mesh", "texture", None], "points": [NAN, "x"]}, unknown_override=False)
    C["pose_photo"]["unknown_config_and_bad_mode"] = lambda: refine({"pose_photo": {UNKNOWN: 1}}, photo="texture")
    C["pose_corr"] = block_cases("pose_corr", refine, {"lw_corr": 1e-2}, {"corr": "dataset"},
                                 {"mode": ["none", "dataset", "match", "votes", None], "delta_px": [NAN, "x"]}, unknown_override=False)
    C["pose_corr"]["unknown_config_and_bad_mode"] = lambda: refine({"pose_corr": {UNKNOWN: 1}}, corr="votes")
    C["mesh_vis"] = block_cases("mesh_vis", lambda c, **o: bare(c).visualize_mesh(**o), {"mesh": "m.ply", "normalize": "reference"},
                                {"mesh": "n.obj", "normalize": "none", "resolution": 64, "alpha": 0.5, "turntable": 4, "clean": "mask",
                                 "extract": "sparse", "simplify": "cells:32"},
                                {"resolution": [2, True, "x", NAN], "alpha": ["x"], "turntable": ["x"], "normalize": ["unit"]},
                                unknown_override=False)
    C["mesh_vis"].update({"refine:" + k: f for k, f in block_cases(
        "mesh_vis", refine, {"mesh": "m.ply", "normalize": "reference", "resolution": 256},
        {"mesh": "n.obj", "normalize": "none", "resolution": 64, "clean": "mask", "extract": "sparse", "simplify": "cells:32"}, {},
        unknown_override=False).items()})
    C["mesh_vis"].update({"mvs_depth:" + k: f for k, f in block_cases(
        "mesh_vis", run_mvs, {"mesh": "m.ply", "normalize": "reference", "resolution": 256},
        {"mesh": "n.obj", "normalize": "none", "resolution": 64, "clean": "mask", "extract": "sparse", "simplify": "cells:32"}, {},
        unknown_override=False).items()})
    # evaluate_mesh's eval: block (a null in it counts as not set): a case ends at the first value that does not convert, at a bad
    # alignment mode, or at the ground-truth file, which does not exist -- each message names the value the layering led to
    run_eval = lambda c, **o: bare(dict(c, eval=dict({"gt_mesh": "default.ply"}, **(c.get("eval") or {})))).evaluate_mesh(**o)
    C["eval"] = block_cases("eval", run_eval, {"gt_mesh": "config.ply", "gt_align": "rigid", "taus": None},
                            {"gt_mesh": "argument.ply", "gt_normalize": "reference", "resolution": "r", "gt_resolution": "g", "n_samples": "n",
                             "taus": ("t",), "gt_align": "affine", "gt_align_init": "local", "align_opts": {"x": 1}},
                            {"gt_mesh": [None, "other.obj"], "gt_align": [None, "similarity", "affine"], "gt_align_init": ["global", "local"],
                             "resolution": [None, "r", NAN], "taus": [None, 3, ("t",)]}, unknown_override=False)
    init = lambda c, **o: bare(c).init_poses(**o)
    init_over = {k: (v * 2 if not isinstance(v, bool) else v) for k, v in pose_init.DEFAULTS.items()}
    C["pose_init"] = block_cases("pose_init", init, {"candidates": 4}, init_over, {"candidates": [0, "x"]})
    C["pose_init"]["bad_normalize"] = lambda: init({"data_info": {"obj_path": "t.ply"}}, normalize="unit")
    C["pose_init"]["bad_normalize_with_mesh"] = lambda: init({}, mesh="t.ply", normalize="unit")
    C["pose_init"]["many_ranks"] = lambda: setattr(r := bare({}), "world", 2) or r.init_poses()
    C["pose_init"]["module:unknown"] = lambda: pose_init.init_poses(None, None, None, **{UNKNOWN: 1})
    return C


def run_cases():
    """{block: {case: result}} of every case, in the order of all_cases()."""
    return {block: {name: record(fn) for name, fn in cases.items()} for block, cases in all_cases().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "runner_settings.json"))
    args = ap.parse_args()
    out = run_cases()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    n = sum(len(v) for v in out.values())
    bad = {b: [k for k, r in v.items() if r.get("error") in ("AttributeError", "NameError", "ImportError")] for b, v in out.items()}
    print(f"{n} cases of {len(out)} blocks -> {args.out}; cases that ended in an Attribute/Name/ImportError: "
          f"{ {b: k for b, k in bad.items() if k} }")


if __name__ == "__main__":
    main()
