"""The one layering of every settings block -- defaults, then the YAML's optional block, then the overrides that are not None -- and
the handful of checks most blocks share.  Plain functions; a block's own domain rules stay in its module.

Which side rejects an unknown key differs from block to block.  That is history, not design, and it is kept as it was (C: the
config's block, O: the overrides, -: nobody):

    mesh_clean, mesh_color, mesh_texture, mesh_extract, mesh_simplify, mesh_vis       -   (the overrides are named arguments)
    eval                                                                              -   (and a null in the block counts as not set)
    surface_render                                                                    C   ("unknown keys", in Runner._surface_conf)
    image_eval                                                                        C   ("unknown keys")
    sdf_init                                                                          C O
    visual_hull, depth_fuse                                                           C O (the block first; an override at None is not looked at)
    mvs                                                                               C O (voxel is the Runner's own key)
    match                                                                             O   (the block: match.check_settings, after the guide mesh)
    pose_sil                                                                          O
    pose_init                                                                         O   (the block: pose_init.init_poses, after the template)
    pose_photo, pose_corr                                                             C   (with the mode, in refine_poses_silhouette's wording)
"""
from __future__ import annotations

import math


def is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def is_num(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def merge(name, defaults, block, overrides=None, *, who=None, check_block=False, check_overrides=False) -> dict:
    """dict(defaults), updated with the YAML's `block` (None: empty), then with the `overrides` that are not None.  check_overrides /
    check_block: ValueError for a key `defaults` does not have (the overrides are looked at first, a None among them too), as
    "<name>: unknown setting(s) [..]" -- "<who>: unknown <name> setting(s) [..]" when the calling mode `who` is given -- with
    " in the config" for the block; check_block="keys": the block's older wording "<name>: unknown keys [..]"."""
    block, overrides = block or {}, overrides or {}
    head = f"{who}: unknown {name} setting(s)" if who else f"{name}: unknown setting(s)"
    for on, src, where in ((check_overrides, overrides, ""), (check_block, block, " in the config")):
        unknown = sorted(set(src) - set(defaults))
        if on and unknown:
            raise ValueError(f"{name}: unknown keys {unknown}; known: {sorted(defaults)}" if on == "keys" else
                             f"{head} {unknown}{where}; known: {sorted(defaults)}")
    return {**defaults, **block, **{k: v for k, v in overrides.items() if v is not None}}


def int_in(block, key, v, lo, hi):
    if not is_int(v) or not lo <= v <= hi:
        raise ValueError(f"{block} {key} must be an integer in [{lo}, {hi}], got {v!r}")


def one_of(block, key, v, choices):
    if v not in choices:
        raise ValueError(f"{block} {key} must be one of {choices}, got {v!r}")


# train.* keys of the priors with a validity (dh_prior_loss; DESIGN_NEXT_ROWS.md section 27).  depth_weight 0 = the depth term off;
# depth_delta = the Huber width in the dataset's depth units (0.02 = 2 % of the unit sphere's radius); depth_start_iter = the first
# iteration with the term; normal_skip_missing = the normal term over the pixels that have a normal.  The first three are first
# settings, not tuned.
PRIOR_DEFAULTS = {"depth_weight": 0.0, "depth_delta": 0.02, "depth_start_iter": 0, "normal_skip_missing": False}


def prior_settings(train: dict) -> dict:
    """The four prior keys of a train: block, checked.  The block holds every other training key too, so only a key that reads as one of
    these -- it starts with depth_ or normal_skip -- and is not one is rejected as unknown."""
    unknown = sorted(k for k in train if (k.startswith("depth_") or k.startswith("normal_skip")) and k not in PRIOR_DEFAULTS)
    if unknown:
        raise ValueError(f"train: unknown setting(s) {unknown}; known: {sorted(PRIOR_DEFAULTS)}")
    pr = {k: train.get(k, v) for k, v in PRIOR_DEFAULTS.items()}
    if not is_num(pr["depth_weight"]) or pr["depth_weight"] < 0:
        raise ValueError(f"train depth_weight must be a number >= 0, got {pr['depth_weight']!r}")
    if not is_num(pr["depth_delta"]) or not pr["depth_delta"] > 0:
        raise ValueError(f"train depth_delta must be a number > 0, got {pr['depth_delta']!r}")
    int_in("train", "depth_start_iter", pr["depth_start_iter"], 0, 2 ** 31 - 1)
    if not isinstance(pr["normal_skip_missing"], bool):
        raise ValueError(f"train normal_skip_missing must be true or false, got {pr['normal_skip_missing']!r}")
    return pr


def warp_settings(train: dict) -> dict:
    """The multi-view photometric term's keys of a train: block (dh_warp_loss; DESIGN_NEXT_ROWS.md section 30), checked: `weight`
    (train.warp_weight, 0 = the term off) and every key of warp_loss.DEFAULTS (train.warp_<key>).  Only a key that starts with warp_ and is
    none of these is rejected as unknown; prior_settings' keys are not looked at."""
    from .warp_loss import DEFAULTS, check_settings
    known = {"warp_weight"} | {"warp_" + k for k in DEFAULTS}
    unknown = sorted(k for k in train if k.startswith("warp_") and k not in known)
    if unknown:
        raise ValueError(f"train: unknown setting(s) {unknown}; known: {sorted(known)}")
    w = train.get("warp_weight", 0.0)
    if not is_num(w) or w < 0:
        raise ValueError(f"train warp_weight must be a number >= 0, got {w!r}")
    s = check_settings({k: train["warp_" + k] for k in DEFAULTS if "warp_" + k in train})
    return {"weight": float(w), **s}
