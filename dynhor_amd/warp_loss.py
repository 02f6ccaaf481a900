"""Multi-view photometric consistency on the training path (csrc/warp_loss.hip, include/dynhor_hip.h; DESIGN_NEXT_ROWS.md section 30).

Per ray of a batch drawn from frame i: the surface point the ray renders (the weight-normalised expected depth, ``ray_depth``) and the
rendered normal span a plane; its homography carries the (2P+1)^2 grey patch about the ray's pixel into the neighbouring frames
(``mvs.neighbours``), each neighbour is scored by normalised cross-correlation on ``match.gray_frames``' grey bytes, and the mean of the
``topk`` smallest 1 - score is the ray's loss (``warp_loss``).  Its exact derivative with respect to the depth and the normal goes into
the renderer's two adjoint channels d_weights and d_nmap (``ray_depth_bwd``).  ``frames_for`` builds the resident tables once.

Every default is a first setting, not tuned.  Limits: no pose or intrinsics adjoint (the Runner refuses train.refine_poses with the
term); no occlusion test in the neighbour beyond the top-k choice and the validity map; the surface point is the weight-normalised
expected depth, not an interpolated zero crossing; the normal is the rendered one; neighbours are chosen by frame offset, not by
baseline; no weight schedule.

The kernels run on the current stream; there is no CPU path.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import _lib
from .settings import int_in, is_num, merge

# defaults of the train.warp_* keys -- first settings, none of them tuned.  min_va None: match's 4 N^2; min_vb None: float(min_va)
DEFAULTS = {"patch": 5, "offsets": (1, 2, 4, 8), "topk": 4, "min_views": 2, "min_cos": 0.1, "min_wsum": 0.5, "sigma": 1.0, "a_min": 0.5,
            "erode_px": 1, "start_iter": 0, "min_va": None, "min_vb": None}
MAX_PATCH, MAX_NEIGHBOURS = 7, 8


def _p(t):
    return None if t is None else _lib.ptr(t)


def check_settings(settings: dict | None = None) -> dict:
    """DEFAULTS updated with `settings`, checked; an unknown key raises ValueError."""
    s = merge("warp", DEFAULTS, None, settings, check_overrides=True)
    int_in("warp", "patch", s["patch"], 1, MAX_PATCH)
    int_in("warp", "topk", s["topk"], 1, MAX_NEIGHBOURS)
    int_in("warp", "min_views", s["min_views"], 1, MAX_NEIGHBOURS)
    int_in("warp", "erode_px", s["erode_px"], 0, 64)
    int_in("warp", "start_iter", s["start_iter"], 0, 2 ** 31 - 1)
    offs = s["offsets"]
    if not isinstance(offs, (list, tuple)) or not 1 <= len(offs) <= MAX_NEIGHBOURS // 2 or any(not isinstance(o, int) or isinstance(o, bool)
                                                                                                or o < 1 for o in offs):
        raise ValueError(f"warp offsets must be 1..{MAX_NEIGHBOURS // 2} positive integers, got {offs!r}")
    s["offsets"] = tuple(offs)
    if not is_num(s["min_cos"]) or not -1.0 <= s["min_cos"] <= 1.0:
        raise ValueError(f"warp min_cos must be a number in [-1, 1], got {s['min_cos']!r}")
    for k in ("min_wsum", "sigma", "a_min"):
        if not is_num(s[k]) or s[k] < 0:
            raise ValueError(f"warp {k} must be a number >= 0, got {s[k]!r}")
    if s["min_va"] is not None:
        int_in("warp", "min_va", s["min_va"], 1, 2 ** 62)
    if s["min_vb"] is not None and (not is_num(s["min_vb"]) or not s["min_vb"] > 0):
        raise ValueError(f"warp min_vb must be a number > 0, got {s['min_vb']!r}")
    return s


def kernel_settings(s: dict) -> SimpleNamespace:
    """The settings dh_warp_loss takes, from a checked settings dict."""
    from .match import default_min_va
    min_va = default_min_va(s["patch"]) if s["min_va"] is None else int(s["min_va"])
    return SimpleNamespace(patch=int(s["patch"]), topk=int(s["topk"]), min_views=int(s["min_views"]), min_cos=float(s["min_cos"]),
                           min_wsum=float(s["min_wsum"]), min_va=min_va, min_vb=float(min_va if s["min_vb"] is None else s["min_vb"]))


def neighbour_table(n_frames: int, train_frames, offsets) -> torch.Tensor:
    """int32 [n_frames, 2 len(offsets)] on the CPU: mvs.neighbours with every frame outside `train_frames` replaced by -1, so a
    held-out frame never enters training."""
    from .mvs import neighbours
    nbr = neighbours(n_frames, offsets)
    keep = torch.zeros(int(n_frames) + 1, dtype=torch.bool)
    keep[torch.as_tensor(list(train_frames), dtype=torch.long)] = True
    keep[-1] = False                                   # where the -1 entries look
    return torch.where(keep[nbr.long()], nbr, torch.full_like(nbr, -1))


def frames_for(dataset, train_frames, **settings) -> SimpleNamespace:
    """The resident tables of the term, built once: gray, valid u8 [F,H,W] (mesh_color.usable_map -> match.gray_frames: 2 bytes per
    pixel and frame, 1.2 GB for 300 frames of 1080 x 1920), nbr int32 [F,Nn] (neighbour_table), K, Kinv f32 [9] and the kernel's
    settings.  The poses are read from the dataset at every call."""
    from .match import gray_frames
    from .mesh_color import usable_map
    from .mvs import _kinv
    s = check_settings(settings)
    usable = usable_map(dataset.label, s["erode_px"])
    gray, valid = gray_frames(dataset.rgb, usable, s["sigma"], s["a_min"])
    dev = gray.device
    nbr = neighbour_table(dataset.n_images, train_frames, s["offsets"]).to(dev).contiguous()
    K = dataset.K.detach().float().reshape(9).contiguous()
    return SimpleNamespace(gray=gray.contiguous(), valid=valid.contiguous(), nbr=nbr, K=K, Kinv=_kinv(dataset.K), settings=kernel_settings(s),
                           raw_settings=s)


def step_input(tables, dataset, frame: int, weight: float, pixels=None) -> SimpleNamespace:
    """The `warp` argument of train_step_core for a batch drawn from `frame`: the tables, the dataset's current poses, the batch's
    pixels (default dataset._last_pixels) as int32 [B,2] and the weight."""
    px, py = dataset._last_pixels if pixels is None else pixels
    pix = torch.stack([px, py], dim=1).to(torch.int32).contiguous()
    return SimpleNamespace(tables=tables, R_all=dataset.R, T_all=dataset.T, frame=int(frame), pix=pix, weight=float(weight),
                           settings=tables.settings)


@torch.no_grad()
def ray_depth(rays, R, z, weights, sample_dist, packed=None, call=None):
    """(t, wsum, zc) f32 [B] of dh_ray_depth (packed = (seg_off, seg_cnt, max_samples): dh_ray_depth_packed, z = t_start, sample_dist =
    the step).  call(name, fn, *args): the renderer's stage timer (default: a plain checked call)."""
    L = _lib.lib()
    B = rays.shape[0]
    t, wsum, zc = (torch.empty(B, device=rays.device) for _ in range(3))
    call = call or (lambda name, fn, *a: _lib.check(fn(*a)))
    if packed is None:
        call("ray_depth", L.dh_ray_depth, _p(rays), _p(R), _p(z), _p(weights), B, int(z.shape[1]), float(sample_dist), _p(t), _p(wsum),
             _p(zc), _lib.stream())
    else:
        off, cnt, max_samples = packed
        call("ray_depth", L.dh_ray_depth_packed, _p(rays), _p(R), _p(z), _p(weights), B, _p(off), _p(cnt), int(max_samples),
             float(sample_dist), _p(t), _p(wsum), _p(zc), _lib.stream())
    return t, wsum, zc


@torch.no_grad()
def warp_loss(gray, valid, R_all, T_all, K, Kinv, nbr, frame, pix, zc, wsum, normal, st, weight=0.0, call=None):
    """(out_f f32 [B,8], out_i int32 [B,4], stats f32 [8]) of dh_warp_loss; st = kernel_settings(..).  No host read."""
    L = _lib.lib()
    F, H, W = gray.shape
    B = pix.shape[0]
    dev = gray.device
    out_f = torch.empty(B, 8, device=dev)
    out_i = torch.empty(B, 4, dtype=torch.int32, device=dev)
    stats = torch.empty(8, device=dev)
    ws = torch.empty(max(16, int(L.dh_warp_loss_workspace(B))), dtype=torch.uint8, device=dev)
    call = call or (lambda name, fn, *a: _lib.check(fn(*a)))
    call("warp_loss", L.dh_warp_loss, _p(gray), _p(valid), F, H, W, _p(R_all), _p(T_all), _p(K), _p(Kinv), _p(nbr), int(nbr.shape[1]),
         int(frame), _p(pix), _p(zc), _p(wsum), _p(normal), B, st.patch, st.min_va, st.min_vb, st.topk, st.min_views, st.min_cos, st.min_wsum,
         float(weight), _p(out_f), _p(out_i), _p(stats), _p(ws), _lib.stream())
    return out_f, out_i, stats


@torch.no_grad()
def ray_depth_bwd(rays, R, z, t, wsum, out_f, stats, sample_dist, weight, d_weights, d_nmap, add_weights=False, add_nmap=False, packed=None,
                  call=None):
    """dh_ray_depth_bwd (packed: dh_ray_depth_bwd_packed): writes, or with add_* adds to, d_weights and d_nmap."""
    L = _lib.lib()
    B = rays.shape[0]
    acc = (1 if add_weights else 0) | (2 if add_nmap else 0)
    call = call or (lambda name, fn, *a: _lib.check(fn(*a)))
    head = (_p(rays), _p(R), _p(z), _p(t), _p(wsum), _p(out_f), _p(stats), B)
    tail = (float(weight), acc, _p(d_weights), _p(d_nmap), _lib.stream())
    if packed is None:
        call("ray_depth_bwd", L.dh_ray_depth_bwd, *head, int(z.shape[1]), float(sample_dist), *tail)
    else:
        off, cnt, max_samples = packed
        call("ray_depth_bwd", L.dh_ray_depth_bwd_packed, *head, _p(off), _p(cnt), int(max_samples), float(sample_dist), *tail)


@torch.no_grad()
def warp_term(w, rays, R, z, weights, nmap, sample_dist, d_weights, d_nmap, add_weights, add_nmap, packed=None, call=None):
    """The whole term on a forward state: ray_depth -> warp_loss -> ray_depth_bwd.  w = step_input(..).  Returns (stats [8], out_f,
    out_i); no host read."""
    tb = w.tables
    R_all = w.R_all.contiguous().float().reshape(-1, 9)
    T_all = w.T_all.contiguous().float().reshape(-1, 3)
    t, wsum, zc = ray_depth(rays, R, z, weights, sample_dist, packed=packed, call=call)
    out_f, out_i, stats = warp_loss(tb.gray, tb.valid, R_all, T_all, tb.K, tb.Kinv, tb.nbr, w.frame, w.pix, zc, wsum, nmap, w.settings,
                                    w.weight, call=call)
    ray_depth_bwd(rays, R, z, t, wsum, out_f, stats, sample_dist, w.weight, d_weights, d_nmap, add_weights, add_nmap, packed=packed,
                  call=call)
    return stats, out_f, out_i
