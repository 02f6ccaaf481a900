"""Volumetric fusion of per-frame depth maps into a mesh (Runner.fuse_depth, --mode fuse_depth): the depth maps of mvs_depth,
integrated into a truncated signed distance field (TSDF) on the visual hull's own grid, with the hull as a weak prior so that the
surface is closed, meshed by mesh.marching_cubes.  Depth maps see what the hull cannot: a concavity lies in front of the hull's surface
in every frame that looks into it, and a frame whose pose is wrong in a way its outline hides still disagrees in depth with the rest.

  * ``integrate`` (dh_tsdf_integrate, csrc/tsdf.hip): per (point, frame) the point is projected (mesh_raster.h's mk_project), the
    nearest pixel's depth zd and weight wt are read, d = zd - z is cut to [-trunc, trunc] (a point further than trunc behind the
    surface is hidden: skipped) and q = rint(min(d / trunc, 1) 65536); num += wt q, den += wt, obs += 1.  The sums are integers:
    the state depends on the set of frames alone, not on their order or their split into calls.
  * ``weights_from_normals``: wt = max(1, round(255 max(0, -n.e / |e|))) where the pixel has a normal (the cosine between the
    surface and the viewing ray e = Kinv (x, y, 1)), floor_weight where it has none.
  * ``fuse_field``: frames in chunks outside, points in 4 x 4 x 4 bricks inside (visual_hull.brick_points), in grid order on return.
  * ``fused_mesh``: the box of the hull's coarse pass, the hull field h on the fine grid, trunc = trunc_cells cell,
    q_h = clamp(h / trunc, -1, 1) 65536, field = (num + prior_weight q_h) / ((den + prior_weight) 65536) in fp64, rounded to fp32,
    mesh = marching_cubes(-field, 0): the hull's sign convention, inside <= 0.
  * ``frame_residuals``: every pixel with a depth, back-projected and looked up in the field: |field| trunc where |field| < 1; per
    frame the median -- the frame that disagrees with the fusion of all is the frame whose pose or depth is off.

Limits.  The distance is projective, along the camera's z: it overstates the distance to a surface seen at a grazing angle.  The
nearest pixel of a sparse grid (mvs step_px > 1) is up to step_px / 2 pixels away.  One outlier depth whose weights sum to more than
prior_weight carves.  The prior pulls the bottom of a concavity towards the hull.

The kernel runs on the current stream; there is no CPU path for ``integrate``.
"""
from __future__ import annotations

import math
import os

import torch

from . import _lib
from . import visual_hull as vh
from ._args import check_cams, device_tensor, lap
from .settings import int_in, is_int, is_num, merge

# First settings, not tuned (as mvs.DEFAULTS).  resolution: grid points per axis (at most visual_hull.MAX_RESOLUTION); trunc_cells: the
# truncation distance in cells of the grid; prior_weight: the weight of the hull's field, 255 = one frame at full weight (> 0:
# without a prior a TSDF grows a back face at -trunc, and marching_cubes has no masked cells); weight: "cos" (weights_from_normals) or
# "uniform" (255 wherever there is a depth); floor_weight: the weight of a pixel with a depth and no normal; frame_chunk /
# point_chunk: the sizes of the two loops (results do not depend on them)
DEPTH_FUSE_DEFAULTS = {"resolution": 128, "trunc_cells": 4, "prior_weight": 255, "weight": "cos", "floor_weight": 64, "frame_chunk": 16,
                       "point_chunk": 1 << 22}
Q_ONE = 65536
N_WORST = 5


def check_settings(c: dict):
    """ValueError unless c is a full, sensible dict over DEPTH_FUSE_DEFAULTS; the message names the unknown, missing or bad key."""
    merge("depth_fuse", DEPTH_FUSE_DEFAULTS, None, c, check_overrides=True)
    missing = sorted(set(DEPTH_FUSE_DEFAULTS) - set(c))
    if missing:
        raise ValueError(f"depth_fuse: missing setting(s) {missing}")
    int_in("depth_fuse", "resolution", c["resolution"], 2, vh.MAX_RESOLUTION)
    if not is_num(c["trunc_cells"]) or not 0 < c["trunc_cells"] <= 64:
        raise ValueError(f"depth_fuse trunc_cells must be a number in (0, 64], got {c['trunc_cells']!r}")
    if not is_num(c["prior_weight"]) or not 0 < c["prior_weight"] <= 1e9:
        raise ValueError("depth_fuse prior_weight must be a number in (0, 1e9] (without the hull as a prior the field grows a back face "
                         f"at -trunc), got {c['prior_weight']!r}")
    if c["weight"] not in ("cos", "uniform"):
        raise ValueError(f"depth_fuse weight must be 'cos' or 'uniform', got {c['weight']!r}")
    int_in("depth_fuse", "floor_weight", c["floor_weight"], 1, 255)
    for k in ("frame_chunk", "point_chunk"):
        if not is_int(c[k]) or c[k] < 1:
            raise ValueError(f"depth_fuse {k} must be a positive integer, got {c[k]!r}")


def fuse_settings(block=None, **overrides) -> dict:
    """DEPTH_FUSE_DEFAULTS, then the YAML's optional depth_fuse: block, then the overrides that are not None; checked (in the order
    of visual_hull.hull_settings)."""
    c = merge("depth_fuse", DEPTH_FUSE_DEFAULTS, block, check_block=True)
    c = merge("depth_fuse", DEPTH_FUSE_DEFAULTS, c, {k: v for k, v in overrides.items() if v is not None}, check_overrides=True)
    check_settings(c)
    return c


merge_settings = fuse_settings           # the name the config tests and earlier callers know


def integrate(points, depth, weight, R, T, K, trunc, num, den, obs):
    """One chunk of frames added to the state, in place (dh_tsdf_integrate): points f32 [n,3], depth f32 [F,H,W] (camera z; inf, NaN
    or <= 1e-3: none), weight u8 [F,H,W] (0: none), R [F,3,3], T [F,3], K [3,3] of the depth image, trunc > 0; num int64 [n], den int32
    [n], obs int32 [n], all started at 0."""
    fn = "integrate"
    for name, t in (("num", num), ("den", den), ("obs", obs)):
        if torch.is_tensor(t) and not t.is_contiguous():
            raise ValueError(f"{fn}: {name} is updated in place and must be contiguous")
    points = device_tensor(fn, "points", points, torch.float32, lambda s: len(s) == 2 and s[1] == 3, "[n,3]")
    n = points.shape[0]
    depth = device_tensor(fn, "depth", depth, torch.float32, lambda s: len(s) == 3, "[F,H,W]")
    F, H, W = depth.shape
    weight = device_tensor(fn, "weight", weight, torch.uint8, lambda s: s == (F, H, W), f"[{F},{H},{W}]")
    R, T, K = check_cams(fn, F, R, T, K, points.device)
    for name, t, dtype in (("num", num, torch.int64), ("den", den, torch.int32), ("obs", obs, torch.int32)):
        device_tensor(fn, name, t, dtype, lambda s: s == (n,), f"[{n}]")
    if len({t.device for t in (points, depth, weight, num, den, obs)}) != 1:
        raise ValueError(f"{fn}: every tensor must be on {points.device}")
    if H < 1 or W < 1:
        raise ValueError(f"{fn}: images of at least 1 x 1 pixels, got {H}x{W}")
    if not is_num(trunc) or not trunc > 0:
        raise ValueError(f"{fn}: trunc must be a positive number, got {trunc!r}")
    with torch.cuda.device(points.device):
        _lib.check(_lib.lib().dh_tsdf_integrate(_lib.ptr(points), n, _lib.ptr(depth), _lib.ptr(weight), _lib.ptr(R), _lib.ptr(T), _lib.ptr(K),
                                                F, H, W, float(trunc), _lib.ptr(num), _lib.ptr(den), _lib.ptr(obs), _lib.stream()))


def decode_normals(enc):
    """(normal f32 [...,3], ok bool [...]) of mvs_depth's monocular_normal png u8 [...,3]: n = u8 / 255 * 2 - 1, normalised; a pixel whose
    three channels are 128 has no normal (mvs.encode_normals)."""
    ok = ~(enc == 128).all(dim=-1)
    n = enc.to(torch.float32) / 255.0 * 2.0 - 1.0
    n = n / n.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return torch.where(ok[..., None], n, torch.zeros_like(n)), ok


def weights_from_normals(normal, ok, Kinv, floor_weight=DEPTH_FUSE_DEFAULTS["floor_weight"]):
    """u8 [...,H,W]: max(1, round(255 max(0, -n.e / |e|))) with e = Kinv (x, y, 1) where ok, floor_weight elsewhere; normal f32
    [...,H,W,3] in the camera frame, ok bool [...,H,W].  Plain torch, on the tensors' device.  The caller zeroes the pixels without a
    depth."""
    H, W = ok.shape[-2:]
    dev = normal.device
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    e = torch.stack([xs, ys, torch.ones_like(xs)], -1) @ Kinv.to(dev, torch.float32).reshape(3, 3).T
    e = e / e.norm(dim=-1, keepdim=True)
    cos = (-(normal.to(torch.float32) * e).sum(dim=-1)).clamp(0.0, 1.0)
    w = torch.floor(255.0 * cos + 0.5).clamp(1, 255).to(torch.uint8)
    return torch.where(ok, w, torch.full_like(w, int(floor_weight)))


def map_weights(depth, normal_enc, Kinv, mode="cos", floor_weight=DEPTH_FUSE_DEFAULTS["floor_weight"]):
    """u8 [F,H,W], the weight of every pixel of depth f32 [F,H,W] (inf or NaN: none -> 0): mode "cos": weights_from_normals of the
    decoded normal_enc u8 [F,H,W,3]; "uniform": 255."""
    if mode == "cos":
        w = weights_from_normals(*decode_normals(normal_enc), Kinv, floor_weight)
    elif mode == "uniform":
        w = torch.full(depth.shape, 255, dtype=torch.uint8, device=depth.device)
    else:
        raise ValueError(f"depth_fuse weight must be 'cos' or 'uniform', got {mode!r}")
    return torch.where(torch.isfinite(depth), w, torch.zeros_like(w))


def read_depth_maps(depth_dir, stems, H, W, who="fuse_depth"):
    """(depth f32 [F,H,W] with inf where there is none, present: [F] bool) of a folder of <stem>.npy, on the CPU.  A frame without a
    file is all inf, a value that is not finite becomes inf, a map of another shape raises ValueError and names the file."""
    import numpy as np
    depth = torch.full((len(stems), H, W), float("inf"), dtype=torch.float32)
    present = []
    for f, stem in enumerate(stems):
        p = os.path.join(depth_dir, str(stem) + ".npy")
        present.append(os.path.exists(p))
        if not present[-1]:
            continue
        z = np.load(p)
        if z.shape != (H, W):
            raise ValueError(f"{who}: {p} holds a map of shape {tuple(z.shape)}, the frames are {H} x {W}")
        z = torch.from_numpy(z.astype(np.float32))
        depth[f] = torch.where(torch.isfinite(z), z, torch.full_like(z, float("inf")))
    return depth, present


def read_maps(mvs_dir, stems, H, W):
    """(depth f32 [F,H,W] with inf where there is none, normal u8 [F,H,W,3] with 128 where there is none, present: [F] bool) of
    mvs_depth's depth/<stem>.npy and monocular_normal/<stem>.png, on the CPU.  A frame without a depth file is all inf; one without a
    normal file is all 128; a map of another shape raises ValueError."""
    import numpy as np
    depth, present = read_depth_maps(os.path.join(mvs_dir, "depth"), stems, H, W)
    normal = torch.full((len(stems), H, W, 3), 128, dtype=torch.uint8)
    for f, stem in enumerate(stems):
        if not present[f]:
            continue
        p = os.path.join(mvs_dir, "monocular_normal", str(stem) + ".png")
        if os.path.exists(p):
            from PIL import Image
            enc = np.asarray(Image.open(p).convert("RGB"))
            if enc.shape != (H, W, 3):
                raise ValueError(f"fuse_depth: {p} holds an image of shape {tuple(enc.shape)}, the frames are {H} x {W}")
            normal[f] = torch.from_numpy(enc.copy())
    return depth, normal, present


def _step_maps(depth, weight, K, step_px):
    """The maps on the grid of step_px and its camera diag(1/s, 1/s, 1) K, exactly as mvs.depth_maps feeds check."""
    s = int(step_px)
    if s < 1:
        raise ValueError(f"depth_fuse: step_px must be >= 1, got {step_px!r}")
    if s == 1:
        return depth, weight, K
    Ks = (torch.diag(torch.tensor([1.0 / s, 1.0 / s, 1.0], dtype=torch.float64)) @ K.cpu().double()).float().to(K.device)
    return depth[:, ::s, ::s].contiguous(), weight[:, ::s, ::s].contiguous(), Ks


@torch.no_grad()
def fuse_field(dataset, depth, weight, lo, hi, N: int, step_px=1, trunc=None, frame_chunk=DEPTH_FUSE_DEFAULTS["frame_chunk"],
               point_chunk=DEPTH_FUSE_DEFAULTS["point_chunk"]):
    """(num int64 [N^3], den int32 [N^3], obs int32 [N^3]) in grid order: depth f32 [F,H,W] and weight u8 [F,H,W] of the dataset's F
    frames at its current poses (Dataset.R / T / K), integrated on the grid of visual_hull.grid_points(lo, hi, N).  Frames run in
    chunks in the outer loop, points in bricks (visual_hull.brick_points) in chunks in the inner one.  step_px s > 1: the maps are
    depth[:, ::s, ::s] under diag(1/s, 1/s, 1) K.  trunc in object units (default: DEPTH_FUSE_DEFAULTS' trunc_cells cells)."""
    dev = dataset.R.device
    F = dataset.n_images
    if tuple(depth.shape) != (F, dataset.H, dataset.W) or tuple(weight.shape) != tuple(depth.shape):
        raise ValueError(f"fuse_field: depth and weight must be [{F},{dataset.H},{dataset.W}], got {tuple(depth.shape)} and {tuple(weight.shape)}")
    if trunc is None:
        trunc = DEPTH_FUSE_DEFAULTS["trunc_cells"] * (float(hi[0]) - float(lo[0])) / (N - 1)
    depth, weight, K = _step_maps(depth, weight, dataset.K, step_px)
    pts, grid_order = vh.brick_points(lo, hi, N, dev)
    n = pts.shape[0]
    num = torch.zeros(n, dtype=torch.int64, device=dev)
    den = torch.zeros(n, dtype=torch.int32, device=dev)
    obs = torch.zeros(n, dtype=torch.int32, device=dev)
    R = dataset.R.reshape(-1, 3, 3)
    for f0 in range(0, F, int(frame_chunk)):
        f1 = min(f0 + int(frame_chunk), F)
        d, w = depth[f0:f1].contiguous(), weight[f0:f1].contiguous()
        for p0 in range(0, n, int(point_chunk)):
            p1 = min(p0 + int(point_chunk), n)
            integrate(pts[p0:p1], d, w, R[f0:f1], dataset.T[f0:f1], K, trunc, num[p0:p1], den[p0:p1], obs[p0:p1])
    del pts
    return grid_order(num), grid_order(den), grid_order(obs)


def field_from_state(num, den, h, trunc, prior_weight):
    """field f32, shaped as h: (num + prior_weight q_h) / ((den + prior_weight) 65536) with q_h = clamp(h / trunc, -1, 1) 65536, in
    fp64, rounded to fp32.  In [-1, 1], in units of trunc; inside <= 0."""
    q_h = (h.double() / float(trunc)).clamp(-1.0, 1.0) * Q_ONE
    pw = float(prior_weight)
    f = (num.double().view_as(q_h) + pw * q_h) / ((den.double().view_as(q_h) + pw) * Q_ONE)
    return f.float()


@torch.no_grad()
def fused_field(dataset, depth, weight, /, step_px=1, hull=None, timer=None, **settings):
    """What fused_mesh meshes: {"field" f32 [N,N,N], "h" (the hull's field), "num", "den", "obs" [N^3], "lo", "hi", "cell", "trunc",
    "settings"}.  hull: the settings of the hull pass (visual_hull.VISUAL_HULL_DEFAULTS' keys; its resolution is not used)."""
    import time
    c = fuse_settings(None, **settings)
    hc = vh.hull_settings(hull)
    dev = dataset.label.device
    N = c["resolution"]
    fc = {k: hc[k] for k in ("min_carve_votes", "min_seen", "outside_value", "band_px", "frame_chunk", "point_chunk")}
    fc["signed_maps"] = {} if hc["bound"] == "auto" and 4 * dataset.label.numel() <= vh.SIGNED_MAP_CACHE_BYTES else None

    t0 = time.perf_counter()
    if hc["bound"] == "auto":
        lo, hi, _ = vh.hull_box(dataset, hc["coarse_resolution"], **fc)
    else:
        lo, hi = [-float(hc["bound"])] * 3, [float(hc["bound"])] * 3
    t0 = lap(timer, "box", t0, dev)
    h = vh.grid_field(dataset, lo, hi, N, **fc)[0]
    fc["signed_maps"] = None
    t0 = lap(timer, "hull", t0, dev)
    cell = (hi[0] - lo[0]) / (N - 1)
    trunc = c["trunc_cells"] * cell
    num, den, obs = fuse_field(dataset, depth, weight, lo, hi, N, step_px=step_px, trunc=trunc, frame_chunk=c["frame_chunk"],
                               point_chunk=c["point_chunk"])
    lap(timer, "integrate", t0, dev)
    return {"field": field_from_state(num, den, h, trunc, c["prior_weight"]), "h": h, "num": num, "den": den, "obs": obs,
            "lo": [float(v) for v in lo], "hi": [float(v) for v in hi], "cell": float(cell), "trunc": float(trunc), "settings": c}


@torch.no_grad()
def fused_mesh(dataset, depth, weight, /, step_px=1, hull=None, timer=None, keep=None, **settings):
    """(verts f32 [V,3], faces int64 [M,3], stats) of the depth maps fused on the hull's grid (module docstring); depth f32 [F,H,W]
    (inf or NaN: none), weight u8 [F,H,W] on the dataset's device; settings: any key of DEPTH_FUSE_DEFAULTS; hull: the settings of the
    hull pass.  An empty field raises ValueError.  stats: resolution, bound_min / bound_max, cell, trunc, verts, faces, inside_cells
    (field <= 0), volume (inside cells x cell^3), carved_cells (inside the hull, outside the fused field: the concavities),
    added_cells (the reverse), observed_cells (den > 0), pixels (per frame, the pixels with a depth and a weight on the grid of
    step_px).  timer: a dict that gains seconds per phase; keep: a dict that gains fused_field's output."""
    import time
    from .mesh import marching_cubes
    out = fused_field(dataset, depth, weight, step_px=step_px, hull=hull, timer=timer, **settings)
    field, h, lo, hi, cell = out["field"], out["h"], out["lo"], out["hi"], out["cell"]
    N = field.shape[0]
    inside, hull_in = field <= 0, h <= 0
    n_inside = int(inside.sum())
    if n_inside == 0:
        raise ValueError(f"fuse_depth: the fused field is empty on the {N}^3 grid over {lo} .. {hi} ({vh._pose_note(dataset)})")
    t0 = time.perf_counter()
    verts, faces = marching_cubes(-field, 0.0, lo, hi)
    if timer is not None:
        torch.cuda.synchronize(field.device)
        timer["mesh"] = time.perf_counter() - t0
    d, w, _ = _step_maps(depth, weight, dataset.K, step_px)
    pixels = (torch.isfinite(d) & (d > 1e-3) & (w > 0)).flatten(1).sum(dim=1).tolist()
    stats = {"resolution": N, "bound_min": lo, "bound_max": hi, "cell": cell, "trunc": out["trunc"], "verts": int(verts.shape[0]),
             "faces": int(faces.shape[0]), "inside_cells": n_inside, "volume": n_inside * cell ** 3,
             "carved_cells": int((hull_in & ~inside).sum()), "added_cells": int((~hull_in & inside).sum()),
             "observed_cells": int((out["den"] > 0).sum()), "pixels": [int(p) for p in pixels]}
    if keep is not None:
        keep.update(out)
    return verts, faces, stats


@torch.no_grad()
def frame_residuals(field, lo, hi, trunc, depth, weight, R, T, K, names=None):
    """Every pixel with a depth (finite, > 1e-3) and a weight, back-projected into the object frame, X = R_f^T (z Kinv (x, y, 1) -
    T_f), and looked up in field f32 [N,N,N] over lo .. hi (trilinear: grid_sample, align_corners=True); the residual is |field| trunc
    where the point lies inside the box and |field| < 1.  {"median": [F] (None for a frame without a residual), "count": [F], "worst":
    the N_WORST frames (names, or indices) with the largest medians, largest first, ties in frame order}.  Plain torch; K is the K of
    the depth image."""
    import torch.nn.functional as Fn
    dev = field.device
    F, H, W = depth.shape
    Kinv = torch.inverse(K.detach().cpu().double().reshape(3, 3)).to(dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    e = torch.stack([xs, ys, torch.ones_like(xs)], -1).reshape(-1, 3) @ Kinv.T
    lo_t = torch.tensor([float(v) for v in lo], dtype=torch.float64, device=dev)
    hi_t = torch.tensor([float(v) for v in hi], dtype=torch.float64, device=dev)
    vol = field.to(torch.float32)[None, None]
    R = R.reshape(-1, 3, 3)
    T = T.reshape(-1, 3)
    med, cnt = [], []
    for f in range(F):
        z = depth[f].reshape(-1)
        ok = torch.isfinite(z) & (z > 1e-3) & (weight[f].reshape(-1) > 0)
        X = (z[ok].double()[:, None] * e[ok] - T[f].double()) @ R[f].double()          # rows: R^T c
        g = (X - lo_t) / (hi_t - lo_t) * 2.0 - 1.0
        inbox = (g.abs() <= 1.0).all(dim=1)
        g = g[inbox].float().flip(-1)                                                # grid_sample: x is the last axis of the volume
        if g.shape[0] == 0:
            med.append(None); cnt.append(0)
            continue
        v = Fn.grid_sample(vol, g[None, None, None], mode="bilinear", padding_mode="border", align_corners=True).reshape(-1).abs()
        v = v[v < 1.0]
        cnt.append(int(v.shape[0]))
        med.append(float(v.median()) * float(trunc) if v.shape[0] else None)
    order = sorted(range(F), key=lambda f: (-(med[f] if med[f] is not None else -1.0), f))[:N_WORST]
    return {"median": med, "count": cnt, "worst": [names[f] if names is not None else f for f in order]}
