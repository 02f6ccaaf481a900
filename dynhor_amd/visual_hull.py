"""Visual hull of the object masks at the current poses (Runner.visual_hull, --mode visual_hull): the object's own shape up to its
concavities, from nothing but the label maps (sam_seg/) and the poses (obj_infos/) every sequence has -- a mesh for init_poses'
successors (refine_poses, match_frames --match_guide mesh, init_sdf) when there is no template, and a per-frame check of poses and
masks that needs no template, no network and no ground truth.

  * ``signed_label_distance``: s f32 [F,H,W], the signed distance in pixels to the outline of the solid pixels (label != 0: object
    OR hand -- a hand pixel hides what is behind it and must never carve): on a solid pixel -(sqrt(d2_bg) - 0.5), elsewhere
    sqrt(min(d2_obj, d2_hand)) - 0.5, from three ``pose_sil.label_edt`` maps (dh_label_edt of the values 0, 1, -1 with rmax =
    ceil(band_px) + 1), clamped to [-band_px, band_px].  The 0.5: the mask is made of pixel centres, its outline runs half a pixel
    outside them.  The window of the distance transform is clipped to the image, so the image border is no outline and never carves.
  * ``hull_accumulate`` (dh_hull_accumulate, csrc/visual_hull.hip): per point the m largest g_f over a chunk of frames, g_f = the
    bilinear sample of s_f at the point's projection times z / K00 (pixels turned into object units at the point's depth), over the
    frames that see the point; with them the frame of the largest value and the number of frames that see the point.  The state
    (topk, arg, seen) is carried from call to call and depends on the multiset of frames alone.
  * ``hull_field``: h = topk[:, k - 1] with k = min_carve_votes where at least max(k, ceil(min_seen F)) frames see the point, else
    outside_value; a point is inside the hull iff h <= 0.  k > 1 tolerates k - 1 bad frames (mesh_clean's min_bg_votes, from the
    other side).  Frame chunks outside (the three distance transforms and the signed map are formed once per chunk), point chunks
    inside.
  * ``visual_hull``: a coarse pass over [-1,1]^3 finds the hull's box, the fine grid covers that box (a cube, padded by two coarse
    cells), mesh.marching_cubes(-h, 0) meshes it.  Grid points reach the kernel in 4 x 4 x 4 bricks (``grid_field``), and the fine
    pass reuses the coarse pass's signed maps while they fit in SIGNED_MAP_CACHE_BYTES.  stats: grid, cell, counts, volume, radius_max, touches_bound and sole_carved -- per
    frame the cells that this frame ALONE carves (topk[:,0] > 0, topk[:,1] <= 0, arg = the frame) and their share of the k = 2 hull:
    a frame whose pose or mask is wrong is the only frame that carves some part of the hull.

Limits.  Concavities are never carved.  A pose error the outline does not show (a rotation about the object's centre that leaves
the silhouette nearly unchanged) is not flagged.  A mask truncated by the image border does not carve there.

The kernels run on the current stream; there is no CPU path.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._args import check_cams, device_tensor, lap
from .settings import int_in, is_int, is_num, merge

MAX_RESOLUTION = 512
# resolution: grid points per axis of the fine grid (at most MAX_RESOLUTION: 512^3 points carry 1.6 GB of coordinates and 2.1 GB of
# state at m = 2); bound "auto" (a coarse pass at coarse_resolution over [-1,1]^3 finds the box) or a number b for [-b,b]^3;
# band_px: the clamp of the signed pixel distance (beyond it a value only says "far"); min_carve_votes k: a point is outside when k
# frames say so; min_seen: the share of the frames that must see a point for it to be judged at all; outside_value: h of a point
# that is not judged; frame_chunk / point_chunk: the sizes of the two loops (results do not depend on them)
VISUAL_HULL_DEFAULTS = {"resolution": 128, "bound": "auto", "coarse_resolution": 48, "band_px": 16, "min_carve_votes": 1, "min_seen": 0.5,
                        "outside_value": 1.0, "frame_chunk": 16, "point_chunk": 1 << 22}
N_WORST = 5
# visual_hull keeps the signed maps of its coarse pass for the fine pass when all of them fit in this many bytes (300 frames of
# 1080 x 1920 are 2.5 GB); beyond it they are formed again, chunk by chunk
SIGNED_MAP_CACHE_BYTES = 4 << 30


def check_settings(c: dict):
    """ValueError unless c is a full, sensible dict over VISUAL_HULL_DEFAULTS; the message names the unknown, missing or bad key."""
    merge("visual_hull", VISUAL_HULL_DEFAULTS, None, c, check_overrides=True)
    missing = sorted(set(VISUAL_HULL_DEFAULTS) - set(c))
    if missing:
        raise ValueError(f"visual_hull: missing setting(s) {missing}")
    for k in ("resolution", "coarse_resolution"):
        int_in("visual_hull", k, c[k], 2, MAX_RESOLUTION)
    if c["bound"] != "auto" and not (is_num(c["bound"]) and c["bound"] > 0):
        raise ValueError(f"visual_hull bound must be 'auto' or a positive number, got {c['bound']!r}")
    if not is_num(c["band_px"]) or not 1 <= c["band_px"] <= 2048:
        raise ValueError(f"visual_hull band_px must be a number in [1, 2048], got {c['band_px']!r}")
    int_in("visual_hull", "min_carve_votes", c["min_carve_votes"], 1, 8)
    if not is_num(c["min_seen"]) or not 0 <= c["min_seen"] <= 1:
        raise ValueError(f"visual_hull min_seen must be a number in [0, 1], got {c['min_seen']!r}")
    if not is_num(c["outside_value"]) or not c["outside_value"] > 0:
        raise ValueError(f"visual_hull outside_value must be a positive number, got {c['outside_value']!r}")
    for k in ("frame_chunk", "point_chunk"):
        if not is_int(c[k]) or c[k] < 1:
            raise ValueError(f"visual_hull {k} must be a positive integer, got {c[k]!r}")


def hull_settings(block=None, **overrides) -> dict:
    """VISUAL_HULL_DEFAULTS, then the YAML's optional visual_hull: block, then the overrides that are not None; checked.  The block's
    keys are looked at first, and an override at None is not looked at at all."""
    c = merge("visual_hull", VISUAL_HULL_DEFAULTS, block, check_block=True)
    c = merge("visual_hull", VISUAL_HULL_DEFAULTS, c, {k: v for k, v in overrides.items() if v is not None}, check_overrides=True)
    check_settings(c)
    return c


merge_settings = hull_settings           # the name the config tests and earlier callers know


def signed_label_distance(label: torch.Tensor, band_px) -> torch.Tensor:
    """s f32 [F,H,W] from a label map i8 [F,H,W] (1 object / 0 background / -1 hand): the signed distance in pixels to the outline
    of the solid pixels (module docstring), negative inside, clamped to [-band_px, band_px].  Exact: the squared distances are
    integers and sqrt is correctly rounded."""
    from .pose_sil import label_edt
    fn = "signed_label_distance"
    label = device_tensor(fn, "label", label, torch.int8, lambda s: len(s) == 3, "[F,H,W]")
    if not is_num(band_px) or not band_px > 0:
        raise ValueError(f"{fn}: band_px must be a positive number, got {band_px!r}")
    rmax = int(math.ceil(band_px)) + 1
    s = label_edt(label, 1, rmax)
    s = torch.minimum(s, label_edt(label, -1, rmax)).sqrt_().sub_(0.5)
    inner = label_edt(label, 0, rmax).sqrt_().sub_(0.5).neg_()
    return torch.where(label != 0, inner, s).clamp_(-float(band_px), float(band_px))


def hull_accumulate(points, sd, R, T, K, frame0: int, topk, arg, seen):
    """One chunk of frames folded into the state, in place (dh_hull_accumulate): points f32 [n,3], sd f32 [F,H,W]
    (signed_label_distance of the chunk), R [F,3,3], T [F,3], K [3,3], frame0 = the global index of the chunk's first frame; topk f32
    [n,m] (m in 1..8, started at -inf), arg int32 [n] (started at -1), seen int32 [n] (started at 0)."""
    fn = "hull_accumulate"
    points = device_tensor(fn, "points", points, torch.float32, lambda s: len(s) == 2 and s[1] == 3, "[n,3]")
    n = points.shape[0]
    sd = device_tensor(fn, "sd", sd, torch.float32, lambda s: len(s) == 3, "[F,H,W]")
    F, H, W = sd.shape
    R, T, K = check_cams(fn, F, R, T, K, points.device)
    for name, t, dtype, ok, txt in (("topk", topk, torch.float32, lambda s: len(s) == 2 and s[0] == n and 1 <= s[1] <= 8, f"[{n},1..8]"),
                                    ("arg", arg, torch.int32, lambda s: s == (n,), f"[{n}]"),
                                    ("seen", seen, torch.int32, lambda s: s == (n,), f"[{n}]")):
        if device_tensor(fn, name, t, dtype, ok, txt) is not t:
            raise ValueError(f"{fn}: {name} is updated in place and must be contiguous")
    if len({t.device for t in (points, sd, topk, arg, seen)}) != 1:
        raise ValueError(f"{fn}: every tensor must be on {points.device}")
    if H < 2 or W < 2:
        raise ValueError(f"{fn}: images of at least 2 x 2 pixels, got {H}x{W}")
    if int(frame0) < 0:
        raise ValueError(f"{fn}: frame0 must be >= 0, got {frame0}")
    with torch.cuda.device(points.device):
        _lib.check(_lib.lib().dh_hull_accumulate(_lib.ptr(points), n, _lib.ptr(sd), _lib.ptr(R), _lib.ptr(T), _lib.ptr(K), F, H, W,
                                                 int(frame0), topk.shape[1], _lib.ptr(topk), _lib.ptr(arg), _lib.ptr(seen),
                                                 _lib.stream()))


def _frame_runs(frames, n_images, chunk):
    """The frame indices (None: all), sorted, cut into runs of consecutive indices of at most `chunk` frames: [(first, count)]."""
    idx = list(range(n_images)) if frames is None else sorted(int(f) for f in frames)
    if any(f < 0 or f >= n_images for f in idx) or len(set(idx)) != len(idx):
        raise ValueError(f"hull_field: frames must be distinct indices in [0, {n_images}), got {list(frames)}")
    runs = []
    for f in idx:
        if runs and runs[-1][0] + runs[-1][1] == f and runs[-1][1] < chunk:
            runs[-1][1] += 1
        else:
            runs.append([f, 1])
    return [(a, b) for a, b in runs], len(idx)


def field_from_state(topk, seen, n_frames: int, min_carve_votes: int, min_seen: float, outside_value: float):
    """h f32 [n]: topk[:, k - 1] where seen >= max(k, ceil(min_seen n_frames)), else outside_value (k = min_carve_votes)."""
    k = int(min_carve_votes)
    need = max(k, int(math.ceil(float(min_seen) * n_frames)))
    return torch.where(seen >= need, topk[:, k - 1], torch.full_like(topk[:, 0], float(outside_value)))


@torch.no_grad()
def hull_field(points, dataset, frames=None, min_carve_votes=None, min_seen=None, outside_value=None, band_px=None, frame_chunk=None,
               point_chunk=None, timer=None, signed_maps=None):
    """(h f32 [n], topk f32 [n,m], arg int32 [n], seen int32 [n]) of points f32 [n,3] against the dataset's labels and current poses
    (Dataset.label / R / T / K), over `frames` (indices; None: all); m = max(min_carve_votes, 2).  Settings left at None take
    VISUAL_HULL_DEFAULTS.  timer: a dict that gains the seconds of "signed_distance" and "accumulate" (it synchronises; None: no
    waiting).  signed_maps: a dict of the caller's in which the signed map of every frame chunk is kept and looked up again, keyed by
    (first frame, count, band_px): a second call over the same frames then forms none (None: nothing is kept)."""
    c = hull_settings(None, min_carve_votes=min_carve_votes, min_seen=min_seen, outside_value=outside_value, band_px=band_px,
                       frame_chunk=frame_chunk, point_chunk=point_chunk)
    points = device_tensor("hull_field", "points", points, torch.float32, lambda s: len(s) == 2 and s[1] == 3, "[n,3]")
    dev, n = points.device, points.shape[0]
    m = max(c["min_carve_votes"], 2)
    topk = torch.full((n, m), float("-inf"), dtype=torch.float32, device=dev)
    arg = torch.full((n,), -1, dtype=torch.int32, device=dev)
    seen = torch.zeros(n, dtype=torch.int32, device=dev)
    runs, n_frames = _frame_runs(frames, dataset.n_images, c["frame_chunk"])
    R = dataset.R.reshape(-1, 3, 3)

    for f0, nf in runs:
        t0 = lap(timer, None, None, dev)
        key = (f0, nf, float(c["band_px"]))
        sd = signed_maps.get(key) if signed_maps is not None else None
        if sd is None:
            sd = signed_label_distance(dataset.label[f0:f0 + nf], c["band_px"])
            if signed_maps is not None:
                signed_maps[key] = sd
        t0 = lap(timer, "signed_distance", t0, dev)
        for p0 in range(0, n, c["point_chunk"]):
            p1 = min(p0 + c["point_chunk"], n)
            hull_accumulate(points[p0:p1], sd, R[f0:f0 + nf], dataset.T[f0:f0 + nf], dataset.K, f0, topk[p0:p1], arg[p0:p1], seen[p0:p1])
        lap(timer, "accumulate", t0, dev)
        del sd
    h = field_from_state(topk, seen, n_frames, c["min_carve_votes"], c["min_seen"], c["outside_value"])
    return h, topk, arg, seen


def grid_points(lo, hi, N: int, device):
    """(points f32 [N^3,3], axes 3 x f32 [N]): the grid of mesh.marching_cubes' field u[i,j,k] at (x_i, y_j, z_k), x-major, the axes
    by torch.linspace as Runner._scene_gt_mesh builds them."""
    ax = [torch.linspace(float(lo[a]), float(hi[a]), N, device=device) for a in range(3)]
    pts = torch.stack(torch.meshgrid(ax[0], ax[1], ax[2], indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
    return pts, ax


BRICK = 4


def brick_points(lo, hi, N: int, device):
    """(points f32 [Np^3,3], grid_order): the points of grid_points(lo, hi, N) in bricks of BRICK^3 -- 64 consecutive points are one
    4 x 4 x 4 brick --, and the function that puts a per-point result [Np^3, ...] back into grid order [N^3, ...].  A grid whose N is no
    multiple of BRICK is padded to Np by repeating its last plane; grid_order cuts the padding off again."""
    ax = [torch.linspace(float(lo[a]), float(hi[a]), N, device=device) for a in range(3)]
    nb = (N + BRICK - 1) // BRICK
    Np = nb * BRICK
    if Np != N:
        ax = [torch.cat([x, x[-1:].expand(Np - N)]) for x in ax]
    pts = torch.stack(torch.meshgrid(ax[0], ax[1], ax[2], indexing="ij"), dim=-1)
    pts = pts.view(nb, BRICK, nb, BRICK, nb, BRICK, 3).permute(0, 2, 4, 1, 3, 5, 6).reshape(-1, 3).contiguous()

    def grid_order(t):
        tail = tuple(t.shape[1:])
        t = t.view(nb, nb, nb, BRICK, BRICK, BRICK, *tail).permute(0, 3, 1, 4, 2, 5, *range(6, 6 + len(tail)))
        return t.reshape(Np, Np, Np, *tail)[:N, :N, :N].reshape(N * N * N, *tail).contiguous()

    return pts, grid_order


def grid_field(dataset, lo, hi, N: int, timer=None, **field_settings):
    """hull_field on the N^3 grid of grid_points(lo, hi, N), returned in grid order: (h [N,N,N], topk [N^3,m], arg [N^3], seen [N^3]).
    The points go to the kernel in bricks of BRICK^3 (``brick_points``: a wave's 64 lanes hold one 4 x 4 x 4 brick, whose projections
    cover a compact patch of pixels; in plain grid order a wave holds a line of 64 points along z): 3.5x faster at 128^3 and 7.6x at
    256^3 on an MI355X (scripts/bench_visual_hull.py).  Every point's result is its own, so the order changes no value."""
    pts, grid_order = brick_points(lo, hi, N, dataset.label.device)
    out = hull_field(pts, dataset, timer=timer, **field_settings)
    del pts
    h, topk, arg, seen = (grid_order(t) for t in out)
    return h.view(N, N, N), topk, arg, seen


def _touches(inside):
    """Whether an inside cell lies on the outer layer of the grid."""
    return bool(inside[0].any() | inside[-1].any() | inside[:, 0].any() | inside[:, -1].any() | inside[:, :, 0].any()
                | inside[:, :, -1].any())


def hull_box(dataset, Nc: int, **field_settings):
    """(lo, hi, touches): the cube the fine grid covers, from a coarse pass at Nc^3 over [-1,1]^3: the coarse hull's box padded by two
    coarse cells, made a cube, moved and cut to lie inside [-1,1]^3; touches: an inside cell on the outer layer of the coarse grid.
    An empty coarse hull raises ValueError."""
    inside = grid_field(dataset, [-1.0] * 3, [1.0] * 3, Nc, **field_settings)[0] <= 0
    if not bool(inside.any()):
        raise ValueError("visual_hull: the coarse hull over [-1,1]^3 is empty: no grid point lies inside the masks of enough frames "
                         f"at these poses ({_pose_note(dataset)}); check the poses, their scale and min_seen / min_carve_votes")
    touches = _touches(inside)
    hc = 2.0 / (Nc - 1)
    idx = inside.nonzero()
    lo = -1.0 + (idx.min(dim=0).values.double() - 2) * hc
    hi = -1.0 + (idx.max(dim=0).values.double() + 2) * hc
    side = min(float((hi - lo).max()), 2.0)
    centre = ((lo + hi) * 0.5).clamp(-1.0 + side / 2, 1.0 - side / 2)
    return (centre - side / 2).tolist(), (centre + side / 2).tolist(), touches


def sole_carved(topk, arg, seen, n_frames: int, min_seen: float, names=None) -> dict:
    """Per frame, the points this frame alone carves out of the k = 2 hull: topk[:,0] > 0, topk[:,1] <= 0, arg = the frame, over the
    points that enough frames see (hull_field's rule at k = 2).  {"hull2_cells", "cells": [F], "share": [F] (cells / hull2_cells, 0
    when that is 0), "share_max", "worst": the N_WORST names (or indices) of the largest shares, largest first, ties in frame order}."""
    need = max(2, int(math.ceil(float(min_seen) * n_frames)))
    judged = seen >= need
    hull2 = int((judged & (topk[:, 1] <= 0)).sum())
    sole = judged & (topk[:, 0] > 0) & (topk[:, 1] <= 0) & (arg >= 0)
    F = max(n_frames, int(arg.max()) + 1 if arg.numel() else 0)
    cells = torch.bincount(arg[sole].long(), minlength=F).tolist()
    share = [c / hull2 if hull2 else 0.0 for c in cells]
    order = sorted(range(F), key=lambda f: (-share[f], f))[:N_WORST]
    return {"hull2_cells": hull2, "cells": cells, "share": share, "share_max": max(share) if share else 0.0,
            "worst": [names[f] if names is not None else f for f in order]}


def _pose_note(dataset):
    T = dataset.T
    return (f"{dataset.n_images} frames of {dataset.H} x {dataset.W}; camera distances |T| in [{float(T.norm(dim=1).min()):.4g}, "
            f"{float(T.norm(dim=1).max()):.4g}]; {int((dataset.label != 0).flatten(1).any(dim=1).sum())} frames have a mask")


@torch.no_grad()
def visual_hull(dataset, timer=None, **settings):
    """(verts f32 [V,3], faces int64 [M,3], stats) of the visual hull of the dataset's masks at its current poses; settings: any key
    of VISUAL_HULL_DEFAULTS.  bound "auto": a coarse pass at coarse_resolution over [-1,1]^3, then the fine grid over the cube around
    the coarse hull's box padded by two coarse cells, moved and cut to lie inside [-1,1]^3; a number b: the fine grid over [-b,b]^3.
    An empty hull raises ValueError.  stats: resolution, bound_min / bound_max, cell, verts, faces, inside_cells, volume (inside cells
    x cell^3), radius_max (the largest vertex norm), touches_bound (an inside cell on the outer layer of the bounding box -- the
    [-1,1]^3 grid of the coarse pass, or [-b,b]^3 --: the hull is cut off, the poses or the scale are off) and sole_carved
    (``sole_carved`` with the frames' names).  timer: a dict that gains seconds per phase."""
    import time
    from .mesh import marching_cubes
    from .schedules import frame_names
    c = hull_settings(None, **settings)
    dev = dataset.label.device
    fc = {k: c[k] for k in ("min_carve_votes", "min_seen", "outside_value", "band_px", "frame_chunk", "point_chunk")}
    F, N = dataset.n_images, c["resolution"]
    touches = False
    keep = c["bound"] == "auto" and 4 * dataset.label.numel() <= SIGNED_MAP_CACHE_BYTES
    fc["signed_maps"] = {} if keep else None
    t_start = time.perf_counter()
    if c["bound"] == "auto":
        lo, hi, touches = hull_box(dataset, c["coarse_resolution"], **fc)
        if timer is not None:
            torch.cuda.synchronize(dev)
            timer["coarse"] = time.perf_counter() - t_start
    else:
        lo, hi = [-float(c["bound"])] * 3, [float(c["bound"])] * 3
    t_fine = time.perf_counter()
    cell = (hi[0] - lo[0]) / (N - 1)
    sub = {} if timer is not None else None
    h, topk, arg, seen = grid_field(dataset, lo, hi, N, timer=sub, **fc)
    inside = h <= 0
    n_inside = int(inside.sum())
    if n_inside == 0:
        raise ValueError(f"visual_hull: the hull is empty on the {N}^3 grid over {lo} .. {hi} ({_pose_note(dataset)})")
    if c["bound"] != "auto":
        touches = _touches(inside)
    sc = sole_carved(topk, arg, seen, F, c["min_seen"], frame_names(F, dataset.stems))
    del topk, arg, seen
    fc["signed_maps"] = None
    if timer is not None:
        torch.cuda.synchronize(dev)
        timer["fine"] = time.perf_counter() - t_fine
        timer.update({"fine_" + k: v for k, v in sub.items()})
    t_mesh = time.perf_counter()
    verts, faces = marching_cubes(-h, 0.0, lo, hi)
    if timer is not None:
        torch.cuda.synchronize(dev)
        timer["mesh"] = time.perf_counter() - t_mesh
    stats = {"resolution": N, "bound_min": [float(v) for v in lo], "bound_max": [float(v) for v in hi], "cell": float(cell),
             "verts": int(verts.shape[0]), "faces": int(faces.shape[0]), "inside_cells": n_inside, "volume": n_inside * float(cell) ** 3,
             "radius_max": float(verts.norm(dim=1).max()) if verts.shape[0] else 0.0, "touches_bound": touches, "sole_carved": sc}
    return verts, faces, stats
