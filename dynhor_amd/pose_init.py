"""Per-frame object poses from nothing but the masks and a template mesh: the first step of the reference's stage 1
(ObjTracker/run.py:130-151, pose_initializtion.py:188-379: a bank of a few thousand random views of the template, retrieval per frame,
depth from the mask's box, a short local fit per candidate, one candidate per frame), on this project's own rasteriser and silhouette
optimiser.  The reference retrieves with DINOv2 features of the cropped image; here the cropped SILHOUETTE is compared bit by bit, so
retrieval is a recall step only (a silhouette hardly tells a pose from its flip) and the choice among the candidates is made by
fitting every one of them at full resolution.  The result goes into Dataset.R / Dataset.T, from where ``pose_sil.refine_poses`` and
training go on.

The retrieval kernels (csrc/pose_init.hip, include/dynhor_hip.h), integer work without float atomics, bitwise reproducible:
  * ``label_boxes``: the tight box (xmin, ymin, xmax, ymax) of label == 1 per image, (W, H, -1, -1) for an image without one.
  * ``crop_squares`` (host, fp64): the square the silhouette is resampled on -- the centre of the tight box, edge b = 1.3 max(box
    width, box height) (the reference's BBOX_EXPANSION_FACTOR, utils/constants.py:4), x0 = cx - b/2, y0 = cy - b/2, step = b / S,
    rounded once to fp32; (0, 0, 0) marks an empty box.  The reference also pads the box by 5 px (run.py:37-40); that is left out:
    5 px are not the same fraction of a 64^2 bank view and of a 1080p frame.
  * ``sil_crop_pack``: S x S samples per image, sample (r, c) at the pixel nearest to (x0 + (c + 0.5) step, y0 + (r + 0.5) step), packed
    one bit per sample into an obj plane (label == 1) and a keep plane (label >= 0: not hand), 0 outside the image.
  * ``sil_bank_score``: (intersection, union) = (popc(fo & bo & fk), popc((fo | bo) & fk)) of every frame against every bank view.

The pipeline (``init_poses``):
  1. every frame packed and scored against the bank; IoU = inter / union in fp64 (0 where the union is 0);
  2. the top `candidates` views per frame by a stable descending sort (a tie goes to the lower view index);
  3. a translation per candidate by the reference's box-driven fixed point (utils/camera.py:132-176, ``depth_from_boxes``);
  4. every hypothesis (frame x candidate) fitted by ``pose_sil.SilhouettePoseOptimizer`` without the smoothness term, `hyp_iters`
     Adam steps with the halo annealed from `hyp_sigma_px` to `hyp_sigma_end_px`, at most `hyp_chunk` hypotheses resident; scored by
     the hard IoU tp / (tp + fp + fn) of its final counts;
  5. one candidate per frame by a Viterbi pass: node cost 1 - IoU_fit, edge cost lw_track angle(R_a, R_b) / 180 degrees (lw_track 0.5 is
     a first guess, not tuned); a frame with an empty box takes the pose of the nearest frame that has candidates;
  6. optionally the joint ``pose_sil.refine_poses``.

Limits.  A hand that hides part of the object shrinks the box and shifts the crop (the reference has the same weakness).  A template
with a mirror or rotational symmetry stays ambiguous.  The bank's rotation is taken as the frame's rotation although the object is
off the optical axis (the reference does the same); the local fit absorbs it.  A photometric term from the template's texture
(dh_mesh_shade_tex) would separate flips the silhouette cannot and is the obvious next step.

The kernels run on the current stream; retrieval and fitting have no CPU path.  The rotations, the square rule, the depth iteration
and the Viterbi pass are plain torch and run wherever their inputs live.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._args import check_faces, check_verts, device_tensor
from .mesh_align import rotation_angle_deg
from .mesh_color import raster_depth
from .pose_sil import DEFAULTS as POSE_SIL_DEFAULTS
from .settings import merge

BOX_EXPANSION = 1.3
# defaults of the YAML's pose_init: block (runner.POSE_INIT_DEFAULTS); DESIGN_NEXT_ROWS.md section 16 says where each comes from
DEFAULTS = {"n_views": 6000, "seed": 0, "render_size": 192, "crop_size": 48, "distance_scale": 3.5, "view_chunk": 256,
            "candidates": 32, "hyp_iters": 40, "hyp_sigma_px": 8.0, "hyp_sigma_end_px": 2.0, "hyp_lr": POSE_SIL_DEFAULTS["lr"],
            "hyp_chunk": 256, "lw_track": 0.5, "final_refine": True}


# ------------------------------------------------------------------------------------------------ plain torch pieces (CPU or device)
def arvo_rotations(n: int, seed: int = 0) -> torch.Tensor:
    """float64 [n,3,3] on the CPU: rotations uniform over SO(3) by Arvo's method ("Fast random rotation matrices", 1992; the
    reference's utils/render.py:56-93) from x = torch.rand(3, n, float64) of a CPU generator seeded with `seed`: a rotation about z by
    2 pi x_0 followed by the point reflection of a Householder mirror, M = (2 v v^T - I) Rz, v = (cos(2 pi x_1) sqrt(x_2),
    sin(2 pi x_1) sqrt(x_2), sqrt(1 - x_2))."""
    g = torch.Generator().manual_seed(int(seed))
    x = torch.rand(3, int(n), dtype=torch.float64, generator=g)
    a, b = 2.0 * math.pi * x[0], 2.0 * math.pi * x[1]
    zero, one = torch.zeros_like(a), torch.ones_like(a)
    Rz = torch.stack([torch.stack([a.cos(), a.sin(), zero], -1), torch.stack([-a.sin(), a.cos(), zero], -1),
                      torch.stack([zero, zero, one], -1)], 1)
    v = torch.stack([b.cos() * x[2].sqrt(), b.sin() * x[2].sqrt(), (1.0 - x[2]).sqrt()], -1)
    M = 2.0 * v[:, :, None] * v[:, None, :] - torch.eye(3, dtype=torch.float64)
    return M @ Rz


def crop_squares(boxes: torch.Tensor, S: int, expansion: float = BOX_EXPANSION) -> torch.Tensor:
    """sq float32 [n,3] = (x0, y0, step) of the module docstring from boxes int [n,4] (label_boxes), computed in fp64 and rounded once;
    (0, 0, 0) for an empty box (xmax < xmin)."""
    b = boxes.to(torch.float64)
    cx, cy = (b[:, 0] + b[:, 2]) * 0.5, (b[:, 1] + b[:, 3]) * 0.5
    edge = float(expansion) * torch.maximum(b[:, 2] - b[:, 0] + 1.0, b[:, 3] - b[:, 1] + 1.0)
    sq = torch.stack([cx - edge * 0.5, cy - edge * 0.5, edge / int(S)], -1)
    sq = torch.where((b[:, 2] >= b[:, 0])[:, None], sq, torch.zeros_like(sq))
    return sq.to(torch.float32).contiguous()


def depth_from_boxes(verts: torch.Tensor, R: torch.Tensor, boxes: torch.Tensor, K: torch.Tensor, iters: int = 10,
                     max_elems: int = 1 << 24) -> torch.Tensor:
    """T float64 [N,3]: for every rotation R [N,3,3] the translation that makes the box of the projected vertices match the 2-D box
    boxes [N,4] = (x0, y0, x1, y1) (continuous: a mask's tight box is [xmin - 0.5, xmax + 0.5]), by the reference's fixed point
    (utils/camera.py:132-176): start at depth 1 on the ray through the box centre; `iters` times project, scale the depth by the ratio
    of the projected box's diagonal to the target's, and shift x, y by the offset of the box centres back-projected at the new
    depth.  K: fx, fy, cx, cy are read (no skew).  fp64; rows go in chunks of at most max_elems / (3 V)."""
    v = verts.to(torch.float64)
    R, boxes, K = R.to(torch.float64), boxes.to(torch.float64), K.to(torch.float64)
    fxy, cxy = torch.stack([K[0, 0], K[1, 1]]), torch.stack([K[0, 2], K[1, 2]])
    out = torch.empty(R.shape[0], 3, dtype=torch.float64, device=R.device)
    rows = max(1, int(max_elems) // max(1, 3 * v.shape[0]))
    for s in range(0, R.shape[0], rows):
        pts = torch.einsum("nij,vj->nvi", R[s:s + rows], v)
        bb = boxes[s:s + rows]
        diag_bb = (bb[:, 2:] - bb[:, :2]).norm(dim=-1)
        centre_bb = (bb[:, :2] + bb[:, 2:]) * 0.5
        z = torch.ones(pts.shape[0], dtype=torch.float64, device=R.device)
        xy = (centre_bb - cxy) * z[:, None] / fxy
        for _ in range(int(iters)):
            cam_z = pts[:, :, 2] + z[:, None]
            uv = (pts[:, :, :2] + xy[:, None, :]) / cam_z[:, :, None] * fxy + cxy
            lo, hi = uv.amin(dim=1), uv.amax(dim=1)
            z = z * ((hi - lo).norm(dim=-1) / diag_bb)
            xy = xy + (centre_bb - (lo + hi) * 0.5) * z[:, None] / fxy
        out[s:s + rows] = torch.cat([xy, z[:, None]], -1)
    return out


def viterbi(node_cost: torch.Tensor, edge_cost) -> list:
    """The path k_0 .. k_{n-1} that minimises sum_f node_cost[f, k_f] + sum_f edge_cost(f)[k_f, k_{f+1}] (node_cost [n,K] fp64 on the
    CPU, edge_cost(f) -> [K,K] between frames f and f + 1); the first minimum on a tie."""
    n, Kc = node_cost.shape
    best = node_cost[0].clone()
    back = []
    for f in range(1, n):
        tot = best[:, None] + edge_cost(f - 1)
        m, arg = tot.min(dim=0)
        back.append(arg)
        best = m + node_cost[f]
    k = int(best.argmin())
    path = [k]
    for arg in reversed(back):
        k = int(arg[k])
        path.append(k)
    return path[::-1]


# ------------------------------------------------------------------------------------------------ kernels
def label_boxes(label) -> torch.Tensor:
    """boxes int32 [n,4] = (xmin, ymin, xmax, ymax) over label == 1 of label i8 [n,H,W]; (W, H, -1, -1) without an object pixel."""
    label = device_tensor("label_boxes", "label", label, torch.int8, lambda s: len(s) == 3 and s[1] > 0 and s[2] > 0, "[n,H,W]")
    n, H, W = label.shape
    boxes = torch.empty(n, 4, dtype=torch.int32, device=label.device)
    if n:
        with torch.cuda.device(label.device):
            _lib.check(_lib.lib().dh_label_boxes(_lib.ptr(label), n, H, W, _lib.ptr(boxes), _lib.stream()))
    return boxes


def sil_crop_pack(label, sq, S: int):
    """(obj, keep) int64 [n, S^2 / 64] (the bits of the kernel's uint64 words): label i8 [n,H,W] resampled on the squares sq f32 [n,3]
    (crop_squares) and packed, sample r S + c at bit (s & 63) of word (s >> 6)."""
    fn = "sil_crop_pack"
    label = device_tensor(fn, "label", label, torch.int8, lambda s: len(s) == 3 and s[1] > 0 and s[2] > 0, "[n,H,W]")
    n, H, W = label.shape
    sq = device_tensor(fn, "sq", sq, torch.float32, lambda s: s == (n, 3), f"[{n},3]")
    S = int(S)
    if S < 8 or S > 128 or S % 8:
        raise ValueError(f"{fn}: S must be a multiple of 8 in [8, 128], got {S}")
    if sq.device != label.device:
        raise ValueError(f"{fn}: every tensor must be on {label.device}")
    obj = torch.empty(n, S * S // 64, dtype=torch.int64, device=label.device)
    keep = torch.empty_like(obj)
    if n:
        with torch.cuda.device(label.device):
            _lib.check(_lib.lib().dh_sil_crop_pack(_lib.ptr(label), n, H, W, _lib.ptr(sq), S, _lib.ptr(obj), _lib.ptr(keep), _lib.stream()))
    return obj, keep


def sil_bank_score(frame_obj, frame_keep, bank_obj, view_chunk: int = 0) -> torch.Tensor:
    """int32 [F,V,2] = (intersection, union) of every frame (obj / keep planes int64 [F,Wd]) against every bank view (int64 [V,Wd]),
    the views in launches of `view_chunk` (0: one launch); the same tensor for every chunking."""
    fn = "sil_bank_score"
    frame_obj = device_tensor(fn, "frame_obj", frame_obj, torch.int64, lambda s: len(s) == 2 and s[1] > 0, "[F,Wd]")
    F, Wd = frame_obj.shape
    frame_keep = device_tensor(fn, "frame_keep", frame_keep, torch.int64, lambda s: s == (F, Wd), f"[{F},{Wd}]")
    bank_obj = device_tensor(fn, "bank_obj", bank_obj, torch.int64, lambda s: len(s) == 2 and s[1] == Wd, f"[V,{Wd}]")
    if frame_keep.device != frame_obj.device or bank_obj.device != frame_obj.device:
        raise ValueError(f"{fn}: every tensor must be on {frame_obj.device}")
    V = bank_obj.shape[0]
    step = V if int(view_chunk) <= 0 else int(view_chunk)
    parts = []
    L = _lib.lib()
    with torch.cuda.device(frame_obj.device):
        for v0 in range(0, V, max(step, 1)):
            b = bank_obj[v0:v0 + step]
            out = torch.empty(F, b.shape[0], 2, dtype=torch.int32, device=frame_obj.device)
            if F:
                _lib.check(L.dh_sil_bank_score(_lib.ptr(frame_obj), _lib.ptr(frame_keep), F, _lib.ptr(b), b.shape[0], Wd, _lib.ptr(out),
                                               _lib.stream()))
            parts.append(out)
    if not parts:
        return torch.empty(F, 0, 2, dtype=torch.int32, device=frame_obj.device)
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


def iou_from_counts(counts: torch.Tensor) -> torch.Tensor:
    """float64 inter / union of sil_bank_score's counts [...,2], 0 where the union is 0."""
    c = counts.to(torch.float64)
    return torch.where(c[..., 1] > 0, c[..., 0] / c[..., 1].clamp(min=1.0), torch.zeros_like(c[..., 0]))


def pack_labels(label, S: int):
    """(obj, keep, boxes int32 [n,4] on the host, sq f32 [n,3] on the device) of label i8 [n,H,W]: boxes, squares, crop and pack."""
    boxes = label_boxes(label)
    sq = crop_squares(boxes.cpu(), S).to(label.device)
    obj, keep = sil_crop_pack(label, sq, S)
    return obj, keep, boxes.cpu(), sq


# ------------------------------------------------------------------------------------------------ the bank
def bank_camera(verts, render_size: int, distance_scale: float):
    """(K f32 [3,3], T f32 [3]) of the bank's views: the template at distance_scale x its largest vertex norm on the optical axis
    (run.py:132-133), focal 1.2 render_size (run.py:121), the principal point at the image centre (render_size - 1) / 2."""
    rs = int(render_size)
    c = (rs - 1) / 2.0
    K = torch.tensor([[1.2 * rs, 0.0, c], [0.0, 1.2 * rs, c], [0.0, 0.0, 1.0]], dtype=torch.float32, device=verts.device)
    radius = float(verts.to(torch.float64).norm(dim=1).max())
    T = torch.tensor([0.0, 0.0, float(distance_scale) * radius], dtype=torch.float32, device=verts.device)
    return K, T


def build_view_bank(verts, faces, n_views=DEFAULTS["n_views"], seed=DEFAULTS["seed"], render_size=DEFAULTS["render_size"],
                    crop_size=DEFAULTS["crop_size"], distance_scale=DEFAULTS["distance_scale"], view_chunk=DEFAULTS["view_chunk"],
                    rotations=None) -> dict:
    """The bank of a template mesh: {"R" float64 [V,3,3] on the CPU (object -> camera; arvo_rotations(n_views, seed) unless
    `rotations` is given), "obj" int64 [V, crop_size^2 / 64] the packed silhouettes, "boxes" int32 [V,4] on the CPU, "K", "T" the
    bank camera, "settings"}.  The views are rendered by mesh_color.raster_depth in chunks of view_chunk at render_size^2; (zbuf != -1)
    is the label the box, crop and pack kernels take."""
    fn = "build_view_bank"
    verts = check_verts(fn, verts)
    faces = check_faces(fn, faces)
    n_views, rs, S, view_chunk = int(n_views), int(render_size), int(crop_size), int(view_chunk)
    if n_views < 1 or rs < 8 or view_chunk < 1 or not float(distance_scale) > 1.0:
        raise ValueError(f"{fn}: n_views >= 1, render_size >= 8, view_chunk >= 1, distance_scale > 1; got {n_views}, {render_size}, "
                         f"{view_chunk}, {distance_scale}")
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        raise ValueError(f"{fn}: the template has no vertices or no faces")
    R64 = arvo_rotations(n_views, seed) if rotations is None else rotations.detach().cpu().to(torch.float64).reshape(-1, 3, 3)
    n_views = R64.shape[0]
    K, T = bank_camera(verts, rs, distance_scale)
    R32 = R64.to(verts.device, torch.float32)
    words, boxes = [], []
    for v0 in range(0, n_views, view_chunk):
        Rc = R32[v0:v0 + view_chunk].contiguous()
        zbuf = raster_depth(verts, faces, Rc, T[None].expand(Rc.shape[0], 3).contiguous(), K, rs, rs)
        label = (zbuf != -1).to(torch.int8)
        del zbuf
        obj, _, bx, _ = pack_labels(label, S)
        words.append(obj)
        boxes.append(bx)
    boxes = torch.cat(boxes)
    empty = int((boxes[:, 2] < 0).sum())
    if empty:
        raise ValueError(f"{fn}: {empty} of {n_views} views show nothing of the template (a vertex behind the camera, or no face "
                         "covering a pixel centre at this render_size)")
    return {"R": R64, "obj": torch.cat(words), "boxes": boxes, "K": K, "T": T,
            "settings": {"n_views": n_views, "seed": int(seed), "render_size": rs, "crop_size": S,
                         "distance_scale": float(distance_scale)}}


def retrieve(label, bank: dict, candidates: int = DEFAULTS["candidates"], view_chunk: int = 0) -> dict:
    """Steps 1 and 2: {"index" int64 [F,K] the top K = min(candidates, V) views per frame, best first, "iou" float64 [F,K], "iou_all"
    float64 [F,V], "boxes" int32 [F,4]} on the CPU.  A frame with an empty box scores 0 everywhere."""
    S = int(bank["settings"]["crop_size"])
    obj, keep, boxes, _ = pack_labels(label, S)
    iou = iou_from_counts(sil_bank_score(obj, keep, bank["obj"], view_chunk).cpu())
    val, idx = torch.sort(iou, dim=1, descending=True, stable=True)
    k = min(int(candidates), iou.shape[1])
    return {"index": idx[:, :k].contiguous(), "iou": val[:, :k].contiguous(), "iou_all": iou, "boxes": boxes}


# ------------------------------------------------------------------------------------------------ the pipeline
def fit_hypotheses(verts, faces, label, R0, T0, K, iters=DEFAULTS["hyp_iters"], sigma_px=DEFAULTS["hyp_sigma_px"],
                   sigma_end_px=DEFAULTS["hyp_sigma_end_px"], lr=DEFAULTS["hyp_lr"], hyp_chunk=DEFAULTS["hyp_chunk"]):
    """Step 4: R0 [F,Kc,3,3], T0 [F,Kc,3] float32 on the device -> (R [F,Kc,3,3], T [F,Kc,3] float32, iou float64 [F,Kc] on the
    CPU).  The frames go in groups of max(1, hyp_chunk // Kc) with their label replicated Kc times; every hypothesis is its own
    "frame" of a SilhouettePoseOptimizer without the smoothness term, so the hypotheses do not see each other."""
    from .pose_sil import SilhouettePoseOptimizer, sigma_at
    F, Kc = R0.shape[0], R0.shape[1]
    per = max(1, int(hyp_chunk) // Kc)
    Rs, Ts, ious = [], [], []
    for f0 in range(0, F, per):
        f1 = min(F, f0 + per)
        lab = label[f0:f1].repeat_interleave(Kc, dim=0).contiguous()
        opt = SilhouettePoseOptimizer(verts, faces, lab, R0[f0:f1].reshape(-1, 3, 3).contiguous(), T0[f0:f1].reshape(-1, 3).contiguous(),
                                      K, lr=lr, sigma_px=sigma_px, lw_smooth=0.0, frame_chunk=64)
        for k in range(int(iters)):
            opt.step(sigma_at(k, int(iters), sigma_px, sigma_end_px))
        c = opt.evaluate(float(sigma_end_px))[:, 14:17].cpu()
        den = c.sum(dim=1)
        ious.append(torch.where(den > 0, c[:, 0] / den.clamp(min=1.0), torch.zeros_like(den)).reshape(f1 - f0, Kc))
        R, T = opt.poses()
        Rs.append(R.reshape(f1 - f0, Kc, 3, 3))
        Ts.append(T.reshape(f1 - f0, Kc, 3))
        del opt, lab
    return torch.cat(Rs), torch.cat(Ts), torch.cat(ious)


def select_track(iou_fit: torch.Tensor, R_fit: torch.Tensor, valid, lw_track: float = DEFAULTS["lw_track"]) -> list:
    """Step 5: the candidate chosen per frame (None for a frame that is not valid) by the Viterbi pass over the valid frames in order:
    node cost 1 - iou_fit [F,Kc], edge cost lw_track angle(R_a, R_b) / 180 degrees between consecutive valid frames (R_fit [F,Kc,3,3]).
    CPU float64."""
    idx = [f for f, ok in enumerate(valid) if ok]
    if not idx:
        raise ValueError("init_poses: no frame has an object pixel, so none has candidates")
    R = R_fit.detach().cpu().to(torch.float64)[idx]
    node = 1.0 - iou_fit.detach().cpu().to(torch.float64)[idx]
    edge = lambda f: float(lw_track) * rotation_angle_deg(R[f][:, None], R[f + 1][None, :]) / 180.0
    path = viterbi(node, edge)
    out = [None] * len(valid)
    for f, k in zip(idx, path):
        out[f] = k
    return out


def init_poses(verts, faces, dataset, bank: dict | None = None, pose_sil: dict | None = None, log=None, **settings) -> dict:
    """Initialise dataset.R / dataset.T (in place) from the masks alone, as the module docstring lays out.  settings: any key of
    DEFAULTS; bank: a build_view_bank result to reuse (else built from the settings); pose_sil: the settings of the final joint
    refine_poses (its own defaults when None).  Returns {"frames": [per frame {stem, view, rank, iou_bank, iou_fit, iou_final,
    angle_prev_deg, filled_from}], "iou_fit_mean", "iou_final_mean", "settings", "bank": its settings, "refine": the refine_poses result
    without its tensors (None without final_refine), "R", "T" (float32 device tensors)}."""
    fn = "init_poses"
    st = merge(fn, DEFAULTS, None, settings, check_overrides=True)
    verts = check_verts(fn, verts)
    faces = check_faces(fn, faces)
    ds = dataset
    F, dev = ds.n_images, verts.device
    if int(st["candidates"]) < 1 or int(st["hyp_iters"]) < 1 or int(st["hyp_chunk"]) < 1 or not float(st["lw_track"]) >= 0.0 or \
            not 0.0 < float(st["hyp_sigma_end_px"]) <= float(st["hyp_sigma_px"]):
        raise ValueError(f"{fn}: candidates, hyp_iters, hyp_chunk >= 1, lw_track >= 0, 0 < hyp_sigma_end_px <= hyp_sigma_px; got {st}")
    if bank is None:
        bank = build_view_bank(verts, faces, n_views=st["n_views"], seed=st["seed"], render_size=st["render_size"],
                               crop_size=st["crop_size"], distance_scale=st["distance_scale"], view_chunk=st["view_chunk"])
    ret = retrieve(ds.label, bank, st["candidates"])
    Kc = ret["index"].shape[1]
    boxes = ret["boxes"]
    valid = (boxes[:, 2] >= 0).tolist()
    if not any(valid):
        raise ValueError(f"{fn}: no frame has an object pixel, so none has candidates")
    if log is not None:
        log({"stage": "retrieve", "frames": F, "views": int(bank["R"].shape[0]), "candidates": Kc,
             "iou_bank_best_mean": float(ret["iou"][:, 0].mean())})
    # step 3: a translation per candidate from the mask's continuous box (an empty box borrows the whole image; its hypotheses are
    # fitted like the others and never chosen)
    R_cand = bank["R"][ret["index"]]                                          # [F,Kc,3,3] float64, CPU
    bb = boxes.to(torch.float64)
    cont = torch.stack([bb[:, 0] - 0.5, bb[:, 1] - 0.5, bb[:, 2] + 0.5, bb[:, 3] + 0.5], -1)
    whole = torch.tensor([-0.5, -0.5, ds.W - 0.5, ds.H - 0.5], dtype=torch.float64)
    cont = torch.where(torch.tensor(valid)[:, None], cont, whole[None])
    T_cand = depth_from_boxes(verts, R_cand.reshape(-1, 3, 3).to(dev), cont.repeat_interleave(Kc, dim=0).to(dev), ds.K).reshape(F, Kc, 3)
    # step 4
    R_fit, T_fit, iou_fit = fit_hypotheses(verts, faces, ds.label, R_cand.to(dev, torch.float32), T_cand.to(torch.float32), ds.K,
                                           iters=st["hyp_iters"], sigma_px=st["hyp_sigma_px"], sigma_end_px=st["hyp_sigma_end_px"],
                                           lr=st["hyp_lr"], hyp_chunk=st["hyp_chunk"])
    # step 5
    choice = select_track(iou_fit, R_fit, valid, st["lw_track"])
    have = [f for f in range(F) if valid[f]]
    source = [f if valid[f] else min(have, key=lambda h: (abs(h - f), h)) for f in range(F)]
    pick = torch.tensor([choice[s] for s in source], dtype=torch.int64, device=dev)
    src = torch.tensor(source, dtype=torch.int64, device=dev)
    R_sel, T_sel = R_fit[src, pick].contiguous(), T_fit[src, pick].contiguous()
    with torch.no_grad():
        ds.R.copy_(R_sel)
        ds.T.copy_(T_sel)
    if log is not None:
        log({"stage": "select", "iou_fit_mean": float(torch.stack([iou_fit[f, choice[f]] for f in have]).mean())})
    # step 6
    refine = None
    if st["final_refine"]:
        from .pose_sil import refine_poses
        refine = refine_poses(verts, faces, ds, **(pose_sil or {}))
        refine.pop("R"); refine.pop("T")
    stems = list(ds.stems) if getattr(ds, "stems", None) is not None else ["{:04d}".format(i) for i in range(F)]
    R_end = ds.R.detach().cpu().to(torch.float64)
    frames = []
    for f in range(F):
        k = choice[f]
        frames.append({"stem": stems[f], "view": int(ret["index"][f, k]) if k is not None else None, "rank": k,
                       "iou_bank": float(ret["iou"][f, k]) if k is not None else None,
                       "iou_fit": float(iou_fit[f, k]) if k is not None else None,
                       "iou_final": (refine["iou_after"][f] if refine is not None else (float(iou_fit[f, k]) if k is not None else None)),
                       "angle_prev_deg": float(rotation_angle_deg(R_end[f - 1], R_end[f])) if f > 0 else None,
                       "filled_from": None if valid[f] else stems[source[f]]})
    mean = lambda xs: (sum(xs) / len(xs)) if xs else None
    return {"frames": frames, "iou_fit_mean": mean([r["iou_fit"] for r in frames if r["iou_fit"] is not None]),
            "iou_final_mean": mean([r["iou_final"] for r in frames if r["iou_final"] is not None]),
            "settings": {k: (float(v) if isinstance(v, float) else v) for k, v in st.items()}, "bank": dict(bank["settings"]),
            "refine": refine, "R": ds.R.detach().clone(), "T": ds.T.detach().clone()}
