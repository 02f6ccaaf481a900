"""Per-frame object poses refined against a mesh by silhouette matching: the last step of the reference's stage 1
(ObjTracker/jointopt.py + utils/losses.py: all frames' 6-D rotations and translations optimised jointly on a silhouette L2 loss gated
by the keep mask plus a temporal vertex-smoothness term, Adam with the rotation at 10x the learning rate), on this project's own
rasteriser.  The mesh is the reconstruction, the stage-1 template or a scan; the result goes back into Dataset.R / Dataset.T.

The loss (csrc/sil.hip, include/dynhor_hip.h).  Per frame f, with the projection, pixel centres and coverage rule of
``mesh_color.raster_depth``:
  * d2(p) = min over the faces of: 0 where the face covers the pixel centre p, else the squared distance in pixels to the nearest of
    its three edge segments (``nearest_faces``: dh_sil_nearest, a 64-bit atomic minimum of (float_bits(d2) << 32) | face).
  * halo h(x) = max(0, exp(-x / sigma^2) - exp(-cut^2)) / (1 - exp(-cut^2)) for x <= (cut sigma)^2, else 0: 1 on covered pixels,
    continuous, 0 beyond cut sigma pixels.  Rendered soft silhouette S = h(d2): it does not depend on the tessellation or the depth
    order, its gradient reaches one face per pixel, and only the band of width cut sigma outside the outline carries any.
  * target M = h(max(0, e - edge_offset_px)^2), e the distance to the nearest object pixel (``label_edt``: dh_label_edt): both
    silhouettes carry the same halo.  edge_offset_px = 0.5: the mask is made of pixel centres, the mesh outline is continuous.
  * weight w = 1 where label >= 0 and no hand pixel (label -1) lies within cut sigma: next to a hand the mask's outline is not the
    object's.
  * L_sil = mean over the frames of [ sum_p w (S - M)^2 / max(1, sum_p w) ].  The reference divides the sum over all frames by the
    total keep count and then by the number of frames again (utils/losses.py:70-75), on 256^2 crops; here every frame of the full
    image gets equal weight, so the reference's loss weights do not carry over.
  * L_smooth (utils/losses.py:80-84) = the mean over (F - 1) V 3 of the squared difference of the posed vertices of consecutive
    frames, from the mesh's moments: with A = R_{f+1} - R_f, b = T_{f+1} - T_f the sum over the vertices is tr(A M2 A^T) + 2 b^T A m1
    + V |b|^2, M2 = sum v v^T, m1 = sum v (fp64, torch autograd).
  * L = lw_sil L_sil + lw_smooth L_smooth over rot6d [F,3,2], trans [F,3] with R = rot6d_to_matrix(rot6d)^T (dynhor_amd/pose.py);
    Adam, the rotation at rot_lr_mult x lr (jointopt.py:125-141).  sigma anneals geometrically from sigma_px to sigma_end_px.
``silhouette_loss_grad`` (dh_sil_loss_grad) reduces a frame to sum w (S - M)^2, sum w, d/dR (9), d/dT (3) and the (tp, fp, fn) counts
of ``mesh_vis.shade``, in fp64 with block-ordered sums: bitwise reproducible for every frame chunking.

Two optional terms run next to the silhouette: a photometric one (dynhor_amd/pose_photo.py: coloured surface points aligned to blurred
frames; ``photo=, lw_photo=``) and a correspondence one (dynhor_amd/pose_corr.py: dense matches between frames, lifted to the mesh;
``corr=, lw_corr=``), on ``SilhouettePoseOptimizer`` and ``refine_poses``.  Each module states its own loss and normalisation; here the
terms are added to the gradient and to the loss in one fixed order.  Without them nothing of this module changes.

The kernels run on the current stream; there is no CPU path.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._args import check_cams, check_faces, check_verts, device_tensor
from .pose import rot6d_to_matrix
from .pose_corr import DEFAULTS as CORR_DEFAULTS
from .pose_photo import DEFAULTS as PHOTO_DEFAULTS, level_at

# defaults of the YAML's pose_sil: block (runner.POSE_SIL_DEFAULTS); DESIGN_NEXT_ROWS.md section 13 says where each comes from
DEFAULTS = {"iters": 120, "lr": 5e-3, "rot_lr_mult": 10.0, "sigma_px": 6.0, "sigma_end_px": 1.5, "cut": 3.0, "edge_offset_px": 0.5,
            "lw_sil": 1.0, "lw_smooth": 0.0, "resolution": 128, "frame_chunk": 16, "report_freq": 20}


def label_edt(label, value: int, rmax: int) -> torch.Tensor:
    """float32 [F,H,W]: the squared Euclidean distance in pixels to the nearest pixel with label == value, searched over |dx|, |dy| <=
    rmax; +inf where the window holds none.  Results <= rmax^2 are the exact distance transform; larger ones only say "farther"."""
    fn = "label_edt"
    label = device_tensor(fn, "label", label, torch.int8, lambda s: len(s) == 3, "[F,H,W]")
    value, rmax = int(value), int(rmax)
    if not -128 <= value <= 127:
        raise ValueError(f"{fn}: value must lie in [-128, 127], got {value}")
    if rmax < 0:
        raise ValueError(f"{fn}: rmax must be >= 0, got {rmax}")
    F, H, W = label.shape
    out = torch.empty(label.shape, dtype=torch.float32, device=label.device)
    if label.numel() == 0:
        return out
    with torch.cuda.device(label.device):
        tmp = torch.empty_like(out)
        _lib.check(_lib.lib().dh_label_edt(_lib.ptr(label), F, H, W, value, rmax, _lib.ptr(tmp), _lib.ptr(out), _lib.stream()))
    return out


def nearest_faces(verts, faces, R, T, K, H: int, W: int, rmax_px: float) -> torch.Tensor:
    """near int64 [F,H,W]: the uint64 keys (float_bits(d2) << 32) | face of the face nearest to each pixel centre, d2 = 0 exactly where
    raster_depth is covered, -1 where no face lies within rmax_px pixels.  near >> 32 (as int32 bits) is d2 as float32."""
    fn = "nearest_faces"
    verts = check_verts(fn, verts)
    faces = check_faces(fn, faces)
    if verts.device != faces.device:
        raise ValueError(f"{fn}: verts on {verts.device}, faces on {faces.device}")
    H, W, rmax_px = int(H), int(W), float(rmax_px)
    if H <= 0 or W <= 0:
        raise ValueError(f"{fn}: empty images {H}x{W}")
    if not 0.0 <= rmax_px <= 4096.0:
        raise ValueError(f"{fn}: rmax_px must lie in [0, 4096], got {rmax_px}")
    F = R.shape[0] if torch.is_tensor(R) and R.dim() >= 1 else -1
    R, T, K = check_cams(fn, F, R, T, K, verts.device)
    near = torch.full((F, H, W), -1, dtype=torch.int64, device=verts.device)
    if F == 0 or faces.shape[0] == 0:
        return near
    L = _lib.lib()
    with torch.cuda.device(verts.device):
        ws = torch.empty(int(L.dh_sil_nearest_workspace(F, H, W)), dtype=torch.uint8, device=verts.device)
        _lib.check(L.dh_sil_nearest(_lib.ptr(verts), verts.shape[0], _lib.ptr(faces), faces.shape[0], _lib.ptr(R), _lib.ptr(T),
                                    _lib.ptr(K), F, H, W, rmax_px, _lib.ptr(near), _lib.ptr(ws), _lib.stream()))
    return near


def silhouette_sums(verts, faces, near, R, T, K, d2_obj, d2_hand, label, sigma: float, cut: float = 3.0,
                    edge_offset_px: float = 0.5) -> torch.Tensor:
    """float64 [F,17] on the device, the layout of dh_sil_loss_grad: [0] sum w (S - M)^2, [1] sum w, [2..10] d[0] / dR row-major,
    [11..13] d[0] / dT, [14..16] tp, fp, fn.  Nothing is read back."""
    fn = "silhouette_loss_grad"
    verts = check_verts(fn, verts)
    faces = check_faces(fn, faces)
    near = device_tensor(fn, "near", near, torch.int64, lambda s: len(s) == 3, "[F,H,W]")
    F, H, W = near.shape
    if H == 0 or W == 0:
        raise ValueError(f"{fn}: empty images {H}x{W}")
    R, T, K = check_cams(fn, F, R, T, K, near.device)
    d2_obj = device_tensor(fn, "d2_obj", d2_obj, torch.float32, lambda s: s == (F, H, W), f"[{F},{H},{W}]")
    d2_hand = device_tensor(fn, "d2_hand", d2_hand, torch.float32, lambda s: s == (F, H, W), f"[{F},{H},{W}]")
    label = device_tensor(fn, "label", label, torch.int8, lambda s: s == (F, H, W), f"[{F},{H},{W}]")
    if any(t.device != near.device for t in (verts, faces, d2_obj, d2_hand, label)):
        raise ValueError(f"{fn}: every tensor must be on {near.device}")
    sigma, cut, edge_offset_px = float(sigma), float(cut), float(edge_offset_px)
    if not (0.0 < sigma <= 4096.0) or not (0.0 < cut <= 16.0) or not (0.0 <= edge_offset_px <= 4096.0):
        raise ValueError(f"{fn}: sigma in (0, 4096], cut in (0, 16] and edge_offset_px in [0, 4096], got {sigma}, {cut}, {edge_offset_px}")
    L = _lib.lib()
    out = torch.empty(F, int(L.dh_sil_loss_sums()), dtype=torch.float64, device=near.device)
    if F == 0:
        return out
    with torch.cuda.device(near.device):
        ws = torch.empty(max(16, int(L.dh_sil_loss_grad_workspace(F, H, W))), dtype=torch.uint8, device=near.device)
        _lib.check(L.dh_sil_loss_grad(_lib.ptr(near), _lib.ptr(verts), verts.shape[0], _lib.ptr(faces), faces.shape[0], _lib.ptr(R),
                                      _lib.ptr(T), _lib.ptr(K), _lib.ptr(d2_obj), _lib.ptr(d2_hand), _lib.ptr(label), F, H, W, sigma, cut,
                                      edge_offset_px, _lib.ptr(out), _lib.ptr(ws), _lib.stream()))
    return out


def silhouette_loss_grad(verts, faces, near, R, T, K, d2_obj, d2_hand, label, sigma: float, cut: float = 3.0,
                         edge_offset_px: float = 0.5):
    """(loss_num [F], weight [F], dR [F,3,3], dT [F,3], counts int64 [F,3]) of the frames whose nearest faces are `near`
    (nearest_faces(..., rmax_px >= cut sigma)); d2_obj, d2_hand: label_edt(label, 1 / -1, rmax >= cut sigma + edge_offset_px).
    loss_num = sum_p w (S - M)^2, weight = sum_p w, dR / dT its gradient w.r.t. the frame's pose (float64); counts = (tp, fp, fn)
    as mesh_vis.shade counts them."""
    s = silhouette_sums(verts, faces, near, R, T, K, d2_obj, d2_hand, label, sigma, cut, edge_offset_px)
    return s[:, 0], s[:, 1], s[:, 2:11].reshape(-1, 3, 3), s[:, 11:14], s[:, 14:17].round().to(torch.int64)


def halo_radius(sigma: float, cut: float) -> float:
    """The search radius handed to nearest_faces for a halo of cut sigma pixels (a hair wider: the kernel compares in fp32)."""
    return float(cut) * float(sigma) * 1.001


def sigma_at(k: int, iters: int, sigma_px: float, sigma_end_px: float) -> float:
    return float(sigma_px) if iters <= 1 else float(sigma_px) * (float(sigma_end_px) / float(sigma_px)) ** (k / (iters - 1))


class SilhouettePoseOptimizer:
    """rot6d [F,3,2] and trans [F,3] (float64 on the device) of all frames, their Adam state, the mesh moments and the per-run distance
    transforms.  `active` (bool [F] or None = all): the frames whose silhouette term is evaluated and whose pose moves; the others stay
    fixed and still anchor the smoothness term.  step(sigma) reads nothing back to the host; stats() does.  The Adam update is written
    out in torch ops (bias-corrected, beta 0.9 / 0.999, eps 1e-8: torch.optim.Adam's defaults, whose parameter groups PoseRefiner uses)
    so that the step is the very arithmetic of the tests' fp64 restatement and stays free of host reads whatever the optimiser's
    implementation does with its step counter."""

    def __init__(self, verts, faces, label, R0, T0, K, lr=DEFAULTS["lr"], rot_lr_mult=DEFAULTS["rot_lr_mult"],
                 sigma_px=DEFAULTS["sigma_px"], cut=DEFAULTS["cut"], edge_offset_px=DEFAULTS["edge_offset_px"],
                 lw_sil=DEFAULTS["lw_sil"], lw_smooth=DEFAULTS["lw_smooth"], frame_chunk=DEFAULTS["frame_chunk"], active=None,
                 photo=None, lw_photo=0.0, corr=None, lw_corr=0.0):
        fn = "SilhouettePoseOptimizer"
        self.verts = check_verts(fn, verts)
        self.faces = check_faces(fn, faces)
        label = device_tensor(fn, "label", label, torch.int8, lambda s: len(s) == 3, "[F,H,W]")
        self.F, self.H, self.W = label.shape
        dev = self.device = label.device
        R0, T0, self.K = check_cams(fn, self.F, R0, T0, K, dev)
        if self.verts.device != dev or self.faces.device != dev:
            raise ValueError(f"{fn}: every tensor must be on {dev}")
        if int(frame_chunk) < 1:
            raise ValueError(f"{fn}: frame_chunk must be >= 1, got {frame_chunk}")
        if not float(sigma_px) > 0 or not float(cut) > 0 or not float(lr) > 0:
            raise ValueError(f"{fn}: sigma_px, cut and lr must be > 0, got {sigma_px}, {cut}, {lr}")
        self.lr, self.rot_lr_mult = float(lr), float(rot_lr_mult)
        self.sigma_px, self.cut, self.edge_offset_px = float(sigma_px), float(cut), float(edge_offset_px)
        self.lw_sil, self.lw_smooth, self.frame_chunk = float(lw_sil), float(lw_smooth), int(frame_chunk)
        if active is None:
            idx = list(range(self.F))
        else:
            idx = [int(i) for i in torch.as_tensor(active).reshape(-1).nonzero().reshape(-1).tolist()]
        if not idx:
            raise ValueError(f"{fn}: no active frame")
        self.active_list = idx
        self.active_idx = torch.tensor(idx, dtype=torch.int64, device=dev)
        mask = torch.zeros(self.F, dtype=torch.float64, device=dev)
        mask[self.active_idx] = 1.0
        self.active_mask = mask
        R0 = R0.reshape(self.F, 3, 3).to(torch.float64)
        self.rot6d = R0.transpose(1, 2)[:, :, :2].clone().requires_grad_(True)
        self.trans = T0.reshape(self.F, 3).to(torch.float64).clone().requires_grad_(True)
        self._adam = [(torch.zeros_like(p), torch.zeros_like(p)) for p in (self.rot6d, self.trans)]
        self.n_steps = 0
        v64 = self.verts.to(torch.float64)
        self.M2, self.m1, self.V = v64.T @ v64, v64.sum(0), self.verts.shape[0]
        # per-run buffers of the active frames: labels and the two distance transforms, wide enough for the widest halo
        self.rmax = int(math.ceil(self.cut * self.sigma_px + self.edge_offset_px)) + 1
        self.label = label[self.active_idx].contiguous() if len(idx) != self.F else label
        self.d2_obj = label_edt(self.label, 1, self.rmax)
        self.d2_hand = label_edt(self.label, -1, self.rmax)
        self.last_sums = None            # float64 [n_active,17] of the most recent step (before its update)
        self.last_smooth = None
        # the optional terms (pose_photo.PhotometricTerm, pose_corr.CorrespondenceTerm).  The order of this list is the order of every
        # sum into the gradient and into the loss: silhouette, photo, corr
        self.terms = [t for t in (photo, corr) if t is not None]
        for t, lw in ((photo, lw_photo), (corr, lw_corr)):
            if t is not None:
                t.bind(self, lw)
        self.term_rows = None            # the terms' float64 rows of the most recent evaluate(), parallel to self.terms

    def poses64(self):
        return rot6d_to_matrix(self.rot6d).transpose(1, 2), self.trans

    @torch.no_grad()
    def poses(self):
        """(R [F,3,3] object -> camera, T [F,3]) float32, in the layout of obj_infos/*.npz."""
        R, T = self.poses64()
        return R.to(torch.float32).contiguous(), T.to(torch.float32).contiguous()

    def smoothness(self, R, T):
        if self.F < 2:
            return torch.zeros((), dtype=torch.float64, device=self.device)
        A, b = R[1:] - R[:-1], T[1:] - T[:-1]
        tot = torch.einsum("fij,jk,fik->", A, self.M2, A) + 2.0 * torch.einsum("fi,fij,j->", b, A, self.m1) + self.V * (b * b).sum()
        return tot / ((self.F - 1) * self.V * 3)

    @torch.no_grad()
    def evaluate(self, sigma: float) -> torch.Tensor:
        """float64 [n_active,17]: silhouette_sums of the active frames at the current poses, in chunks of frame_chunk frames.  Every
        term's rows at the same poses (of all frames) go to self.term_rows."""
        if float(sigma) > self.sigma_px * (1.0 + 1e-9):
            raise ValueError(f"SilhouettePoseOptimizer: sigma {sigma} exceeds sigma_px {self.sigma_px} the distance transforms were made for")
        R32, T32 = self.poses()
        self.term_rows = [t.sums(self.verts, self.faces, R32, T32, self.K) for t in self.terms]
        R32, T32 = R32[self.active_idx], T32[self.active_idx]
        n = len(self.active_list)
        out = []
        for f0 in range(0, n, self.frame_chunk):
            f1 = min(n, f0 + self.frame_chunk)
            Rc, Tc = R32[f0:f1].contiguous(), T32[f0:f1].contiguous()
            near = nearest_faces(self.verts, self.faces, Rc, Tc, self.K, self.H, self.W, halo_radius(sigma, self.cut))
            out.append(silhouette_sums(self.verts, self.faces, near, Rc, Tc, self.K, self.d2_obj[f0:f1], self.d2_hand[f0:f1],
                                       self.label[f0:f1], sigma, self.cut, self.edge_offset_px))
            del near
        return torch.cat(out)

    def step(self, sigma: float):
        """One Adam step on L at halo width `sigma`: the kernels' d/dR, d/dT are chained into rot6d / trans with torch.autograd.backward
        over rot6d_to_matrix, as PoseRefiner.step chains ray adjoints."""
        sums = self.evaluate(sigma)
        n = len(self.active_list)
        scale = (self.lw_sil / n) / sums[:, 1].clamp(min=1.0)
        gR = torch.zeros(self.F, 3, 3, dtype=torch.float64, device=self.device)
        gT = torch.zeros(self.F, 3, dtype=torch.float64, device=self.device)
        gR[self.active_idx] = sums[:, 2:11].reshape(n, 3, 3) * scale[:, None, None]
        gT[self.active_idx] = sums[:, 11:14] * scale[:, None]
        for t, rows in zip(self.terms, self.term_rows):
            t.add_grads(rows, gR, gT)
        for p in (self.rot6d, self.trans):
            p.grad = None
        R, T = self.poses64()
        outs, grads = [R, T], [gR, gT]
        smooth = None
        if self.lw_smooth != 0.0 and self.F > 1:
            smooth = self.smoothness(R, T)
            outs.append(smooth)
            grads.append(torch.full((), self.lw_smooth, dtype=torch.float64, device=self.device))
        torch.autograd.backward(outs, grads)
        self.n_steps += 1
        b1, b2, eps, k = 0.9, 0.999, 1e-8, self.n_steps
        with torch.no_grad():
            for p, (m, v), lr in zip((self.rot6d, self.trans), self._adam, (self.lr * self.rot_lr_mult, self.lr)):
                g = p.grad * self.active_mask.view(-1, *([1] * (p.dim() - 1)))
                m.mul_(b1).add_(g, alpha=1.0 - b1)
                v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
                p.sub_(lr * (m / (1.0 - b1 ** k)) / ((v / (1.0 - b2 ** k)).sqrt() + eps))
        self.last_sums = sums
        self.last_smooth = smooth.detach() if smooth is not None else None

    @torch.no_grad()
    def stats(self) -> dict:
        """Loss terms and silhouette IoU of the most recent step's evaluation (host reads; the terms' share is read from
        self.term_rows, so before any further evaluate())."""
        if self.last_sums is None:
            raise RuntimeError("SilhouettePoseOptimizer.stats: no step taken yet")
        s = self.last_sums.cpu()
        l_sil = float((s[:, 0] / s[:, 1].clamp(min=1.0)).mean())
        l_sm = float(self.last_smooth) if self.last_smooth is not None else float(self.smoothness(*self.poses64()))
        counts = s[:, 14:17]                                            # tp, fp, fn
        iou = counts[:, 0] / counts.sum(dim=1).clamp(min=1.0)
        st = {"iter": self.n_steps, "loss": self.lw_sil * l_sil + self.lw_smooth * l_sm, "loss_sil": l_sil, "loss_smooth": l_sm,
              "iou_mean": float(iou.mean()), "iou_min": float(iou.min())}
        for t, rows in zip(self.terms, self.term_rows):
            l_term, extra = t.stats(rows.cpu())
            st.update(loss=st["loss"] + t.weight * l_term, **extra)
        return st


def _iou(counts) -> list:
    c = counts.cpu().to(torch.float64)
    d = c.sum(dim=1)
    return [float(c[k, 0] / d[k]) if float(d[k]) > 0 else None for k in range(c.shape[0])]


def select_frames(frames, stems, iou) -> list:
    """Frame indices of a selection: None / "all"; "worst:N" (the N lowest IoUs of `iou`, lowest first, ties in frame order); a
    comma-separated string or a list of stems or indices."""
    n = len(stems)
    if frames is None or (isinstance(frames, str) and frames == "all"):
        return list(range(n))
    if isinstance(frames, str) and frames.startswith("worst:"):
        try:
            k = int(frames[6:])
        except ValueError:
            k = 0
        if k < 1:
            raise ValueError(f"refine_poses: frames 'worst:N' needs an integer N >= 1, got {frames!r}")
        scored = sorted((v, i) for i, v in enumerate(iou) if v is not None)
        return sorted(i for _, i in scored[:k])
    items = [s for s in frames.split(",") if s] if isinstance(frames, str) else list(frames)
    index = {s: i for i, s in enumerate(stems)}
    out = []
    for it in items:
        if isinstance(it, str) and it in index:
            out.append(index[it])
        elif isinstance(it, int) and not isinstance(it, bool) and 0 <= it < n:
            out.append(it)
        else:
            raise ValueError(f"refine_poses: frames names {it!r}, which is neither a frame stem nor an index in 0..{n - 1}")
    if not out:
        raise ValueError("refine_poses: frames selects no frame")
    return sorted(set(out))


def refine_poses(verts, faces, dataset, iters=DEFAULTS["iters"], lr=DEFAULTS["lr"], rot_lr_mult=DEFAULTS["rot_lr_mult"],
                 sigma_px=DEFAULTS["sigma_px"], sigma_end_px=DEFAULTS["sigma_end_px"], cut=DEFAULTS["cut"],
                 edge_offset_px=DEFAULTS["edge_offset_px"], lw_sil=DEFAULTS["lw_sil"], lw_smooth=DEFAULTS["lw_smooth"],
                 frame_chunk=DEFAULTS["frame_chunk"], report_freq=DEFAULTS["report_freq"], frames=None, log=None, photo=None,
                 lw_photo=None, corr=None, lw_corr=None) -> dict:
    """Refine the dataset's poses against the mesh (verts, faces) and write them into dataset.R / dataset.T in place.  frames: None /
    "all", "worst:N", or stems / indices: restricts the silhouette term and the update to those frames; the others stay fixed and
    still anchor the smoothness term.  log(stats dict) is called every report_freq iterations.  Returns {frames (the indices refined),
    stems, iou_before, iou_after (per frame of the dataset, None where a frame has neither object nor mesh pixels), iou_mean_before /
    after, curve (the stats of the reported iterations), R, T (float32 device tensors), settings}.
    photo: a pose_photo.PhotometricTerm of coloured points on this mesh over the dataset's frames, or None.  With it the colour term is
    added at weight lw_photo (default pose_photo.DEFAULTS), iteration k at the blur level photo.levels[floor(k len(levels) / iters)]
    (the frames are blurred again when the level changes); every curve entry gains loss_photo, photo_pairs (per refined frame),
    photo_inliers and blur_sigma, and the result gains photo_pairs (the last iteration's) and settings["photo"].
    corr: a pose_corr.CorrespondenceTerm over the dataset's frames, or a callable active -> CorrespondenceTerm (active: bool [F], the
    frames that move, known only once `frames` is resolved; e.g. lambda a: pose_corr.make_term(dataset, active=a)), or None.  With it
    the correspondence term is added at weight lw_corr (default pose_corr.DEFAULTS); every curve entry gains loss_corr, corr_matches
    and corr_inliers (the mean over the live pairs of sum c rho / sum c, the counted matches, their share inside delta_px), and the
    result gains settings["corr"],
    corr_resid_before / corr_resid_after (per refined frame, the median |r| in pixels of the counted matches whose source frame it is,
    None where there is none) and corr_worst (the five refined frames with the largest median after, as [frame, median])."""
    from .mesh_vis import overlay_frames
    iters, report_freq = int(iters), int(report_freq)
    lw_photo = float(PHOTO_DEFAULTS["lw_photo"] if lw_photo is None else lw_photo)
    lw_corr = float(CORR_DEFAULTS["lw_corr"] if lw_corr is None else lw_corr)
    if iters < 1:
        raise ValueError(f"refine_poses: iters must be >= 1, got {iters}")
    if not 0.0 < float(sigma_end_px) <= float(sigma_px):
        raise ValueError(f"refine_poses: 0 < sigma_end_px <= sigma_px, got {sigma_end_px}, {sigma_px}")
    verts = check_verts("refine_poses", verts)
    faces = check_faces("refine_poses", faces)
    ds = dataset
    stems = list(ds.stems) if ds.stems is not None else ["{:04d}".format(i) for i in range(ds.n_images)]
    before = _iou(overlay_frames(verts, faces, ds, frame_chunk=frame_chunk))
    sel = select_frames(frames, stems, before)
    active = torch.zeros(ds.n_images, dtype=torch.bool)
    active[sel] = True
    if corr is not None:
        corr = corr(active) if callable(corr) else corr
        resid_before = corr.residuals(verts, faces, ds.R, ds.T, ds.K)
    opt = SilhouettePoseOptimizer(verts, faces, ds.label, ds.R, ds.T, ds.K, lr=lr, rot_lr_mult=rot_lr_mult, sigma_px=sigma_px, cut=cut,
                                  edge_offset_px=edge_offset_px, lw_sil=lw_sil, lw_smooth=lw_smooth, frame_chunk=frame_chunk,
                                  active=None if len(sel) == ds.n_images else active, photo=photo, lw_photo=lw_photo, corr=corr,
                                  lw_corr=lw_corr)
    curve = []
    for k in range(iters):
        sigma = sigma_at(k, iters, sigma_px, sigma_end_px)
        if photo is not None:
            photo.set_level(level_at(k, iters, photo.levels))
        opt.step(sigma)
        if (report_freq > 0 and k % report_freq == 0) or k == iters - 1:
            st = dict(opt.stats(), sigma=sigma)
            if photo is not None:
                st["blur_sigma"] = photo.sigma
            curve.append(st)
            if log is not None:
                log(st)
    R, T = opt.poses()
    with torch.no_grad():
        if len(sel) != ds.n_images:            # the fixed frames keep their bits
            keep = ~active.to(R.device)
            R[keep], T[keep] = ds.R[keep], ds.T[keep]
        ds.R.copy_(R)
        ds.T.copy_(T)
    after = _iou(overlay_frames(verts, faces, ds, frame_chunk=frame_chunk))
    scored_before, scored_after = [x for x in before if x is not None], [x for x in after if x is not None]
    mean = lambda xs: sum(xs) / len(xs) if xs else None
    res = {"frames": sel, "stems": stems, "iou_before": before, "iou_after": after, "iou_mean_before": mean(scored_before),
            "iou_mean_after": mean(scored_after), "iou_min_before": min(scored_before, default=None),
            "iou_min_after": min(scored_after, default=None), "curve": curve, "R": R, "T": T,
            "settings": {"iters": iters, "lr": float(lr), "rot_lr_mult": float(rot_lr_mult), "sigma_px": float(sigma_px),
                         "sigma_end_px": float(sigma_end_px), "cut": float(cut), "edge_offset_px": float(edge_offset_px),
                         "lw_sil": float(lw_sil), "lw_smooth": float(lw_smooth), "frame_chunk": int(frame_chunk)}}
    if photo is not None:
        res["photo_pairs"] = curve[-1]["photo_pairs"]
        res["settings"]["photo"] = photo.settings()
    if corr is not None:
        resid_after = corr.residuals(verts, faces, ds.R, ds.T, ds.K)
        res["corr_resid_before"], res["corr_resid_after"] = [resid_before[f] for f in sel], [resid_after[f] for f in sel]
        worst = sorted(((resid_after[f], f) for f in sel if resid_after[f] is not None), key=lambda x: (-x[0], x[1]))[:5]
        res["corr_worst"] = [[f, m] for m, f in worst]
        res["settings"]["corr"] = corr.settings()
    return res
