"""Warm start of the SDF network from a template mesh (Runner.init_sdf, --mode init_sdf): an Adam fit of the network of either model
family to the template's signed distance (dynhor_amd/mesh_sdf.py), through the hooks the training step itself uses
(NeuSRenderer._net_forward / _net_backward and their HashNeuSRenderer overrides, ParamStore.adam_step).

Every iteration draws `points` samples on the device from one seeded torch.Generator:
  * share_near of them on the surface (metrics.sample_surface, area-weighted), displaced by an isotropic Gaussian of sigma_near;
  * share_far of them likewise with sigma_far (a few centimetres at unit scale: the band in which training samples its rays);
  * the rest uniformly in the unit ball (the whole domain the renderer queries: far from the surface the fit only has to keep the
    sign and roughly the distance).
The loss is  mean |sdf_net - sdf_mesh| + eik_weight * mean (|d sdf_net / d x| - 1)^2;  its two adjoints are formed with torch
elementwise ops and handed to _net_backward together with a zero colour adjoint, so the colour network's gradient is exactly zero
and, with fresh Adam moments, its parameters and the variance do not move at all.  (The colour stage still runs: the hooks are the
training step's, unchanged; what that costs is measured by scripts/bench_mesh_sdf.py.)

The template is a category-level prior: the fit starts training near a plausible shape, and training then moves away from it.
"""
from __future__ import annotations

import time

import torch

from . import _lib
from .mesh_sdf import MeshSDF
from .settings import is_int

# iters x points: 2000 x 65,536 samples against a 5,000-face template is 6.6e11 (point, face) pairs in all.  lr is the training
# default's double (no warm-up: the fit is short and starts from the geometric initialisation, which is already a distance field);
# eik_weight is training's igr_weight.  sigma_near = 0.005 is one voxel of a 200^3 grid over the unit cube (the scale at which the
# reconstruction is meshed), sigma_far = 0.05 a tenth of the canonical object radius.  ray_points: the samples are presented to the
# network hooks as pseudo-rays of this many points with one fixed unit direction (only the colour stage reads it).
SDF_INIT_DEFAULTS = {"iters": 2000, "points": 65536, "ray_points": 8, "lr": 1e-3, "eik_weight": 0.1, "seed": 0,
                     "share_near": 0.5, "share_far": 0.25, "sigma_near": 0.005, "sigma_far": 0.05,
                     "heldout_points": 16384, "heldout_seed": 987654321, "report_freq": 100, "resolution": 128}


def check_settings(c: dict):
    """ValueError unless the settings (a full dict over SDF_INIT_DEFAULTS) make sense."""
    for k in ("iters", "points", "ray_points", "heldout_points", "report_freq", "resolution"):
        if not is_int(c[k]) or c[k] < (0 if k == "iters" else 1):
            raise ValueError(f"sdf_init {k} must be a {'non-negative' if k == 'iters' else 'positive'} integer, got {c[k]!r}")
    for k in ("seed", "heldout_seed"):
        if not is_int(c[k]):
            raise ValueError(f"sdf_init {k} must be an integer, got {c[k]!r}")
    if c["points"] % c["ray_points"]:
        raise ValueError(f"sdf_init points ({c['points']}) must be a multiple of ray_points ({c['ray_points']})")
    for k in ("lr", "sigma_near", "sigma_far"):
        if isinstance(c[k], bool) or not isinstance(c[k], (int, float)) or not c[k] > 0:
            raise ValueError(f"sdf_init {k} must be a positive number, got {c[k]!r}")
    for k in ("eik_weight", "share_near", "share_far"):
        if isinstance(c[k], bool) or not isinstance(c[k], (int, float)) or not c[k] >= 0:
            raise ValueError(f"sdf_init {k} must be a non-negative number, got {c[k]!r}")
    if c["share_near"] + c["share_far"] > 1:
        raise ValueError(f"sdf_init share_near + share_far must not exceed 1, got {c['share_near']} + {c['share_far']}")


def draw_samples(verts, faces, points: int, generator, share_near, share_far, sigma_near, sigma_far):
    """[points,3] fp32 samples of one iteration (module docstring), on the device of verts, from `generator`."""
    from .metrics import sample_surface
    dev = verts.device
    n_near, n_far = int(points * share_near), int(points * share_far)
    n_ball = points - n_near - n_far
    parts = []
    if n_near + n_far:
        s = sample_surface(verts, faces, n_near + n_far, generator)[0]
        sigma = torch.cat([torch.full((n_near, 1), float(sigma_near), device=dev), torch.full((n_far, 1), float(sigma_far), device=dev)])
        parts.append(s + sigma * torch.randn(n_near + n_far, 3, device=dev, generator=generator))
    if n_ball:
        d = torch.randn(n_ball, 3, device=dev, generator=generator)
        r = torch.rand(n_ball, 1, device=dev, generator=generator) ** (1.0 / 3.0)
        parts.append(d / d.norm(dim=1, keepdim=True).clamp(min=1e-12) * r)
    return torch.cat(parts).contiguous()


@torch.no_grad()
def fit_forward(renderer, pts: torch.Tensor, ray_points: int):
    """_net_forward on pts [P,3] as P / ray_points pseudo-rays with the fixed direction (0, 0, 1): the state with sdf [P], normals
    [P,3] (d sdf / d x) and what _net_backward needs."""
    P = int(pts.shape[0])
    if P % ray_points:
        raise ValueError(f"fit_forward: {P} points are not a multiple of ray_points ({ray_points})")
    packed = renderer.store.ensure_packed(renderer._arith())
    dirs = torch.zeros(P // ray_points, 3, device=pts.device)
    dirs[:, 2] = 1.0
    s = renderer.net_state(pts.contiguous(), dirs, int(ray_points), 1)
    renderer._net_forward(s, packed)
    return s


@torch.no_grad()
def fit_backward(renderer, s, sdf_mesh: torch.Tensor, eik_weight: float):
    """The loss (a 0-dim device tensor) of the forward state s against the targets sdf_mesh [P], and its flat parameter gradient in
    the store's gradient bucket (also store.grad_flat): the colour slots exactly zero, the variance slot zero."""
    st = renderer.store
    renderer._check_backward(s)
    P = s.P
    diff = s.sdf - sdf_mesh
    gn = s.normals.norm(dim=1)
    loss = diff.abs().mean() + eik_weight * ((gn - 1.0) ** 2).mean()
    d_sdf = (torch.sign(diff) / P).contiguous()
    d_normals = ((2.0 * eik_weight / P) * (gn - 1.0) / gn.clamp(min=1e-12)).unsqueeze(1) * s.normals
    d_colors = torch.zeros(P, 3, device=s.pts.device)
    grad = st.grad_bucket()
    renderer._net_backward(s, d_sdf, d_normals.contiguous(), d_colors, grad)
    grad[st.var_off] = 0.0                     # (_net_backward leaves the variance slot to its caller)
    st.grad_flat = grad
    return loss


def fit_step(renderer, pts, sdf_mesh, lr: float, eik_weight: float, ray_points: int, step: bool = True):
    """One iteration on given samples and targets: forward, loss, backward and (step) Adam.  Returns (loss, the forward state): the
    loss a 0-dim device tensor, nothing is read back."""
    s = fit_forward(renderer, pts, ray_points)
    loss = fit_backward(renderer, s, sdf_mesh, eik_weight)
    if step:
        renderer.store.adam_step(lr)
    return loss, s


@torch.no_grad()
def heldout_error(renderer, pts, sdf_mesh, chunk=1 << 18) -> float:
    """mean |sdf_net - sdf_mesh| over a fixed point set (the no-grad SDF kernel)."""
    tot = torch.zeros((), dtype=torch.float64, device=pts.device)
    for s0 in range(0, pts.shape[0], chunk):
        tot += (renderer.sdf(pts[s0:s0 + chunk]).view(-1) - sdf_mesh[s0:s0 + chunk]).abs().double().sum()
    return float(tot) / max(1, pts.shape[0])


def fit_sdf_to_mesh(renderer, verts, faces, iters=None, points=None, lr=None, eik_weight=None, seed=None, ray_points=None,
                    share_near=None, share_far=None, sigma_near=None, sigma_far=None, heldout_points=None, heldout_seed=None,
                    report_freq=None, resolution=None, sample_log=None, report=None):
    """Fit renderer's SDF network to the signed distance of the mesh (verts [V,3], faces [F,3], device tensors in the canonical
    frame).  Every setting left at None takes SDF_INIT_DEFAULTS (resolution is the caller's: the grid of the level set Runner.init_sdf
    writes).  Uses the store's Adam moments as they are (Runner.init_sdf starts from and returns to fresh ones).  check_range() runs
    at report iterations and at the end.  sample_log: a list that receives (pts, sdf_mesh) of every iteration (tests); report: a
    callable(iteration, loss) at report iterations.  Returns {"loss": [per iteration], "heldout_before", "heldout_after", "seconds",
    "faces", and the settings}.  Two runs from the same parameters with the same seed give bit-identical parameters."""
    c = dict(SDF_INIT_DEFAULTS)
    given = dict(iters=iters, points=points, lr=lr, eik_weight=eik_weight, seed=seed, ray_points=ray_points, share_near=share_near,
                 share_far=share_far, sigma_near=sigma_near, sigma_far=sigma_far, heldout_points=heldout_points,
                 heldout_seed=heldout_seed, report_freq=report_freq, resolution=resolution)
    c.update({k: v for k, v in given.items() if v is not None})
    check_settings(c)
    dev = renderer.store.device
    verts = verts.to(dev, torch.float32).contiguous()
    faces = faces.to(dev, torch.int64).contiguous()
    mesh = MeshSDF(verts, faces)
    mix = {k: c[k] for k in ("share_near", "share_far", "sigma_near", "sigma_far")}
    hp = draw_samples(verts, faces, c["heldout_points"], torch.Generator(device=dev).manual_seed(c["heldout_seed"]), **mix)
    hd = mesh.query(hp)[0]
    before = heldout_error(renderer, hp, hd)
    gen = torch.Generator(device=dev).manual_seed(c["seed"])
    losses = torch.zeros(c["iters"], device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    s = None
    for it in range(c["iters"]):
        pts = draw_samples(verts, faces, c["points"], gen, **mix)
        target = mesh.query(pts)[0]
        if sample_log is not None:
            sample_log.append((pts, target))
        loss, s = fit_step(renderer, pts, target, c["lr"], c["eik_weight"], c["ray_points"])
        losses[it] = loss
        if (it + 1) % c["report_freq"] == 0:
            renderer.check_range(state=s)
            if report is not None:
                report(it + 1, float(loss))
    if s is not None:
        renderer.check_range(state=s)
    torch.cuda.synchronize(dev)
    seconds = time.perf_counter() - t0
    curve = losses.tolist()
    if any(v != v or v in (float("inf"), float("-inf")) for v in curve):
        raise _lib.DynhorHipError("fit_sdf_to_mesh: non-finite loss (the fit has diverged: lower sdf_init lr)")
    after = heldout_error(renderer, hp, hd)
    return dict(c, loss=curve, heldout_before=before, heldout_after=after, seconds=seconds, faces=int(faces.shape[0]))
