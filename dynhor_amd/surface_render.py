"""Novel views, depth and normal maps by sphere tracing the SDF (csrc/trace.hip; DESIGN_NEXT_ROWS.md section 17).

A trained NeuS is a surface, so a picture of it needs far fewer network evaluations than volume rendering spends (64 coarse + 64
up-sampling no-grad queries and 128 full forward passes per pixel): the tracer marches every ray of any pose through the unit sphere
with relaxed sphere-tracing steps, brackets the first sign change and closes the bracket by clamped secant steps, and only the hit
points get one full forward pass (SDF gradient for the normal, colour network).  The heavy kernel is the no-grad SDF chain the
renderer already has; this module drives it round by round over a densely packed, order-preserving list of the live rays.

    trace(sdf_fn, R, T, K, H, W, ...)          the per-ray arrays (state, t, ...) and stats, for any field [n,3] -> [n,1]
    render_surface(renderer, R, T, K, H, W)    rgb / depth / normal / hit images of a trained network
    interpolate_pose(R0, T0, R1, T1, ratio)    the geodesic between two object poses (fp64)
    volume_rays(R, T, K, H, W, level)          the same rays with the volume renderer's mid +- 1 bounds (renderer.render_rays)

Limits (the guarantee of the chord scan): a ray that is still marching after max_steps rounds gets the rest of its chord sampled every
scan_step, so no crossing whose negative run along the ray is longer than scan_step is lost; a thinner sliver grazed by a ray can be
stepped over by the marching itself only if the field's Lipschitz constant exceeds 1 / relax.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from . import _lib
from .settings import is_int

MARCH, REFINE, HIT, MISS, FAIL = 0, 1, 2, 3, 4
STATE_NAMES = ("march", "refine", "hit", "miss", "fail")
FLAG_INSIDE, FLAG_CAPPED, FLAG_SCANNED = 1, 2, 4
BACKGROUNDS = ("white", "black", "frame")
TRACE_DEFAULTS = {"eps": 2e-4, "relax": 0.8, "min_step": 1e-3, "max_step": 0.1, "refine_steps": 8, "max_steps": 48,
                  "scan_step": 0.01, "compact_every": 1}
MAX_RAYS = 1 << 21           # rays traced at once (render_surface chunks the views)
SCAN_CHUNK = 1 << 20         # chord-scan samples per query

_NULL = None


def _p(t):
    return _lib.ptr(t) if t is not None else _NULL


def _check_image(fn, H, W, level):
    for name, v in (("H", H), ("W", W), ("level", level)):
        if not is_int(v) or v < 1:
            raise ValueError(f"{fn}: {name} must be an integer >= 1, got {v!r}")


def _check_trace_params(fn, bound, eps, relax, min_step, max_step, refine_steps, max_steps, scan_step, compact_every):
    def pos(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0:
            raise ValueError(f"{fn}: {name} must be a positive number, got {v!r}")
    for name, v in (("bound", bound), ("eps", eps), ("relax", relax), ("min_step", min_step), ("max_step", max_step),
                    ("scan_step", scan_step)):
        pos(name, v)
    if max_step < min_step:
        raise ValueError(f"{fn}: max_step {max_step!r} is below min_step {min_step!r}")
    if not is_int(refine_steps) or not 1 <= refine_steps <= 255:
        raise ValueError(f"{fn}: refine_steps must be an integer in [1, 255], got {refine_steps!r}")
    if not is_int(max_steps) or max_steps < 1:
        raise ValueError(f"{fn}: max_steps must be an integer >= 1, got {max_steps!r}")
    if not is_int(compact_every) or compact_every < 1:
        raise ValueError(f"{fn}: compact_every must be an integer >= 1, got {compact_every!r}")


def _check_poses(fn, R, T, K, device=None):
    """R [F,3,3] (or [3,3]), T [F,3] (or [3]), K [3,3] as float32 tensors -> (R [F,9], T [F,3], Kinv [9], F) on `device` (default R's)."""
    for name, v in (("R", R), ("T", T), ("K", K)):
        if not isinstance(v, torch.Tensor):
            raise TypeError(f"{fn}: {name} must be a tensor, got {type(v).__name__}")
    if R.dim() == 2:
        R, T = R[None], T.reshape(1, -1)
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or R.shape[0] < 1:
        raise ValueError(f"{fn}: R must be [F,3,3] with F >= 1, got {tuple(R.shape)}")
    F = R.shape[0]
    if T.numel() != 3 * F:
        raise ValueError(f"{fn}: T must be [{F},3], got {tuple(T.shape)}")
    if tuple(K.shape) != (3, 3):
        raise ValueError(f"{fn}: K must be [3,3], got {tuple(K.shape)}")
    if not bool(torch.isfinite(R).all()) or not bool(torch.isfinite(T).all()) or not bool(torch.isfinite(K).all()):
        raise ValueError(f"{fn}: R, T and K must be finite")
    dev = R.device if device is None else torch.device(device)
    Kinv = torch.inverse(K.detach().to("cpu", torch.float32)).reshape(9)       # as Dataset does
    return (R.detach().to(dev, torch.float32).reshape(F, 9).contiguous(), T.detach().to(dev, torch.float32).reshape(F, 3).contiguous(),
            Kinv.to(dev).contiguous(), F)


def image_size(H: int, W: int, level: int):
    """(h, w) of the pixel grid 0, level, 2 level, ... (Dataset.gen_rays_at)."""
    return (H + level - 1) // level, (W + level - 1) // level


# ---------------------------------------------------------------------------------------------------------------- poses
def interpolate_pose(R0, T0, R1, T1, ratio: float):
    """The pose at `ratio` of the way from (R0, T0) to (R1, T1) -- the object moving in front of a fixed camera, x_cam = R x_obj + T:
    R = R0 exp(ratio log(R0^T R1)) (the geodesic of SO(3)), T linear.  Computed in fp64 on the CPU; returns (R [3,3], T [3]) fp64."""
    fn = "interpolate_pose"
    mats = []
    for name, v, shape in (("R0", R0, (3, 3)), ("T0", T0, (3,)), ("R1", R1, (3, 3)), ("T1", T1, (3,))):
        v = torch.as_tensor(v).detach().to("cpu", torch.float64)
        if v.numel() != (9 if shape == (3, 3) else 3) or (shape == (3, 3) and tuple(v.shape) != (3, 3)):
            raise ValueError(f"{fn}: {name} must have shape {shape}, got {tuple(v.shape)}")
        if not bool(torch.isfinite(v).all()):
            raise ValueError(f"{fn}: {name} must be finite")
        mats.append(v.reshape(shape))
    R0, T0, R1, T1 = mats
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not math.isfinite(ratio):
        raise ValueError(f"{fn}: ratio must be a finite number, got {ratio!r}")
    for name, Rm in (("R0", R0), ("R1", R1)):
        if float((Rm @ Rm.T - torch.eye(3, dtype=torch.float64)).abs().max()) > 1e-4 or float(torch.linalg.det(Rm)) < 0:
            raise ValueError(f"{fn}: {name} is not a rotation")
    D = R0.T @ R1
    c = ((torch.trace(D) - 1.0) * 0.5).clamp(-1.0, 1.0)
    W = 0.5 * (D - D.T)
    axis_s = torch.stack([W[2, 1], W[0, 2], W[1, 0]])                        # sin(angle) * axis
    s = axis_s.norm()
    angle = torch.atan2(s, c)
    if float(s) < 1e-12:
        if float(c) > 0:                                                     # no rotation between the two
            return R0.clone() if ratio != 1 else R1.clone(), (1.0 - ratio) * T0 + ratio * T1
        # a half turn: the axis is the eigenvector of D for the eigenvalue 1
        S = D + torch.eye(3, dtype=torch.float64)
        axis = S[:, int(S.diagonal().argmax())]
        axis = axis / axis.norm()
    else:
        axis = axis_s / s
    a = float(angle) * float(ratio)
    Kx = torch.tensor([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]], dtype=torch.float64)
    E = torch.eye(3, dtype=torch.float64) + math.sin(a) * Kx + (1.0 - math.cos(a)) * (Kx @ Kx)
    R = R1.clone() if ratio == 1 else (R0.clone() if ratio == 0 else R0 @ E)
    return R, (1.0 - ratio) * T0 + ratio * T1


def volume_rays(R, T, K, H: int, W: int, level: int = 1):
    """(rays_o [N,3], rays_d [N,3], near [N,1], far [N,1], h, w) of the poses R [F,3,3], T [F,3]: the tracer's rays (dh_trace_init)
    with the volume renderer's bounds mid -+ 1 (Dataset.near_far_from_sphere), for renderer.render_rays at a pose no frame has."""
    fn = "volume_rays"
    _check_image(fn, H, W, level)
    R9, T3, Kinv, F = _check_poses(fn, R, T, K)
    if not R9.is_cuda:
        raise ValueError(f"{fn}: R must be on the GPU")
    h, w = image_size(H, W, level)
    a = _init(R9, T3, Kinv, F, H, W, level, 1.0)
    o = a.o.repeat_interleave(h * w, dim=0)
    aa = (a.d * a.d).sum(-1, keepdim=True)
    b = 2.0 * (o * a.d).sum(-1, keepdim=True)
    mid = 0.5 * (-b) / aa
    return o, a.d, mid - 1.0, mid + 1.0, h, w


# ---------------------------------------------------------------------------------------------------------------- the tracer
def _init(R9, T3, Kinv, F, H, W, level, bound):
    dev = R9.device
    h, w = image_size(H, W, level)
    N = F * h * w
    a = SimpleNamespace(F=F, h=h, w=w, N=N, rays_per_view=h * w, H=H, W=W, level=level, R=R9, T=T3,
                        o=torch.empty(F, 3, device=dev), d=torch.empty(N, 3, device=dev), t=torch.empty(N, device=dev),
                        t_far=torch.empty(N, device=dev), state=torch.empty(N, dtype=torch.uint8, device=dev),
                        t_lo=torch.zeros(N, device=dev), s_lo=torch.zeros(N, device=dev), t_hi=torch.zeros(N, device=dev),
                        s_hi=torch.zeros(N, device=dev), nq=torch.zeros(N, dtype=torch.int16, device=dev),
                        nref=torch.zeros(N, dtype=torch.uint8, device=dev), flags=torch.zeros(N, dtype=torch.uint8, device=dev))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dh_trace_init(_p(R9), _p(T3), _p(Kinv), F, H, W, level, float(bound), _p(a.o), _p(a.d), _p(a.t), _p(a.t_far),
                                            _p(a.state), _lib.stream()))
    return a


def trace_step(a, idx, count, s, pts, n_max, eps, relax, min_step, max_step, refine_steps):
    """dh_trace_step on the arrays `a` (trace's namespace): idx int32 [>= n_max], count int32 [1] on the device or None, s f32
    [>= n_max], pts f32 [>= n_max, 3] (out)."""
    _lib.check(_lib.lib().dh_trace_step(_p(idx), _p(count), _p(s), _p(a.o), _p(a.d), a.rays_per_view, a.N, _p(a.t), _p(a.t_far), _p(a.t_lo),
                                        _p(a.s_lo), _p(a.t_hi), _p(a.s_hi), _p(a.state), _p(a.nq), _p(a.nref), _p(a.flags), float(eps),
                                        float(relax), float(min_step), float(max_step), int(refine_steps), int(n_max), _p(pts),
                                        _lib.stream()))


def trace_points(a, idx):
    """dh_trace_points: the query points fma(t, d, o) [n,3] of the rays idx (int tensor [n]) of trace's arrays, as the kernels form them
    (one rounding per coordinate; o + t * d as a tensor expression rounds twice and lands a few 1e-8 away)."""
    n = int(idx.numel())
    pts = torch.empty(n, 3, device=a.d.device)
    if n:
        with torch.cuda.device(a.d.device):
            _lib.check(_lib.lib().dh_trace_points(_p(idx.to(torch.int32).contiguous()), _p(a.o), _p(a.d), _p(a.t), a.rays_per_view, a.N, n,
                                                  _p(pts), _lib.stream()))
    return pts


def merge_stats(stats, st):
    """trace's stats of two chunks of views as one (stats None: st)."""
    if stats is None:
        return dict(st)
    out = {}
    for k, v in st.items():
        out[k] = max(stats[k], v) if k == "queries_max" else stats[k] + v
    tot = stats["rays_in_sphere"] + st["rays_in_sphere"]
    out["queries_mean"] = (stats["queries_mean"] * stats["rays_in_sphere"] + st["queries_mean"] * st["rays_in_sphere"]) / max(tot, 1)
    return out


def trace_compact(a, idx, count, n_max, idx_out, count_out, pts_out, ws=None):
    """dh_trace_compact: the live rays of the list (idx None: all N rays) -> idx_out, pts_out, count_out [1] (device)."""
    nb = (int(n_max) + 255) // 256
    if ws is None or ws.numel() < nb:
        ws = torch.empty(max(nb, 1), dtype=torch.int32, device=a.d.device)
    _lib.check(_lib.lib().dh_trace_compact(_p(idx), _p(count), _p(a.state), _p(a.o), _p(a.d), _p(a.t), a.rays_per_view, a.N, int(n_max),
                                           _p(ws), _p(idx_out), _p(count_out), _p(pts_out), _lib.stream()))


def _query(sdf_fn, pts):
    s = sdf_fn(pts)
    if not isinstance(s, torch.Tensor) or s.numel() != pts.shape[0]:
        raise ValueError(f"trace: sdf_fn must map [n,3] to [n,1]; got {tuple(s.shape) if isinstance(s, torch.Tensor) else type(s).__name__} "
                         f"for n = {pts.shape[0]}")
    return s.reshape(-1).to(torch.float32).contiguous()


@torch.no_grad()
def trace(sdf_fn, R, T, K, H: int, W: int, level: int = 1, bound: float = 1.0, eps: float = TRACE_DEFAULTS["eps"],
          relax: float = TRACE_DEFAULTS["relax"], min_step: float = TRACE_DEFAULTS["min_step"], max_step: float = TRACE_DEFAULTS["max_step"],
          refine_steps: int = TRACE_DEFAULTS["refine_steps"], max_steps: int = TRACE_DEFAULTS["max_steps"],
          scan_step: float = TRACE_DEFAULTS["scan_step"], compact_every: int = TRACE_DEFAULTS["compact_every"]):
    """Sphere-trace the field sdf_fn ([n,3] device points -> [n,1] values; e.g. renderer.sdf) from the poses R [F,3,3], T [F,3]
    (x_cam = R x_obj + T) with intrinsics K, pixels 0, level, 2 level, ... of an H x W image, inside the sphere of radius `bound`.

    dh_trace_init, then up to max_steps rounds of one sdf_fn call on the live rays' points followed by dh_trace_step; every
    compact_every-th round the list is compacted (dh_trace_compact: order-preserving, so the batch a point is queried in is a pure
    function of the inputs) and the live count is read back -- the one host read per compaction; between compactions finished rays
    ride along.  Rays still marching after max_steps (grazing rays that creep along the surface) are not dropped: the rest of their
    chord [t, t_far] is sampled every scan_step in batched queries, the first sample with s <= eps gives a hit or a bracket, and the
    brackets close through the same REFINE steps; rays without such a sample are misses.

    Returns (arrays, stats): arrays = a namespace of o [F,3], d [N,3], t [N] (depth along the ray at a hit), t_far, state u8 [N]
    (MARCH .. FAIL; only HIT and MISS remain), flags u8 [N] (FLAG_*), queries int32 [N] (per ray, the chord scan's included), h, w,
    N, rays_per_view, R [F,9], T [F,3];  stats = counts per state, inside, capped, scanned, rays_in_sphere, queries_mean / queries_max
    over the rays that meet the sphere, rounds, count_reads.  A non-finite field value raises DynhorHipError."""
    fn = "trace"
    if not callable(sdf_fn):
        raise TypeError(f"{fn}: sdf_fn must be callable")
    _check_image(fn, H, W, level)
    _check_trace_params(fn, bound, eps, relax, min_step, max_step, refine_steps, max_steps, scan_step, compact_every)
    R9, T3, Kinv, F = _check_poses(fn, R, T, K)
    if not R9.is_cuda:
        raise ValueError(f"{fn}: R must be on the GPU")
    dev = R9.device
    par = (eps, relax, min_step, max_step, refine_steps)
    with torch.cuda.device(dev):
        a = _init(R9, T3, Kinv, F, H, W, level, bound)
        N = a.N
        in_sphere = a.state == MARCH
        lists = [torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2)]
        points = [torch.empty(N, 3, device=dev) for _ in range(2)]
        counts = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2)]     # ping-pong with the lists: compaction reads one, writes the other
        ws = torch.empty((N + 255) // 256 + 1, dtype=torch.int32, device=dev)
        cur = 0
        trace_compact(a, None, None, N, lists[0], counts[0], points[0], ws)
        n = int(counts[0].item())
        reads, rounds = 1, 0
        extra_q = torch.zeros(N, dtype=torch.int32, device=dev)

        def run_rounds(limit, n, cur, rounds, reads, every):
            k = 0
            while n > 0 and k < limit:
                s = _query(sdf_fn, points[cur][:n])
                trace_step(a, lists[cur], counts[cur], s, points[cur], n, *par)
                k += 1
                rounds += 1
                if k % every == 0 or k == limit:
                    trace_compact(a, lists[cur], counts[cur], n, lists[1 - cur], counts[1 - cur], points[1 - cur], ws)
                    cur = 1 - cur
                    n = int(counts[cur].item())
                    reads += 1
            return n, cur, rounds, reads

        n, cur, rounds, reads = run_rounds(max_steps, n, cur, rounds, reads, compact_every)
        if n > 0:
            # ---- the chord scan of the rays still marching; rays in REFINE only need their remaining steps
            live = lists[cur][:n].long()
            mr = live[a.state[live] == MARCH]
            per = max(1, SCAN_CHUNK // (int(2.0 * bound / scan_step) + 2))         # rays per batched query (a chord is at most 2 bound long)
            for c0 in range(0, mr.numel(), per):
                rr = mr[c0:c0 + per]
                t0, tf = a.t[rr], a.t_far[rr]
                m = int(torch.ceil((tf - t0).max() / scan_step).item()) + 1
                reads += 1
                ts = torch.minimum(t0[:, None] + scan_step * torch.arange(m, device=dev, dtype=torch.float32)[None, :], tf[:, None])
                o = a.o[rr // a.rays_per_view]
                pts = (o[:, None, :] + ts[:, :, None] * a.d[rr][:, None, :]).reshape(-1, 3).contiguous()
                s = _query(sdf_fn, pts).reshape(-1, m)
                bad = ~torch.isfinite(s)
                found = (s <= eps) | bad
                first = torch.where(found.any(dim=1), found.float().argmax(dim=1), torch.full_like(rr, m))
                has = first < m
                a.flags[rr] |= FLAG_SCANNED
                extra_q[rr] += torch.where(has, first, torch.full_like(first, m)).to(torch.int32)
                a.state[rr[~has]] = MISS
                rh, jf = rr[has], first[has]
                if rh.numel():
                    sh = s[has]
                    ar = torch.arange(rh.numel(), device=dev)
                    # the sample before the first one at or below eps is the last positive one (j = 0: the ray's own t_lo stays)
                    prev = (jf - 1).clamp(min=0)
                    a.t_lo[rh] = torch.where(jf > 0, ts[has][ar, prev], a.t_lo[rh])
                    a.s_lo[rh] = torch.where(jf > 0, sh[ar, prev], a.s_lo[rh])
                    a.t[rh] = ts[has][ar, jf]
                    # one step on the found sample: HIT, or MARCH -> REFINE with its first secant point (FAIL for a non-finite value)
                    li = rh.to(torch.int32).contiguous()
                    pp = torch.empty(rh.numel(), 3, device=dev)
                    trace_step(a, li, None, sh[ar, jf].contiguous(), pp, rh.numel(), *par)
            trace_compact(a, lists[cur], counts[cur], n, lists[1 - cur], counts[1 - cur], points[1 - cur], ws)
            cur = 1 - cur
            n = int(counts[cur].item())
            reads += 1
            n, cur, rounds, reads = run_rounds(refine_steps + 1, n, cur, rounds, reads, 1)
        st = a.state
        counts = torch.bincount(st.long(), minlength=5).tolist()
        if counts[FAIL] > 0:
            raise _lib.DynhorHipError("trace: non-finite SDF values on the rays (split_f16 range exceeded, or the network has diverged); "
                                      "use arithmetic 'split_bf16' for queries this far out")
        if counts[MARCH] or counts[REFINE]:
            raise _lib.DynhorHipError(f"trace: {counts[MARCH] + counts[REFINE]} rays did not finish (internal error)")
        a.queries = (a.nq.to(torch.int32) & 0xFFFF) + extra_q
        qs = a.queries[in_sphere]
        stats = {STATE_NAMES[i]: int(counts[i]) for i in range(5)}
        stats.update(rays=N, rays_in_sphere=int(in_sphere.sum()),
                     inside=int(((a.flags & FLAG_INSIDE) != 0).sum()), capped=int(((a.flags & FLAG_CAPPED) != 0).sum()),
                     scanned=int(((a.flags & FLAG_SCANNED) != 0).sum()),
                     queries_mean=float(qs.double().mean()) if qs.numel() else 0.0, queries_max=int(qs.max()) if qs.numel() else 0,
                     rounds=rounds, count_reads=reads)
    return a, stats


# ---------------------------------------------------------------------------------------------------------------- images
def compose(a, slot, normals, colors, background="white", frame_rgb=None, frame_idx=None):
    """dh_trace_compose on trace's arrays: slot int32 [N] (row of normals / colors [n_hits,3] per ray, -1: none).  Returns rgb u8
    [F,h,w,3], depth f32 [F,h,w], normal u8 [F,h,w,3], hit u8 [F,h,w]."""
    if background not in BACKGROUNDS:
        raise ValueError(f"compose: background must be one of {BACKGROUNDS}, got {background!r}")
    if background == "frame" and (frame_rgb is None or frame_idx is None):
        raise ValueError("compose: background 'frame' needs frame_rgb and frame_idx")
    dev = a.d.device
    F, h, w = a.F, a.h, a.w
    rgb = torch.empty(F, h, w, 3, dtype=torch.uint8, device=dev)
    depth = torch.empty(F, h, w, device=dev)
    normal = torch.empty(F, h, w, 3, dtype=torch.uint8, device=dev)
    hit = torch.empty(F, h, w, dtype=torch.uint8, device=dev)
    n_frames = 0
    if background == "frame":
        if frame_rgb.dtype != torch.uint8 or frame_rgb.dim() != 4 or tuple(frame_rgb.shape[1:]) != (a.H, a.W, 3) or not frame_rgb.is_contiguous():
            raise ValueError(f"compose: frame_rgb must be a contiguous u8 [n,{a.H},{a.W},3], got {tuple(frame_rgb.shape)} {frame_rgb.dtype}")
        n_frames = frame_rgb.shape[0]
        frame_idx = torch.as_tensor(frame_idx, dtype=torch.int32).reshape(-1)
        if frame_idx.numel() != F or int(frame_idx.min()) < 0 or int(frame_idx.max()) >= n_frames:
            raise ValueError(f"compose: frame_idx must hold {F} frame indices in [0, {n_frames})")
        frame_idx = frame_idx.to(dev).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dh_trace_compose(_p(a.state), _p(a.t), _p(a.d), _p(slot), _p(normals), _p(colors), int(normals.shape[0]), _p(a.R),
                                               F, a.H, a.W, a.level, BACKGROUNDS.index(background),
                                               _p(frame_rgb) if background == "frame" else _NULL,
                                               _p(frame_idx) if background == "frame" else _NULL, n_frames,
                                               _p(rgb), _p(depth), _p(normal), _p(hit), _lib.stream()))
    return rgb, depth, normal, hit


@torch.no_grad()
def network_at_hits(renderer, pts, dirs):
    """(normals [P,3] = the SDF gradient, colors [P,3]) of the renderer's networks at pts seen along dirs (renderer.eval_points)."""
    return renderer.eval_points(pts, dirs, "render_surface")


@torch.no_grad()
def render_surface(renderer, R, T, K, H: int, W: int, level: int = 1, background: str = "white", frames=None, frame_rgb=None,
                   sdf_fn=None, return_arrays: bool = False, **trace_args):
    """Images of the renderer's networks from the poses R [F,3,3], T [F,3]: trace (sdf_fn default renderer.sdf), one forward pass at the
    hit points for normals and colours (both model families), dh_trace_compose.  background "white" | "black" | "frame" (the pixels of
    frame_rgb u8 [n,H,W,3] at the frame indices `frames`, one per view).  Views go in chunks of at most MAX_RAYS rays.
    Returns a dict: rgb u8 [F,h,w,3], depth f32 [F,h,w] (camera z, inf off the surface), normal u8 [F,h,w,3] (camera frame,
    validate_image's encoding), hit u8 [F,h,w], stats (trace's, summed over the chunks); return_arrays adds `arrays` (one namespace per
    chunk, with slot / normals / colors of the hits)."""
    fn = "render_surface"
    _check_image(fn, H, W, level)
    if background not in BACKGROUNDS:
        raise ValueError(f"{fn}: background must be one of {BACKGROUNDS}, got {background!r}")
    R9, T3, _, F = _check_poses(fn, R, T, K)
    if not R9.is_cuda:
        raise ValueError(f"{fn}: R must be on the GPU")
    if background == "frame":
        if frames is None or frame_rgb is None:
            raise ValueError(f"{fn}: background 'frame' needs frames (one frame index per view) and frame_rgb")
        frames = [int(f) for f in frames]
        if len(frames) != F:
            raise ValueError(f"{fn}: frames must hold one frame index per view ({F}), got {len(frames)}")
    unknown = set(trace_args) - (set(TRACE_DEFAULTS) | {"bound"})
    if unknown:
        raise TypeError(f"{fn}: unknown arguments {sorted(unknown)}")
    sdf_fn = renderer.sdf if sdf_fn is None else sdf_fn
    h, w = image_size(H, W, level)
    per = max(1, MAX_RAYS // (h * w))
    outs, arrays, stats = [], [], None
    for f0 in range(0, F, per):
        f1 = min(F, f0 + per)
        a, st = trace(sdf_fn, R9[f0:f1].view(-1, 3, 3), T3[f0:f1], K, H, W, level=level, **trace_args)
        is_hit = a.state == HIT
        slot = (torch.cumsum(is_hit, 0, dtype=torch.int32) - 1)
        slot = torch.where(is_hit, slot, torch.full_like(slot, -1)).contiguous()
        hi = is_hit.nonzero().reshape(-1)
        d = a.d[hi]
        pts = trace_points(a, hi)              # where the tracer saw |s| <= eps, bit for bit: the network is evaluated there
        normals, colors = network_at_hits(renderer, pts, d)
        outs.append(compose(a, slot, normals, colors, background, frame_rgb, frames[f0:f1] if background == "frame" else None))
        if return_arrays:
            a.slot, a.normals, a.colors, a.hit_points = slot, normals, colors, pts
            arrays.append(a)
        stats = merge_stats(stats, st)
    res = {k: torch.cat([o[i] for o in outs]) for i, k in enumerate(("rgb", "depth", "normal", "hit"))}
    res["stats"] = stats
    if return_arrays:
        res["arrays"] = arrays
    return res


# ---------------------------------------------------------------------------------------------------------------- view specs
def parse_views(spec: str, n_frames: int):
    """A --views string -> ("frames",) | ("interpolate", i, j, n) | ("orbit", n).  Frames must lie in [0, n_frames), n >= 1."""
    if not isinstance(spec, str):
        raise ValueError(f"views must be a string, got {spec!r}")
    parts = spec.split(":")
    try:
        nums = [int(p) for p in parts[1:]]
    except ValueError:
        raise ValueError(f"views {spec!r}: the fields after the name must be integers") from None
    if parts[0] == "frames" and not nums:
        return ("frames",)
    if parts[0] == "interpolate" and len(nums) == 3:
        i, j, n = nums
        for f in (i, j):
            if not 0 <= f < n_frames:
                raise ValueError(f"views {spec!r}: frame {f} is outside [0, {n_frames})")
        if n < 1:
            raise ValueError(f"views {spec!r}: n must be >= 1")
        return ("interpolate", i, j, n)
    if parts[0] == "orbit" and len(nums) == 1:
        if nums[0] < 1:
            raise ValueError(f"views {spec!r}: n must be >= 1")
        return ("orbit", nums[0])
    raise ValueError(f"views {spec!r}: expected frames | interpolate:i:j:n | orbit:n")


def view_poses(spec, R, T):
    """(names, R [V,3,3], T [V,3] fp64 on the CPU, frame index per view or None) of a parsed view spec over the dataset poses R, T.
    interpolate: n poses from frame i to frame j (ratios k / (n - 1); n = 1: frame i alone) and back again without repeating the turning
    point, as upstream's video; orbit: frame 0's pose with the object turned about its z axis by 2 pi k / n."""
    R64 = R.detach().to("cpu", torch.float64).reshape(-1, 3, 3)
    T64 = T.detach().to("cpu", torch.float64).reshape(-1, 3)
    if spec[0] == "frames":
        F = R64.shape[0]
        return ["{:04d}".format(i) for i in range(F)], R64, T64, list(range(F))
    if spec[0] == "interpolate":
        _, i, j, n = spec
        ratios = [k / (n - 1) for k in range(n)] if n > 1 else [0.0]
        ratios = ratios + ratios[-2::-1]
        poses = [interpolate_pose(R64[i], T64[i], R64[j], T64[j], r) for r in ratios]
        return ["{:04d}".format(k) for k in range(len(poses))], torch.stack([p[0] for p in poses]), torch.stack([p[1] for p in poses]), None
    _, n = spec
    Rs = []
    for k in range(n):
        a = 2.0 * math.pi * k / n
        Rz = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
        Rs.append(R64[0] @ Rz)
    return ["{:04d}".format(k) for k in range(n)], torch.stack(Rs), T64[0].expand(n, 3).clone(), None
