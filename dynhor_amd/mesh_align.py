"""Registration of a ground-truth mesh to the reconstruction before it is scored (metrics.mesh_metrics gt_align=...): trimmed ICP
with a closed-form similarity (Umeyama) or rigid (Horn / Kabsch) update, point-to-point or point-to-plane.

The ground truth is the cloud that moves, x' = s R x + t; the prediction (the target) is never touched, so every distance stays in
the canonical frame's units.  Source = ground-truth samples, target = prediction samples: residue of the hand on the prediction is
then never a correspondence, and parts the prediction lacks fall into the trimmed share.

One iteration, for H hypotheses at once:

  1. nearest target sample of every transformed source sample (``icp_correspond``: dh_icp_correspond, the sweep of the metric's own
     nearest-neighbour kernel with the source transformed on load by the fp32 rounding of s R and t);
  2. the trim threshold: the ceil(trim N)-th smallest squared distance of each hypothesis (torch.kthvalue on the device);
  3. the moment sums of the pairs inside it (``icp_moments``: dh_icp_moments, fp64, bitwise reproducible);
  4. the 3 x 3 (point) or 7 x 7 (plane; 6 x 6 rigid) problem in fp64 on the host: ``umeyama_from_moments`` / ``plane_update_from_moments``;
  5. stop when the update moves no point of the source's bounding sphere by more than tol x the target's bounding radius (an upper
     bound of the samples' own displacement, computed on the host from the two transforms), or after max_iters.

init "identity" starts one hypothesis from the transform it is given.  init "global" starts from the centroids and RMS radii of the
two sample sets (translation and scale) and ``rotation_seeds(n_seeds)`` rotations: all of them run a coarse level on prefixes of the
sample sets (the samples are independent draws, so a prefix is a sub-sample), the n_refine with the smallest trimmed residual -- one
per basin: a candidate whose rotation is within second_min_deg of a better one is passed over -- are refined on all samples, and the winner is the one with the smallest TWO-SIDED trimmed mean distance (source -> target and target ->
source): a wrong basin of a shape made of similar parts explains the source well but leaves target parts far from it.

There is no CPU path: the two entry points are HIP, and tensors on the CPU raise DynhorHipError.
"""
from __future__ import annotations

import math

import torch

from . import _lib

MODES = ("none", "rigid", "similarity")
INITS = ("identity", "global")
METHODS = ("point", "plane")

# Defaults that needed a measurement, chosen on the three-box fixture of tests/mesh_align_util.py with the fp64 restatement there (at
# reduced size on the CPU: meshes at 64 / 80, 4,000 - 5,000 samples; DESIGN_NEXT_ROWS.md section 12 has the rows).
#   n_align 100,000: sample spacing sqrt(area / n) ~ 2e-3 on the canonical object, under half the finest F-score threshold; one
#     iteration is 10^10 pairs.
#   trim 0.9: a tenth of the ground truth may have no counterpart (the sole of a shoe on the table, a part the hand always hides).
#   n_seeds 256: from a start 40 degrees off (8 random axes) the coarse level ends within 7 degrees of the truth, which the refinement
#     closes; from 50 degrees it is still up to 19 degrees off after its 30 iterations, from 60 degrees up to 39.  The design relies
#     on a 40-degree basin, so the seed set's covering radius must stay below that: 59.8 degrees for 64 seeds, 44.3 for 128, 35.3 for 256
#     (tests/test_cpu_mesh_align.py measures and asserts it).  A coarse iteration of 256 hypotheses is 10^9 pairs.
#   n_refine 4: seeds that reach the same basin end on the same transform (with 256 seeds the four best of the fixture were all the
#     right one), so the four are taken from different basins, which also gives residual_second its runner-up; the fixture's
#     wrong basins (100 - 160 degrees off) have one-sided residuals within 10 % of the right one's and are told apart only by the
#     two-sided residual (0.0039 against 0.075).
#   coarse 1024 x 4096 samples, 30 point-to-point iterations: ranks the basins; point-to-point because the linearised plane step is not
#     to be trusted tens of degrees away from the answer.
#   method "plane" for the refinement, max_iters 60, tol 1e-5: 15 degrees off, point-to-plane stops after 9 iterations 0.08 degrees
#     from the truth; point-to-point is 0.10 degrees off after 60 iterations and still moving 1e-4 per iteration (it slides along
#     smooth faces), so the cap is what ends it.
ALIGN_DEFAULTS = {"n_align": 100_000, "trim": 0.9, "method": "plane", "max_iters": 60, "tol": 1e-5, "n_seeds": 256, "n_refine": 4,
                  "coarse_src": 1024, "coarse_tgt": 4096, "coarse_iters": 30, "second_min_deg": 10.0}

POINT_SUMS, PLANE_SUMS = 19, 36


# ------------------------------------------------------------------------------------------------ rotations
def rotation_seeds(n: int) -> torch.Tensor:
    """n proper rotations [n,3,3] fp64 spread over SO(3): the super-Fibonacci spiral (Alexa, "Super-Fibonacci Spirals: Fast,
    Low-Discrepancy Sampling of SO(3)", CVPR 2022).  Sample i of n is the unit quaternion
    (r sin a, r cos a, q sin b, q cos b), r = sqrt(u), q = sqrt(1 - u), u = (i + 1/2) / n, a = 2 pi (i + 1/2) / phi,
    b = 2 pi (i + 1/2) / psi with phi = sqrt(2) and psi = 1.533751168755204288118041 (the paper's constants).  Deterministic."""
    if n < 1:
        raise ValueError(f"rotation_seeds: n must be >= 1, got {n}")
    i = torch.arange(n, dtype=torch.float64) + 0.5
    u = i / n
    a, b = 2.0 * math.pi * i / math.sqrt(2.0), 2.0 * math.pi * i / 1.533751168755204288118041
    r, q = u.sqrt(), (1.0 - u).sqrt()
    return quat_to_matrix(torch.stack([r * a.sin(), r * a.cos(), q * b.sin(), q * b.cos()], dim=1))


def quat_to_matrix(q: torch.Tensor) -> torch.Tensor:
    """Rotation matrices [...,3,3] of unit quaternions [...,4] = (x, y, z, w)."""
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).reshape(q.shape[:-1] + (3, 3))


def rotvec_to_matrix(w: torch.Tensor) -> torch.Tensor:
    """Rodrigues: rotation matrices [...,3,3] of rotation vectors [...,3] (fp64)."""
    half = 0.5 * w.norm(dim=-1, keepdim=True)
    # sin(half) / |w| with its limit 1/2 at 0
    k = torch.where(half > 1e-12, half.sin() / (2.0 * half).clamp(min=1e-300), torch.full_like(half, 0.5))
    return quat_to_matrix(torch.cat([w * k, half.cos()], dim=-1))


def rotation_angle_deg(Ra: torch.Tensor, Rb: torch.Tensor) -> torch.Tensor:
    """Angle in degrees of the rotation Ra^T Rb (broadcasts over leading dimensions)."""
    tr = (Ra * Rb).sum(dim=(-2, -1))
    return torch.rad2deg(torch.acos(((tr - 1.0) / 2.0).clamp(-1.0, 1.0)))


# ------------------------------------------------------------------------------------------------ closed forms (host, fp64)
def umeyama_from_moments(mom, origin_src, origin_tgt, with_scale: bool = True):
    """The similarity (with_scale) or rigid transform that minimises sum |s R p + t - q|^2 over the pairs whose sums are `mom`
    ([19] or [H,19] fp64: the point-to-point layout of dh_icp_moments, p and q centred on origin_src / origin_tgt [3]).  Umeyama
    1991: R = U diag(1, 1, det(U V^T)) V^T of the cross-covariance's SVD (never a reflection), s = tr(D S) / var(p), t = mean q -
    s R mean p; rigid mode returns s == 1 exactly.  Returns (s [H], R [H,3,3], t [H,3]) fp64 (no leading dimension for a [19] input).
    ValueError: fewer than 3 pairs, or a cross-covariance of rank < 2 (collinear points: the rotation about their line is free)."""
    mom = torch.as_tensor(mom, dtype=torch.float64, device="cpu")
    single = mom.dim() == 1
    m = mom.reshape(-1, POINT_SUMS)
    os_, ot = (torch.as_tensor(o, dtype=torch.float64, device="cpu").reshape(3) for o in (origin_src, origin_tgt))
    n = m[:, 0]
    if bool((n < 3).any()):
        raise ValueError(f"umeyama_from_moments: fewer than 3 inliers ({int(n.min())}): the transform is not determined")
    mp, mq = m[:, 1:4] / n[:, None], m[:, 4:7] / n[:, None]
    cov = m[:, 7:16].reshape(-1, 3, 3) / n[:, None, None] - mq[:, :, None] * mp[:, None, :]
    var_p = m[:, 16] / n - (mp * mp).sum(dim=1)
    var_q = m[:, 17] / n - (mq * mq).sum(dim=1)
    U, D, Vh = torch.linalg.svd(cov)
    # rank: singular values against the clouds' own spread (sqrt(var_p var_q) bounds D[0])
    floor = 1e-10 * (var_p * var_q).clamp(min=0.0).sqrt()
    if bool((D[:, 1] <= floor).any()) or bool((var_p <= 0).any()):
        raise ValueError("umeyama_from_moments: the inliers are collinear (cross-covariance of rank < 2): the rotation about their line "
                         "is not determined")
    sign = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vh))
    S = torch.ones_like(D)
    S[:, 2] = torch.where(sign < 0, -torch.ones_like(sign), torch.ones_like(sign))
    R = (U * S[:, None, :]) @ Vh
    s = (D * S).sum(dim=1) / var_p if with_scale else torch.ones_like(n)
    t = (mq + ot) - s[:, None] * (R @ (mp + os_)[:, :, None])[:, :, 0]
    return (s[0], R[0], t[0]) if single else (s, R, t)


def plane_update_from_moments(mom, s, R, t, origin_tgt, with_scale: bool = True):
    """One Gauss-Newton step of the point-to-plane residual from the sums `mom` [H,36] (the plane layout of dh_icp_moments) at the
    transforms (s [H], R [H,3,3], t [H,3]): solve sum J^T J d = sum J^T b for d = (rotation vector w, translation u, log-scale l; rigid:
    the 6 x 6 block, l = 0) and compose about origin_tgt: x' = origin_tgt + e^l Rot(w) (x - origin_tgt) + u.  Returns the new
    (s, R, t).  ValueError: fewer than 7 pairs.  A singular normal matrix (a surface of revolution, a plane) is solved in the
    least-squares sense: the free direction gets no update."""
    mom = torch.as_tensor(mom, dtype=torch.float64, device="cpu").reshape(-1, PLANE_SUMS)
    ot = torch.as_tensor(origin_tgt, dtype=torch.float64, device="cpu").reshape(3)
    H = mom.shape[0]
    if bool((mom[:, 35] < 7).any()):
        raise ValueError(f"plane_update_from_moments: fewer than 7 inliers ({int(mom[:, 35].min())}): the transform is not determined")
    iu = torch.triu_indices(7, 7)
    N = torch.zeros(H, 7, 7, dtype=torch.float64)
    N[:, iu[0], iu[1]] = mom[:, :28]
    N[:, iu[1], iu[0]] = mom[:, :28]
    g = mom[:, 28:35]
    k = 7 if with_scale else 6
    d = torch.zeros(H, 7, dtype=torch.float64)
    d[:, :k] = torch.linalg.lstsq(N[:, :k, :k], g[:, :k, None], rcond=1e-12, driver="gelsd").solution[:, :, 0]
    Rot = rotvec_to_matrix(d[:, 0:3])
    e = d[:, 6].exp()
    R2 = Rot @ R
    s2 = s * e if with_scale else s.clone()
    t2 = ot + e[:, None] * (Rot @ (t - ot)[:, :, None])[:, :, 0] + d[:, 3:6]
    return s2, R2, t2


def pack_transforms(s, R, t) -> torch.Tensor:
    """[H,12] fp32 CPU: A = s R row-major, then t -- the fp64 product rounded ONCE to fp32 (what the kernels apply)."""
    A = (s[:, None, None] * R).reshape(-1, 9)
    return torch.cat([A, t], dim=1).float().contiguous()


# ------------------------------------------------------------------------------------------------ the two entry points (HIP)
def _check_cloud(fn, name, x, dtype=torch.float32, cols=3):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _lib.DynhorHipError(f"{fn}: {name} must be a device tensor (the HIP kernel has no CPU fallback)")
    if x.dtype != dtype or x.dim() != 2 or x.shape[1] != cols:
        raise ValueError(f"{fn}: {name} must be {dtype} [N,{cols}], got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def icp_correspond(src: torch.Tensor, tgt: torch.Tensor, xf: torch.Tensor):
    """(d2 [H,N] float32, idx [H,N] int32): for hypothesis h the nearest target point of A_h src[i] + t_h (xf [H,12] float32 on the
    device: A row-major then t; dh_icp_correspond -- bit for bit metrics.nearest_sqdist on the transformed cloud)."""
    src, tgt = _check_cloud("icp_correspond", "src", src), _check_cloud("icp_correspond", "tgt", tgt)
    xf = _check_cloud("icp_correspond", "xf", xf, cols=12)
    n, m, h = src.shape[0], tgt.shape[0], xf.shape[0]
    L = _lib.lib()
    with torch.cuda.device(src.device):
        d2 = torch.empty(h, n, device=src.device)
        idx = torch.empty(h, n, dtype=torch.int32, device=src.device)
        nbytes = int(L.dh_icp_correspond_workspace(n, m, h))
        if nbytes < 0:
            _lib.check(nbytes)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device) if nbytes > 0 else None
        _lib.check(L.dh_icp_correspond(_lib.ptr(src), n, _lib.ptr(tgt), m, _lib.ptr(xf), h, _lib.ptr(d2), _lib.ptr(idx),
                                       _lib.ptr(ws) if ws is not None else None, _lib.stream()))
    return d2, idx


def icp_moments(src, tgt, tgt_normals, xf, idx, d2, thr, origin_src, origin_tgt) -> torch.Tensor:
    """[H,19] (tgt_normals None: point-to-point) or [H,36] (point-to-plane) float64 on the device: the sums of dh_icp_moments over the
    pairs with d2[h,i] <= thr[h] (layout: include/dynhor_hip.h).  origin_src / origin_tgt: [3] float32 device tensors."""
    fn = "icp_moments"
    src, tgt = _check_cloud(fn, "src", src), _check_cloud(fn, "tgt", tgt)
    xf = _check_cloud(fn, "xf", xf, cols=12)
    n, m, h = src.shape[0], tgt.shape[0], xf.shape[0]
    plane = tgt_normals is not None
    if plane:
        tgt_normals = _check_cloud(fn, "tgt_normals", tgt_normals)
        if tgt_normals.shape[0] != m:
            raise ValueError(f"{fn}: {tgt_normals.shape[0]} normals for {m} target points")
    idx, d2 = _check_cloud(fn, "idx", idx, torch.int32, n), _check_cloud(fn, "d2", d2, torch.float32, n)
    if idx.shape[0] != h or d2.shape[0] != h:
        raise ValueError(f"{fn}: idx / d2 must be [{h},{n}], got {tuple(idx.shape)} / {tuple(d2.shape)}")
    vec = lambda name, v, k: _check_cloud(fn, name, v.reshape(1, -1), cols=k)
    thr, origin_src, origin_tgt = vec("thr", thr, h), vec("origin_src", origin_src, 3), vec("origin_tgt", origin_tgt, 3)
    L = _lib.lib()
    with torch.cuda.device(src.device):
        out = torch.empty(h, int(L.dh_icp_moments_sums(int(plane))), dtype=torch.float64, device=src.device)
        nbytes = int(L.dh_icp_moments_workspace(n, h, int(plane)))
        if nbytes < 0:
            _lib.check(nbytes)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=src.device)
        _lib.check(L.dh_icp_moments(_lib.ptr(src), _lib.ptr(tgt), _lib.ptr(tgt_normals) if plane else None, _lib.ptr(xf), _lib.ptr(idx),
                                    _lib.ptr(d2), _lib.ptr(thr), _lib.ptr(origin_src), _lib.ptr(origin_tgt), n, m, h, _lib.ptr(out),
                                    _lib.ptr(ws), _lib.stream()))
    return out


# ------------------------------------------------------------------------------------------------ the loop
def step_bound(s0, R0, t0, s1, R1, t1, center, radius):
    """Upper bound [H] of |x1 - x0| over the ball (center [3], radius) for the transforms x_k = s_k R_k x + t_k:
    |dA (x - c)| + |dA c + dt| <= ||dA||_2 radius + |dA c + dt|."""
    dA = s1[:, None, None] * R1 - s0[:, None, None] * R0
    shift = (dA @ center[None, :, None])[:, :, 0] + (t1 - t0)
    return torch.linalg.matrix_norm(dA, ord=2) * radius + shift.norm(dim=1)


def _trim_count(n, trim):
    return min(n, max(3, int(math.ceil(trim * n))))


def icp(src, tgt, tgt_normals, s, R, t, with_scale=True, method="point", trim=0.9, max_iters=60, tol=1e-5):
    """Trimmed ICP of the device clouds src [N,3] -> tgt [M,3] (float32; tgt_normals [M,3] for method "plane") from the H start
    transforms (s [H], R [H,3,3], t [H,3]; fp64 CPU), every hypothesis until its own stop.  Returns (s, R, t, stats) with stats a dict
    of per-hypothesis lists: iters, converged, last_step (the bound of the final update's displacement), residual (trimmed mean
    distance at the returned transform), inliers."""
    if method not in METHODS:
        raise ValueError(f"icp: method must be one of {METHODS}, got {method!r}")
    if method == "plane" and tgt_normals is None:
        raise ValueError("icp: method 'plane' needs the target normals")
    if not 0.0 < trim <= 1.0:
        raise ValueError(f"icp: trim must be in (0, 1], got {trim!r}")
    dev = src.device
    s, R, t = (torch.as_tensor(v, dtype=torch.float64, device="cpu").clone() for v in (s, R, t))
    s, R, t = s.reshape(-1), R.reshape(-1, 3, 3), t.reshape(-1, 3)
    H, n = s.shape[0], src.shape[0]
    k = _trim_count(n, trim)
    c_src64, c_tgt64 = src.double().mean(dim=0), tgt.double().mean(dim=0)
    o_src, o_tgt = c_src64.float(), c_tgt64.float()                                     # the origins the kernel subtracts (fp32)
    o_src64, o_tgt64 = o_src.double().cpu(), o_tgt.double().cpu()
    r_src = float((src.double() - c_src64).norm(dim=1).max())
    r_tgt = float((tgt.double() - c_tgt64).norm(dim=1).max())
    c_src = c_src64.cpu()
    nrm = tgt_normals if method == "plane" else None
    iters, conv, last = [0] * H, [False] * H, [math.inf] * H
    act = list(range(H))
    for _ in range(int(max_iters)):
        if not act:
            break
        a = torch.tensor(act)
        xf = pack_transforms(s[a], R[a], t[a]).to(dev)
        d2, idx = icp_correspond(src, tgt, xf)
        thr = torch.kthvalue(d2, k, dim=1).values
        mom = icp_moments(src, tgt, nrm, xf, idx, d2, thr, o_src, o_tgt).cpu()
        if method == "plane":
            s1, R1, t1 = plane_update_from_moments(mom, s[a], R[a], t[a], o_tgt64, with_scale)
        else:
            s1, R1, t1 = umeyama_from_moments(mom, o_src64, o_tgt64, with_scale)
        step = step_bound(s[a], R[a], t[a], s1, R1, t1, c_src, r_src)
        s[a], R[a], t[a] = s1, R1, t1
        still = []
        for j, h in enumerate(act):
            iters[h] += 1
            last[h] = float(step[j])
            if last[h] <= tol * r_tgt:
                conv[h] = True
            else:
                still.append(h)
        act = still
    # the residual and the inlier count AT the returned transforms
    xf = pack_transforms(s, R, t).to(dev)
    d2, idx = icp_correspond(src, tgt, xf)
    thr = torch.kthvalue(d2, k, dim=1).values
    mom = icp_moments(src, tgt, None, xf, idx, d2, thr, o_src, o_tgt).cpu()
    stats = {"iters": iters, "converged": conv, "last_step": last, "residual": (mom[:, 18] / mom[:, 0]).tolist(),
             "inliers": [int(v) for v in mom[:, 0]]}
    return s, R, t, stats


def reverse_residual(src, tgt, s, R, t, trim=0.9) -> float:
    """Trimmed mean distance target -> transformed source (the other half of the two-sided residual): the source samples are
    transformed in fp64 and searched with metrics.nearest_sqdist."""
    from .metrics import nearest_sqdist
    A = (float(s) * R).to(src.device)
    x = (src.double() @ A.T + t.to(src.device)).float().contiguous()
    d2 = nearest_sqdist(tgt, x)
    k = _trim_count(d2.shape[0], trim)
    return float(torch.topk(d2, k, largest=False).values.double().sqrt().mean())


def global_starts(src, tgt, n_seeds, with_scale=True):
    """The H = n_seeds start transforms of init "global": s0 = RMS radius of the target samples / that of the source samples (1 in rigid
    mode), R_k = rotation_seeds(n_seeds)[k], t_k = centroid(tgt) - s0 R_k centroid(src).  fp64 CPU."""
    s64, t64 = src.double(), tgt.double()
    cs, ct = s64.mean(dim=0), t64.mean(dim=0)
    rs, rt = float((s64 - cs).pow(2).sum(dim=1).mean().sqrt()), float((t64 - ct).pow(2).sum(dim=1).mean().sqrt())
    s0 = rt / rs if with_scale else 1.0
    R = rotation_seeds(n_seeds)
    cs, ct = cs.cpu(), ct.cpu()
    t = ct[None, :] - s0 * (R @ cs[None, :, None])[:, :, 0]
    return torch.full((n_seeds,), s0, dtype=torch.float64), R, t


def align_clouds(src, tgt, tgt_normals, mode="similarity", init="identity", start=None, **opts):
    """Register the device cloud src [N,3] (the ground truth's samples) to tgt [M,3] (the prediction's; tgt_normals [M,3]).  mode
    "rigid" | "similarity"; init "identity" (from `start` = (s, R, t), default the identity) | "global" (module docstring); opts over
    ALIGN_DEFAULTS (method, trim, max_iters, tol, n_seeds, n_refine, coarse_src, coarse_tgt, coarse_iters, second_min_deg).
    Returns (s float, R [3,3], t [3] fp64 CPU, stats): residual, residual_two_sided, iters, inliers, n_align, seeds, converged,
    last_step, method, and residual_second -- the two-sided residual of the best refined candidate whose rotation is more than
    second_min_deg from the winner's (None when there is none: a small gap to residual_two_sided means an ambiguous pose)."""
    if mode not in MODES[1:]:
        raise ValueError(f"align_clouds: mode must be 'rigid' or 'similarity', got {mode!r}")
    if init not in INITS:
        raise ValueError(f"align_clouds: init must be one of {INITS}, got {init!r}")
    unknown = set(opts) - set(ALIGN_DEFAULTS)
    if unknown:
        raise ValueError(f"align_clouds: unknown options {sorted(unknown)} (known: {sorted(ALIGN_DEFAULTS)})")
    o = dict(ALIGN_DEFAULTS, **opts)
    with_scale = mode == "similarity"
    run = dict(with_scale=with_scale, trim=float(o["trim"]), tol=float(o["tol"]))
    if init == "identity":
        s0, R0, t0 = start if start is not None else (1.0, torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
        s, R, t, st = icp(src, tgt, tgt_normals, torch.tensor([float(s0)]), R0, t0, method=o["method"], max_iters=int(o["max_iters"]), **run)
        seeds = 1
    else:
        seeds = int(o["n_seeds"])
        s, R, t = global_starts(src, tgt, seeds, with_scale)
        s, R, t, cst = icp(src[:int(o["coarse_src"])].contiguous(), tgt[:int(o["coarse_tgt"])].contiguous(), None, s, R, t, method="point",
                           max_iters=int(o["coarse_iters"]), **run)
        order = []                                # the n_refine best by residual, one per basin: a candidate within second_min_deg
        for h in sorted(range(seeds), key=lambda h: cst["residual"][h]):        # of a better one would only be refined onto it
            if all(float(rotation_angle_deg(R[h], R[k])) > float(o["second_min_deg"]) for k in order):
                order.append(h)
            if len(order) >= max(1, int(o["n_refine"])):
                break
        pick = torch.tensor(order)
        s, R, t, st = icp(src, tgt, tgt_normals, s[pick], R[pick], t[pick], method=o["method"], max_iters=int(o["max_iters"]), **run)
    rev = [reverse_residual(src, tgt, s[h], R[h], t[h], run["trim"]) for h in range(s.shape[0])]
    two = [0.5 * (st["residual"][h] + rev[h]) for h in range(s.shape[0])]
    w = min(range(len(two)), key=lambda h: two[h])
    far = [two[h] for h in range(len(two)) if float(rotation_angle_deg(R[w], R[h])) > float(o["second_min_deg"])]
    stats = {"residual": st["residual"][w], "residual_two_sided": two[w], "residual_second": min(far) if far else None,
             "iters": st["iters"][w], "inliers": st["inliers"][w], "n_align": int(src.shape[0]), "seeds": seeds,
             "converged": bool(st["converged"][w]), "last_step": st["last_step"][w], "method": o["method"]}
    return float(s[w]), R[w].clone(), t[w].clone(), stats


def align_meshes(gt_v, gt_f, pred_v, pred_f, mode="similarity", init="identity", seed=0, device=None, **opts):
    """align_clouds on n_align area-weighted samples of each mesh (metrics.sample_surface; a generator of its own seeded with `seed`,
    prediction first), the ground truth (gt_v, gt_f) moving onto the prediction (pred_v, pred_f).  Returns (s, R, t, stats) with
    x' = s R x + t bringing ground-truth vertices into the prediction's frame."""
    from .metrics import sample_surface
    if device is None:
        device = pred_v.device if pred_v.is_cuda else torch.device("cuda", torch.cuda.current_device())
    n = int(opts.pop("n_align", ALIGN_DEFAULTS["n_align"]))
    if n < 3:
        raise ValueError(f"align_meshes: n_align must be >= 3, got {n}")
    g = torch.Generator(device=device).manual_seed(int(seed))
    tgt, tgt_n = sample_surface(pred_v.to(device, torch.float32), pred_f, n, g)
    src, _ = sample_surface(gt_v.to(device, torch.float32), gt_f, n, g)
    return align_clouds(src, tgt, tgt_n, mode=mode, init=init, **opts)


def apply_transform(verts: torch.Tensor, s, R, t) -> torch.Tensor:
    """s R x + t of verts [V,3] in fp64, returned in the dtype and on the device of verts."""
    R = torch.as_tensor(R, dtype=torch.float64).reshape(3, 3).to(verts.device)
    t = torch.as_tensor(t, dtype=torch.float64).reshape(3).to(verts.device)
    return (float(s) * (verts.double() @ R.T) + t).to(verts.dtype)
