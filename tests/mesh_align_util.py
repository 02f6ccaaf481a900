"""Shared helper of the mesh-alignment tests: the fixtures, and a plain-torch fp64 RESTATEMENT of dynhor_amd/mesh_align.py's
algorithm (chunked brute-force nearest neighbours, kthvalue trim, Umeyama / Gauss-Newton update computed from the pairs themselves, not
from moment sums).  The reference project has no registration to compare with, so this restatement is the yardstick; it runs on
whatever device its inputs live on (the CPU at reduced size, the GPU through torch at test size) and shares no code with the product
except the rotation seed set, which has tests of its own."""
import math

import torch

# ---- the fixture with no near-symmetry: three boxes of different lengths along the three axes, joined at one corner ---------------
BOXES = (((0.15, 0.0, 0.0), (0.25, 0.05, 0.05)), ((0.0, 0.09, 0.0), (0.05, 0.14, 0.05)), ((0.0, 0.0, 0.04), (0.05, 0.05, 0.09)))


def three_box_sdf(p: torch.Tensor) -> torch.Tensor:
    """Signed distance of the union of BOXES (centre, half extents): exact outside, a lower bound inside (min of box SDFs)."""
    out = None
    for c, h in BOXES:
        q = (p - torch.tensor(c, dtype=p.dtype, device=p.device)).abs() - torch.tensor(h, dtype=p.dtype, device=p.device)
        d = q.clamp(min=0).norm(dim=-1) + q.max(dim=-1).values.clamp(max=0)
        out = d if out is None else torch.minimum(out, d)
    return out


def sdf_mesh(sdf, resolution: int, device="cpu", bound=0.5):
    """mesh.marching_cubes of the zero level set of `sdf` over [-bound, bound]^3."""
    from dynhor_amd.mesh import marching_cubes
    N = int(resolution)
    ax = torch.linspace(-bound, bound, N, device=device)
    p = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)
    u = torch.cat([-sdf(p[s:s + (1 << 21)]) for s in range(0, p.shape[0], 1 << 21)])
    v, f = marching_cubes(u.view(N, N, N), 0.0, [-bound] * 3, [bound] * 3)
    return v, f


def three_box_mesh(resolution: int, device="cpu"):
    return sdf_mesh(three_box_sdf, resolution, device)


def mesh_area(v, f) -> float:
    t = v.double()[f]
    return float(0.5 * torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).norm(dim=1).sum())


def axis_angle(axis, deg) -> torch.Tensor:
    """Rotation matrix [3,3] fp64 about `axis` by `deg` degrees (Rodrigues, written out)."""
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    th = math.radians(deg)
    return torch.eye(3, dtype=torch.float64) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def moved(verts, s, R, t):
    """x' = s R x + t in fp64, as float32."""
    return (s * (verts.double().cpu() @ R.T) + t).float()


def inverse(s, R, t):
    """The similarity that undoes x' = s R x + t."""
    return 1.0 / s, R.T.clone(), -(R.T @ t) / s


def angle_deg(Ra, Rb) -> float:
    tr = float((Ra.double().cpu() * Rb.double().cpu()).sum())
    return math.degrees(math.acos(max(-1.0, min(1.0, (tr - 1.0) / 2.0))))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def ref_nearest(x, tgt, chunk=1024):
    """(d2 [N], idx [N]) of every row of x [N,3] against tgt [M,3], fp64, every pair (direct difference form)."""
    d, i = [], []
    for s in range(0, x.shape[0], chunk):
        dd = ((x[s:s + chunk, None, :] - tgt[None, :, :]) ** 2).sum(dim=-1)
        m = dd.min(dim=1)
        d.append(m.values); i.append(m.indices)
    return torch.cat(d), torch.cat(i)


def ref_umeyama(p, q, with_scale=True):
    """Umeyama 1991 from the pairs themselves: argmin sum |s R p + t - q|^2 (fp64)."""
    mp, mq = p.mean(dim=0), q.mean(dim=0)
    pc, qc = p - mp, q - mq
    cov = qc.T @ pc / p.shape[0]
    U, D, Vh = torch.linalg.svd(cov)
    S = torch.ones(3, dtype=torch.float64, device=p.device)
    if float(torch.linalg.det(U) * torch.linalg.det(Vh)) < 0:
        S[2] = -1.0
    R = U @ torch.diag(S) @ Vh
    s = float((D * S).sum() / pc.pow(2).sum(dim=1).mean()) if with_scale else 1.0
    return s, R, mq - s * (R @ mp)


def _rodrigues(w):
    th = float(w.norm())
    if th < 1e-300:
        return torch.eye(3, dtype=torch.float64, device=w.device)
    a = w / th
    K = torch.zeros(3, 3, dtype=torch.float64, device=w.device)
    K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -a[2], a[1], a[2], -a[0], -a[1], a[0]
    return torch.eye(3, dtype=torch.float64, device=w.device) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def ref_plane_step(x, q, n, s, R, t, origin, with_scale=True):
    """One Gauss-Newton step of sum (n . (x' - q))^2 with x' = origin + e^l Rot(w) (x - origin) + u, linearised at (w, u, l) = 0."""
    y = x - origin
    J = torch.cat([torch.linalg.cross(y, n), n, (n * y).sum(dim=1, keepdim=True)], dim=1)
    b = -(n * (x - q)).sum(dim=1)
    k = 7 if with_scale else 6
    d = torch.zeros(7, dtype=torch.float64, device=x.device)
    d[:k] = torch.linalg.lstsq((J[:, :k].T @ J[:, :k]).cpu(), (J[:, :k].T @ b).cpu()[:, None], rcond=1e-12, driver="gelsd").solution[:, 0].to(x.device)
    Rot, e = _rodrigues(d[:3]), math.exp(float(d[6]))
    return (s * e if with_scale else s), Rot @ R, origin + e * (Rot @ (t - origin)) + d[3:6]


def ref_icp(src, tgt, tgt_normals, s, R, t, with_scale=True, method="point", trim=0.9, max_iters=60, tol=1e-5):
    """The loop of mesh_align.icp for one hypothesis, in fp64 on the device of src.  Returns (s, R, t, stats) with stats iters,
    converged, last_step (the same bounding-sphere bound of the final update's displacement), residual."""
    dev = src.device
    src, tgt = src.double(), tgt.double()
    nrm = tgt_normals.double() if tgt_normals is not None else None
    R, t = R.double().to(dev), t.double().to(dev)
    s = float(s)
    n = src.shape[0]
    k = min(n, max(3, int(math.ceil(trim * n))))
    c_src, c_tgt = src.mean(dim=0), tgt.mean(dim=0)
    r_src, r_tgt = float((src - c_src).norm(dim=1).max()), float((tgt - c_tgt).norm(dim=1).max())
    iters, conv, last = 0, False, math.inf
    for _ in range(max_iters):
        x = s * (src @ R.T) + t
        d2, idx = ref_nearest(x, tgt)
        keep = d2 <= torch.kthvalue(d2, k).values
        if method == "plane":
            s1, R1, t1 = ref_plane_step(x[keep], tgt[idx[keep]], nrm[idx[keep]], s, R, t, c_tgt, with_scale)
        else:
            s1, R1, t1 = ref_umeyama(src[keep], tgt[idx[keep]], with_scale)
        dA = s1 * R1 - s * R
        last = float(torch.linalg.matrix_norm(dA, ord=2) * r_src + (dA @ c_src + t1 - t).norm())
        s, R, t = s1, R1, t1
        iters += 1
        if last <= tol * r_tgt:
            conv = True
            break
    x = s * (src @ R.T) + t
    d2, _ = ref_nearest(x, tgt)
    res = float(torch.topk(d2, k, largest=False).values.sqrt().mean())
    return s, R.cpu(), t.cpu(), {"iters": iters, "converged": conv, "last_step": last, "residual": res}


def ref_reverse_residual(src, tgt, s, R, t, trim=0.9):
    x = s * (src.double() @ R.double().to(src.device).T) + t.double().to(src.device)
    d2, _ = ref_nearest(tgt.double(), x)
    k = min(d2.shape[0], max(3, int(math.ceil(trim * d2.shape[0]))))
    return float(torch.topk(d2, k, largest=False).values.sqrt().mean())


def ref_align_global(src, tgt, tgt_normals, seeds_R, with_scale=True, method="plane", trim=0.9, coarse=(1024, 4096), coarse_iters=30,
                     n_refine=4, max_iters=60, tol=1e-5, second_min_deg=10.0):
    """init "global" restated: centroid / RMS-radius start, every seed rotation through the coarse point-to-point level on sample
    prefixes, the n_refine best by residual (one per basin: none within second_min_deg of a better one) refined on all samples,
    ranked by the two-sided residual.  Returns (s, R, t, stats) with
    residual, residual_two_sided, residual_second, and `refined`: the (start, end) transforms of every refined candidate."""
    s64, t64 = src.double(), tgt.double()
    cs, ct = s64.mean(dim=0), t64.mean(dim=0)
    s0 = float((t64 - ct).pow(2).sum(dim=1).mean().sqrt() / (s64 - cs).pow(2).sum(dim=1).mean().sqrt()) if with_scale else 1.0
    cands = []
    for Rk in seeds_R:
        Rk = Rk.double().to(src.device)
        cands.append(ref_icp(src[:coarse[0]], tgt[:coarse[1]], None, s0, Rk, ct - s0 * (Rk @ cs), with_scale, "point", trim, coarse_iters, tol))
    cands.sort(key=lambda c: c[3]["residual"])
    best = []                                                          # one candidate per basin
    for c in cands:
        if all(angle_deg(c[1], b[1]) > second_min_deg for b in best):
            best.append(c)
        if len(best) >= n_refine:
            break
    out = []
    for (s, R, t, _) in best:
        s1, R1, t1, st = ref_icp(src, tgt, tgt_normals, s, R, t, with_scale, method, trim, max_iters, tol)
        two = 0.5 * (st["residual"] + ref_reverse_residual(src, tgt, s1, R1, t1, trim))
        out.append((two, s1, R1, t1, st, (s, R, t)))
    out.sort(key=lambda c: c[0])
    two, s, R, t, st, _ = out[0]
    far = [c[0] for c in out[1:] if angle_deg(R, c[2]) > second_min_deg]
    stats = dict(st, residual_two_sided=two, residual_second=min(far) if far else None,
                 refined=[{"start": c[5], "end": (c[1], c[2], c[3]), "two_sided": c[0]} for c in out])
    return s, R, t, stats


def transform_gap(a, b, center, radius) -> float:
    """Upper bound of |x_a - x_b| over the ball (center, radius) for two similarities a = (s, R, t), b likewise: how far apart two
    registrations put the source (the same bound the stop rule uses for one update)."""
    (sa, Ra, ta), (sb, Rb, tb) = a, b
    dA = float(sa) * Ra.double().cpu() - float(sb) * Rb.double().cpu()
    c = torch.as_tensor(center, dtype=torch.float64).cpu()
    return float(torch.linalg.matrix_norm(dA, ord=2) * radius + (dA @ c + ta.double().cpu() - tb.double().cpu()).norm())


def ref_chamfer_l1(pred_v, pred_f, gt_v, gt_f, n, seed=0):
    """chamfer_l1 of metrics.mesh_metrics restated: n samples of each mesh from one generator (prediction first), the mean of the two
    directed mean nearest distances, fp64 brute force on the device of pred_v."""
    from dynhor_amd.metrics import sample_surface
    g = torch.Generator(device=pred_v.device).manual_seed(int(seed))
    p, _ = sample_surface(pred_v.float(), pred_f, n, g)
    q, _ = sample_surface(gt_v.float().to(pred_v.device), gt_f, n, g)
    a, _ = ref_nearest(p.double(), q.double())
    c, _ = ref_nearest(q.double(), p.double())
    return 0.5 * (float(a.sqrt().mean()) + float(c.sqrt().mean()))


def fma32(a, b, c):
    """fp32 fma(a, b, c), correctly rounded, restated in torch: the product of two fp32 numbers is exact in fp64, the sum is formed
    rounded to odd (TwoSum error term), and rounding that to fp32 is then a single correct rounding (53 >= 24 + 2)."""
    p = a.double() * b.double()
    cd = c.double()
    s = p + cd
    bb = s - p
    err = (p - (s - bb)) + (cd - bb)
    even = (s.view(torch.int64) & 1) == 0
    toward = torch.where(err > 0, torch.full_like(s, math.inf), torch.full_like(s, -math.inf))
    s = torch.where((err != 0) & even, torch.nextafter(s, toward), s)
    return s.float()


def transform32(p, xf):
    """The documented fp32 formula of dh_icp_correspond for one hypothesis (xf [12]: A row-major, then t):
    x_r = fma(A_r2, p.z, fma(A_r1, p.y, fma(A_r0, p.x, t_r)))."""
    rows = []
    for r in range(3):
        a0, a1, a2, t = (xf[3 * r].expand(p.shape[0]), xf[3 * r + 1].expand(p.shape[0]), xf[3 * r + 2].expand(p.shape[0]),
                         xf[9 + r].expand(p.shape[0]))
        rows.append(fma32(a2, p[:, 2], fma32(a1, p[:, 1], fma32(a0, p[:, 0], t))))
    return torch.stack(rows, dim=1).contiguous()
