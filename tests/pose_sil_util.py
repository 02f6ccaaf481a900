"""fp64 torch restatement of the silhouette pose loss (dynhor_amd/pose_sil.py, csrc/sil.hip): the yardstick of the pose_sil tests.

Everything is brute force and runs on the CPU: point-to-segment distances over all faces, a distance transform by pairwise distances,
autograd for the gradient, a plain Adam loop.  tests/test_cpu_pose_sil.py licenses it before anything is compared with it.

Per frame f (x_cam = R_f x + T_f, u = (K0 . x_cam) / z, w = (K1 . x_cam) / z, pixel centres at integer (u, w)):
  d2_j(p) = 0 where face j covers p (edge(a, b, p) = (b.u - a.u)(p.w - a.w) - (b.w - a.w)(p.u - a.u) of (v1,v2), (v2,v0), (v0,v1) all
            >= 0 or all <= 0, their sum != 0), else the squared distance to the nearest of its three edge segments; a face with a vertex
            at z <= 1e-3 or zero screen area is skipped;  d2 = min_j d2_j, j* the smallest face that attains it
  halo(x) = x <= (c sigma)^2 ? max(0, exp(-x / sigma^2) - exp(-c^2)) / (1 - exp(-c^2)) : 0        ((c sigma)^2 formed in fp32, as the kernel does)
  S = halo(d2);  M = halo(max(0, e - delta)^2), e the distance to the nearest pixel with label 1
  w = label >= 0 and no pixel with label -1 within c sigma;   L_sil = mean_f [ sum_p w (S - M)^2 / max(1, sum_p w) ]
  L_smooth = mean over (F - 1) V 3 of the squared difference of the posed vertices of consecutive frames
"""
import math

import numpy as np
import torch

F64 = torch.float64
FAR = float("inf")


def rot6d_to_matrix(x):
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    b3 = torch.linalg.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-1)


def matrix_to_rot6d(R):
    """rot6d of a saved pose R (object -> camera): the first two columns of R^T."""
    return R.transpose(1, 2)[:, :, :2].clone()


def poses_of(rot6d, trans):
    return rot6d_to_matrix(rot6d).transpose(1, 2), trans


def project(verts, R, T, K):
    """(uv [V,2], z [V]) of one frame."""
    cam = verts @ R.T + T.reshape(1, 3)
    z = cam[:, 2]
    u = (K[0, 0] * cam[:, 0] + K[0, 1] * cam[:, 1] + K[0, 2] * z) / z
    w = (K[1, 0] * cam[:, 0] + K[1, 1] * cam[:, 1] + K[1, 2] * z) / z
    return torch.stack([u, w], -1), z


def pixel_grid(H, W):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    return torch.stack([xx.reshape(-1), yy.reshape(-1)], -1)          # [P,2] = (u, w), row-major over (y, x)


def _edge(a, b, p):
    return (b[..., 0] - a[..., 0]) * (p[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (p[..., 0] - a[..., 0])


def seg_d2(a, b, p):
    """Squared distance from p to the segment a b (broadcast over leading dimensions)."""
    ab, ap = b - a, p - a
    den = (ab * ab).sum(-1)
    t = torch.where(den > 0, (ap * ab).sum(-1) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    t = t.clamp(0.0, 1.0)
    r = ap - t[..., None] * ab
    return (r * r).sum(-1)


def face_d2(tri, ok, p):
    """d2_j(p) [P,n] for screen triangles tri [n,3,2] (ok [n]: not skipped) and pixel centres p [P,2]; inf for a skipped face."""
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    q = p[:, None, :]
    e0, e1, e2 = _edge(b, c, q), _edge(c, a, q), _edge(a, b, q)
    cov = (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & ((e0 + e1 + e2) != 0)
    d = torch.minimum(torch.minimum(seg_d2(a, b, q), seg_d2(b, c, q)), seg_d2(c, a, q))
    d = torch.where(cov, torch.zeros_like(d), d)
    return torch.where(ok[None, :], d, torch.full_like(d, FAR))


def nearest(verts, faces, R, T, K, H, W, face_chunk=512):
    """(d2 [H,W] fp64, face [H,W] int64, -1 where no face is valid) of one frame, by brute force over all faces."""
    with torch.no_grad():
        uv, z = project(verts, R, T, K)
        tri, zt = uv[faces], z[faces]
        area = _edge(tri[:, 0], tri[:, 1], tri[:, 2])
        ok = (zt > 1e-3).all(-1) & torch.isfinite(tri).all(-1).all(-1) & (area != 0)
        p = pixel_grid(H, W)
        best = torch.full((H * W,), FAR, dtype=F64)
        arg = torch.full((H * W,), -1, dtype=torch.int64)
        for s in range(0, faces.shape[0], face_chunk):
            d = face_d2(tri[s:s + face_chunk], ok[s:s + face_chunk], p)
            m = d.min(dim=1).values
            first = (d == m[:, None]).to(torch.int8).argmax(dim=1) + s       # argmax returns the first maximal index
            better = m < best
            best = torch.where(better, m, best)
            arg = torch.where(better, first, arg)
        return best.view(H, W), arg.view(H, W)


def edt_exact(label, value):
    """[F,H,W] fp64: the exact Euclidean distance SQUARED to the nearest pixel with label == value (inf when the frame has none)."""
    F, H, W = label.shape
    p = pixel_grid(H, W)
    out = torch.full((F, H * W), FAR, dtype=F64)
    for f in range(F):
        src = p[(label[f].reshape(-1) == value)]
        if src.shape[0]:
            out[f] = (torch.cdist(p, src) ** 2).min(dim=1).values.round()
    return out.view(F, H, W)


def edt_window(label, value, rmax):
    """[F,H,W] fp32: min of dx^2 + dy^2 over |dx|, |dy| <= rmax (clipped to the image) with label == value, inf where there is none."""
    F, H, W = label.shape
    hit = label == value
    out = torch.full((F, H, W), FAR, dtype=torch.float32)
    for dy in range(-rmax, rmax + 1):
        for dx in range(-rmax, rmax + 1):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            cand = torch.where(hit[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx], float(dx * dx + dy * dy), FAR).to(torch.float32)
            out[:, y0:y1, x0:x1] = torch.minimum(out[:, y0:y1, x0:x1], cand)
    return out


def halo_consts(sigma, cut):
    """(cs2 formed in fp32 as the kernel forms it, sigma^2, exp(-cut^2))."""
    cs = np.float32(cut) * np.float32(sigma)
    return float(np.float32(cs * cs)), float(np.float32(sigma)) ** 2, math.exp(-float(np.float32(cut)) ** 2)


def halo(x, sigma, cut):
    cs2, s2, ec = halo_consts(sigma, cut)
    h = (torch.exp(-x / s2) - ec).clamp(min=0.0) / (1.0 - ec)
    return torch.where(x <= cs2, h, torch.zeros_like(h))


def target_and_weight(label, sigma, cut, delta, d2_obj=None, d2_hand=None):
    """(M [F,H,W], w [F,H,W]) fp64 of the label maps i8 [F,H,W]."""
    d2_obj = edt_exact(label, 1) if d2_obj is None else d2_obj.to(F64)
    d2_hand = edt_exact(label, -1) if d2_hand is None else d2_hand.to(F64)
    cs2 = halo_consts(sigma, cut)[0]
    e = (d2_obj.sqrt() - float(np.float32(delta))).clamp(min=0.0)
    M = halo(e * e, sigma, cut)
    w = ((label >= 0) & ~(d2_hand <= cs2)).to(F64)
    return M, w


def soft_silhouette(verts, faces, R, T, K, H, W, sigma, cut):
    """(S [H,W] differentiable w.r.t. R, T; d2 [H,W]; face [H,W]) of one frame: the winning face comes from the brute-force search, the
    distance to it is then recomputed with autograd, so the gradient reaches one face per pixel."""
    d2, face = nearest(verts, faces, R.detach(), T.detach(), K, H, W)
    uv, _ = project(verts, R, T, K)
    band = ((d2 > 0) & torch.isfinite(d2) & (face >= 0)).reshape(-1)
    S = (d2 == 0).to(F64).reshape(-1)
    if band.any():
        p = pixel_grid(H, W)[band]
        tri = uv[faces[face.reshape(-1)[band]]]                              # [n,3,2]
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        d = torch.stack([seg_d2(a, b, p), seg_d2(b, c, p), seg_d2(c, a, p)], -1).min(dim=-1).values
        S = S.index_put((band.nonzero().reshape(-1),), halo(d, sigma, cut))
    return S.view(H, W), d2, face


def sil_terms(verts, faces, R, T, K, label, sigma, cut=3.0, delta=0.5, M=None, w=None):
    """(num [F], weight [F], counts int64 [F,3]) with num differentiable: sum_p w (S - M)^2, sum_p w and (tp, fp, fn)."""
    F, H, W = label.shape
    if M is None or w is None:
        M, w = target_and_weight(label, sigma, cut, delta)
    nums, wts, counts = [], [], []
    for f in range(F):
        S, d2, _ = soft_silhouette(verts, faces, R[f], T[f], K, H, W, sigma, cut)
        nums.append((w[f] * (S - M[f]) ** 2).sum())
        wts.append(w[f].sum())
        cov, lab = d2 == 0, label[f]
        counts.append(torch.stack([(cov & (lab == 1)).sum(), (cov & (lab == 0)).sum(), (~cov & (lab == 1)).sum()]))
    return torch.stack(nums), torch.stack(wts), torch.stack(counts)


def sil_loss(verts, faces, rot6d, trans, K, label, sigma, cut=3.0, delta=0.5, M=None, w=None):
    R, T = poses_of(rot6d, trans)
    num, wt, counts = sil_terms(verts, faces, R, T, K, label, sigma, cut, delta, M, w)
    return (num / wt.clamp(min=1.0)).mean(), counts


def smooth_direct(verts, R, T):
    posed = torch.einsum("frc,vc->fvr", R, verts) + T[:, None, :]
    return ((posed[1:] - posed[:-1]) ** 2).mean()


def smooth_moments(verts, R, T):
    V = verts.shape[0]
    M2, m1 = verts.T @ verts, verts.sum(0)
    A, b = R[1:] - R[:-1], T[1:] - T[:-1]
    tot = torch.einsum("fij,jk,fik->", A, M2, A) + 2.0 * torch.einsum("fi,fij,j->", b, A, m1) + V * (b * b).sum()
    return tot / ((R.shape[0] - 1) * V * 3)


def iou(counts):
    c = counts.to(F64)
    return c[:, 0] / c.sum(dim=1).clamp(min=1.0)


def reprojection_error(verts, R, T, R_true, T_true, K):
    """Mean distance in pixels between the vertices projected with (R, T) and with the true poses, per frame [F]."""
    out = []
    for f in range(R.shape[0]):
        a, _ = project(verts, R[f], T[f], K)
        b, _ = project(verts, R_true[f], T_true[f], K)
        out.append((a - b).norm(dim=-1).mean())
    return torch.stack(out)


def sigma_at(k, iters, sigma0, sigma1):
    return float(sigma0) if iters <= 1 else float(sigma0) * (float(sigma1) / float(sigma0)) ** (k / (iters - 1))


def refine(verts, faces, R0, T0, K, label, iters, lr, rot_lr_mult=10.0, sigma_px=4.0, sigma_end_px=1.5, cut=3.0, delta=0.5,
           lw_sil=1.0, lw_smooth=0.0, active=None, log=None):
    """A plain Adam loop over (rot6d, trans) on L = lw_sil L_sil + lw_smooth L_smooth with sigma annealed geometrically.  Returns
    (R, T, curve) with curve = [(iteration, sigma, L_sil, L_smooth)]."""
    rot6d = matrix_to_rot6d(R0.to(F64)).requires_grad_(True)
    trans = T0.to(F64).reshape(-1, 3).clone().requires_grad_(True)
    F = label.shape[0]
    act = torch.ones(F, dtype=torch.bool) if active is None else active
    idx = act.nonzero().reshape(-1)
    d2o, d2h = edt_exact(label[idx], 1), edt_exact(label[idx], -1)
    state = [(torch.zeros_like(p), torch.zeros_like(p)) for p in (rot6d, trans)]
    b1, b2, eps = 0.9, 0.999, 1e-8
    curve = []
    for k in range(iters):
        sigma = sigma_at(k, iters, sigma_px, sigma_end_px)
        M, w = target_and_weight(label[idx], sigma, cut, delta, d2o, d2h)
        R, T = poses_of(rot6d, trans)
        num, wt, _ = sil_terms(verts, faces, R[idx], T[idx], K, label[idx], sigma, cut, delta, M, w)
        l_sil = (num / wt.clamp(min=1.0)).mean()
        l_sm = smooth_moments(verts, R, T) if F > 1 else torch.zeros((), dtype=F64)
        loss = lw_sil * l_sil + lw_smooth * l_sm
        g = torch.autograd.grad(loss, (rot6d, trans), allow_unused=True)
        curve.append((k, sigma, float(l_sil.detach()), float(l_sm.detach())))
        if log is not None:
            log(curve[-1])
        with torch.no_grad():
            for p, gi, (m, v), step in zip((rot6d, trans), g, state, (lr * rot_lr_mult, lr)):
                gi = torch.zeros_like(p) if gi is None else gi * act.to(F64).view(-1, *([1] * (p.dim() - 1)))
                m.mul_(b1).add_(gi, alpha=1 - b1)
                v.mul_(b2).addcmul_(gi, gi, value=1 - b2)
                p.sub_(step * (m / (1 - b1 ** (k + 1))) / ((v / (1 - b2 ** (k + 1))).sqrt() + eps))
    R, T = poses_of(rot6d.detach(), trans.detach())
    return R, T, curve


# ---------------------------------------------------------------------------------------------------------------- small test scenes
def bent_ellipsoid(n_lat=9, n_lon=18):
    """An asymmetric closed shape of 2 n_lon (n_lat - 1) faces: an ellipsoid (radii 0.45, 0.28, 0.2) bent along x and bulged on one side."""
    vs = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2.0 * math.pi * j / n_lon
            vs.append((math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)))
    vs.append((0.0, 0.0, -1.0))
    v = torch.tensor(vs, dtype=F64)
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    fs = []
    for j in range(n_lon):
        fs.append((0, ring(1, j), ring(1, j + 1)))
        fs.append((len(vs) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            fs.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            fs.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    bulge = 1.0 + 0.35 * torch.exp(-((x - 0.6) ** 2 + (y - 0.5) ** 2) * 3.0)
    out = torch.stack([0.45 * x, 0.28 * y * bulge + 0.25 * (0.45 * x) ** 2 / 0.45, 0.2 * z * (1.0 + 0.3 * x)], -1)
    return out, torch.tensor(fs, dtype=torch.int64)


def look_at(pos, up=(0.0, 1.0, 0.2)):
    """(R [3,3], T [3]) of a camera at `pos` looking at the origin (x_cam = R x + T, z forward)."""
    pos = torch.as_tensor(pos, dtype=F64)
    fwd = -pos / pos.norm()
    right = torch.linalg.cross(fwd, torch.as_tensor(up, dtype=F64))
    right = right / right.norm()
    down = torch.linalg.cross(fwd, right)
    R = torch.stack([right, down, fwd])
    return R, -R @ pos


def axis_angle(axis, deg):
    a = torch.as_tensor(axis, dtype=F64)
    a = a / a.norm()
    Kx = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=F64)
    t = math.radians(deg)
    return torch.eye(3, dtype=F64) + math.sin(t) * Kx + (1.0 - math.cos(t)) * (Kx @ Kx)


def render_labels(verts, faces, R, T, K, H, W, hand=True):
    """label i8 [F,H,W]: 1 where the mesh covers the pixel centre at the given poses, a hand rectangle (-1) over part of the outline
    (the object wins where they overlap, as in Dataset.label), 0 elsewhere."""
    F = R.shape[0]
    lab = torch.zeros(F, H, W, dtype=torch.int8)
    for f in range(F):
        d2, _ = nearest(verts, faces, R[f], T[f], K, H, W)
        obj = d2 == 0
        if hand:
            ys, xs = obj.nonzero(as_tuple=True)
            cx, cy = int(xs.max()), int(ys.to(F64).mean())
            hh, hw = max(2, H // 8), max(2, W // 6)
            lab[f, max(0, cy - hh // 2 + 3 * f):min(H, cy + hh // 2 + 3 * f), max(0, cx - hw // 2):min(W, cx + hw // 2)] = -1
        lab[f][obj] = 1
    return lab


def small_scene(n_frames=4, H=96, W=96, seed=3, rot_deg=8.0, shift=(0.06, 0.12), hand=True, n_lat=9, n_lon=18):
    """A reduced pose problem: the bent ellipsoid seen from n_frames cameras on an arc, its labels rendered at the TRUE poses, and start
    poses off by rot_deg about random axes and by a translation of a length drawn from `shift`."""
    g = torch.Generator().manual_seed(seed)
    verts, faces = bent_ellipsoid(n_lat, n_lon)
    K = torch.tensor([[1.1 * W, 0.0, (W - 1) / 2.0], [0.0, 1.1 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]], dtype=F64)
    Rs, Ts = [], []
    for f in range(n_frames):
        az = math.radians(-40.0 + 80.0 * f / max(1, n_frames - 1))
        R, T = look_at((1.6 * math.sin(az), 0.35, 1.6 * math.cos(az)))
        Rs.append(R); Ts.append(T)
    R_true, T_true = torch.stack(Rs), torch.stack(Ts)
    label = render_labels(verts, faces, R_true, T_true, K, H, W, hand=hand)
    R0, T0 = [], []
    for f in range(n_frames):
        axis = torch.randn(3, generator=g, dtype=F64)
        dirn = torch.randn(3, generator=g, dtype=F64)
        dirn = dirn / dirn.norm()
        length = shift[0] + (shift[1] - shift[0]) * float(torch.rand((), generator=g, dtype=F64))
        dR = axis_angle(axis, rot_deg)
        R0.append(R_true[f] @ dR)
        T0.append(T_true[f] + length * dirn * torch.tensor([1.0, 1.0, 0.5], dtype=F64))
    return {"verts": verts, "faces": faces, "K": K, "label": label, "R_true": R_true, "T_true": T_true, "R0": torch.stack(R0),
            "T0": torch.stack(T0), "H": H, "W": W}
