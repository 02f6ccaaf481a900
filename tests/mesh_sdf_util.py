"""Restatement of the mesh distance tests' mathematics in plain torch (fp64 unless a dtype is given; fp32 gives the "float32
restatement" whose own deviation from fp64 sets the tolerances): closest point on a triangle by its seven regions, the solid-angle
sum of the generalised winding number, the closed-form box distance, the warm start's loss.  Shares no code with dynhor_amd.
Everything is a dense [N, F] tensor expression, evaluated in chunks of points; it runs on whatever device the inputs are on."""
import math

import torch


def _dot(a, b):
    return (a * b).sum(-1)


def closest_on_triangles(p, a, b, c):
    """Closest point of each triangle (a, b, c [F,3]) to each point p [N,3]: (q [N,F,3], region [N,F]) with region 0 / 1 / 2 = the
    corners a / b / c, 3 / 4 / 5 = the edges ab / ac / bc, 6 = the interior.  The textbook region walk (Ericson, Real-Time Collision
    Detection 5.1.5), every branch evaluated and the first that holds kept."""
    p = p[:, None, :]
    ab, ac = (b - a)[None], (c - a)[None]
    ap = p - a[None]
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b[None]
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c[None]
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    one = torch.ones_like(d1)

    def safe(num, den):
        return num / torch.where(den == 0, one, den)

    cand = [
        (d1 <= 0) & (d2 <= 0), a[None].expand_as(ap),
        (d3 >= 0) & (d4 <= d3), b[None].expand_as(ap),
        (d6 >= 0) & (d5 <= d6), c[None].expand_as(ap),
        (vc <= 0) & (d1 >= 0) & (d3 <= 0), a[None] + safe(d1, d1 - d3)[..., None] * ab,
        (vb <= 0) & (d2 >= 0) & (d6 <= 0), a[None] + safe(d2, d2 - d6)[..., None] * ac,
        (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b[None] + safe(d4 - d3, (d4 - d3) + (d5 - d6))[..., None] * (c - b)[None],
    ]
    den = safe(one, va + vb + vc)
    q = a[None] + (vb * den)[..., None] * ab + (vc * den)[..., None] * ac
    region = torch.full(d1.shape, 6, dtype=torch.int64, device=d1.device)
    # Ericson's order of tests: a, b, ab, c, ac, bc -- apply them in reverse so that the earliest holds
    for k in (5, 4, 2, 3, 1, 0):
        m, qk = cand[2 * k], cand[2 * k + 1]
        q = torch.where(m[..., None], qk, q)
        region = torch.where(m, torch.full_like(region, k), region)
    return q, region


def solid_angles(p, a, b, c):
    """Signed solid angle [N,F] of every triangle seen from every point (Van Oosterom & Strackee)."""
    A, B, C = a[None] - p[:, None], b[None] - p[:, None], c[None] - p[:, None]
    la, lb, lc = A.norm(dim=-1), B.norm(dim=-1), C.norm(dim=-1)
    det = _dot(A, torch.cross(B, C, dim=-1))
    den = la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb
    return 2.0 * torch.atan2(det, den)


def mesh_distance(pts, verts, faces, dtype=torch.float64, chunk=512, skip=None):
    """(dist [N], face [N] the lowest index of the minimum, wind [N], dist_to_face [N,F] if the mesh is small else None) in `dtype`.
    skip: bool [F], faces left out of the distance (set to +inf) and of the winding sum."""
    p = pts.to(dtype)
    v = verts.to(dtype)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    F = faces.shape[0]
    keep_all = F <= 400
    dist, face, wind, full = [], [], [], []
    for s in range(0, p.shape[0], chunk):
        pc = p[s:s + chunk]
        q, _ = closest_on_triangles(pc, a, b, c)
        d = (pc[:, None, :] - q).norm(dim=-1)
        om = solid_angles(pc, a, b, c)
        if skip is not None:
            d = torch.where(skip[None], torch.full_like(d, float("inf")), d)
            om = torch.where(skip[None], torch.zeros_like(om), om)
        m, i = d.min(dim=1)
        # torch.min gives no promise about ties: take the lowest index that attains the minimum
        i = (d == m[:, None]).to(torch.int8).argmax(dim=1)
        dist.append(m); face.append(i)
        wind.append(om.to(torch.float64).sum(dim=1) / (4.0 * math.pi))
        if keep_all:
            full.append(d)
    return torch.cat(dist), torch.cat(face), torch.cat(wind), (torch.cat(full) if keep_all else None)


def distance_to_faces(pts, verts, faces, idx, dtype=torch.float64):
    """dist [N] of point i to face idx[i] alone."""
    p = pts.to(dtype)
    v = verts.to(dtype)
    f = faces[idx]
    out = []
    for s in range(0, p.shape[0], 4096):
        a, b, c = v[f[s:s + 4096, 0]], v[f[s:s + 4096, 1]], v[f[s:s + 4096, 2]]
        pc = p[s:s + 4096]
        q = _closest_pairwise(pc, a, b, c)
        out.append((pc - q).norm(dim=-1))
    return torch.cat(out)


def _closest_pairwise(p, a, b, c):
    """closest_on_triangles for point i against triangle i only ([N,3] each): through the same function, one face at a time would be
    slow, so the points are shifted into each triangle's frame and the [N,1] problem is batched by treating N as the face axis."""
    # p_i against triangle i == origin against triangle (a_i - p_i, b_i - p_i, c_i - p_i)
    z = torch.zeros(1, 3, dtype=p.dtype, device=p.device)
    q, _ = closest_on_triangles(z, a - p, b - p, c - p)
    return q[0] + p


def box_sdf(p, center, half):
    """Closed-form signed distance to an axis-aligned box."""
    q = (p - center).abs() - half
    return q.clamp(min=0).norm(dim=-1) + q.max(dim=-1).values.clamp(max=0)


def cube_mesh(center=(0.05, -0.03, 0.02), half=0.3):
    """(verts [8,3] float32, faces [12,3] int64): an axis-aligned cube, faces wound counter-clockwise seen from outside."""
    cx, cy, cz = center
    v = [(cx + sx * half, cy + sy * half, cz + sz * half) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    # vertex index = 4 * (x > 0) + 2 * (y > 0) + (z > 0)
    f = [(0, 1, 3), (0, 3, 2),      # x = -h
         (4, 6, 7), (4, 7, 5),      # x = +h
         (0, 4, 5), (0, 5, 1),      # y = -h
         (2, 3, 7), (2, 7, 6),      # y = +h
         (0, 2, 6), (0, 6, 4),      # z = -h
         (1, 5, 7), (1, 7, 3)]      # z = +h
    return torch.tensor(v, dtype=torch.float32), torch.tensor(f, dtype=torch.int64)


def sample_points(verts, faces, n, seed):
    """The tests' point mix, [n,3] float32 on the CPU: the first 32 vertices and the first 32 face centroids exactly (as many as the
    mesh and n allow), then thirds of uniform-ball samples (radius 1) and surface samples displaced by sigma = 0.01 and 0.05."""
    g = torch.Generator().manual_seed(seed)
    v = verts.double()
    tri = v[faces]
    exact = torch.cat([v[:32], tri[:32].mean(dim=1)])[:max(0, min(64, n // 2))]
    m = n - exact.shape[0]
    nb = m - 2 * (m // 3)
    d = torch.randn(nb, 3, generator=g, dtype=torch.float64)
    ball = d / d.norm(dim=-1, keepdim=True) * torch.rand(nb, 1, generator=g, dtype=torch.float64) ** (1.0 / 3.0)
    area = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1).norm(dim=-1)
    area = torch.where(area > 0, area, torch.full_like(area, 1e-30))
    parts = [exact, ball]
    for sigma in (0.01, 0.05):
        k = m // 3
        fi = torch.multinomial(area / area.sum(), k, replacement=True, generator=g)
        u = torch.rand(k, 2, generator=g, dtype=torch.float64)
        su = u[:, :1].sqrt()
        bary = torch.cat([1 - su, su * (1 - u[:, 1:]), su * u[:, 1:]], dim=1)
        s = (tri[fi] * bary[..., None]).sum(dim=1)
        parts.append(s + sigma * torch.randn(k, 3, generator=g, dtype=torch.float64))
    return torch.cat(parts).float()[:n].contiguous()


def fit_loss(sdf_net, grad_net, sdf_mesh, eik_weight):
    """The warm start's loss: mean |sdf_net - sdf_mesh| + eik_weight * mean (|grad| - 1)^2."""
    return (sdf_net.reshape(-1) - sdf_mesh.reshape(-1)).abs().mean() + eik_weight * ((grad_net.norm(dim=-1) - 1.0) ** 2).mean()
