"""Shared by tests/test_cpu_mesh_texture.py and tests/test_gpu_mesh_texture.py: small scenes, an fp64 brute-force z-buffer, and fp64
restatements of dh_texture_bake and dh_mesh_shade_tex in plain torch.  Everything here runs on CPU and device tensors alike, so the
restatement's own properties (the share of ambiguous texels, the PSNR it reaches) are checked without a GPU."""
import math

import torch

# tolerances within which a decision of the bake counts as ambiguous between fp32 and fp64
TOL_Z = 1e-6           # camera depth against 1e-3
TOL_DEPTH = 1e-5       # camera depth against z-buffer depth + depth_eps
TOL_COS = 2e-6         # cosine against min_cos
TOL_PX = 1e-4          # pixel coordinates against an image border or a nearest-pixel boundary, plus TOL_POINT * f / z
TOL_POINT = 1e-6       # the fp32 error of the interpolated surface point (three weights of ~3 ulp on |v| <= 0.5), times 3


def cameras(n, H, W, radius=2.5, seed=0, device="cpu"):
    """n look-at cameras on a sphere of `radius` (Fibonacci directions, jittered), intrinsics f = 1.2 min(H, W)."""
    from dynhor_amd.scene import look_at_pose
    Rs, Ts = [], []
    g = torch.Generator().manual_seed(seed)
    for i in range(n):
        z = 1 - 2 * (i + 0.5) / n
        phi = i * math.pi * (3 - math.sqrt(5)) + float(torch.rand(1, generator=g))
        d = torch.tensor([math.sqrt(1 - z * z) * math.cos(phi), math.sqrt(1 - z * z) * math.sin(phi), z])
        R, T = look_at_pose(d * radius, up=torch.tensor([0.0, 0.0, 1.0]) if abs(z) < 0.95 else torch.tensor([1.0, 0.0, 0.0]))
        Rs.append(R); Ts.append(T)
    f = 1.2 * min(H, W)
    K = torch.tensor([[f, 0, W // 2], [0, f, H // 2], [0, 0, 1]], dtype=torch.float32)
    return torch.stack(Rs).float().to(device), torch.stack(Ts).float().to(device), K.to(device)


def camera_at(pos, device="cpu"):
    """(R [1,3,3], T [1,3]) of one look-at camera at `pos` looking at the origin."""
    from dynhor_amd.scene import look_at_pose
    R, T = look_at_pose(torch.tensor(pos, dtype=torch.float32), up=torch.tensor([0.0, 0.0, 1.0]))
    return R[None].float().to(device), T[None].float().to(device)


def sphere_mesh(center, r, N=20, device="cpu", drop_last=False):
    """Marching-cubes sphere on an N^3 grid; drop_last removes one face (an odd face count)."""
    from dynhor_amd.mesh import marching_cubes
    lo, hi = [c - r * 1.2 for c in center], [c + r * 1.2 for c in center]
    ax = [torch.linspace(lo[i], hi[i], N, device=device) for i in range(3)]
    gx, gy, gz = torch.meshgrid(*ax, indexing="ij")
    p = torch.stack([gx, gy, gz], -1)
    v, f = marching_cubes(r - torch.linalg.norm(p - torch.tensor(center, device=device), dim=-1), 0.0, lo, hi)
    if drop_last:
        f = f[:-1]
    return v.float().contiguous(), f.long().contiguous()


def smooth_noisy_frames(F, H, W, seed=0, noise=4, device="cpu"):
    """u8 [F,H,W,3]: low-frequency waves (at most ~2 levels per pixel) plus uniform integer noise in [-noise, noise]."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    out = torch.empty(F, H, W, 3, dtype=torch.float64)
    for f in range(F):
        for k in range(3):
            a, b, c = (torch.rand(3, generator=g) * 0.08 + 0.02).tolist()
            out[f, ..., k] = 128 + 55 * torch.sin(a * xs + 0.7 * f + k) * torch.cos(b * ys - 0.3 * k) + 40 * torch.sin(c * (xs + ys))
    out = out + torch.randint(-noise, noise + 1, out.shape, generator=g).double()
    return out.round().clamp(0, 255).to(torch.uint8).to(device)


# ------------------------------------------------------------------------------------------------ atlas
def bilinear_taps(s, t):
    """The four (column, row) taps of a bilinear fetch at (s, t) in texel units: floor(s - 0.5) and + 1, likewise t.  [n,4,2] int64."""
    i0, j0 = torch.floor(s - 0.5).long(), torch.floor(t - 0.5).long()
    return torch.stack([torch.stack([i0, j0], -1), torch.stack([i0 + 1, j0], -1), torch.stack([i0, j0 + 1], -1),
                        torch.stack([i0 + 1, j0 + 1], -1)], 1)


# ------------------------------------------------------------------------------------------------ z-buffer
def _edge(au, aw, bu, bw, pu, pw):
    return (bu - au) * (pw - aw) - (bw - aw) * (pu - au)


def project64(v, R, T, K):
    c = v @ R.double().T + T.double()
    z = c[..., 2]
    return c, z, (c @ K[0].double()) / z, (c @ K[1].double()) / z


def raster_fp64(verts, faces, R, T, K, H, W):
    """int64 [F,H,W] keys in dh_mesh_raster_depth's format ((float32 bits of the depth) << 32 | face, -1 where empty), by brute force in
    fp64: the nearest face whose screen triangle covers the pixel centre (faces with a vertex at z <= 1e-3 or no area skipped)."""
    v = verts.double()
    dev = verts.device
    out = torch.full((R.shape[0], H, W), -1, dtype=torch.int64, device=dev)
    xs = torch.arange(W, device=dev, dtype=torch.float64)
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    for f in range(R.shape[0]):
        _, z, u, w = project64(v, R[f], T[f], K)
        ok = (z[a] > 1e-3) & (z[b] > 1e-3) & (z[c] > 1e-3) & (_edge(u[a], w[a], u[b], w[b], u[c], w[c]) != 0)
        for y in range(H):
            px, py = xs[:, None], torch.full((W, 1), float(y), dtype=torch.float64, device=dev)
            e0 = _edge(u[b], w[b], u[c], w[c], px, py)
            e1 = _edge(u[c], w[c], u[a], w[a], px, py)
            e2 = _edge(u[a], w[a], u[b], w[b], px, py)
            cov = ok & (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & ((e0 + e1 + e2) != 0)
            depth = (e0 + e1 + e2) / (e0 / z[a] + e1 / z[b] + e2 / z[c])
            depth = torch.where(cov, depth, torch.full_like(depth, float("inf")))
            dm, arg = depth.min(dim=1)
            key = (dm.float().view(torch.int32).long() << 32) | arg
            out[f, y] = torch.where(torch.isfinite(dm), key, torch.full_like(key, -1))
    return out


def zbuf_depth64(zbuf):
    d = (zbuf >> 32).to(torch.int32).view(torch.float32).double()
    return torch.where(zbuf == -1, torch.full_like(d, float("inf")), d)


# ------------------------------------------------------------------------------------------------ bake
def texel_geometry64(verts, normals, faces, uv, owner):
    """(index of the texels dh_texture_bake works on, their points [n,3] and normals [n,3] in fp64)."""
    S = owner.shape[0]
    nf, nv = faces.shape[0], verts.shape[0]
    o = owner.reshape(-1).long()
    oc = o.clamp(0, max(nf - 1, 0))
    tri = faces[oc]
    t = uv.double()[oc]
    area = _edge(t[:, 0, 0], t[:, 0, 1], t[:, 1, 0], t[:, 1, 1], t[:, 2, 0], t[:, 2, 1])
    act = (o >= 0) & (o < nf) & ((tri >= 0) & (tri < nv)).all(1) & (area != 0)
    idx = act.nonzero().squeeze(1)
    t, tri, area = t[idx], tri[idx], area[idx]
    qx, qy = (idx % S).double() + 0.5, (idx // S).double() + 0.5
    b = torch.stack([_edge(t[:, 1, 0], t[:, 1, 1], t[:, 2, 0], t[:, 2, 1], qx, qy),
                     _edge(t[:, 2, 0], t[:, 2, 1], t[:, 0, 0], t[:, 0, 1], qx, qy),
                     _edge(t[:, 0, 0], t[:, 0, 1], t[:, 1, 0], t[:, 1, 1], qx, qy)], -1) / area[:, None]
    b = b.clamp(min=0.0)
    b = b / b.sum(-1, keepdim=True)
    p = (b[:, :, None] * verts.double()[tri]).sum(1)
    n = (b[:, :, None] * normals.double()[tri]).sum(1)
    return idx, p, n


def bilinear64(img, u, w):
    """Bilinear fetch of img [H,W,3] (any dtype) / 255 at pixel coordinates (u, w), pixel centres at integers, 0 <= u <= W - 1."""
    H, W = img.shape[0], img.shape[1]
    x0, y0 = torch.floor(u).long(), torch.floor(w).long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    fx, fy = (u - x0)[:, None], (w - y0)[:, None]
    im = img.double()
    top = im[y0, x0] * (1 - fx) + im[y0, x1] * fx
    bot = im[y1, x0] * (1 - fx) + im[y1, x1] * fx
    return (top * (1 - fy) + bot * fy) / 255.0


def bake_fp64(verts, normals, faces, uv, owner, rgb, usable, zbuf, R, T, K, depth_eps=0.01, min_cos=0.1, sharpen=2):
    """dh_texture_bake restated in fp64 on the given z-buffer: (acc f64 [S,S,4], n_views int64 [S,S], ambiguous bool [S,S], worked
    bool [S,S]).  ambiguous: some decision of some frame lies within its tolerance (module constants) of its threshold."""
    S = owner.shape[0]
    dev = verts.device
    F, H, W = usable.shape
    idx, p, n = texel_geometry64(verts, normals, faces, uv, owner)
    nlen = n.norm(dim=1)
    acc = torch.zeros(idx.shape[0], 4, dtype=torch.float64, device=dev)
    cnt = torch.zeros(idx.shape[0], dtype=torch.int64, device=dev)
    amb = torch.zeros(idx.shape[0], dtype=torch.bool, device=dev)
    depth = zbuf_depth64(zbuf)
    fpx = float(max(K[0, 0], K[1, 1]))
    for f in range(F):
        _, z, u, w = project64(p, R[f], T[f], K)
        front = z > 1e-3
        ins = front & (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1)
        us, ws = torch.where(ins, u, torch.zeros_like(u)), torch.where(ins, w, torch.zeros_like(w))
        px, py = torch.floor(us + 0.5).long(), torch.floor(ws + 0.5).long()
        dz = depth[f, py, px]
        C = -(R[f].double().T @ T[f].double())
        d = C - p
        cs = (n * d).sum(1) / d.norm(dim=1) / nlen
        seen = ins & (usable[f, py, px] != 0) & torch.isfinite(dz)
        vis = seen & (z <= dz + depth_eps) & (cs >= min_cos)
        tol = TOL_PX + TOL_POINT * fpx / z.abs().clamp(min=1e-9)
        near = lambda q: (q - q.round()).abs() < tol
        border = ((u.abs() < tol) | ((u - (W - 1)).abs() < tol) | (w.abs() < tol) | ((w - (H - 1)).abs() < tol))
        amb |= ((z - 1e-3).abs() < TOL_Z) | (front & border) | (ins & (near(u + 0.5) | near(w + 0.5))) | \
               (seen & ((z - dz - depth_eps).abs() < TOL_DEPTH)) | (seen & ((cs - min_cos).abs() < TOL_COS))
        wgt = cs.clone()
        for _ in range(int(sharpen)):
            wgt = wgt * wgt
        col = bilinear64(rgb[f], us, ws)
        acc[:, :3] += torch.where(vis[:, None], wgt[:, None] * col, torch.zeros_like(col))
        acc[:, 3] += torch.where(vis, wgt, torch.zeros_like(wgt))
        cnt += vis

    def full(x, fill):
        out = torch.full((S * S,) + tuple(x.shape[1:]), fill, dtype=x.dtype, device=dev)
        out[idx] = x
        return out.view((S, S) + tuple(x.shape[1:]))

    worked = torch.zeros(S * S, dtype=torch.bool, device=dev)
    worked[idx] = True
    return full(acc, 0.0), full(cnt, 0), full(amb, False), worked.view(S, S)


def texture_from_sums(acc, n_views, owner, grey=0.5):
    """u8 [S,S,3] as mesh_texture.bake_texture forms it in mode "views" from (acc, n_views)."""
    seen = n_views > 0
    col = torch.where(seen[..., None], acc[..., :3] / acc[..., 3:], torch.zeros_like(acc[..., :3]))
    col[(owner >= 0) & ~seen] = grey
    return (col.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8)


# ------------------------------------------------------------------------------------------------ textured shade
def shade_tex_fp64(verts, normals, faces, uv, tex, zbuf, R, T, K, rgb=None, alpha=1.0, lit=False):
    """dh_mesh_shade_tex restated in fp64 on the given z-buffer: (255 o before rounding, f64 [F,H,W,3]; covered bool [F,H,W])."""
    dev = verts.device
    F, H, W = zbuf.shape
    nf, nv = faces.shape[0], verts.shape[0]
    Sh, Sw = tex.shape[0], tex.shape[1]
    v, nr, t, tx = verts.double(), normals.double(), uv.double(), tex.double()
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                            indexing="ij")
    out = torch.empty(F, H, W, 3, dtype=torch.float64, device=dev)
    cov = torch.zeros(F, H, W, dtype=torch.bool, device=dev)
    for f in range(F):
        key = zbuf[f]
        fi = key & 0xFFFFFFFF
        fc = fi.clamp(max=max(nf - 1, 0))
        tri = faces[fc]
        cv = (key != -1) & (fi < nf) & ((tri >= 0) & (tri < nv)).all(-1)
        tri = tri.clamp(0, nv - 1)
        _, z, u, w = project64(v, R[f], T[f], K)
        a, b, c = tri[..., 0], tri[..., 1], tri[..., 2]
        e0 = _edge(u[b], w[b], u[c], w[c], xs, ys) / z[a]
        e1 = _edge(u[c], w[c], u[a], w[a], xs, ys) / z[b]
        e2 = _edge(u[a], w[a], u[b], w[b], xs, ys) / z[c]
        den = e0 + e1 + e2
        ok = (den.abs() > 0) & torch.isfinite(den)
        third = torch.full_like(den, 1.0 / 3.0)
        l = torch.stack([torch.where(ok, e0 / den, third), torch.where(ok, e1 / den, third), torch.where(ok, e2 / den, third)], -1)
        st = (l[..., None] * t[fc]).sum(-2) - 0.5
        i0, j0 = torch.floor(st[..., 0]), torch.floor(st[..., 1])
        fx, fy = (st[..., 0] - i0)[..., None], (st[..., 1] - j0)[..., None]
        ia, ib = i0.clamp(0, Sw - 1).long(), (i0 + 1).clamp(0, Sw - 1).long()
        ja, jb = j0.clamp(0, Sh - 1).long(), (j0 + 1).clamp(0, Sh - 1).long()
        top = tx[ja, ia] * (1 - fx) + tx[ja, ib] * fx
        bot = tx[jb, ia] * (1 - fx) + tx[jb, ib] * fx
        col = (top * (1 - fy) + bot * fy) / 255.0
        if lit:
            n = (l[..., None] * nr[tri]).sum(-2)
            ncz = n @ R[f].double()[2]
            ln = n.norm(dim=-1)
            s = torch.where(ln > 0, ncz.abs() / ln.clamp(min=1e-300), torch.zeros_like(ln))
            col = (col * (0.3 + 0.7 * s)[..., None]).clamp(0.0, 1.0)
        bg = rgb[f].double() / 255.0 if rgb is not None else torch.ones(H, W, 3, dtype=torch.float64, device=dev)
        o = alpha * col + (1.0 - alpha) * bg
        out[f] = 255.0 * torch.where(cv[..., None], o, bg)
        cov[f] = cv
    return out, cov


def to_bytes(x255):
    return torch.floor(x255 + 0.5).clamp(0, 255).to(torch.uint8)


def psnr(out, rgb, mask):
    """(pooled PSNR over the masked pixels, sse, count) of two u8 [F,H,W,3] images."""
    d = (out.long() - rgb.long())[mask]
    sse, count = int((d * d).sum()), int(mask.sum())
    return 10.0 * math.log10(255.0 ** 2 * 3.0 * count / sse), sse, count


# ------------------------------------------------------------------------------------------------ analytic sphere
SPHERE_R = 0.45


def analytic_sphere_frames(R, T, K, H, W, r=SPHERE_R):
    """(rgb u8 [F,H,W,3], label i8 [F,H,W]) of the sphere |p| = r whose colour is 0.5 + 0.4 p / r, by ray-sphere intersection in fp64
    through the pixel centres; background 0.05 grey, label 0."""
    dev = R.device
    F = R.shape[0]
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, device=dev)], -1).double()
    rgb = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    label = torch.empty(F, H, W, dtype=torch.int8, device=dev)
    for f in range(F):
        d = torch.nn.functional.normalize(pix @ torch.inverse(K.double()).T, dim=1) @ R[f].double()
        o = -(R[f].double().T @ T[f].double())
        b = d @ o
        disc = b * b - (o @ o - r * r)
        t = -b - torch.sqrt(disc.clamp(min=0))
        hit = (disc > 0) & (t > 0)
        p = o + t[:, None] * d
        col = torch.where(hit[:, None], 0.5 + 0.4 * p / r, torch.full_like(p, 0.05))
        rgb[f] = (col * 255).round().clamp(0, 255).to(torch.uint8).view(H, W, 3)
        label[f] = hit.to(torch.int8).view(H, W)
    return rgb, label


def erode_object(label, px):
    """u8 [F,H,W]: mesh_color.usable_map restated with max_pool2d (CPU or device)."""
    not_obj = (label != 1).float()[:, None]
    if px > 0:
        not_obj = torch.nn.functional.max_pool2d(not_obj, 2 * px + 1, 1, px)
    return (not_obj[:, 0] == 0).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ the scenes of the tests
class Frames:
    """What the bake reads of a Dataset: rgb, label, R, T, K, n_images, H, W."""

    def __init__(self, rgb, label, R, T, K):
        self.rgb, self.label, self.R, self.T, self.K = rgb.contiguous(), label.contiguous(), R.contiguous(), T.contiguous(), K.contiguous()
        self.n_images, self.H, self.W = rgb.shape[0], rgb.shape[1], rgb.shape[2]


def atlas_size_with_margin(nf, cell=10, margin=3):
    """A size whose cells are `cell` texels and leave `margin` texels outside every cell (g c < S; odd, so S^2 is no multiple of 256)."""
    g = math.isqrt((nf + 1) // 2 - 1) + 1
    S = g * cell + margin
    assert S // g == cell and S % 2 == 1
    return S


def bake_scene(device="cpu"):
    """The bake tests' scene: an N = 20 sphere with one face dropped (odd count), 64 x 96 frames, four look-at cameras and one inside
    the sphere (part of the mesh behind it, part projecting outside the image), smooth plus noisy frames, labels with a hand band
    (-1) and a background band (0)."""
    H, W = 64, 96
    R, T, K = cameras(4, H, W, seed=1, device=device)
    Ri, Ti = camera_at((0.3, 0.02, 0.05), device=device)
    R, T = torch.cat([R, Ri]).contiguous(), torch.cat([T, Ti]).contiguous()
    verts, faces = sphere_mesh((0.05, -0.02, 0.03), 0.4, N=20, device=device, drop_last=True)
    rgb = smooth_noisy_frames(R.shape[0], H, W, seed=2, device=device)
    label = torch.ones(R.shape[0], H, W, dtype=torch.int8, device=device)
    label[:, :, 40:44] = -1
    label[:, 20:23, :] = 0
    return verts, faces, Frames(rgb, label, R, T, K)


def e2e_scene(device="cpu"):
    """The end-to-end test's scene: the N = 20 sphere of radius SPHERE_R about the origin, five cameras at distance 2.2, analytic
    96 x 128 frames and labels."""
    H, W = 96, 128
    R, T, K = cameras(5, H, W, radius=2.2, seed=3, device=device)
    verts, faces = sphere_mesh((0.0, 0.0, 0.0), SPHERE_R, N=20, device=device)
    rgb, label = analytic_sphere_frames(R, T, K, H, W)
    return verts, faces, Frames(rgb, label, R, T, K)


def e2e_restatement(verts, faces, ds, uv, owner, zbuf, erode_px=1):
    """Bake and unlit re-render of the end-to-end scene in fp64 on the given z-buffer: (texture u8 [S,S,3], image u8 [F,H,W,3], usable
    covered mask bool [F,H,W])."""
    from dynhor_amd.mesh_color import vertex_normals
    normals = vertex_normals(verts, faces)
    usable = erode_object(ds.label, erode_px)
    acc, cnt, _, _ = bake_fp64(verts, normals, faces, uv, owner, ds.rgb, usable, zbuf, ds.R, ds.T, ds.K)
    tex = texture_from_sums(acc, cnt, owner)
    img, cov = shade_tex_fp64(verts, normals, faces, uv, tex, zbuf, ds.R, ds.T, ds.K, rgb=ds.rgb)
    return tex, to_bytes(img), cov & (usable != 0)
