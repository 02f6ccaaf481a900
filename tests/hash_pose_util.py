"""Pose refinement of the hash-grid family: what the tests of the point / direction adjoints share (tests/test_cpu_hash_pose.py,
tests/test_gpu_hash_pose.py, scripts/bench_hash_pose.py).

One fact shapes every comparison.  The encoding's derivative with respect to the point jumps at cell faces; its value does not.  A
point whose pos = x01 * scale_l + 0.5 lies within rounding of an integer -- at any of the 16 levels, 3 axes and the 7 evaluations
{0, +-fd_eps} -- may be put into different cells by the fp32 kernel and the fp64 oracle, and the two then differ by a whole slope,
legitimately.  `ambiguous` marks those points; a test that leaves them out asserts that they are at most MAX_MARKED of its inputs."""
import torch

from oracle import hashgrid_oracle as HO

MAX_MARKED = 0.10
MARGIN = 2.0 ** -21          # |pos - round(pos)| < MARGIN * (scale + 1): 8 ulp of pos; the kernel's expression has ~3.5 roundings


def ambiguous(pts, radius=1.0, eps=1e-3, enc=None):
    """[n] bool: some pos of the point lies within MARGIN * (scale_l + 1) of an integer.  fp64 arithmetic on the fp32 points."""
    enc = enc if enc is not None else HO.HashGridEncoding()
    x = pts.detach().double()
    scales = torch.tensor(enc.scales, dtype=torch.float64, device=x.device)                       # [16]
    shifts = torch.tensor([0.0, eps, -eps], dtype=torch.float64, device=x.device)                 # [3]
    x01 = (x[:, :, None] + shifts[None, None, :] + radius) / (2 * radius)                         # [n,3,3]
    pos = x01[..., None] * scales + 0.5                                                           # [n,3,3,16]
    near = (pos - torch.round(pos)).abs() < MARGIN * (scales + 1.0)
    return near.reshape(x.shape[0], -1).any(dim=1)


def unmarked_points(n, seed, radius_ball=0.9, device="cpu"):
    """n fp32 points uniform in the ball, none of them marked; also the marked share of the pool they were drawn from."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    pool = max(2 * n, 8192)              # (large enough that the share of a small n is not sampling noise)
    x = torch.randn(pool, 3, generator=g)
    x = (x / x.norm(dim=1, keepdim=True) * torch.rand(pool, 1, generator=g) ** (1 / 3) * radius_ball).float()
    bad = ambiguous(x)
    share = bad.float().mean().item()
    keep = x[~bad]
    assert keep.shape[0] >= n, "the pool is too small for its marked share"
    return keep[:n].contiguous().to(device), share


def geo_cotangents(n, seed, device="cpu"):
    """Random cotangents of sdf [n], feature [n,13] and the finite-difference normal [n,3]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(n, generator=g).to(device), torch.randn(n, 13, generator=g).to(device), torch.randn(n, 3, generator=g).to(device))


def oracle_point_adjoint(net, x, d_sdf, d_feat, d_grad):
    """d / d x of <d_sdf, sdf> + <d_feat, feature> + <d_grad, FD normal> by autograd on HO.HashSDFNetwork with the point as a leaf, in
    the network's dtype."""
    dt = next(net.parameters()).dtype
    x = x.detach().to(dt).clone().requires_grad_(True)
    out = net(x)
    f = (out[:, 0] * d_sdf.to(dt)).sum() + (out[:, 1:] * d_feat.to(dt)).sum() + (net.gradient(x).squeeze(1) * d_grad.to(dt)).sum()
    return torch.autograd.grad(f, x)[0]


def point_adjoint_rule(net, x, d_sdf, d_feat, d_grad):
    """The rule of dh_hash_geo_backward_rays (include/dynhor_hip.h) restated: the E = 7 evaluations' input adjoints din_e from the MLP
    alone, then  (1 / radius) sum_e din_e[0..2]  +  sum_e sum_l (scale_l / (2 radius)) sum_corners (d w_corner / d pos) <table[corner],
    din_e[l]>  with the corner loops written out.  In the network's dtype."""
    enc, r, eps = net.encoding, net.radius, net.fd_eps
    dt = next(net.parameters()).dtype
    x = x.detach().to(dt)
    n = x.shape[0]
    offs = torch.eye(3, dtype=dt, device=x.device) * eps
    evals = [(x, None, 1.0)] + [(x + sg * offs[a], a, sg) for a in range(3) for sg in (1.0, -1.0)]
    total = torch.zeros_like(x)
    for xe, axis, sg in evals:
        x01 = (xe + r) / (2 * r)
        inp = torch.cat([x01 * 2 - 1, enc(x01)], dim=-1).detach().requires_grad_(True)
        out = net.lin1(torch.nn.functional.softplus(net.lin0(inp), beta=100))
        if axis is None:
            f = (out[:, 0] * d_sdf.to(dt)).sum() + (out * d_feat.to(dt)).sum()
        else:
            f = (out[:, 0] * d_grad.to(dt)[:, axis] * (sg * 0.5 / eps)).sum()
        din = torch.autograd.grad(f, inp)[0].detach()
        total += din[:, :3] / r
        for l in range(enc.L):
            pos = x01 * enc.scales[l] + 0.5
            pg = torch.floor(pos)
            w = pos - pg
            pg = pg.to(torch.int64)
            dl = din[:, 3 + 2 * l:5 + 2 * l]
            acc = torch.zeros(n, 3, dtype=dt, device=x.device)
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        row = enc.table[enc.level_index(l, pg[:, 0] + dx, pg[:, 1] + dy, pg[:, 2] + dz)].to(dt).detach()
                        s = (row * dl).sum(dim=1)
                        wx = w[:, 0] if dx else 1 - w[:, 0]
                        wy = w[:, 1] if dy else 1 - w[:, 1]
                        wz = w[:, 2] if dz else 1 - w[:, 2]
                        acc[:, 0] += (1.0 if dx else -1.0) * wy * wz * s
                        acc[:, 1] += (1.0 if dy else -1.0) * wx * wz * s
                        acc[:, 2] += (1.0 if dz else -1.0) * wx * wy * s
            total += acc * (enc.scales[l] / (2 * r))
    return total


def sh4_grad_rule(d, dy):
    """sum_k dy[:, k] d y_k / d d of the 16 SH-4 polynomials of HO.sh4 (an unnormalised d), term by term: [n,3]."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    c1, c2, c3, c5 = 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.54627421529603959
    c6, c7, c8, c9, c10 = 0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 1.4453057213202769
    q, t = 1.0 - 5.0 * zz, 3.0 * (yy - xx)
    g = dy
    gx = (-c1 * g[:, 3] + c2 * (y * g[:, 4] - z * g[:, 7]) + 2 * c5 * x * g[:, 8] - 6 * c6 * xy * g[:, 9] + c7 * yz * g[:, 10]
          + c8 * q * g[:, 13] + 2 * c10 * xz * g[:, 14] + c6 * t * g[:, 15])
    gy = (-c1 * g[:, 1] + c2 * (x * g[:, 4] - z * g[:, 5]) - 2 * c5 * y * g[:, 8] + c6 * t * g[:, 9] + c7 * xz * g[:, 10]
          + c8 * q * g[:, 11] - 2 * c10 * yz * g[:, 14] + 6 * c6 * xy * g[:, 15])
    gz = (c1 * g[:, 2] - c2 * (y * g[:, 5] + x * g[:, 7]) + 2 * c3 * z * g[:, 6] + c7 * xy * g[:, 10]
          - 10 * c8 * z * (y * g[:, 11] + x * g[:, 13]) + c9 * (15 * zz - 3) * g[:, 12] + c10 * (xx - yy) * g[:, 14])
    return torch.stack([gx, gy, gz], dim=-1)


def two_errors(got, ref):
    """(error norm / reference norm, largest per-point error / largest per-point magnitude), both in fp64."""
    e = (got.double() - ref.double())
    return (e.norm() / ref.double().norm().clamp_min(1e-300)).item(), (e.norm(dim=-1).max() / ref.double().norm(dim=-1).max().clamp_min(1e-300)).item()
