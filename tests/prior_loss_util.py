"""The rule of dh_prior_loss / dh_prior_loss_packed (include/dynhor_hip.h) restated in torch, in any dtype: the fp64 evaluation is the
reference of tests/test_gpu_prior_loss.py and tests/test_gpu_prior_training.py, the fp32 evaluation of the same code gives the error
the kernel is allowed four times of (tests/ray_kernels_util.py:ErrorLedger), and tests/test_cpu_prior_loss.py licenses it: its
analytic adjoints equal torch autograd of its own loss.

Builders draw from a seeded CPU generator and return CPU fp32 tensors.  Every quantity the rule branches on is kept away from its
switch: |e| from depth_delta and from 0, a prior from 1e-3, a decoded normal's squared norm from 0.25."""
import torch

F32, F64 = torch.float32, torch.float64
KINDS = ("inlier", "outlier", "inf", "nan", "zero", "negative", "masked", "empty")     # what ray i of a batch is: KINDS[(i + seed) % 8]
DELTA = 0.02


def midpoints(z, sample_dist):
    """m_k = z_k + 0.5 (z_{k+1} - z_k), sample_dist for the last sample."""
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], sample_dist)], -1)
    return z + 0.5 * dist


def huber(e, delta):
    a = e.abs()
    return torch.where(a <= delta, e * e / (2.0 * delta), a - 0.5 * delta)


def huber_grad(e, delta):
    return torch.where(e.abs() <= delta, e / delta, torch.sign(e))


def has_prior(prior):
    """[B] bool, decided on the values as given (fp32): inf, NaN and values <= 1e-3 mean no prior."""
    return torch.isfinite(prior) & (prior > 1e-3)


def has_normal(rays):
    mono = rays[:, 11:14]
    return (mono * mono).sum(-1) >= 0.25


def depth_term(rays, R, mid, weights, prior, delta, dtype, has_sample=None):
    """The depth term in `dtype`: dict(t_hat [B], e [B], v [B] bool, c_z [B], L, rays (= sum v), abs (= mean |e|)).  mid, weights
    [B,n] (a packed batch: padded with zero weights); has_sample [B] bool for packed rays."""
    r, Rm = rays.to(dtype), R.to(dtype).reshape(3, 3)
    t_hat = (weights.to(dtype) * mid.to(dtype)).sum(-1)
    c_z = Rm[2, 0] * r[:, 3] + Rm[2, 1] * r[:, 4] + Rm[2, 2] * r[:, 5]
    v = (rays[:, 9] * rays[:, 10] > 0) & has_prior(prior)
    if has_sample is not None:
        v = v & has_sample
    p = torch.where(v, prior, torch.zeros_like(prior)).to(dtype)
    e = torch.where(v, t_hat * c_z - p, torch.zeros_like(t_hat))
    vs = v.to(dtype).sum()
    L = (huber(e, delta) * v.to(dtype)).sum() / (vs + 1e-5)
    return {"t_hat": t_hat, "e": e, "v": v, "c_z": c_z, "L": L, "rays": vs, "abs": (e.abs() * v.to(dtype)).sum() / (vs + 1e-5)}


def depth_adjoint(d, mid, depth_weight, delta, dtype):
    """d_weights [B,n] = depth_weight v rho'(e) c_z / (sum v + 1e-5) m_k of a depth_term result."""
    coef = depth_weight * d["v"].to(dtype) * huber_grad(d["e"], delta) * d["c_z"] / (d["rays"] + 1e-5)
    return coef[:, None] * mid.to(dtype)


def normal_term(rays, R, nmap, dtype):
    """The masked normal term in `dtype`: dict(L, rays (= sum q), q [B]); loss_kernel's L1 + (1 - cos) with q = obj keep [has normal]."""
    r, Rm, no = rays.to(dtype), R.to(dtype).reshape(3, 3), nmap.to(dtype)
    q = r[:, 9] * r[:, 10] * has_normal(rays).to(dtype)
    nc = no @ Rm.T
    nh = nc / (nc.norm(dim=-1, keepdim=True) + 1e-6)
    mono = r[:, 11:14]
    cost = (nh - mono).abs().sum(-1) + 1.0 - (nh * mono).sum(-1)
    qs = q.sum()
    return {"L": (cost * q).sum() / (qs + 1e-5), "rays": qs, "q": q}


def normal_adjoint(rays, R, nmap, normal_weight, dtype):
    """d_normal_map [B,3] = normal_weight d L_n / d normal_map, written out as loss_kernel writes it (exact zeros where q = 0)."""
    r, Rm, no = rays.to(dtype), R.to(dtype).reshape(3, 3), nmap.to(dtype)
    q = r[:, 9] * r[:, 10] * has_normal(rays).to(dtype)
    nc = no @ Rm.T
    nn = nc.norm(dim=-1, keepdim=True)
    nrm = nn + 1e-6
    nh = nc / nrm
    mono = r[:, 11:14]
    dnh = (normal_weight * q / (q.sum() + 1e-5))[:, None] * (torch.sign(nh - mono) - mono)
    dd = (dnh * nc).sum(-1, keepdim=True)
    dnc = dnh / nrm - torch.where(nn > 0, nc * dd / (nn * nrm * nrm), torch.zeros_like(nc))
    return torch.where(q[:, None] > 0, dnc @ Rm, torch.zeros_like(dnc))


def stats_ref(d, nrm, depth_weight, normal_weight):
    """stats [8] of the entry from a depth_term and a normal_term result (either None: zeros)."""
    z = torch.zeros((), dtype=(d or nrm)["L"].dtype)
    dl, dv, da = (d["L"], d["rays"], d["abs"]) if d is not None else (z, z, z)
    nl, nq = (nrm["L"], nrm["rays"]) if nrm is not None else (z, z)
    return torch.stack([dl, dv, da, depth_weight * dl, nl, nq, normal_weight * nl, z])


# ------------------------------------------------------------------------------------------------ inputs
def encode_normal(n):
    """unit normal -> the bytes of a monocular normal map -> the decoded fp32 normal of dh_gen_rays (b / 255 * 2 - 1)."""
    b = ((n * 0.5 + 0.5).clamp(0, 1) * 255.0).round()
    return (b / 255.0 * 2.0 - 1.0).to(F32)


GREY = torch.full((3,), 128.0 / 255.0 * 2.0 - 1.0, dtype=F32)     # what grey 128 decodes to


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(int(seed))


def make_rays(B, g, seed, grey_every=0):
    """rays [B,14] fp32 and R [9] fp32: unit directions that look down the camera's +z (c_z in [0.6, 1]), obj = keep = 1 except on the
    "masked" rays (obj 0 and keep 0 in turn), byte-encoded unit monocular normals (grey 128 on every grey_every-th ray)."""
    R = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))[0]
    dc = torch.randn(B, 3, generator=g, dtype=F64) * 0.4
    dc[:, 2] = 1.0
    dc = torch.nn.functional.normalize(dc, dim=-1)
    rays = torch.zeros(B, 14, dtype=F64)
    rays[:, 0:3] = -2.5 * (dc @ R)
    rays[:, 3:6] = dc @ R
    rays[:, 6:9] = torch.rand(B, 3, generator=g, dtype=F64)
    rays[:, 9:11] = 1.0
    i = torch.arange(B)
    kind = (i + seed) % 8
    masked = kind == KINDS.index("masked")
    rays[masked & (i % 2 == 0), 9] = 0.0
    rays[masked & (i % 2 == 1), 10] = 0.0
    rays = rays.to(F32)
    rays[:, 11:14] = encode_normal(torch.nn.functional.normalize(torch.randn(B, 3, generator=g, dtype=F64), dim=-1))
    if grey_every:
        rays[(i + seed) % grey_every == 0, 11:14] = GREY
    return rays, R.to(F32).reshape(9).contiguous(), kind


def make_weights(B, n, g, kind, counts=None):
    """Compositing weights [B,n] fp32: a bump around a random sample times a random opacity in [0.5, 1]; exact zeros on "empty" rays.
    counts [B]: only the first counts[b] samples of ray b exist (a packed batch, padded); the rest are exact zeros."""
    cnt = torch.full((B, 1), float(n), dtype=F64) if counts is None else counts.double()[:, None]
    k = torch.arange(n, dtype=F64)[None, :]
    c = torch.rand(B, 1, generator=g, dtype=F64) * (cnt - 1).clamp(min=0)
    w = torch.exp(-0.5 * ((k - c) / (0.05 * cnt + 0.5)) ** 2) * (0.2 + torch.rand(B, n, generator=g, dtype=F64)) * (k < cnt)
    w = w / w.sum(-1, keepdim=True).clamp(min=1e-300) * (0.5 + 0.5 * torch.rand(B, 1, generator=g, dtype=F64))
    w[kind == KINDS.index("empty")] = 0.0
    return w.to(F32)


def make_prior(z_hat64, kind, g, delta=DELTA):
    """prior [B] fp32 by kind: z^ + s delta with |s| in [0.2, 0.7] ("inlier": the quadratic branch, |e| >= 0.2 delta from 0 and 0.3
    delta from delta), |s| in [2, 4] ("outlier" and "masked": the linear branch), inf, NaN, 0, -1; "empty" rays (z^ = 0) get 1.0."""
    B = z_hat64.shape[0]
    sgn = torch.where(torch.rand(B, generator=g, dtype=F64) < 0.5, -1.0, 1.0)
    u = torch.rand(B, generator=g, dtype=F64)
    p = z_hat64 + sgn * delta * (2.0 + 2.0 * u)
    p = torch.where(kind == 0, z_hat64 + sgn * delta * (0.2 + 0.5 * u), p)
    p = torch.where(kind == KINDS.index("inf"), torch.full_like(p, float("inf")), p)
    p = torch.where(kind == KINDS.index("nan"), torch.full_like(p, float("nan")), p)
    p = torch.where(kind == KINDS.index("zero"), torch.zeros_like(p), p)
    p = torch.where(kind == KINDS.index("negative"), torch.full_like(p, -1.0), p)
    p = torch.where(kind == KINDS.index("empty"), torch.ones_like(p), p)
    return p.to(F32)


def dense_inputs(B, n, seed, grey_every=0):
    """One dense batch: dict(rays, R, z, weights, prior, nmap, sample_dist, kind).  Ray i is KINDS[(i + seed) % 8]."""
    g = _gen(1000 * B + 10 * n + seed)
    rays, R, kind = make_rays(B, g, seed, grey_every)
    sd = 2.0 / 64
    z = (1.5 + torch.sort(torch.rand(B, n, generator=g, dtype=F64) * 2.0, dim=-1).values).to(F32)
    w = make_weights(B, n, g, kind)
    d = depth_term(rays, R, midpoints(z.double(), sd), w, torch.ones(B), DELTA, F64)
    prior = make_prior(d["t_hat"] * d["c_z"], kind, g)
    nmap = (torch.randn(B, 3, generator=g, dtype=F64) * 0.8).to(F32)
    return {"rays": rays, "R": R, "z": z, "weights": w, "prior": prior, "nmap": nmap, "sample_dist": sd, "kind": kind}


def packed_inputs(counts, seed, step=1.0 / 256):
    """One packed batch with the given per-ray sample counts (ragged offsets = their exclusive prefix sum): dict(rays, R, t_start [N],
    weights [N], prior, nmap, step, off i64, cnt i32, kind) plus the same batch padded to [B, max count] (mid_pad, w_pad)."""
    B = len(counts)
    g = _gen(77 + seed)
    rays, R, kind = make_rays(B, g, seed)
    cnt = torch.tensor(counts, dtype=torch.int64)
    off = torch.cumsum(cnt, 0) - cnt
    nmax = max(max(counts), 1)
    start = 1.5 + torch.rand(B, 1, generator=g, dtype=F64)
    # occupied steps only: a ray's samples are a random increasing subset of its steps
    gaps = torch.randint(1, 3, (B, nmax), generator=g).cumsum(-1) - 1
    t_pad = (start + gaps.double() * step).to(F32)
    w_pad = make_weights(B, nmax, g, kind, cnt)
    live = torch.arange(nmax)[None, :] < cnt[:, None]
    mid_pad = torch.where(live, t_pad.double() + 0.5 * float(torch.tensor(step, dtype=F32)), torch.zeros_like(t_pad, dtype=F64))
    d = depth_term(rays, R, mid_pad, w_pad, torch.ones(B), DELTA, F64)
    prior = make_prior(d["t_hat"] * d["c_z"], kind, g)
    prior = torch.where(cnt == 0, torch.ones_like(prior), prior)        # a ray without samples must not count although it has a prior
    nmap = (torch.randn(B, 3, generator=g, dtype=F64) * 0.8).to(F32)
    return {"rays": rays, "R": R, "t_start": t_pad[live].contiguous(), "weights": w_pad[live].contiguous(), "prior": prior, "nmap": nmap,
            "step": float(torch.tensor(step, dtype=F32)), "off": off, "cnt": cnt.to(torch.int32), "kind": kind, "live": live,
            "mid_pad": mid_pad, "w_pad": w_pad}


def margins(x, mid, weights, has_sample=None, delta=DELTA):
    """The smallest distances of a batch (mid, weights [B,n]) from the rule's switches, on the fp64 reference: delta = min | |e| - delta |
    / delta over the counted rays, zero = min |e| / delta, prior = min |prior - 1e-3| over the finite priors, normal = min |mono^2 -
    0.25|; and the counted rays on either Huber branch."""
    d = depth_term(x["rays"], x["R"], mid, weights, x["prior"], delta, F64, has_sample)
    e = d["e"][d["v"]].abs()
    fin = x["prior"][torch.isfinite(x["prior"])].double()
    mono2 = (x["rays"][:, 11:14].double() ** 2).sum(-1)
    inf = float("inf")
    return {"delta": ((e - delta).abs() / delta).min().item() if e.numel() else inf, "zero": (e / delta).min().item() if e.numel() else inf,
            "prior": (fin - 1e-3).abs().min().item() if fin.numel() else inf, "normal": (mono2 - 0.25).abs().min().item(),
            "inliers": int((e <= delta).sum()), "outliers": int((e > delta).sum())}
