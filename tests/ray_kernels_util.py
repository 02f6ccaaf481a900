"""Shared pieces of the kernel-level tests of csrc/kernels_ray.hip and csrc/optim.hip (tests/test_gpu_ray_sampling.py,
test_gpu_ray_scan.py, test_gpu_loss_adam.py; licensed on the CPU by tests/test_cpu_ray_kernels_ref.py).

  * Canary: every buffer a kernel writes is allocated between two pads holding a fixed NaN bit pattern; the payload starts
    with the same pattern.  After the launch the pads must be unchanged (no out-of-range write) and no payload word may still hold
    the pattern (no missing write).  Nothing is provoked: a wrong index shows up as a changed pad word or a stale payload word.
  * ctypes callers of the entry points, one per kernel, that allocate their outputs through a Canary.
  * the fp64 references: oracle/neus_oracle.py driven with stub networks that return prescribed leaf tensors (render_core,
    up_sample, sample_z, neus_losses) and a plain restatement of torch.optim.Adam.
  * input builders that keep every quantity a kernel branches on away from its switch by a stated margin, and the functions that
    measure those margins on the fp64 reference (nothing is excluded: the tests assert the minimum over every element).
  * the criteria: error against fp64 bounded by 4 x the error of the oracle's own fp32 evaluation, the CDF-space residual of the
    inverse-CDF samples.

Builders draw from a seeded CPU generator and return CPU fp32 tensors, so the CPU test can assert the margins of exactly the inputs
the GPU tests use."""
import ctypes
import math

import torch

from oracle import neus_oracle as O

F32, F64 = torch.float32, torch.float64
U32 = 2.0 ** -24                      # fp32 unit round-off (half an ulp of 1)
CANARY_BITS = 0x7FC0DEAD              # a quiet NaN no kernel here produces
PAD = 64                              # words before and after every payload


# ------------------------------------------------------------------------------------------------ canary padding
class Canary:
    def __init__(self, device):
        self.device = torch.device(device)
        self.items = []

    def _raw(self, name, numel):
        raw = torch.full((PAD + numel + PAD,), CANARY_BITS, dtype=torch.int32, device=self.device)
        self.items.append((name, raw, numel))
        return raw[PAD:PAD + numel]

    def out(self, name, *shape):
        """A fp32 output buffer of `shape`, payload pre-filled with the NaN pattern."""
        return self._raw(name, int(math.prod(shape))).view(F32).view(*shape)

    def inout(self, name, t):
        """A padded copy of t for kernels that update in place (only the pads are watched)."""
        v = self._raw(name, t.numel()).view(F32).view(t.shape)
        v.copy_(t)
        self.items[-1] = (name, self.items[-1][1], -t.numel())
        return v

    def check(self, untouched=()):
        for name, raw, numel in self.items:
            n = abs(numel)
            assert bool((raw[:PAD] == CANARY_BITS).all()) and bool((raw[PAD + n:] == CANARY_BITS).all()), \
                f"{name}: a word outside the buffer was written"
            if numel < 0:
                continue
            stale = int((raw[PAD:PAD + n] == CANARY_BITS).sum())
            if name in untouched:
                assert stale == n, f"{name}: must stay untouched, {n - stale} words were written"
            else:
                assert stale == 0, f"{name}: {stale} of {n} output words were never written"


# ------------------------------------------------------------------------------------------------ ctypes callers
def hip(name, *args):
    """Call an entry point: tensors -> device pointers, None -> NULL, the current stream appended; waits for the result."""
    from dynhor_amd import _lib
    conv = [ctypes.c_void_p(0) if a is None else (_lib.ptr(a) if torch.is_tensor(a) else a) for a in args]
    _lib.check(getattr(_lib.lib(), name)(*conv, _lib.stream()))
    torch.cuda.synchronize()


def hip_coarse(o, d, near, far, t_rand, n):
    B = o.shape[0]
    c = Canary(o.device)
    z, pts = c.out("z", B, n), c.out("pts", B * n, 3)
    hip("dh_coarse_samples", o, d, near, far, t_rand, B, n, z, pts)
    c.check()
    return z, pts


def hip_midpoints(o, d, z, sample_dist):
    B, n = z.shape
    c = Canary(o.device)
    pts = c.out("pts", B * n, 3)
    hip("dh_midpoints", o, d, z, B, n, float(sample_dist), pts)
    c.check()
    return pts


def hip_upsample(o, d, z, sdf, n_new, inv_s):
    B, n = z.shape
    c = Canary(o.device)
    z_new, pts_new = c.out("z_new", B, n_new), c.out("pts_new", B * n_new, 3)
    hip("dh_upsample_step", o, d, z, sdf, B, n, n_new, float(inv_s), z_new, pts_new)
    c.check()
    return z_new, pts_new


def hip_merge(z, z_new, sdf, sdf_new, with_sdf=True):
    B, n = z.shape
    k = z_new.shape[1]
    c = Canary(z.device)
    z_out = c.out("z_out", B, n + k)
    sdf_out = c.out("sdf_out", B, n + k) if with_sdf else None
    hip("dh_merge_samples", z, z_new, sdf if with_sdf else None, sdf_new if with_sdf else None, B, n, k, z_out, sdf_out)
    c.check()
    return z_out, sdf_out


def hip_scan_fwd(x, car, bg, want_nmap):
    B, n = x["z"].shape
    c = Canary(x["z"].device)
    r = {"weights": c.out("weights", B, n), "color": c.out("color", B, 3), "wsum": c.out("wsum", B), "wmax": c.out("wmax", B),
         "cdf": c.out("cdf", B, n), "inside": c.out("inside", B, n), "eik": c.out("eik", B, 2),
         "nmap": c.out("nmap", B, 3) if want_nmap else None}
    hip("dh_render_scan_fwd", x["o"], x["d"], x["z"], x["sdf"], x["normals"], x["colors"], x["inv_s"], float(car),
        float(x["sample_dist"]), bg, B, n, r["weights"], r["color"], r["wsum"], r["wmax"], r["cdf"], r["inside"], r["eik"], r["nmap"])
    c.check()
    return r


def hip_scan_bwd(x, car, bg, cot, rays=False):
    """cot: d_color [B,3] (always), d_wsum [B] / d_weights [B,n] / d_gradients [B*n,3] / d_nmap [B,3] (None = NULL), ec [1]."""
    B, n = x["z"].shape
    c = Canary(x["z"].device)
    r = {"d_sdf": c.out("d_sdf", B * n), "d_normals": c.out("d_normals", B * n, 3), "d_colors": c.out("d_colors", B * n, 3),
         "d_inv_s": c.out("d_inv_s", B)}
    args = [x["o"], x["d"], x["z"], x["sdf"], x["normals"], x["colors"], x["inv_s"], float(car), float(x["sample_dist"]), bg, B, n,
            cot["d_color"], cot.get("d_wsum"), cot.get("d_weights"), cot.get("d_gradients"), cot.get("d_nmap"), cot["ec"],
            r["d_sdf"], r["d_normals"], r["d_colors"], r["d_inv_s"]]
    if rays:
        r["d_rays_d"] = c.out("d_rays_d", B, 3)
        hip("dh_render_scan_bwd_rays", *args, r["d_rays_d"])
    else:
        hip("dh_render_scan_bwd", *args)
    c.check()
    return r


def hip_loss(color, wsum, nmap, eik, rays, R, igr_w, mask_w, normal_w, null_normal=False):
    """null_normal: normal_map, R and d_normal_map are passed as NULL (allowed when normal_w == 0); otherwise d_normal_map is a
    canary buffer, which the kernel must leave untouched when normal_w == 0."""
    B = color.shape[0]
    c = Canary(color.device)
    r = {"stats": c.out("stats", 8), "d_color": c.out("d_color", B, 3), "d_wsum": c.out("d_wsum", B),
         "d_nmap": None if null_normal else c.out("d_nmap", B, 3), "eik_coef": c.out("eik_coef", 1)}
    hip("dh_neus_loss", color, wsum, None if null_normal else nmap, eik, rays, None if null_normal else R, B, float(igr_w),
        float(mask_w), float(normal_w), r["stats"], r["d_color"], r["d_wsum"], r["d_nmap"], r["eik_coef"])
    c.check(untouched=("d_nmap",) if normal_w <= 0.0 else ())
    return r


def hip_adam(p, g, m, v, n, lr, b1, b2, eps, step, grad_scale):
    """p, m, v: tensors with MORE than n elements; returns the updated copies (all elements, so that the tail can be compared)."""
    c = Canary(p.device)
    p2, m2, v2 = c.inout("p", p), c.inout("m", m), c.inout("v", v)
    hip("dh_adam_step", p2, g, m2, v2, n, float(lr), float(b1), float(b2), float(eps), int(step), float(grad_scale))
    c.check()
    return p2, m2, v2


# ------------------------------------------------------------------------------------------------ error criterion
def measure(got, ref64, ref32):
    """(max |got - ref64|, max |ref32 - ref64|, one fp32 ulp of the largest reference element, relative L2 error)."""
    ref64 = ref64.to(F64)
    both_inf = torch.isinf(ref64) & (got.to(F64) == ref64)
    diff = torch.where(both_inf, torch.zeros_like(ref64), got.to(F64) - ref64)
    d32 = torch.where(torch.isinf(ref64) & (ref32.to(F64) == ref64), torch.zeros_like(ref64), ref32.to(F64) - ref64)
    fin = torch.where(torch.isinf(ref64), torch.zeros_like(ref64), ref64)
    nrm = fin.norm().item()
    rel = (diff.norm().item() / nrm) if nrm > 0 else (0.0 if diff.norm().item() == 0 else float("inf"))
    return diff.abs().max().item(), d32.abs().max().item(), 2.0 * U32 * fin.abs().max().item(), rel


PER_RAY_OUTPUTS = ("color", "wsum", "wmax", "eik", "nmap", "d_inv_s", "d_rays_d")


def pooled(name, B, n):
    """Whether an output of a batch is judged together with the other small batches of the same n instead of on its own.
    "4 x the fp32 oracle's error on the same inputs" and a relative L2 are statements about a sample of elements.  They are applied
    case by case wherever a case holds one: every batch of 130 rays, and the per-sample outputs (weights, cdf, d_sdf, d_normals,
    d_colors) of every batch with n >= 64.  What is pooled is (a) every output of B <= 5 rays with n <= 3 -- at most 15 samples: one
    ray of one sample can consist of nothing but the 1e-5 floor of alpha (cos_anneal_ratio 1 and a normal facing away), and the fp32
    oracle itself is then > 1e-4 off in relative L2 -- and (b) the per-ray outputs of B <= 5 rays at any n: at most 15 numbers, each
    what is left of cancelling sums (the fp32 oracle's d_inv_s of four rays misses 1e-4 as well).  A pool is ONE case: every element
    under the element-wise bound of the pool, the relative L2 taken over the pool."""
    return B <= 5 and (n <= 3 or name in PER_RAY_OUTPUTS)


class ErrorLedger:
    """Collects (max error, the fp32 oracle's error, bound) per output and asserts
        max |got - fp64| <= 4 * max(e32, ulp)          e32 = max |fp32 oracle - fp64| on the same inputs,
                                                       ulp = one fp32 ulp of the largest reference element
        relative L2 error < rel_tol                    (1e-4: the project's figure for the packed scan)
    The ulp floor is the format's own resolution: in a case as small as one ray with one sample the fp32 oracle can be exact by
    luck, and an equally valid fp32 evaluation order cannot be asked to be closer than the last bit."""

    def __init__(self, rel_tol=1e-4):
        self.rel_tol = rel_tol
        self.worst = {}
        self.pools = {}

    def flush(self, case="pooled batches of <= 5 rays"):
        for name, items in self.pools.items():
            self.add(name, *(torch.cat([it[i] for it in items]) for i in range(3)), case=case)
        self.pools = {}

    def add(self, name, got, ref64, ref32, case="", pool=False):
        """pool: keep the tensors and judge them together in flush() -- see pooled()."""
        assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
        if pool:
            self.pools.setdefault(name, []).append((got.reshape(-1), ref64.reshape(-1), ref32.reshape(-1)))
            return
        assert bool(torch.isfinite(got).all()) or bool(torch.isinf(ref64).any()), f"{name} {case}: non-finite output"
        err, e32, ulp, rel = measure(got, ref64, ref32)
        bound = 4.0 * max(e32, ulp)
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        w = self.worst.get(name)
        if w is None or ratio > w[0]:
            self.worst[name] = (ratio, err, e32, ulp, rel, case)
        self.worst[name + "/rel"] = max(self.worst.get(name + "/rel", (0.0,)), (rel, case))
        assert err <= bound, f"{name} {case}: max err {err:.3e} > 4 x max(fp32 oracle {e32:.3e}, ulp {ulp:.3e})"
        assert rel < self.rel_tol, f"{name} {case}: relative L2 {rel:.3e} >= {self.rel_tol:g}"

    def report(self, title):
        print(title)
        for k, w in self.worst.items():
            if k.endswith("/rel"):
                continue
            print(f"  {k:12s} worst err/bound {w[0]:.3f}: err {w[1]:.3e}, fp32 oracle {w[2]:.3e}, ulp {w[3]:.3e} -> bound "
                  f"{4 * max(w[2], w[3]):.3e}; worst rel L2 {self.worst[k + '/rel'][0]:.2e}   [{w[5]}]")


# ------------------------------------------------------------------------------------------------ rays
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(int(seed))


def make_rays(B, g, b_lo, b_hi):
    """Rays that pass the origin at distance b in [b_lo, b_hi], starting 2.5 in front of the closest point.  Returns fp32 o, d and,
    from those fp32 values in fp64, t0 (depth of the closest point) and b."""
    dirn = torch.nn.functional.normalize(torch.randn(B, 3, generator=g, dtype=F64), dim=-1)
    perp = torch.nn.functional.normalize(torch.linalg.cross(dirn, torch.randn(B, 3, generator=g, dtype=F64)), dim=-1)
    b = b_lo + (b_hi - b_lo) * torch.rand(B, 1, generator=g, dtype=F64)
    o = (-2.5 * dirn + b * perp).to(F32)
    d = dirn.to(F32)
    o64, d64 = o.double(), d.double()
    t0 = -(o64 * d64).sum(-1, keepdim=True) / (d64 * d64).sum(-1, keepdim=True)
    b = (o64 + t0 * d64).norm(dim=-1, keepdim=True)
    return o, d, t0, b


def radius64(o, d, t):
    return (o.double()[:, None, :] + d.double()[:, None, :] * t.double()[..., None]).norm(dim=-1)


# ------------------------------------------------------------------------------------------------ up-sampling
UPS_FAMILIES = ("bumpy sphere", "thin slab", "miss", "opaque first section")
UPS_RADIUS_MARGIN = 1e-5              # |radius(z_i) - 1| of every sample; fp32 evaluates a radius <= 4 to ~5e-7


def upsample_inputs(B, n_cur, seed):
    """fp32 (o, d, z [B,n_cur] strictly ascending, sdf [B,n_cur]) and the family id of every ray ((ray + seed) % 4).  For n_cur >
    64 the samples past the 64th cluster around the surface, as after earlier up-sampling steps (except on rays that miss)."""
    g = _gen(1000 * n_cur + seed)
    o, d, t0, b = make_rays(B, g, 0.05, 0.25)
    fam = (torch.arange(B) + seed) % 4
    half = torch.where(fam == 3, 0.95, 1.15).to(F64)[:, None]          # family 3 starts inside the unit sphere, the others outside
    n_a = min(n_cur, 64)
    j = torch.arange(n_a, dtype=F64)[None, :]
    z = t0 - half + 2.0 * half * (j + 0.5 + 0.6 * (torch.rand(B, n_a, generator=g, dtype=F64) - 0.5)) / n_a
    ts = t0 - 0.45 + 0.3 * torch.rand(B, 1, generator=g, dtype=F64)    # where the surface is met
    if n_cur > n_a:
        z = torch.cat([z, ts + 0.05 * torch.randn(B, n_cur - n_a, generator=g, dtype=F64)], -1).sort(-1)[0]
        # a ray that misses has no surface to cluster around: its 1e-5 weight floor gives every section the same mass, however
        # narrow, and F64 would then be ill-conditioned in z inside a section a few fp32 ulps wide; it keeps regular samples
        jj = torch.arange(n_cur, dtype=F64)[None, :]
        zr = t0 - half + 2.0 * half * (jj + 0.5 + 0.6 * (torch.rand(B, n_cur, generator=g, dtype=F64) - 0.5)) / n_cur
        z = torch.where((fam == 2)[:, None], zr, z)
    z = z.to(F32)
    for _ in range(100):                                               # keep every sample off the unit sphere
        bad = ((radius64(o, d, z) - 1.0).abs() < 2 * UPS_RADIUS_MARGIN).any(-1)
        strict = (z[:, 1:] > z[:, :-1]).all(-1) if n_cur > 1 else torch.ones(B, dtype=torch.bool)
        if not bool(bad.any()) and bool(strict.all()):
            break
        z[bad] += 7e-5
        if not bool(strict.all()):                                     # (two clustered samples rounded to one fp32 value)
            z[~strict] = (z[~strict].double() + 1e-6 * torch.arange(n_cur, dtype=F64)).to(F32)
    o64, d64, z64 = o.double(), d.double(), z.double()
    p = o64[:, None, :] + d64[:, None, :] * z64[..., None]
    if n_cur >= 2:
        ts = torch.where((fam == 3)[:, None], 0.5 * (z64[:, :1] + z64[:, 1:2]), ts)
    nrm = torch.nn.functional.normalize(d64 + 0.3 * torch.randn(B, 3, generator=g, dtype=F64), dim=-1)
    hit = o64 + d64 * ts
    sphere = p.norm(dim=-1) - (hit.norm(dim=-1, keepdim=True)) + 0.03 * torch.sin(9 * p[..., 0] + 5 * p[..., 1]) * torch.cos(7 * p[..., 2])
    slab = (((p - hit[:, None, :]) * nrm[:, None, :]).sum(-1)).abs() - 0.03
    perp = torch.nn.functional.normalize(o64 + t0 * d64, dim=-1)
    miss = (p - (o64 + t0 * d64 + 1.3 * perp)[:, None, :]).norm(dim=-1) - 0.3
    t = z64 - ts
    opaque = -0.3 * t - 2.0 * t.clamp_min(0.0) ** 2
    sdf = torch.stack([sphere, slab, miss, opaque], 0)[fam, torch.arange(B)]
    return o, d, z, sdf.to(F32), fam


def oracle_upsample(o, d, z, sdf, n_new, inv_s, dtype):
    """The oracle's up_sample in `dtype` on the given fp32 inputs: (z_new [B,n_new], cdf [B,n]).  The weights are read where
    up_sample hands them to sample_pdf; the CDF is formed from them exactly as sample_pdf does."""
    seen = {}
    orig = O.sample_pdf

    def spy(bins, weights, n_samples, det=False):
        seen["w"] = weights
        return orig(bins, weights, n_samples, det=det)

    R = O.NeuSRenderer(None, None, None, None, z.shape[1], n_new, 0, 1, 0.0)
    O.sample_pdf = spy
    try:
        z_new = R.up_sample(o.to(dtype), d.to(dtype), z.to(dtype), sdf.to(dtype), n_new, float(inv_s))
    finally:
        O.sample_pdf = orig
    w = seen["w"] + 1e-5
    cdf = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
    return z_new, torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)


def cdf_residual(z, cdf64, zq, n_new):
    """|F64(zq_k) - u_k| with F64 the piecewise-linear fp64 CDF through (z_i, cdf_i) and u_k = (k + 0.5) / n_new.  zq outside
    [z_0, z_{n-1}] is clamped (the range assertion is separate)."""
    z, zq, cdf64 = z.double().contiguous(), zq.double().contiguous(), cdf64.double()
    n = z.shape[1]
    i = (torch.searchsorted(z, zq, right=True) - 1).clamp(0, max(n - 2, 0))
    i1 = (i + 1).clamp(max=n - 1)
    za, zb = torch.gather(z, 1, i), torch.gather(z, 1, i1)
    w = zb - za
    t = torch.where(w > 0, (zq - za) / torch.where(w > 0, w, torch.ones_like(w)), torch.zeros_like(w)).clamp(0.0, 1.0)
    F = torch.gather(cdf64, 1, i) + t * (torch.gather(cdf64, 1, i1) - torch.gather(cdf64, 1, i))
    u = (torch.arange(n_new, dtype=F64, device=z.device) + 0.5) / n_new
    return (F - u[None, :]).abs()


def upsample_margins(o, d, z):
    return (radius64(o, d, z) - 1.0).abs().min().item()


# ------------------------------------------------------------------------------------------------ dense scan
SCAN_RADIUS_MARGIN = 2e-5     # |pn - 1.0|, |pn - 1.2| of every mid-point; fp32 evaluates pn (<= 4) to ~5e-7
SCAN_COS_MARGIN = 1e-5        # |d.n|, |d.n - 1| of every non-zero normal; three fp32 roundings of O(1) terms: ~3e-7
SCAN_ALPHA_MARGIN = 2e-6      # |alpha_raw| ; fp32 error of (prev - next + 1e-5) / (prev + 1e-5): ~3e-7 (see scan_margins)
SCAN_SAMPLE_DIST = 2.0 / 64   # exact in fp32
SCAN_INV_S = 40.0


def _scan_geometry(o, d, z, sample_dist):
    z64 = z.double()
    dist = torch.cat([z64[:, 1:] - z64[:, :-1], torch.full_like(z64[:, :1], sample_dist)], -1)
    mid = z64 + 0.5 * dist
    return dist, mid, radius64(o, d, mid)


def scan_inputs(B, n, seed):
    """fp32 inputs of the dense scan with every switch populated on both sides and kept off by the SCAN_* margins:
      rays (ray + seed) % 8 in 0..3 : the LAST mid-point sits 2..8 margins inside / outside radius 1.0 / 1.2
      rays (ray + seed) % 5 == 3    : one locally DECREASING depth (negative section length -> alpha_raw < 0: the clip gates)
      rays (ray + seed) % 3 == 0    : cross a surface (transmittance ends far below 1e-4); == 1: graze; == 2: a thin sheet
      points  p % 11 == 5           : normal exactly zero
      points  p % 7 == 2            : d.n placed 2..8 margins either side of 0 or 1"""
    g = _gen(100000 + 1000 * n + 7 * B + seed)
    sd = SCAN_SAMPLE_DIST
    o, d, t0, b = make_rays(B, g, 0.05, 0.9)
    ray = torch.arange(B)
    kind = (ray + seed) % 8
    lo = t0 - 1.3
    hi = t0 + 1.3
    target = torch.tensor([1.0, 1.0, 1.2, 1.2], dtype=F64)[kind.clamp(max=3)][:, None]
    side = torch.tensor([-1.0, 1.0, -1.0, 1.0], dtype=F64)[kind.clamp(max=3)][:, None]
    delta = (2.0 + 6.0 * torch.rand(B, 1, generator=g, dtype=F64)) * SCAN_RADIUS_MARGIN
    z_last = t0 + torch.sqrt((target + side * delta) ** 2 - b * b) - 0.5 * sd
    placed = (kind < 4)[:, None]
    z_last = torch.where(placed, z_last, hi)
    u = torch.rand(B, n, generator=g, dtype=F64)
    j = torch.arange(n, dtype=F64)[None, :]
    z = lo + (z_last - lo) * (j + 0.8 * u) / max(n - 1, 1)
    z[:, -1:] = z_last
    if n >= 3:
        dec = ((ray + seed) % 5 == 3)
        jd = torch.randint(0, n - 2, (B,), generator=g)
        zd = z[ray, jd] - 0.4 * (z[ray, jd + 1] - z[ray, jd])
        z[ray[dec], jd[dec] + 1] = zd[dec]
    else:
        dec, jd = torch.zeros(B, dtype=torch.bool), torch.zeros(B, dtype=torch.long)
    z = z.to(F32)
    for _ in range(200):
        _, _, pn = _scan_geometry(o, d, z, sd)
        bad = (((pn - 1.0).abs() < 1.5 * SCAN_RADIUS_MARGIN) | ((pn - 1.2).abs() < 1.5 * SCAN_RADIUS_MARGIN)).any(-1)
        if not bool(bad.any()):
            break
        z[bad] += 4e-5
    dist, mid, pn = _scan_geometry(o, d, z, sd)
    P = B * n
    pidx = torch.arange(P)
    # normals
    nd = torch.nn.functional.normalize(torch.randn(P, 3, generator=g, dtype=F64), dim=-1) * (0.7 + 0.6 * torch.rand(P, 1, generator=g, dtype=F64))
    dP = d.double()[:, None, :].expand(B, n, 3).reshape(P, 3)
    tgt = torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=F64)[(pidx // 7) % 4]
    sgn = torch.tensor([-1.0, 1.0, -1.0, 1.0], dtype=F64)[(pidx // 7) % 4]
    dl = (2.0 + 6.0 * torch.rand(P, generator=g, dtype=F64)) * SCAN_COS_MARGIN
    put = pidx % 7 == 2
    corr = ((tgt + sgn * dl) - (dP * nd).sum(-1)) / (dP * dP).sum(-1)
    nd = torch.where(put[:, None], nd + corr[:, None] * dP, nd)
    zero = pidx % 11 == 5
    nd[zero] = 0.0
    normals = nd.to(F32)
    for _ in range(200):
        tc = (dP * normals.double()).sum(-1)
        bad = ((tc.abs() < 1.5 * SCAN_COS_MARGIN) | ((tc - 1.0).abs() < 1.5 * SCAN_COS_MARGIN)) & ~zero
        if not bool(bad.any()):
            break
        normals[bad] = (normals[bad].double() + 4.0 * SCAN_COS_MARGIN * dP[bad]).to(F32)
    # sdf at the mid-points
    fam = ((ray + seed) % 3)[:, None]
    ts = t0 - 0.3 + 0.6 * torch.rand(B, 1, generator=g, dtype=F64)
    noise = torch.randn(B, n, generator=g, dtype=F64)
    cross = (0.25 * (ts - mid)).clamp(-0.3, 0.3) + 0.02 * noise
    graze = 0.06 + 0.05 * noise
    sheet = (mid - ts).abs() - 0.05 + 0.01 * noise
    sdf = torch.where(fam == 0, cross, torch.where(fam == 1, graze, sheet))
    if n >= 3:
        sdf[ray[dec], jd[dec]] = 0.01 * noise[ray[dec], jd[dec]]       # the section of negative length: sigmoids unsaturated
    colors = torch.rand(P, 3, generator=g, dtype=F64)
    return {"o": o, "d": d, "z": z, "sdf": sdf.reshape(P).to(F32), "normals": normals, "colors": colors.to(F32),
            "inv_s": torch.tensor([SCAN_INV_S], dtype=F32), "sample_dist": sd}


def scan_cotangents(B, n, seed):
    g = _gen(777 + 31 * n + B + seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64).to(F32)
    return {"d_color": r(B, 3), "d_wsum": r(B), "d_weights": r(B, n), "d_gradients": 0.1 * r(B * n, 3), "d_nmap": r(B, 3),
            "ec": torch.tensor([0.37], dtype=F32)}


COT_OPTIONAL = ("d_wsum", "d_weights", "d_gradients", "d_nmap")
COT_CONFIGS = ((), COT_OPTIONAL) + tuple((k,) for k in COT_OPTIONAL)      # all NULL, all set, each set singly


class _StubSDF:
    def __init__(self, sdf, normals):
        self.s, self.n, self.pts = sdf.reshape(-1, 1), normals.reshape(-1, 3), None

    def __call__(self, pts):
        self.pts = pts
        return self.s

    def sdf(self, pts):
        return self.s

    def gradient(self, pts):
        return self.n.unsqueeze(1)


class _StubColor:
    def __init__(self, colors):
        self.c = colors.reshape(-1, 3)

    def __call__(self, points, normals, view_dirs, feature_vectors):
        return self.c


class _StubDeviation:
    def __init__(self, inv_s):
        self.inv_s = inv_s

    def __call__(self, x):
        return self.inv_s.reshape(1, 1)


def scan_reference(x, car, bg, cot=None, use=(), dtype=F64):
    """oracle render_core with stub networks in `dtype`.  Returns (forward dict, gradient dict or None).  cot / use: the random
    linear functional  sum d_color.color [+ d_wsum.wsum + d_weights.weights + d_gradients.gradients + d_nmap.normal_map for the
    names in `use`] + ec (sum relax + 1e-5) gradient_error, differentiated by autograd w.r.t. sdf, normals, colours, inv_s and
    rays_d (which enters only through true_cos: the stubs ignore the points)."""
    dev = x["z"].device
    c = lambda t: t.to(dtype).clone()
    B, n = x["z"].shape
    sdf, normals, colors, inv_s, d = c(x["sdf"]), c(x["normals"]), c(x["colors"]), c(x["inv_s"]), c(x["d"])
    leaves = (sdf, normals, colors, inv_s, d)
    if cot is not None:
        for t in leaves:
            t.requires_grad_(True)
    net = _StubSDF(sdf, normals)
    R = O.NeuSRenderer(None, net, _StubDeviation(inv_s), _StubColor(colors), 64, 0, 0, 4, 0.0)
    out = R.render_core(c(x["o"]), d, c(x["z"]), x["sample_dist"], background_rgb=None if bg is None else bg.to(dtype),
                        cos_anneal_ratio=car)
    w = out["weights"]
    pn = torch.linalg.norm(net.pts.detach(), dim=-1).reshape(B, n)
    relax = (pn < 1.2).to(dtype)
    nn_ = torch.linalg.norm(normals.reshape(B, n, 3), dim=-1)
    eik = torch.stack([(relax * (nn_ - 1.0) ** 2).sum(-1), relax.sum(-1)], -1)
    nmap = (out["gradients"] * w[:, :, None]).sum(1)
    fwd = {"weights": w, "color": out["color"], "wsum": w.sum(-1), "wmax": w.max(-1)[0], "cdf": out["cdf"],
           "inside": out["inside_sphere"], "eik": eik, "nmap": nmap, "pts": net.pts.detach()}
    if cot is None:
        return {k: v.detach() for k, v in fwd.items()}, None
    k = lambda name: cot[name].to(device=dev, dtype=dtype)
    L = (fwd["color"] * k("d_color")).sum() + k("ec")[0] * (eik[:, 1].sum().detach() + 1e-5) * out["gradient_error"]
    if "d_wsum" in use:
        L = L + (fwd["wsum"] * k("d_wsum")).sum()
    if "d_weights" in use:
        L = L + (w * k("d_weights")).sum()
    if "d_gradients" in use:
        L = L + (out["gradients"].reshape(-1, 3) * k("d_gradients")).sum()
    if "d_nmap" in use:
        L = L + (nmap * k("d_nmap")).sum()
    # the part of the functional that depends on inv_s, ray by ray, and its derivative per ray (one batched backward pass)
    per_ray = (fwd["color"] * k("d_color")).sum(-1)
    if "d_wsum" in use:
        per_ray = per_ray + fwd["wsum"] * k("d_wsum")
    if "d_weights" in use:
        per_ray = per_ray + (w * k("d_weights")).sum(-1)
    if "d_nmap" in use:
        per_ray = per_ray + (nmap * k("d_nmap")).sum(-1)
    eye = torch.eye(B, dtype=dtype, device=dev)
    d_inv_rays = torch.autograd.grad(per_ray, inv_s, grad_outputs=eye, is_grads_batched=True, retain_graph=True)[0].reshape(B)
    gs = torch.autograd.grad(L, leaves, allow_unused=True)
    gs = [torch.zeros_like(t) if g_ is None else g_ for g_, t in zip(gs, leaves)]
    grads = {"d_sdf": gs[0], "d_normals": gs[1], "d_colors": gs[2], "d_inv_s": gs[3].reshape(()), "d_rays_d": gs[4],
             "d_inv_s_rays": d_inv_rays}
    return {k_: v.detach() for k_, v in fwd.items()}, grads


def scan_margins(x, car):
    """Measured on fp64 from the fp32 inputs: the smallest distance of every branched-on quantity from its switch, and how many
    elements lie on each side.  alpha_raw = (prev - next + 1e-5) / (prev + 1e-5) is restated here (the oracle does not return it).
    alpha_raw <= 1 always (next > 0, and fp32 rounding is monotone: fl(prev - next + 1e-5) <= fl(prev + 1e-5)), so the clip has
    two sides only at 0.  A zero normal has d.n == 0 exactly in every precision, where relu' is 0 in torch and in the kernel
    alike; the margin around d.n = 0 is therefore asserted on the non-zero normals, and the zero ones are counted."""
    B, n = x["z"].shape
    dist, mid, pn = _scan_geometry(x["o"], x["d"], x["z"], x["sample_dist"])
    nrm = x["normals"].double().reshape(B, n, 3)
    zero = (nrm == 0).all(-1)
    tc = (x["d"].double()[:, None, :] * nrm).sum(-1)
    ic = -(torch.relu(-tc * 0.5 + 0.5) * (1.0 - car) + torch.relu(-tc) * car)
    s = x["sdf"].double().reshape(B, n)
    inv_s = float(x["inv_s"][0])
    prev, nxt = torch.sigmoid((s - ic * dist * 0.5) * inv_s), torch.sigmoid((s + ic * dist * 0.5) * inv_s)
    araw = (prev - nxt + 1e-5) / (prev + 1e-5)
    T_end = torch.cumprod(1.0 - araw.clip(0.0, 1.0) + 1e-7, -1)[:, -1]
    big = torch.tensor(float("inf"), dtype=F64)
    nz = ~zero
    near = lambda v, c0, sgn: int(((sgn * (v - c0) > 0) & ((v - c0).abs() < 20 * SCAN_RADIUS_MARGIN)).sum())
    return {
        "radius": torch.minimum((pn - 1.0).abs().min(), (pn - 1.2).abs().min()).item(),
        "cos": torch.minimum(tc[nz].abs().min(), (tc[nz] - 1.0).abs().min()).item() if bool(nz.any()) else big.item(),
        "alpha": araw.abs().min().item(),
        "alpha_max": araw.max().item(),
        "zero_normals": int(zero.sum()), "zero_tc_exact": bool((tc[zero] == 0).all()),
        "sides": {"r<1": int((pn < 1.0).sum()), "1<=r<1.2": int(((pn >= 1.0) & (pn < 1.2)).sum()), "r>=1.2": int((pn >= 1.2).sum()),
                  "tc<0": int((tc[nz] < 0).sum()), "0<tc<1": int(((tc[nz] > 0) & (tc[nz] < 1)).sum()), "tc>1": int((tc[nz] > 1).sum()),
                  "alpha_raw<0": int((araw < 0).sum()), "alpha_raw>0": int((araw > 0).sum()),
                  "T<1e-4": int((T_end < 1e-4).sum()), "T>=1e-4": int((T_end >= 1e-4).sum()),
                  "just r<1": near(pn, 1.0, -1), "just r>1": near(pn, 1.0, 1), "just r<1.2": near(pn, 1.2, -1),
                  "just r>1.2": near(pn, 1.2, 1)},
    }


def add_sides(total, sides):
    for k_, v in sides.items():
        total[k_] = total.get(k_, 0) + v
    return total


# ------------------------------------------------------------------------------------------------ loss
LOSS_CLIP_MARGIN = 1e-5       # |ws - 1e-3|, |ws - (1 - 1e-3)|: the fp32 and fp64 thresholds differ by 5e-11 and 1.3e-8


def loss_inputs(B, mask_mode, seed):
    """fp32 inputs of dh_neus_loss.  mask_mode: "hand" (keep = 0 everywhere), "background" (obj = 0), "mixed".
    weight sums below / inside / above the BCE clip, some 2..8 margins from either threshold; colours bitwise equal to the target
    in every 5th entry; every 7th normal-map row exactly zero."""
    g = _gen(5000 + B + seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    rays = torch.zeros(B, 14, dtype=F64)
    rays[:, 6:9] = r(B, 3)
    i = torch.arange(B)
    if mask_mode == "hand":
        obj, keep = torch.zeros(B), torch.zeros(B)
    elif mask_mode == "background":
        obj, keep = torch.zeros(B), torch.ones(B)
    else:
        lab = (i * 7 + seed) % 5                      # 0,1: object; 2,3: background; 4: hand
        obj, keep = (lab < 2).double(), (lab < 4).double()
    rays[:, 9], rays[:, 10] = obj, keep
    rays[:, 11:14] = torch.nn.functional.normalize(torch.randn(B, 3, generator=g, dtype=F64), dim=-1)
    rays = rays.to(F32)
    color = r(B, 3).to(F32)
    eq = (torch.arange(B * 3) % 5 == 1).view(B, 3)
    color = torch.where(eq, rays[:, 6:9], color)
    lo, hi = 1e-3, 1.0 - 1e-3
    dl = (2.0 + 6.0 * r(B)) * LOSS_CLIP_MARGIN
    ws = torch.stack([1e-4 + 7e-4 * r(B), lo - dl, lo + dl, 0.01 + 0.98 * r(B), 0.01 + 0.98 * r(B), hi - dl, hi + dl,
                      1.0 - 8e-4 * r(B), torch.zeros(B, dtype=F64), torch.ones(B, dtype=F64) + 1e-6], 0)[(i + seed) % 10, i].to(F32)
    nmap = (torch.randn(B, 3, generator=g, dtype=F64) * 0.8)
    nmap[i % 7 == 3] = 0.0
    eik = torch.stack([3.0 * r(B), torch.floor(40.0 * r(B))], -1).to(F32)
    A = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))[0]
    return {"color": color, "wsum": ws, "nmap": nmap.to(F32), "eik": eik, "rays": rays, "R": A.to(F32).contiguous()}


def loss_margin(x):
    ws = x["wsum"].double()
    return torch.minimum((ws - 1e-3).abs().min(), (ws - (1.0 - 1e-3)).abs().min()).item()


def loss_reference(x, igr_w, mask_w, normal_w, dtype=F64):
    """O.neus_losses + autograd in `dtype`: (stats [8] as the kernel lays them out, d_color, d_wsum, d_nmap or None, eik_coef).
    gradients = nmap[:, None, :] with weights = 1 makes the oracle's n_obj the given normal map."""
    c = lambda t: t.to(dtype).clone()
    color, ws, nmap = c(x["color"]).requires_grad_(True), c(x["wsum"]).reshape(-1, 1).requires_grad_(True), c(x["nmap"]).requires_grad_(True)
    eik, rays = c(x["eik"]), c(x["rays"])
    B = color.shape[0]
    ge = eik[:, 0].sum() / (eik[:, 1].sum() + 1e-5)
    out = {"color_fine": color, "weight_sum": ws, "gradient_error": ge, "gradients": nmap[:, None, :],
           "weights": torch.ones(B, 1, dtype=dtype, device=color.device)}
    ref = O.neus_losses(out, rays[:, 6:9], rays[:, 9:10], rays[:, 10:11], igr_w, mask_w, normal_w, rays[:, 11:14], c(x["R"]))
    gs = torch.autograd.grad(ref["loss"], (color, ws, nmap), allow_unused=True)
    m = rays[:, 9] * rays[:, 10]
    stats = torch.stack([ref["loss"], ref["color_loss"], ref["eikonal_loss"], ref["mask_loss"],
                         ref.get("normal_loss", torch.zeros((), dtype=dtype, device=color.device)), ref["psnr"],
                         m.sum() + 1e-5, rays[:, 10].sum() + 1e-5]).detach()
    return {"stats": stats, "d_color": gs[0], "d_wsum": gs[1].reshape(-1), "d_nmap": gs[2] if normal_w > 0 else None,
            "eik_coef": (igr_w / (eik[:, 1].sum() + 1e-5)).reshape(1)}


# ------------------------------------------------------------------------------------------------ Adam
def adam_reference(p, g, m, v, lr, b1, b2, eps, step, grad_scale):
    """torch.optim.Adam (no weight decay, no amsgrad) restated in fp64 on the fp32 state; the hyper-parameters are the fp32 values the
    C ABI receives.  Returns (p', m', v', update, scale) with p' = p - update and scale = (lr / bc1) (|b1 m| + |(1 - b1) g|) / denom,
    the size the update would have without cancellation between the old moment and the new gradient (what rounding is relative to)."""
    f = lambda s: float(torch.tensor(s, dtype=F32))
    lr, b1, b2, eps, gs = f(lr), f(b1), f(b2), f(eps), f(grad_scale)
    p, g, m, v = p.double(), g.double() * gs, m.double(), v.double()
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = v2.sqrt() / math.sqrt(bc2) + eps
    upd = (lr / bc1) * (m2 / denom)
    scale = (lr / bc1) * ((b1 * m).abs() + ((1.0 - b1) * g).abs()) / denom
    return p - upd, m2, v2, upd, scale


# Bound on one Adam step from identical fp32 state (derivation; each fp32 operation contributes a relative 2^-24 = U32):
#   g s                          1 rounding
#   m' = b1 m + (1 - b1) g s     two products and a sum on top of it:  |err m'| <= 4 U32 (|b1 m| + |(1 - b1) g s|)
#   v' = b2 v + (1 - b2) (g s)^2 all terms >= 0:  rel err <= 6 U32  (g s twice, its square, two products, the sum)
#   denom = sqrt(v') / sqrt(bc2) + eps:  3 (half of v') + 1 (sqrt) + 1 (sqrt(bc2) as fp32) + 1 (quotient) + 1 (sum) = 7 U32
#   (lr / bc1) (m' / denom):  bc1 as fp32, two quotients, one product: 4 U32
# so |update - update64| <= (4 + 7 + 4) U32 scale, scale as in adam_reference; 16 is asserted.  p' = p - update adds half an ulp
# of p' (U32 max(|p|, |p'|)).  (g s)^2 below the fp32 normal range (|g s| < 1e-19) may lose bits or flush: that moves sqrt(v') by
# at most sqrt(2^-126) = 1.1e-19, against eps = 1e-8 a relative 1e-11 of denom -- far inside the 16th unit.  v' itself is compared
# with an absolute allowance of 2^-126 for that reason.
ADAM_UPDATE_UNITS = 16.0
ADAM_M_UNITS = 4.0
ADAM_V_UNITS = 6.0
FP32_MIN_NORMAL = 2.0 ** -126


# ------------------------------------------------------------------------------------------------ the cases (shared by the CPU and GPU tests)
UPS_N_CUR = (2, 3, 64, 65, 80, 96, 112, 127, 128)
UPS_N_NEW = (1, 2, 16, 64)
UPS_INV_S = (64.0, 128.0, 256.0, 512.0)
UPS_B = (1, 3, 5, 257)


def upsample_cases():
    """(B, n_cur, n_new, inv_s, seeds): the full product of the shapes at B = 257 (64 rays of every family in one batch), and every
    n_cur at B = 1, 3, 5 with n_new / inv_s rotating.  A batch of one ray is too small a sample for "4 x the fp32 oracle's error on the
    same inputs" to mean anything, so a small-B case is a SET of launches (32 / 12 / 8 seeds, every family in turn) and the criteria
    are evaluated on the union of their rays, every launch still being checked for range, order and canaries on its own."""
    cases = [(257, n, k, s, (0,)) for n in UPS_N_CUR for k in UPS_N_NEW for s in UPS_INV_S]
    for bi, (B, S) in enumerate(((1, 32), (3, 12), (5, 8))):
        for ni, n in enumerate(UPS_N_CUR):
            cases.append((B, n, UPS_N_NEW[(ni + bi) % 4], UPS_INV_S[(ni + 2 * bi + 1) % 4], tuple(range(S))))
    return cases


def check_upsample_case(case, run, device="cpu"):
    """Run one case through `run(o, d, z, sdf, n_new, inv_s) -> (z_new, pts_new or None)` and assert every criterion of the up-sampling
    test; returns the measurements.  Asserted on EVERY sample:
      range / order   finite, z_0 <= z_new <= z_{n-1}, non-decreasing along the ray (the contract of merge_kernel)
      CDF space       |F64(z_new_k) - u_k| <= tol,  tol = 4 x the largest residual of the oracle evaluated in fp32 on the same rays,
                      and tol < 0.25 / n_new (asserted: a sample in a wrong populated section is then at least 3 tol away)
      z space         max |z_new - z_new64| <= 4 x the fp32 oracle's maximum; share above 1e-4 <= 2 x the fp32 oracle's share
      points          pts_new = o + d z_new from the kernel's own z_new, to 2 ulp of the larger of |o_c| and |d_c z_new|
                      (one rounding of the product, one of the sum; a fused multiply-add needs less)
    and on the reference: every sample radius at least UPS_RADIUS_MARGIN off the unit sphere."""
    B, n, k, inv_s, seeds = case
    res, res32, dz, dz32 = [], [], [], []
    for seed in seeds:
        o, d, z, sdf, fam = (t.to(device) for t in upsample_inputs(B, n, seed))
        assert upsample_margins(o, d, z) >= UPS_RADIUS_MARGIN, (case, seed)
        z64, cdf64 = oracle_upsample(o, d, z, sdf, k, inv_s, F64)
        z32, _ = oracle_upsample(o, d, z, sdf, k, inv_s, F32)
        zn, pts = run(o, d, z, sdf, k, inv_s)
        assert zn.shape == (B, k) and bool(torch.isfinite(zn).all()), (case, seed, "non-finite sample")
        znd, zd = zn.double(), z.double()
        assert bool((znd >= zd[:, :1]).all()) and bool((znd <= zd[:, -1:]).all()), (case, seed, "sample outside [z_0, z_{n-1}]")
        assert bool((znd[:, 1:] >= znd[:, :-1]).all()), (case, seed, "new samples not ascending: merge_kernel's contract")
        if pts is not None:
            o64, d64 = o.double()[:, None, :], d.double()[:, None, :]
            want = o64 + d64 * znd[..., None]
            scale = torch.maximum(o64.abs().expand_as(want), (d64 * znd[..., None]).abs())
            assert bool(((pts.double().view(B, k, 3) - want).abs() <= 4.0 * U32 * scale).all()), (case, seed, "pts_new")
        res.append(cdf_residual(z, cdf64, znd, k)); res32.append(cdf_residual(z, cdf64, z32, k))
        dz.append((znd - z64).abs()); dz32.append((z32.double() - z64).abs())
    res, res32, dz, dz32 = (torch.cat(t).reshape(-1) for t in (res, res32, dz, dz32))
    m = {"case": case, "tol": 4.0 * res32.max().item(), "cap": 0.25 / k, "res": res.max().item(), "dz": dz.max().item(),
         "dz32": dz32.max().item(), "share": (dz > 1e-4).double().mean().item(), "share32": (dz32 > 1e-4).double().mean().item()}
    assert m["tol"] < m["cap"], f"{case}: the reference alone breaks the cap: 4 x {res32.max().item():.3e} >= {m['cap']:.3e}"
    assert m["res"] <= m["tol"], f"{case}: CDF-space residual {m['res']:.3e} > tol {m['tol']:.3e} (fp32 oracle x 4)"
    assert m["dz"] <= 4.0 * m["dz32"], f"{case}: max |dz| {m['dz']:.3e} > 4 x fp32 oracle {m['dz32']:.3e}"
    assert m["share"] <= 2.0 * m["share32"], f"{case}: share of |dz| > 1e-4 {m['share']:.3e} > 2 x fp32 oracle {m['share32']:.3e}"
    return m


# ------------------------------------------------------------------------------------------------ merge / coarse / mid-points
MERGE_N_CUR = (1, 2, 63, 64, 65, 127, 128)
MERGE_N_NEW = (1, 2, 16, 63, 64)
MERGE_B = (1, 3, 4, 5, 257)
MERGE_MODES = ("ties", "random", "before", "after")


def merge_inputs(B, n, k, mode, seed=0):
    """Ascending old depths [B,n] and new depths [B,k] with their sdf.  "ties": both lists live on a grid of 24 values, so new depths
    are bitwise equal to old ones and each list repeats values; "before" / "after": all new depths below / above all old ones."""
    g = _gen(31 * n + 7 * k + B + seed)
    if mode == "ties":
        q = lambda *s: torch.randint(0, 24, s, generator=g).to(F32) / 16.0 + 1.5
        z, zn = q(B, n), q(B, k)
    else:
        z, zn = 1.5 + 2.0 * torch.rand(B, n, generator=g), 1.5 + 2.0 * torch.rand(B, k, generator=g)
        if mode == "before":
            zn = zn - 2.5
        elif mode == "after":
            zn = zn + 2.5
    return z.sort(-1)[0], zn.sort(-1)[0], torch.randn(B, n, generator=g), torch.randn(B, k, generator=g)


def merge_matches(got_z, got_sdf, want_z, want_sdf):
    """The merge criterion: depths and gathered sdf bit for bit (sdf None = not requested)."""
    return torch.equal(got_z, want_z) and (got_sdf is None or torch.equal(got_sdf, want_sdf))


def merge_reference(z, zn, sdf, sdf_new):
    """cat_z_vals' sort: torch.sort(cat[z, z_new], stable) and the sdf gathered alongside."""
    zz, idx = torch.sort(torch.cat([z, zn], -1), dim=-1, stable=True)
    return zz, torch.gather(torch.cat([sdf, sdf_new], -1), 1, idx)


def coarse_inputs(B, seed=0):
    g = _gen(900 + B + seed)
    o, d, t0, _ = make_rays(B, g, 0.05, 0.9)
    near, far = (t0 - 1.0).to(F32).reshape(B), (t0 + 1.0).to(F32).reshape(B)
    return o, d, near, far, torch.rand(B, generator=g)


def coarse_reference(o, d, near, far, t_rand, n):
    """The oracle's sample_z without importance samples, fp64: near + (far - near) linspace(0, 1, n) + (t_rand - 0.5) 2 / n."""
    R = O.NeuSRenderer(None, None, None, None, n, 0, 0, 4, 1.0 if t_rand is not None else 0.0)
    return R.sample_z(o.double(), d.double(), near.double()[:, None], far.double()[:, None],
                      t_rand=None if t_rand is None else t_rand.double()[:, None])


def midpoints_reference(o, d, z, sample_dist):
    """The points render_core hands to the SDF network, fp64."""
    B, n = z.shape
    zero = torch.zeros(B * n, 3, dtype=F64, device=z.device)
    net = _StubSDF(zero[:, 0], zero)
    R = O.NeuSRenderer(None, net, _StubDeviation(torch.ones(1, dtype=F64, device=z.device)), _StubColor(zero), 64, 0, 0, 4, 0.0)
    R.render_core(o.double(), d.double(), z.double(), sample_dist)
    return net.pts


SCAN_N = (1, 2, 3, 64, 127, 128)
SCAN_B = (1, 3, 4, 5, 130)
SCAN_CAR = (0.0, 0.37, 1.0)


def scan_seeds(B):
    """Single-ray batches run with eight seeds, so that the one ray is of every kind in turn (and d_inv_s is compared per ray)."""
    return tuple(range(8)) if B == 1 else (0,)


def scan_required_sides(n):
    """The sides that a given n can populate: a negative section needs three samples, an opaque ray a long one."""
    req = ["r<1", "1<=r<1.2", "r>=1.2", "tc<0", "0<tc<1", "tc>1", "alpha_raw>0", "T>=1e-4", "just r<1", "just r>1", "just r<1.2", "just r>1.2"]
    if n >= 3:
        req.append("alpha_raw<0")
    if n >= 64:
        req.append("T<1e-4")
    return req


def assert_scan_margins(mg, where):
    assert mg["radius"] >= SCAN_RADIUS_MARGIN, (where, "radius", mg["radius"])
    assert mg["cos"] >= SCAN_COS_MARGIN, (where, "d.n", mg["cos"])
    assert mg["alpha"] >= SCAN_ALPHA_MARGIN and mg["alpha_max"] <= 1.0, (where, "alpha_raw", mg["alpha"], mg["alpha_max"])
    assert mg["zero_tc_exact"], where
