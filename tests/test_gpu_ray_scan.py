"""GPU: the dense volume-rendering scan of csrc/kernels_ray.hip (dh_render_scan_fwd / _bwd / _bwd_rays) on its own, against
oracle/neus_oracle.py's render_core in fp64 driven with stub networks that return prescribed sdf, normals and colours (tests/
ray_kernels_util.py).  The inputs reach what the networks never produce: sections of negative length (alpha_raw < 0: the clip gates
of forward and backward), normals exactly zero, mid-points a few 1e-5 either side of radius 1.0 and 1.2, d.n either side of 0 and 1,
rays whose transmittance ends below 1e-4, n = 1, 2, 3, 127.  Margins: every branched-on quantity is at least SCAN_RADIUS_MARGIN (2e-5),
SCAN_COS_MARGIN (1e-5), SCAN_ALPHA_MARGIN (2e-6) away from its switch -- asserted below on the fp64 reference over every element,
together with both sides of every switch being populated.  Also a packed case that compares d_inv_s and passes d_weights / d_gradients
(tests/test_gpu_occgrid.py does neither).

Tolerances (ray_kernels_util.ErrorLedger): relative L2 < 1e-4, and element-wise max error <= 4 x max(the oracle's own fp32 result on
the same inputs, one fp32 ulp of the tensor's largest element); the worst case of every output is printed with the measurements the
bound came from.  Applied case by case wherever a case holds a sample of elements; the outputs of at most 15 numbers (B <= 5 rays
with n <= 3, and the per-ray outputs of B <= 5 rays) are judged together per n: ray_kernels_util.pooled says which and why."""
import pytest
import torch

from oracle import occgrid_oracle as G
from tests import ray_kernels_util as U

pytestmark = pytest.mark.gpu

F32, F64 = U.F32, U.F64
FWD = ("weights", "color", "wsum", "wmax", "cdf", "eik", "nmap")
BG = (0.2, 0.5, 0.9)


def _cuda(x):
    return {k: (v.cuda().contiguous() if torch.is_tensor(v) else v) for k, v in x.items()}


@pytest.mark.parametrize("n", U.SCAN_N)
def test_scan_forward_matches_oracle(n):
    """B in {1, 3, 4, 5, 130} x cos_anneal_ratio in {0, 0.37, 1} x background NULL / set x normal_map NULL / set."""
    led, sides = U.ErrorLedger(), {}
    bg_t = torch.tensor(BG, device="cuda")
    for B in U.SCAN_B:
        for seed in U.scan_seeds(B):
            x_cpu = U.scan_inputs(B, n, seed)
            x = _cuda(x_cpu)
            for car in U.SCAN_CAR:
                mg = U.scan_margins(x_cpu, car)
                U.assert_scan_margins(mg, (n, B, seed, car))
                U.add_sides(sides, mg["sides"])
                for bg in (None, bg_t):
                    r64, _ = U.scan_reference(x, car, bg, dtype=F64)
                    r32, _ = U.scan_reference(x, car, bg, dtype=F32)
                    for want_nmap in (False, True):
                        case = f"B {B} seed {seed} car {car} bg {'set' if bg is not None else 'NULL'} nmap {'set' if want_nmap else 'NULL'}"
                        got = U.hip_scan_fwd(x, car, bg, want_nmap)
                        assert torch.equal(got["inside"], r64["inside"].float()), case
                        for k in FWD:
                            if k == "nmap" and not want_nmap:
                                assert got[k] is None
                                continue
                            led.add(k, got[k], r64[k], r32[k], case, pool=U.pooled(k, B, n))
    led.flush()
    missing = [k for k in U.scan_required_sides(n) if sides.get(k, 0) == 0]
    assert not missing, f"a side of a switch never occurred: {missing}"
    led.report(f"dense scan forward, n = {n}: populated sides {sides}")


def _check_sum(d_inv_s, g64, g32, case):
    """d_inv_s as the caller uses it: summed over the rays.  The per-ray terms cancel in the sum, so "relative" is relative to what
    the roundings are relative to, the sum of the per-ray magnitudes (on 4 rays the fp32 oracle's own sum is already 1.2e-4 off
    relative to the cancelled total): |sum - sum64| <= 1e-4 sum |ref_b|, and <= 4 x max(the fp32 oracle's error of the sum, one ulp
    of sum |ref_b|)."""
    err = abs(d_inv_s.double().sum().item() - g64["d_inv_s"].item())
    e32 = abs(g32["d_inv_s"].double().item() - g64["d_inv_s"].item())
    mag = g64["d_inv_s_rays"].abs().sum().item()
    assert abs(g64["d_inv_s_rays"].sum().item() - g64["d_inv_s"].item()) <= 1e-12 * max(mag, 1e-300), case
    assert err <= 1e-4 * mag and err <= 4.0 * max(e32, 2.0 * U.U32 * mag), f"{case}: sum of d_inv_s off by {err:.3e} (fp32 oracle {e32:.3e}, sum |ref| {mag:.3e})"


@pytest.mark.parametrize("n", U.SCAN_N)
def test_scan_backward_matches_oracle_autograd(n):
    """A random linear functional of all outputs; d_weight_sum, d_weights, d_gradients, d_normal_map all NULL, all set, and each set
    singly (U.COT_CONFIGS) for every B; cos_anneal_ratio, background and the entry point (dh_render_scan_bwd /
    dh_render_scan_bwd_rays, which adds d_rays_d through true_cos) rotate so that every n sees every combination of them.  d_inv_s is
    compared ray by ray (the reference differentiates the per-ray functionals in one batched backward pass) and as the sum over rays."""
    led, sides = U.ErrorLedger(), {}
    bg_t = torch.tensor(BG, device="cuda")
    combos = set()
    for bi, B in enumerate(U.SCAN_B):
        for seed in U.scan_seeds(B):
            x_cpu = U.scan_inputs(B, n, seed)
            x = _cuda(x_cpu)
            cot = _cuda(U.scan_cotangents(B, n, seed))
            for ci, use in enumerate(U.COT_CONFIGS):
                car = U.SCAN_CAR[(bi + ci + seed) % 3]
                bg = bg_t if (bi + ci // 3 + seed) % 2 else None
                rays = (ci + seed) % 2 == 0
                combos.add((car, bg is not None, rays))
                mg = U.scan_margins(x_cpu, car)
                U.assert_scan_margins(mg, (n, B, seed, car))
                U.add_sides(sides, mg["sides"])
                case = f"B {B} seed {seed} car {car} bg {'set' if bg is not None else 'NULL'} cotangents {use or 'all NULL'} rays {rays}"
                passed = {k: cot[k] for k in ("d_color", "ec") + tuple(use)}
                got = U.hip_scan_bwd(x, car, bg, passed, rays=rays)
                _, g64 = U.scan_reference(x, car, bg, cot, use, F64)
                _, g32 = U.scan_reference(x, car, bg, cot, use, F32)
                names = ("d_sdf", "d_normals", "d_colors") + (("d_rays_d",) if rays else ())
                for k in names:
                    led.add(k, got[k], g64[k], g32[k], case, pool=U.pooled(k, B, n))
                led.add("d_inv_s", got["d_inv_s"], g64["d_inv_s_rays"], g32["d_inv_s_rays"], case, pool=U.pooled("d_inv_s", B, n))   # ray by ray
                if B > 5:                                            # (the sum of at most five rays: judged ray by ray, in the pool)
                    _check_sum(got["d_inv_s"], g64, g32, case)
    led.flush()
    assert len(combos) == 12, combos
    missing = [k for k in U.scan_required_sides(n) if sides.get(k, 0) == 0]
    assert not missing, f"a side of a switch never occurred: {missing}"
    led.report(f"dense scan backward, n = {n}")


def test_two_scan_launches_are_bitwise_equal():
    x = _cuda(U.scan_inputs(130, 127, 0))
    cot = _cuda(U.scan_cotangents(130, 127, 0))
    a, b = U.hip_scan_fwd(x, 0.37, None, True), U.hip_scan_fwd(x, 0.37, None, True)
    assert all(torch.equal(a[k], b[k]) for k in a)
    a, b = U.hip_scan_bwd(x, 0.37, None, cot, rays=True), U.hip_scan_bwd(x, 0.37, None, cot, rays=True)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_packed_scan_adjoint_with_d_inv_s_d_weights_and_d_gradients():
    """Packed rays with hand-made segments of 0, 1, 2, 127, 128, 129 and 300 samples (one, two and three trips of the wave): forward,
    and the adjoint with EVERY cotangent set, d_inv_s included, against oracle/occgrid_oracle.py's render_packed in fp64."""
    g = torch.Generator(device="cpu").manual_seed(11)
    B = 37
    o, d, t0, _ = U.make_rays(B, g, 0.05, 0.9)
    cnt = torch.tensor([0, 1, 2, 127, 128, 129, 300], dtype=torch.int32)[torch.arange(B) % 7]
    off = (torch.cumsum(cnt.long(), 0) - cnt.long())
    N = int(cnt.sum())
    ray_idx = torch.repeat_interleave(torch.arange(B), cnt.long())
    pos = torch.arange(N) - off[ray_idx]
    step = float(torch.tensor(2.2 / 300, dtype=F32))
    t_start = ((t0.reshape(B) - 1.1)[ray_idx] + pos.double() * step).to(F32)
    pts = (o.double()[ray_idx] + d.double()[ray_idx] * (t_start.double() + 0.5 * step)[:, None])
    pn = pts.norm(dim=-1)
    assert torch.minimum((pn - 1.0).abs().min(), (pn - 1.2).abs().min()).item() >= U.SCAN_RADIUS_MARGIN, "mid-point radii off the switches"
    sdf = (0.15 + 0.2 * torch.randn(N, generator=g)).to(F32)
    normals = (torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1) * (0.7 + 0.6 * torch.rand(N, 1, generator=g))).to(F32)
    tc = (d.double()[ray_idx] * normals.double()).sum(-1)
    assert torch.minimum(tc.abs().min(), (tc - 1.0).abs().min()).item() >= 1e-6, "d.n off the relu switches"
    colors = torch.rand(N, 3, generator=g)
    car = 0.3
    cot = {"d_color": torch.randn(B, 3, generator=g), "d_wsum": torch.randn(B, generator=g), "d_weights": torch.randn(N, generator=g),
           "d_gradients": 0.1 * torch.randn(N, 3, generator=g), "d_nmap": torch.randn(B, 3, generator=g), "ec": torch.tensor([0.37])}
    dev = lambda t: t.cuda().contiguous()
    o, d, t_start, sdf, normals, colors, off, cnt, ray_idx, pts = map(dev, (o, d, t_start, sdf, normals, colors, off, cnt, ray_idx, pts))
    cot = {k: dev(v) for k, v in cot.items()}
    inv_s = torch.tensor([35.0], device="cuda")
    bg = torch.tensor(BG, device="cuda")

    def reference(dtype):
        s, nr, c, iv = (t.to(dtype).clone().requires_grad_(True) for t in (sdf, normals, colors, inv_s))
        r = G.render_packed(pts.to(dtype), s, nr, c, d.to(dtype), ray_idx, off, cnt.long(), step, iv[0], car, bg.to(dtype))
        relax = (pts.norm(dim=-1) < 1.2).to(dtype)
        k = lambda name: cot[name].to(dtype)
        L = ((r["color_fine"] * k("d_color")).sum() + (r["weight_sum"][:, 0] * k("d_wsum")).sum() + (r["weights"] * k("d_weights")).sum()
             + (nr * k("d_gradients")).sum() + (r["normal_map"] * k("d_nmap")).sum() + k("ec")[0] * (relax.sum() + 1e-5) * r["gradient_error"])
        per_ray = ((r["color_fine"] * k("d_color")).sum(-1) + r["weight_sum"][:, 0] * k("d_wsum") + (r["normal_map"] * k("d_nmap")).sum(-1)
                   + torch.zeros(B, dtype=dtype, device="cuda").index_add(0, ray_idx, r["weights"] * k("d_weights")))
        rays_ = torch.autograd.grad(per_ray, iv, grad_outputs=torch.eye(B, dtype=dtype, device="cuda"), is_grads_batched=True, retain_graph=True)[0].reshape(B)
        gs = torch.autograd.grad(L, (s, nr, c, iv))
        fwd = {"weights": r["weights"].detach(), "color": r["color_fine"].detach(), "wsum": r["weight_sum"][:, 0].detach(), "nmap": r["normal_map"].detach()}
        return fwd, {"d_sdf": gs[0], "d_normals": gs[1], "d_colors": gs[2], "d_inv_s": gs[3].reshape(()), "d_inv_s_rays": rays_}

    f64, g64 = reference(F64)
    f32, g32 = reference(F32)
    c = U.Canary("cuda")
    w, col, ws, wm = c.out("weights", N), c.out("color", B, 3), c.out("wsum", B), c.out("wmax", B)
    cdf, ins, eik, nm = c.out("cdf", N), c.out("inside", N), c.out("eik", B, 2), c.out("nmap", B, 3)
    U.hip("dh_render_scan_fwd_packed", o, d, t_start, sdf, normals, colors, inv_s, car, step, bg, B, off, cnt, w, col, ws, wm, cdf, ins, eik, nm)
    c.check()
    led = U.ErrorLedger()
    for name, got in (("weights", w), ("color", col), ("wsum", ws), ("nmap", nm)):
        led.add(name, got, f64[name], f32[name], "packed")
    c = U.Canary("cuda")
    d_sdf, d_n, d_c, d_is = c.out("d_sdf", N), c.out("d_normals", N, 3), c.out("d_colors", N, 3), c.out("d_inv_s", B)
    U.hip("dh_render_scan_bwd_packed", o, d, t_start, sdf, normals, colors, inv_s, car, step, bg, B, off, cnt, cot["d_color"], cot["d_wsum"],
          cot["d_weights"], cot["d_gradients"], cot["d_nmap"], cot["ec"], d_sdf, d_n, d_c, d_is)
    c.check()
    assert bool((d_is[cnt == 0] == 0).all()), "an empty segment contributes nothing to d_inv_s"
    for name, got in (("d_sdf", d_sdf), ("d_normals", d_n), ("d_colors", d_c)):
        led.add(name, got, g64[name], g32[name], "packed")
    led.add("d_inv_s", d_is, g64["d_inv_s_rays"], g32["d_inv_s_rays"], "packed, ray by ray")
    _check_sum(d_is, g64, g32, "packed")
    led.report("packed scan, segments of 0..300 samples, every cotangent set")
