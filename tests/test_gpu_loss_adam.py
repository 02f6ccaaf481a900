"""GPU: the fused loss (dh_neus_loss) and fused Adam (dh_adam_step) of csrc/optim.hip on their own.

Loss: all eight statistics, the three adjoint arrays and eik_coef against oracle/neus_oracle.py's neus_losses + autograd in fp64
(gradients = nmap[:, None, :], weights = 1, so that the oracle's n_obj is the given normal map), over B around the 1024-thread
block and its strided loop, every mask mix, weight sums below / inside / above the BCE clip (at least LOSS_CLIP_MARGIN = 1e-5 from
either threshold, some within 8e-5), colours bitwise equal to the target, zero normal-map rows, and normal_weight = 0 with NULL
pointers.  Adam: against a fp64 restatement of torch.optim.Adam (licensed against torch.optim.Adam itself in
tests/test_cpu_ray_kernels_ref.py) with a derived bound on the update."""
import pytest
import torch

from tests import ray_kernels_util as U

pytestmark = pytest.mark.gpu

F32, F64 = U.F32, U.F64
U32 = U.U32


def _cuda(x):
    return {k: (v.cuda().contiguous() if torch.is_tensor(v) else v) for k, v in x.items()}


# Statistics.  Each is a sum of at most 3 B <= 15000 terms of one sign, reduced as: <= 15 sequential additions per thread (5 rays x 3
# channels), 6 shuffle steps, 16 sequential partials = 37 additions, on terms that carry <= 3 roundings of their own (difference,
# product with the mask; logf is accurate to 2 ulp), then one quotient: (37 + 3 + 1) U32 -> 48 U32 = 2.9e-6 relative is asserted.
#   loss   = colour + igr w eikonal + mask w mask + normal w normal: the same 48 U32 on the sum of the magnitudes of its parts.
#   mask   : 1 - 1e-3 is not an fp32 number: the kernel (and any fp32 evaluation) clips at fl(1 - fl(1e-3)) = 0.99900001287, the fp64
#            oracle at 0.999, so -log(1 - wc) of a clipped element differs by 1.29e-5; as a mean over the kept rays that is at most
#            1.29e-5 absolute on the mask loss (times mask_weight on the total).  At the lower threshold the difference is 5e-8.
#   psnr   = 20 log10(1 / sqrt(sq / (3 msum))): d psnr = (10 / ln 10) x relative error of the quotient = 4.35 x 48 U32, plus 4 ulp
#            of the result for sqrt, quotient and log10f.
#   msum, ksum: integer counts below 2^24 are exact; adding 1e-5 rounds once: 2 U32 relative.
STAT_UNITS = 48.0
CLIP_CONSTANT = 1.29e-5
STAT_NAMES = ("loss", "colour", "eikonal", "mask", "normal", "psnr", "mask sum", "keep sum")


def _stat_bounds(ref, igr_w, mask_w, normal_w):
    r = ref.abs()
    rel = STAT_UNITS * U32
    parts = r[1] + igr_w * r[2] + mask_w * r[3] + normal_w * r[4]
    return [rel * parts.item() + mask_w * CLIP_CONSTANT, rel * r[1].item(), rel * r[2].item(), rel * r[3].item() + CLIP_CONSTANT,
            rel * r[4].item(), 4.35 * rel + 8 * U32 * (r[5].item() if torch.isfinite(r[5]) else 0.0), 2 * U32 * r[6].item(), 2 * U32 * r[7].item()]


@pytest.mark.parametrize("B", (1, 2, 1023, 1024, 1025, 2048, 5000))
def test_neus_loss_against_oracle(B):
    igr_w, mask_w = 0.1, 0.1
    led = U.ErrorLedger()
    worst = [0.0] * 8
    for mode in ("hand", "background", "mixed"):
        for seed in range(10 if B <= 2 else 1):              # one or two rays: ten seeds walk the ray through every weight-sum class
            x_cpu = U.loss_inputs(B, mode, seed)
            assert U.loss_margin(x_cpu) >= U.LOSS_CLIP_MARGIN
            x = _cuda(x_cpu)
            for normal_w, null_normal in ((0.05, False), (0.0, False), (0.0, True)):
                case = f"B {B} masks {mode} seed {seed} normal_w {normal_w} {'NULL normal pointers' if null_normal else ''}"
                got = U.hip_loss(x["color"], x["wsum"], x["nmap"], x["eik"], x["rays"], x["R"], igr_w, mask_w, normal_w, null_normal)
                again = U.hip_loss(x["color"], x["wsum"], x["nmap"], x["eik"], x["rays"], x["R"], igr_w, mask_w, normal_w, null_normal)
                for k in ("stats", "d_color", "d_wsum", "eik_coef") + (("d_nmap",) if normal_w > 0 else ()):
                    assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), (case, k, "two launches differ: the sums are not fixed-order")
                r64 = U.loss_reference(x, igr_w, mask_w, normal_w, F64)
                r32 = U.loss_reference(x, igr_w, mask_w, normal_w, F32)
                bounds = _stat_bounds(r64["stats"], igr_w, mask_w, normal_w)
                for i, name in enumerate(STAT_NAMES):
                    g_, w_ = got["stats"][i].double().item(), r64["stats"][i].item()
                    if w_ == float("inf"):
                        assert g_ == w_, (case, name)           # psnr of an empty mask
                        continue
                    err = abs(g_ - w_)
                    worst[i] = max(worst[i], err / bounds[i] if bounds[i] > 0 else (0.0 if err == 0 else float("inf")))
                    assert err <= bounds[i], f"{case}: {name} {g_!r} vs {w_!r}: err {err:.3e} > bound {bounds[i]:.3e} (fp32 oracle err {abs(r32['stats'][i].item() - w_):.3e})"
                led.add("d_color", got["d_color"], r64["d_color"], r32["d_color"], case, pool=B <= 2)
                led.add("d_wsum", got["d_wsum"], r64["d_wsum"], r32["d_wsum"], case, pool=B <= 2)
                led.add("eik_coef", got["eik_coef"], r64["eik_coef"], r32["eik_coef"], case, pool=B <= 2)
                if normal_w > 0:
                    led.add("d_nmap", got["d_nmap"], r64["d_nmap"], r32["d_nmap"], case, pool=B <= 2)
    led.flush("the 30 launches of this B judged together")     # B <= 2: three or six numbers are no sample (ErrorLedger.add)
    print(f"loss B = {B}: worst statistic error / derived bound: " + ", ".join(f"{n_} {w:.3f}" for n_, w in zip(STAT_NAMES, worst)))
    led.report(f"loss adjoints, B = {B}")


# ------------------------------------------------------------------------------------------------ Adam
ADAM_TAIL = 300


def _adam_state(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    N = n + ADAM_TAIL
    mag = lambda lo, hi: 10.0 ** (lo + (hi - lo) * torch.rand(N, generator=g, dtype=F64))
    sign = lambda: torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0).double()
    i = torch.arange(N)
    grad = sign() * mag(-20, 4)
    grad[i % 9 == 4] = 0.0
    m = sign() * mag(-8, 2)
    v = (mag(-8, 2)) ** 2
    dead = i % 13 == 6                                        # never touched by a gradient: the eps path, update exactly 0
    grad[dead] = 0.0; m[dead] = 0.0; v[dead] = 0.0
    p = torch.randn(N, generator=g, dtype=F64) * mag(-3, 1)
    return tuple(t.to(F32) for t in (p, grad, m, v)), dead


def _check_adam_step(p, g, m, v, n, lr, b1, b2, eps, step, gs, case):
    """One kernel step from the fp32 state (p, m, v); asserts the derived bounds (ray_kernels_util: ADAM_*_UNITS) on the first n
    elements and that the elements past n are untouched.  Returns the kernel's new state."""
    p2, m2, v2 = U.hip_adam(p, g, m, v, n, lr, b1, b2, eps, step, gs)
    for a, b_, name in ((p2, p, "p"), (m2, m, "m"), (v2, v, "v")):
        assert torch.equal(a[n:].view(torch.int32), b_[n:].view(torch.int32)), (case, name, "an element past n changed")
    pr, mr, vr, upd, scale = U.adam_reference(p[:n], g[:n], m[:n], v[:n], lr, b1, b2, eps, step, gs)
    f = lambda s: float(torch.tensor(s, dtype=F32))
    gg = g[:n].double() * f(gs)
    m_bound = U.ADAM_M_UNITS * U32 * ((f(b1) * m[:n].double()).abs() + ((1.0 - f(b1)) * gg).abs())
    v_bound = U.ADAM_V_UNITS * U32 * vr + U.FP32_MIN_NORMAL
    p_bound = U.ADAM_UPDATE_UNITS * U32 * scale + U32 * torch.maximum(p[:n].double().abs(), pr.abs())
    em, ev, ep = (m2[:n].double() - mr).abs(), (v2[:n].double() - vr).abs(), (p2[:n].double() - pr).abs()
    assert bool(torch.isfinite(p2[:n]).all()), case
    assert bool((em <= m_bound).all()), (case, "exp_avg", (em / m_bound.clamp_min(1e-300)).max().item())
    assert bool((ev <= v_bound).all()), (case, "exp_avg_sq", (ev / v_bound).max().item())
    assert bool((ep <= p_bound).all()), (case, "parameter", (ep / p_bound.clamp_min(1e-300)).max().item())
    return p2, m2, v2, ((ep / p_bound.clamp_min(1e-300)).max().item(), (upd.abs() > 0).double().mean().item())


@pytest.mark.parametrize("n", (1, 255, 256, 257, 100003))
def test_adam_step_against_fp64_restatement(n):
    """grad_scale in {1, 0.125, 1/3} x step in {1, 2, 1000, 10^6}; gradients from 1e-20 to 1e4 with zeros; elements whose gradient and
    moments are all zero (update exactly 0); lr = 0 (parameters bitwise unchanged, moments still updated); elements past n unchanged."""
    worst = 0.0
    for si, gs in enumerate((1.0, 0.125, 1.0 / 3.0)):
        for ti, step in enumerate((1, 2, 1000, 10 ** 6)):
            (p, g, m, v), dead = _adam_state(n, 100 * si + ti)
            p, g, m, v, dead = p.cuda(), g.cuda(), m.cuda(), v.cuda(), dead.cuda()
            case = f"n {n} grad_scale {gs} step {step}"
            p2, m2, v2, (ratio, moving) = _check_adam_step(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, step, gs, case)
            worst = max(worst, ratio)
            assert torch.equal(p2[:n][dead[:n]], p[:n][dead[:n]]), (case, "zero gradient with zero moments must not move the parameter")
            assert moving > 0.5 or n == 1
            p3, m3, v3, _ = _check_adam_step(p, g, m, v, n, 0.0, 0.9, 0.999, 1e-8, step, gs, case + " lr 0")
            assert torch.equal(p3.view(torch.int32), p.view(torch.int32)), (case, "lr = 0 changed a parameter")
            assert torch.equal(m3, m2) and torch.equal(v3, v2), (case, "the moments do not depend on lr")
    print(f"Adam n = {n}: worst |p' - p'64| / (16 U32 scale + U32 |p|) = {worst:.3f}")


@pytest.mark.parametrize("n", (257, 100003))
def test_adam_moments_carried_over_steps(n):
    """Six consecutive steps from zero moments with the kernel's own state carried forward and a new gradient every step (grad_scale
    1/3): every step is within the one-step bound of the fp64 restatement started from the same fp32 state."""
    g0 = torch.Generator(device="cpu").manual_seed(n)
    N = n + ADAM_TAIL
    p = torch.randn(N, generator=g0).cuda()
    m, v = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    p0 = p.clone()
    for step in range(1, 7):
        grad = (torch.randn(N, generator=g0) * 10.0 ** torch.randint(-6, 3, (N,), generator=g0).float()).cuda()
        p, m, v, _ = _check_adam_step(p, grad, m, v, n, 1e-3, 0.9, 0.999, 1e-8, step, 1.0 / 3.0, f"n {n} carried step {step}")
    assert bool((m[:n] != 0).all()) and bool((v[:n] > 0).all())
    moved = (p[:n] - p0[:n]).abs()
    # |one Adam update| <= lr (1 - b1) / sqrt(1 - b2) = 3.17 lr whatever the gradients are
    assert moved.max().item() <= 6 * 3.17e-3 and moved.min().item() > 0, "six steps: every parameter moved, none by more than Adam's own bound"
