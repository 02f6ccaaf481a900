import pytest
import torch

from oracle import neus_oracle as O
from tests.test_gpu_render_forward import make_pair, make_rays

pytestmark = pytest.mark.gpu


def _loss_inputs(B, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    rgb = torch.rand(B, 3, generator=g).to(dev)
    obj = (torch.rand(B, 1, generator=g) > 0.4).float().to(dev)
    keep = (torch.rand(B, 1, generator=g) > 0.2).float().to(dev)
    mono = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1).to(dev)
    R = torch.linalg.qr(torch.randn(3, 3, generator=g))[0].to(dev)
    return rgb, obj, keep, mono, R


def check_parameter_gradients(B, ns, ni, car, normal_w, bg, arithmetic=None, stale_batch=None, up_sample_steps=4):
    """Loss and every parameter gradient of one render against the oracle's autograd (fp64, and fp32 as the yardstick).
    arithmetic: the product renderer's (None: the library default).  stale_batch: render and differentiate that many rays first, so
    that the renderer's reused, uninitialised workspace holds another launch's tiles when the case itself runs."""
    dev = "cuda:0"
    o_r, p_r = make_pair(seed=21, jitter=0.05, n_samples=ns, n_importance=ni, up_sample_steps=up_sample_steps)
    if arithmetic is not None:
        p_r.arithmetic = arithmetic
    if stale_batch is not None:
        so, sd, snear, sfar, st_rand = make_rays(stale_batch, seed=900 + stale_batch)
        out = p_r.render(so, sd, snear, sfar, cos_anneal_ratio=car, t_rand=st_rand)
        srgb, sobj, skeep, smono, sR = _loss_inputs(stale_batch, dev, seed=stale_batch)
        O.neus_losses(out, srgb, sobj, skeep, igr_weight=0.1, mask_weight=0.1, normal_weight=normal_w, mono_normal=smono,
                      R=sR)["loss"].backward()
        torch.cuda.synchronize()
        assert p_r._ws.numel() > 0
        for m in (p_r.sdf_network, p_r.deviation_network, p_r.color_network):
            m.zero_grad(set_to_none=True)
    o, d, near, far, t_rand = make_rays(B, seed=300 + B)
    z = o_r.sample_z(o, d, near, far, t_rand=t_rand)
    rgb, obj, keep, mono, R = _loss_inputs(B, dev, seed=B)
    bg_rgb = torch.ones(1, 3, device=dev) if bg else None

    def run(renderer):
        out = renderer.render(o, d, near, far, background_rgb=bg_rgb, cos_anneal_ratio=car, z_vals=z)
        losses = O.neus_losses(out, rgb, obj, keep, igr_weight=0.1, mask_weight=0.1, normal_weight=normal_w,
                               mono_normal=mono, R=R)
        return losses["loss"]

    # oracle in fp64 (tight) and fp32 (what torch itself achieves)
    mods = (o_r.sdf_network, o_r.deviation_network, o_r.color_network)
    ref = {}
    for dtype in (torch.float32, torch.float64):
        for m in mods:
            m.to(dtype); m.zero_grad()
        o, d, near, far, z, rgb, obj, keep, mono, R = [t.to(dtype) for t in (o, d, near, far, z, rgb, obj, keep, mono, R)]
        bg_rgb = bg_rgb.to(dtype) if bg_rgb is not None else None
        loss = run(o_r)
        loss.backward()
        ref[dtype] = (loss.item(), [p.grad.detach().double().clone() for m in mods for p in m.parameters()])
    for m in mods:
        m.float()
    o, d, near, far, z, rgb, obj, keep, mono, R = [t.float() for t in (o, d, near, far, z, rgb, obj, keep, mono, R)]
    bg_rgb = bg_rgb.float() if bg_rgb is not None else None

    pm = (p_r.sdf_network, p_r.deviation_network, p_r.color_network)
    loss = run(p_r)
    loss.backward()
    torch.cuda.synchronize()
    got = [p.grad.detach().double() for m in pm for p in m.parameters()]
    names = [f"{mn}.{n}" for mn, m in zip(("sdf", "var", "col"), pm) for n, _ in m.named_parameters()]
    print(f"loss hip={loss.item():.8f} f32={ref[torch.float32][0]:.8f} f64={ref[torch.float64][0]:.8f}")
    assert abs(loss.item() - ref[torch.float64][0]) < 1e-5
    worst = 0.0
    for name, g, g32, g64 in zip(names, got, ref[torch.float32][1], ref[torch.float64][1]):
        assert g.shape == g64.shape, name
        assert torch.isfinite(g).all(), name
        scale = g64.norm().item() + 1e-12
        e_hip = (g - g64).norm().item() / scale
        e_t32 = (g32 - g64).norm().item() / scale
        worst = max(worst, e_hip)
        if e_hip > 1e-4:
            print(f"{name}: rel err hip={e_hip:.3e} torch32={e_t32:.3e} |g|={scale:.3e}")
        # stated tolerance: relative L2 error of every parameter gradient <= 2e-4 vs the fp64 oracle
        # (or within 10x of torch-fp32's own error)
        assert e_hip < 2e-4 or e_hip < 10 * e_t32, (name, e_hip, e_t32)
    print("worst rel err", worst)
    # flat gradient buffer is what the fused optimiser / all-reduce consume
    flat = p_r.store.grad_flat
    assert flat is not None and flat.numel() == 802491


@pytest.mark.parametrize("B,ns,ni,car,normal_w,bg", [(16, 64, 64, 0.3, 0.05, False), (130, 64, 64, 1.0, 0.0, True),
                                                     (48, 32, 32, 0.0, 0.05, False)])
def test_parameter_gradients_match_oracle_autograd(B, ns, ni, car, normal_w, bg):
    check_parameter_gradients(B, ns, ni, car, normal_w, bg)


def test_workspace_overwrite_is_detected():
    o_r, p_r = make_pair(seed=3, n_samples=32, n_importance=32)
    o, d, near, far, t_rand = make_rays(8, seed=1)
    out1 = p_r.render(o, d, near, far, cos_anneal_ratio=0.5, t_rand=t_rand)
    with torch.no_grad():
        p_r.render(o, d, near, far, cos_anneal_ratio=0.5, t_rand=t_rand)
    with pytest.raises(RuntimeError):
        out1["color_fine"].sum().backward()
