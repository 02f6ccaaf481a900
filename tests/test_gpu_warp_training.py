"""GPU: the multi-view photometric term (dh_warp_loss, DESIGN_NEXT_ROWS.md section 30) on the training path: the fused step of both
families and both samplers against the oracle's fp64 step plus the restated term (tests/warp_loss_util.py) backpropagated by autograd
to every parameter, the stacking on the other terms' adjoints, the Runner with the term off and on, and the effect of the term on the
photometric score of a short training.

The synthetic cameras stand 360 / n_frames degrees apart in azimuth and up to 69 degrees apart in elevation, and the object is some 32 px
wide at 96 x 96, so a ray seldom finds a neighbour that holds its whole patch: the oracle tests take 24 frames, a 5 x 5 patch and the
four nearest frames on either side (the hash family, whose initial surface is rougher, a 3 x 3 patch), and draw their 128 rays so that
most of those that can count are among them (_pick_pixels).  At
the networks' initialisation the surface is a sphere of radius 0.5 about an object of radius 0.3, so the scores are poor; the tests
are about the adjoints."""
import os

import numpy as np
import pytest
import torch

from oracle import neus_oracle as O
from oracle import occgrid_oracle as G
from tests import prior_loss_util as P
from tests import warp_loss_util as U
from tests.test_gpu_prior_training import _adam_state, _oracle_hash_models, _runner
from tests.test_gpu_render_forward import make_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
SETTINGS = dict(patch=2, offsets=(1, 2, 3, 4), topk=2, min_views=1, min_wsum=0.02)       # min_wsum low: the networks are at their initialisation
SETTINGS_HASH = dict(SETTINGS, patch=1)       # the hash family's initial surface is rougher: fewer rays keep a whole 5 x 5 patch valid


def _close_video():
    """(dataset, tables) where the DEFAULT settings count (min_wsum apart: the networks are at their initialisation): 9 cameras 2 degrees
    apart on an arc of radius 2.3 about the origin, 96 x 96, every pixel an object pixel with a smooth texture of its own per frame.
    The texture belongs to no surface -- the scores mean nothing -- but the 11 x 11 patch of a ray that meets the initial sphere lies
    inside every neighbour, so the two-slot kernel and all of offsets 1, 2, 4 run in the step."""
    import math
    from dynhor_amd import warp_loss
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.scene import look_at_pose
    F, H, W = 9, 96, 96
    f = 1.2 * H
    K = torch.tensor([[f, 0, W // 2], [0, f, H // 2], [0, 0, 1]], dtype=torch.float32)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    Rs, Ts, rgb = [], [], []
    for i in range(F):
        az = math.radians(2.0 * (i - F // 2))
        R, T = look_at_pose(torch.tensor([2.3 * math.cos(0.2) * math.cos(az), 2.3 * math.cos(0.2) * math.sin(az), 2.3 * math.sin(0.2)]))
        Rs.append(R); Ts.append(T)
        x = xs + 2.0 * i
        g = 128 + 50 * torch.sin(0.55 * x + 0.3) * torch.cos(0.47 * ys + 1.0) + 40 * torch.sin(0.23 * x + 0.31 * ys + 2.0)
        rgb.append(torch.stack([g, g * 0.9 + 10, 255 - g], -1).round().clamp(0, 255).to(torch.uint8))
    frames = {"rgb": torch.stack(rgb), "label": torch.ones(F, H, W, dtype=torch.int8), "normal": torch.full((F, H, W, 3), 128, dtype=torch.uint8),
              "R": torch.stack(Rs).float(), "T": torch.stack(Ts).float(), "K": K}
    ds = Dataset(frames=frames, device=DEV)
    return ds, warp_loss.frames_for(ds, range(F), min_wsum=0.02)


@pytest.fixture(scope="module")
def video():
    """(dataset, tables): 24 frames of 96 x 96 and the term's tables over all of them."""
    from dynhor_amd import warp_loss
    from dynhor_amd.dataset import Dataset
    ds = Dataset.from_synthetic(n_frames=24, H=96, W=96, seed=7, device=DEV, depth=True)
    return ds, warp_loss.frames_for(ds, range(24), **SETTINGS)


def _pick_pixels(ds, tb, frame, B, seed, step):
    """B pixels of a frame for a step test.  Candidates: up to 1024 pixels whose source patch the kernel accepts
    (match.usable_sources).  step(rays, near, far, warp) runs the family's fused step on all of them once and the flags the term left
    say which rays count at the networks' present state; up to 3 B / 4 of those and, to fill up, rays that do not count are taken.
    Returns (px, py, sel): sel indexes the candidates, so a caller that fixed the candidates' samples (z_vals, or the marcher's u) in
    `step` gives the chosen rays the very samples they had there, and a ray's flags, which depend on that ray alone, stay what they
    were."""
    from dynhor_amd import warp_loss
    from dynhor_amd.match import usable_sources
    ok = usable_sources(tb.gray[frame:frame + 1], tb.valid[frame:frame + 1], tb.settings.patch, tb.settings.min_va)[0]
    idx = ok.reshape(-1).nonzero().reshape(-1)
    g = torch.Generator(device="cpu").manual_seed(seed)
    idx = idx[torch.randperm(idx.numel(), generator=g).to(idx.device)][:1024]
    W = tb.gray.shape[2]
    px, py = (idx % W).contiguous(), (idx // W).contiguous()
    rays = ds.gen_rays_at_pixels(frame, px, py)
    near, far = ds._last_near_far
    flags = step(rays, near, far, warp_loss.step_input(tb, ds, frame, 0.5, pixels=(px, py)))
    counted, other = (flags == 0).nonzero().reshape(-1), (flags != 0).nonzero().reshape(-1)
    sel = torch.cat([counted[:3 * B // 4], other])[:B]
    assert sel.numel() == B, (sel.numel(), idx.numel())
    return px[sel].contiguous(), py[sel].contiguous(), sel


def _restated(ds, tb, frame, pix, rays, R, weights, mid, nmap, cells_from):
    """The term's L in fp64 on the CPU, differentiable w.r.t. the oracle's weights [B,n] (zero-padded) and normal map [B,3] through
    .cpu(); the cells and the wsum gate are the float32 form's on the kernel's own inputs cells_from = (zc, wsum, nmap) of the HIP step."""
    c = lambda t: t.detach().cpu()
    args = (c(tb.gray), c(tb.valid), c(ds.R).float(), c(ds.T).float(), c(tb.K), c(tb.Kinv), c(tb.nbr), frame, c(pix))
    zc32, w32, n32 = (c(t).float() for t in cells_from)
    r32 = U.warp_eval(*args, zc32, w32, n32, tb.settings, dtype=torch.float32, grad=False)
    W = weights.sum(1)
    Ws = torch.where(W > 0, W, torch.ones_like(W))
    t = (weights * mid).sum(1) / Ws
    Rm = R.double().reshape(9)
    d = rays[:, 3:6].double()
    zc = t * (Rm[6] * d[:, 0] + Rm[7] * d[:, 1] + Rm[8] * d[:, 2])
    r = U.warp_rule(*args, zc.cpu(), w32, nmap.cpu(), tb.settings, dtype=F64, cells=r32["cells"])
    cnt = int(r["counts"].sum())
    return r["l"].sum() / max(cnt, 1), cnt, r


def _kernel_inputs(ren, tb, rays, R, z, packed=None):
    """(zc, wsum, nmap) as the step's own kernels formed them, from the renderer's last state."""
    from dynhor_amd.warp_loss import ray_depth
    s = ren.last_state
    t, wsum, zc = ray_depth(rays, R.contiguous().float(), z, s.weights, s.m.step if packed else s.sample_dist, packed=packed)
    return zc, wsum, s.nmap


def _flat_grad(mods):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for m in mods for p in m.parameters()])


@pytest.mark.parametrize("family", ["neus", "hash", "neus_default_patch"])
def test_fused_train_step_with_the_term_matches_oracle(video, family):
    """neus_default_patch: the MLP family on _close_video with the module's default settings (patch 5, offsets 1 2 4 8, topk 4,
    min_views 2), the configuration a training runs."""
    from dynhor_amd import warp_loss
    ds, tb = _close_video() if family == "neus_default_patch" else video
    if family.startswith("neus"):
        o_r, p_r = make_pair(seed=41, jitter=0.05, n_samples=32, n_importance=32)
        sd, nw = 2.0 / 32, 0.0                       # normal_weight 0: the term alone makes the d_nmap path
    else:
        from tests.test_gpu_hash_family import make_hash_pair
        o_r, p_r = make_hash_pair(seed=5)
        sd, nw = 2.0 / 16, 0.05
        tb = warp_loss.frames_for(ds, range(24), **SETTINGS_HASH)
    # hash: the frame of the 24 whose usable pixels most often find a neighbour at that family's initial surface (between 6 and 303 of
    # them, frame by frame)
    B, frame, car, ww = 128, {"neus": 5, "hash": 18, "neus_default_patch": 4}[family], 0.4, 0.5
    R = ds.R[frame]
    g = torch.Generator(device=DEV); g.manual_seed(5)
    kept = {}

    def first(rays_, near_, far_, warp_):
        with torch.no_grad():
            kept["z"] = o_r.sample_z(rays_[:, :3], rays_[:, 3:6], near_, far_, t_rand=torch.rand(rays_.shape[0], 1, device=DEV, generator=g))
        p_r.sample_z = lambda *a, **k: kept["z"]
        p_r.train_step_core(rays_, near_, far_, R, car, 0.1, 0.1, nw, warp=warp_)
        return p_r.last_warp_rays[1][:, 2].clone()

    px, py, sel = _pick_pixels(ds, tb, frame, B, 5, first)
    rays = ds.gen_rays_at_pixels(frame, px, py)
    near, far = ds._last_near_far
    warp = warp_loss.step_input(tb, ds, frame, ww)
    z = kept["z"][sel].contiguous()
    p_r.sample_z = lambda *a, **k: z
    torch.cuda.set_sync_debug_mode("error")
    try:
        stats = p_r.train_step_core(rays, near, far, R, car, 0.1, 0.1, nw, warp=warp).clone()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    ws = p_r.last_warp_stats.clone()
    got = p_r.store.grad_flat.double().clone()
    cells_from = _kernel_inputs(p_r, tb, rays, R, z)
    p_r.train_step_core(rays, near, far, R, car, 0.1, 0.1, nw)
    plain = p_r.store.grad_flat.double().clone()
    mods = (o_r.sdf_network, o_r.deviation_network, o_r.color_network)
    for m in mods:
        m.double(); m.zero_grad()
    r64 = rays.double()
    out = o_r.render(r64[:, :3], r64[:, 3:6], near.double(), far.double(), cos_anneal_ratio=car, z_vals=z.double())
    ref = O.neus_losses(out, r64[:, 6:9], r64[:, 9:10], r64[:, 10:11], 0.1, 0.1, nw, r64[:, 11:14], R.double())
    nmap = (out["gradients"] * out["weights"][:, :, None]).sum(dim=1)
    L, cnt, r = _restated(ds, tb, frame, warp.pix, rays, R, out["weights"], P.midpoints(z.double(), sd), nmap, cells_from)
    total = ref["loss"] + ww * L.to(DEV)
    total.backward()
    gref = _flat_grad(mods)
    for m in mods:
        m.float()
    rel = ((got - gref).norm() / gref.norm()).item()
    print(f"{family}: loss {stats[0].item():.6f} (oracle {total.item():.6f}); L {ws[0].item():.6f} ({L.item():.6f}) over {int(ws[1])} rays ({cnt}); "
          f"mean score {ws[2].item():.4f}; lost to flags 1/2/8/wsum {ws[4:].tolist()}; grad rel err {rel:.2e}; "
          f"with vs without the term {((plain - gref).norm() / gref.norm()).item():.2e}")
    assert cnt >= 40 and int(ws[1]) == cnt
    assert abs(ws[0].item() - L.item()) < 2e-5 * max(1.0, abs(L.item()))
    assert abs(stats[0].item() - total.item()) < 2e-5 * max(1.0, abs(total.item()))
    assert rel < 1e-4
    assert ((plain - gref).norm() / gref.norm()).item() > 1e-3, "the term really contributes"


def test_fused_step_on_packed_rays_with_the_term_matches_oracle(tmp_path):
    """The pattern of tests/test_gpu_prior_training.py::test_fused_step_on_packed_rays_with_priors_matches_oracle, with its
    gradient bounds; the loss within 2e-5 max(1, |loss|) as on the other two paths."""
    from dynhor_amd import warp_loss
    r = _runner(tmp_path, "hash", "occgrid", train={"batch_size": 128, "learning_rate": 5e-3},
                synthetic={"n_frames": 24, "H": 96, "W": 96, "seed": 7})
    ren, ds = r.renderer, r.dataset
    dev = torch.device(DEV)
    tb = warp_loss.frames_for(ds, range(24), **SETTINGS_HASH)
    gj = torch.Generator(device=dev); gj.manual_seed(17)
    with torch.no_grad():
        r.sdf_network.lin0.weight_v.add_(0.05 * torch.randn(r.sdf_network.lin0.weight_v.shape, device=dev, generator=gj))
        r.sdf_network.encoding.table.add_(0.005 * torch.randn(r.sdf_network.encoding.table.shape, device=dev, generator=gj))
    r.store.bump()
    o_sdf, o_col, o_var = _oracle_hash_models(r, dev)
    g = torch.Generator(device=dev); g.manual_seed(3)
    ren.update_grid(jitter=torch.rand(ren.grid.res ** 3, 3, device=dev, generator=g))
    B, frame, car, ww = 128, 20, 0.2, 0.5      # the frame whose usable pixels most often find a neighbour at this renderer's initial surface
    kept = {}

    def first(rays_, near_, far_, warp_):
        kept["u"] = torch.rand(rays_.shape[0], 1, device=dev, generator=g)
        ren._march_iter = 1
        ren.train_step_core(rays_, near_, far_, ds.R[frame], car, 0.1, 0.1, 0.0, t_rand=kept["u"], warp=warp_)
        return ren.last_warp_rays[1][:, 2].clone()

    px, py, sel = _pick_pixels(ds, tb, frame, B, 3, first)
    rays = ds.gen_rays_at_pixels(frame, px, py)
    near, far = ds._last_near_far
    warp = warp_loss.step_input(tb, ds, frame, ww)
    u = kept["u"][sel].contiguous()
    ren._march_iter = 1
    stats = ren.train_step_core(rays, near, far, ds.R[frame], car, 0.1, 0.1, 0.0, t_rand=u, warp=warp).clone()
    torch.cuda.synchronize()
    ws = ren.last_warp_stats.clone()
    got = r.store.grad_flat.double().clone()
    m = ren.last_state.m
    cells_from = _kernel_inputs(ren, tb, rays, ds.R[frame], m.t_start, packed=(m.off, m.cnt, ren._cap_ladder[0]))
    cells_from = tuple(t.clone() for t in cells_from)
    N = int(m.n_dev)
    pts, dirs, ridx, t_start = m.pts[:N].double(), m.dirs[:N].double(), m.ray_idx[:N].long(), m.t_start[:N].clone()
    off, cnt_ = m.off.clone(), m.cnt.clone()
    for mod in (o_sdf, o_col, o_var):
        mod.double(); mod.zero_grad()
    out = o_sdf(pts)
    nrm = o_sdf.gradient(pts).reshape(-1, 3)
    colr = o_col(pts, nrm, dirs, out[:, 1:])
    inv_s = o_var(torch.zeros(1, 3, device=dev, dtype=F64))[:, :1].clip(1e-6, 1e6).reshape(())
    ro = G.render_packed(pts, out[:, 0], nrm, colr, rays[:, 3:6].double(), ridx, off, cnt_.long(), float(m.step), inv_s, car)
    rd = {"color_fine": ro["color_fine"], "weight_sum": ro["weight_sum"], "gradient_error": ro["gradient_error"]}
    r64 = rays.double()
    ref = O.neus_losses(rd, r64[:, 6:9], r64[:, 9:10], r64[:, 10:11], 0.1, 0.1, 0.0)
    k = torch.arange(N, device=dev) - off[ridx]
    nmax = int(cnt_.max())
    w_pad = torch.zeros(B, nmax, dtype=F64, device=dev).index_put((ridx, k), ro["weights"])
    mid_pad = torch.zeros(B, nmax, dtype=F64, device=dev).index_put((ridx, k), (t_start + 0.5 * torch.tensor(m.step, device=dev)).double())
    L, cnt, _ = _restated(ds, tb, frame, warp.pix, rays, ds.R[frame], w_pad, mid_pad, ro["normal_map"], cells_from)
    total = ref["loss"] + ww * L.to(dev)
    total.backward()
    print(f"occgrid: loss {stats[0].item():.6f} (oracle {total.item():.6f}); L {ws[0].item():.6f} ({L.item():.6f}) over {int(ws[1])} rays ({cnt}); "
          f"lost to flags 1/2/8/wsum {ws[4:].tolist()}")
    assert cnt >= 40 and int(ws[1]) == cnt
    assert abs(stats[0].item() - total.item()) < 2e-5 * max(1.0, abs(total.item()))
    assert abs(ws[0].item() - L.item()) < 2e-5 * max(1.0, abs(L.item()))
    named = {}
    for mod, pre in ((o_sdf, "sdf."), (o_var, "var."), (o_col, "col.")):
        for n_, p in mod.named_parameters():
            named[pre + n_] = p.grad
    st = r.store
    tab = named["sdf.encoding.table"]
    (_, off0, cnt0) = st.slices[0]
    rel_tab = ((got[off0:off0 + cnt0].view_as(tab) - tab).norm() / tab.norm()).item()
    flat_ref = torch.cat([named[k_].reshape(-1) for k_ in named if "table" not in k_ and k_.startswith("sdf.")]
                         + [named["var.variance"].reshape(-1)] + [named[k_].reshape(-1) for k_ in named if k_.startswith("col.")])
    rel_rest = ((got[off0 + cnt0:] - flat_ref).norm() / flat_ref.norm()).item()
    print(f"occgrid with the term: table grad rel {rel_tab:.2e}; MLP + variance gradients rel {rel_rest:.2e}")
    assert rel_tab < 2e-3 and rel_rest < 2e-3
    ren._march_iter = 1
    ren.train_step_core(rays, near, far, ds.R[frame], car, 0.1, 0.1, 0.0, t_rand=u)
    assert ((r.store.grad_flat.double()[off0 + cnt0:] - flat_ref).norm() / flat_ref.norm()).item() > 1e-3, "the term really contributes"
    for mod in (o_sdf, o_col, o_var):
        mod.float()


def test_term_stacks_on_the_other_terms_in_the_step():
    """With the correspondence term, the depth term and normal_skip_missing all on: the loss and the gradient are linear in the terms."""
    from dynhor_amd import warp_loss
    from dynhor_amd.dataset import Dataset
    ds = Dataset.from_synthetic(n_frames=24, H=96, W=96, seed=7, device=DEV, correspondences=256, depth=True)
    tb = warp_loss.frames_for(ds, range(24), **SETTINGS_HASH)
    _, p_r = make_pair(seed=41, jitter=0.05, n_samples=32, n_importance=32)
    sample_z = p_r.sample_z
    # 96 rays through matched pixels, 32 anywhere: of six frames the one where most of them count
    best = None
    for frame in (0, 2, 5, 18, 20, 22):
        g = torch.Generator(device=DEV); g.manual_seed(5)
        rays, corr, _ = ds.gen_corr_rays_at(frame, 128, 96, generator=g)
        warp = warp_loss.step_input(tb, ds, frame, 0.5)
        prior = ds.prior_depth_at(frame, *ds._last_pixels)
        near, far = ds._last_near_far
        z = sample_z(rays[:, :3].contiguous(), rays[:, 3:6].contiguous(), near, far, t_rand=torch.rand(128, 1, device=DEV, generator=g))
        p_r.sample_z = lambda *a, z=z, **k: z
        p_r.train_step_core(rays, near, far, ds.R[frame], 0.4, 0.1, 0.1, 0.05, warp=warp)
        n = int(p_r.last_warp_stats[1])
        if best is None or n > best[0]:
            best = (n, frame, rays, corr, warp, prior, near, far, z)
    n, frame, rays, corr, warp, prior, near, far, z = best
    print(f"stacking: frame {frame}, {n} of 128 rays count")
    p_r.sample_z = lambda *a, **k: z
    others = dict(corr=corr, corr_weight=0.5, corr_frames=ds.corr_frames(), corr_delta_px=4.0, prior_depth=prior, depth_weight=0.5,
                  normal_skip_missing=True)
    step = lambda nw, **kw: (p_r.train_step_core(rays, near, far, ds.R[frame], 0.4, 0.1, 0.1, nw, **kw).clone(),
                             p_r.store.grad_flat.double().clone())
    both, g_both = step(0.05, warp=warp, **others)
    assert int(p_r.last_warp_stats[1]) == n >= 20, "rays must count for the term to be there"
    only_others, g_others = step(0.05, **others)
    only_warp, g_warp = step(0.05, warp=warp)
    plain, g_plain = step(0.05)
    assert abs((both[0] - only_others[0] - only_warp[0] + plain[0]).item()) < 1e-5
    want = g_others + g_warp - g_plain
    assert ((g_both - want).norm() / want.norm()).item() < 1e-4
    assert ((g_both - g_others).norm() / g_others.norm()).item() > 1e-3
    # normal_weight 0: the term alone makes the d_nmap path, and it is the same term
    w0, g_w0 = step(0.0, warp=warp)
    p0, g_p0 = step(0.0)
    assert ((g_w0 - g_p0).norm() / g_p0.norm()).item() > 1e-3
    d1, d0 = g_warp - g_plain, g_w0 - g_p0
    assert ((d1 - d0).norm() / d0.norm()).item() < 1e-3, "the term's own gradient does not depend on the normal term being on"
    with pytest.raises(ValueError, match="pose adjoint"):
        p_r.train_step_core(rays, near, far, ds.R[frame], 0.4, 0.1, 0.1, 0.0, warp=warp, ray_grads=True)


NEW_TAGS = ("ray_depth", "warp_loss", "ray_depth_bwd")
VIDEO = {"n_frames": 16, "H": 64, "W": 64, "seed": 11}
ON = {"warp_weight": 0.5, "warp_patch": 1, "warp_offsets": [1, 2, 3, 4], "warp_topk": 2, "warp_min_views": 1, "warp_min_wsum": 0.02}


def test_runner_with_the_term_off_launches_nothing_new(tmp_path):
    from dynhor_amd.runner import DEFAULT_CONF
    from dynhor_amd.warp_loss import DEFAULTS
    a = _runner(tmp_path / "a", train={"warp_weight": 0.0, "warp_patch": 3})
    b = _runner(tmp_path / "b")
    a.renderer.timer.enabled = True
    for _ in range(5):
        a.train_iteration(); b.train_iteration()
    torch.cuda.synchronize()
    assert not set(NEW_TAGS) & set(a.renderer.timer.records), "with the weight at 0 no new kernel is launched"
    assert a.warp_tables is None and not hasattr(a.renderer, "last_warp_stats")
    assert all(torch.equal(x, y) for x, y in zip(_adam_state(a), _adam_state(b)))
    assert DEFAULT_CONF["train"]["warp_weight"] == 0.0 and all("warp_" + k in DEFAULT_CONF["train"] for k in DEFAULTS)


def test_runner_refuses_the_term_with_pose_refinement(tmp_path):
    with pytest.raises(ValueError, match=r"warp_weight.*refine_poses"):
        _runner(tmp_path, train={"warp_weight": 0.5, "refine_poses": True})
    with pytest.raises(ValueError, match="warp_wieght"):
        _runner(tmp_path, train={"warp_wieght": 0.5})


@pytest.mark.parametrize("family,sampler", [("neus", None), ("hash", "hierarchical"), ("hash", "occgrid")])
def test_runner_trains_with_the_term_on(tmp_path, family, sampler):
    from dynhor_amd import warp_loss
    train = dict(ON, warp_start_iter=3, holdout="every:4", report_freq=10)
    r = _runner(tmp_path / "a", family, sampler, synthetic=VIDEO, train=train)
    r.renderer.timer.enabled = True
    built = []
    orig = warp_loss.frames_for
    warp_loss.frames_for = lambda *a, **k: (built.append(1), orig(*a, **k))[1]
    try:
        for i in range(20):
            s = r.train_iteration()
            if i < 3:
                assert r.warp_tables is None, "the tables wait for warp_start_iter"
    finally:
        warp_loss.frames_for = orig
    torch.cuda.synchronize()
    assert len(built) == 1 and r.warp_tables is not None, "the grey tables are built once"
    assert set(NEW_TAGS) <= set(r.renderer.timer.records) and all(len(r.renderer.timer.records[t]) == 17 for t in NEW_TAGS)
    held = set(r.holdout_frames)
    assert held and not held & set(r.warp_tables.nbr.reshape(-1).tolist()), "a held-out frame never appears in nbr"
    assert torch.isfinite(s).all() and torch.isfinite(r.store.flat).all()
    rec = r.report(s)
    for k in ("Loss/warp_loss", "Statistics/warp_score", "Statistics/warp_rays"):
        assert k in rec and np.isfinite(rec[k]), k
    from dynhor_amd.tb_events import read_scalars
    r.close()
    d = os.path.join(r.base_exp_dir, "board")
    tags = {tag for fn in os.listdir(d) for _, tag, _ in read_scalars(os.path.join(d, fn))}
    assert {"Loss/warp_loss", "Statistics/warp_score", "Statistics/warp_rays"} <= tags, tags
    # a second run of 20 iterations: every parameter and both Adam moments bit for bit
    r2 = _runner(tmp_path / "b", family, sampler, synthetic=VIDEO, train=train)
    for _ in range(20):
        r2.train_iteration()
    assert all(torch.equal(x, y) for x, y in zip(_adam_state(r), _adam_state(r2)))


def test_runner_resumes_with_the_term(tmp_path):
    from dynhor_amd.runner import Runner
    conf = {"seq_name": "warp", "exp_name": "resume", "data_info": {"synthetic": VIDEO},
            "train": dict(ON, batch_size=256, report_freq=10 ** 9, save_freq=10 ** 9, val_freq=0, warm_up_end=4, end_iter=100)}
    a = Runner(conf=conf, device=DEV, exp_root=str(tmp_path))
    a.train(6)
    a.save_checkpoint()
    a.train(5)
    b = Runner(conf=conf, device=DEV, exp_root=str(tmp_path), is_continue=True)
    assert b.iter_step == 6 and b.warp_tables is None
    b.train(5)
    assert b.warp_tables is not None and torch.equal(a.store.flat, b.store.flat), "the resumed run reproduces the uninterrupted one bit for bit"


def test_term_raises_the_photometric_score_of_a_short_training(tmp_path):
    """8 frames of 64 x 64, batch 512, 200 iterations, the same seeds, without the term and with it at weight 0.5; scored as the mean
    chosen score of ONE fixed set of 256 object rays through the term's own kernels at weight 0 (stats[2]).  Only the order is asserted;
    both scores, the counted rays and the mean |z^ - z_true| of those rays (dh_prior_loss's stats[2], the measure of section 27) are
    printed (DESIGN_NEXT_ROWS.md section 30 records them as measured).  The cameras of 8 synthetic frames stand 45 degrees apart and
    the object is some 21 px wide: a 3 x 3 patch, every other frame as a neighbour, one view; on the analytic surface 39 of the 171
    pixels with a usable source patch count then (CPU restatement), so the mean is asked to stand on at least 10 rays."""
    from dynhor_amd import warp_loss
    from dynhor_amd.renderer import prior_loss
    from tests.test_gpu_prior_training import _mixed_pixels
    keys = {"warp_patch": 1, "warp_offsets": [1, 2, 3, 4], "warp_topk": 2, "warp_min_views": 1}
    score = {}
    for name, w in (("without", 0.0), ("with", 0.5)):
        r = _runner(tmp_path / name, synthetic={"n_frames": 8, "depth": True}, train=dict(keys, batch_size=512, warp_weight=w))
        r.train(200)
        ds, ren = r.dataset, r.renderer
        frame = 1
        px, py = _mixed_pixels(ds, frame, 512, seed=21)
        px, py = px[:256].contiguous(), py[:256].contiguous()                 # the object half
        rays = ds.gen_rays_at_pixels(frame, px, py)
        near, far = ds._last_near_far
        prior = ds.prior_depth_at(frame, px, py)
        o, d = rays[:, :3].contiguous(), rays[:, 3:6].contiguous()
        z = ren.sample_z(o, d, near, far, perturb_overwrite=0)
        st = ren._forward_core(o, d, z, 1.0, None, want_nmap=True, infer_only=True)
        tb = warp_loss.frames_for(ds, r.train_frames, patch=1, offsets=(1, 2, 3, 4), topk=2, min_views=1)
        Rf = ds.R[frame].contiguous()
        ws, _, _ = warp_loss.warp_term(warp_loss.step_input(tb, ds, frame, 0.0, pixels=(px, py)), rays, Rf, z, st.weights, st.nmap,
                                       st.sample_dist, None, None, False, False)
        ps = prior_loss(rays, Rf, z, st.weights, None, prior, st.sample_dist, 0.0, P.DELTA, 0.0, False, torch.empty_like(st.weights), None)
        score[name] = (ws[2].item(), int(ws[1].item()), ps[2].item())
    print(f"mean chosen score over 256 fixed object rays after 200 iterations: without the term {score['without'][0]:.4f} "
          f"({score['without'][1]} rays count), with it {score['with'][0]:.4f} ({score['with'][1]}); mean |z^ - z_true| without "
          f"{score['without'][2]:.5f}, with {score['with'][2]:.5f}")
    assert score["with"][1] >= 10 and score["without"][1] >= 10
    assert score["with"][0] > score["without"][0]
