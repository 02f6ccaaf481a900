"""GPU: pose refinement of the hash-grid family on both samplers (DESIGN_NEXT_ROWS.md section 28).  Kernel by kernel -- the point
adjoint of the geometry network (dh_hash_geo_backward_rays), the direction adjoint of the colour network
(dh_hash_color_backward_rays), the packed scan with the direction adjoint (dh_render_scan_bwd_packed_rays), the per-ray fold
(dh_ray_adjoint_packed) -- then the whole training step against the oracle with the rays as fp64 leaves, then the Runner.

Tolerance rule: every allowance is 4 x the deviation of the same oracle run eagerly in fp32 from its fp64 run on the same inputs (the
+-0.5 / fd_eps cotangents of the finite-difference normals cancel in fp32, in the oracle as in the kernels).  Points whose cell the fp32
kernel and the fp64 oracle may assign differently are marked by tests/hash_pose_util.ambiguous and left out where a test says so; the
share left out is asserted to be at most 10 %.  Each test prints the measured error next to its allowance."""
import pytest
import torch

from oracle import neus_oracle as O
from oracle import occgrid_oracle as G
from tests import hash_pose_util as U
from tests.test_gpu_hash_family import make_hash_pair
from tests.test_gpu_occgrid import _blob_grid, _hip_march, _oracle_hash_models, _rays

pytestmark = pytest.mark.gpu
MARGIN = 4.0
SENTINEL = -777.25


def _p(t):
    from dynhor_amd.renderer import _p as p
    return p(t)


@pytest.fixture(scope="module")
def pair():
    return make_hash_pair()


def _check(name, got, ref, eager, margin=MARGIN):
    """Both errors of `got` against the fp64 `ref` within margin x those of the fp32 eager oracle `eager`; prints all of them."""
    e, a = U.two_errors(got, ref), U.two_errors(eager, ref)
    print(f"{name}: error norm / reference norm {e[0]:.2e} (allowance {margin:g} x {a[0]:.2e}); worst row / largest row {e[1]:.2e} "
          f"(allowance {margin:g} x {a[1]:.2e})")
    assert ref.double().norm().item() > 0
    assert e[0] <= margin * a[0] and e[1] <= margin * a[1], name
    return e, a


# ------------------------------------------------------------------ 1. point adjoint of the geometry network
def _geo_backward(p_r, x, cot, rays, cap=None, n_act=None):
    """Forward (saving) + geometry backward through the C ABI at capacity `cap` (default: all n rows in use).  Returns (d_pts or None,
    the workspace's bits)."""
    from dynhor_amd import _lib
    L, st = _lib.lib(), p_r.store
    n = x.shape[0]
    P = n if cap is None else cap
    pad = lambda t: torch.cat([t, torch.zeros(P - n, *t.shape[1:], device=t.device)]).contiguous()
    pts, (d_sdf, d_feat, d_grad) = pad(x), [pad(c) for c in cot]
    s = p_r.net_state(pts, pts, 1, 1, n_active=n_act)
    p_r._net_forward(s, st.ensure_packed())
    head = (_p(st.flat), _p(st.packed), _p(pts), _p(d_sdf), _p(d_feat), _p(d_grad), P, p_r.radius, p_r.fd_eps, _p(s.ws), _p(n_act))
    d_pts = None
    if rays:
        d_pts = torch.full((P, 3), SENTINEL, device=x.device)
        _lib.check(L.dh_hash_geo_backward_rays(*head, _p(d_pts), _lib.stream()))
    else:
        _lib.check(L.dh_hash_geo_backward(*head, _lib.stream()))
    torch.cuda.synchronize()
    return d_pts, s.ws[:p_r._workspace_need(P, False)].view(torch.int32).clone()


@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_point_adjoint_matches_fp64_autograd(pair, n):
    o_r, p_r = pair
    x, share = U.unmarked_points(n, seed=n, device="cuda")
    assert share <= U.MAX_MARKED                          # drawn from a pool, filtered before the call: every row is compared
    cot = U.geo_cotangents(n, seed=n + 1, device="cuda")
    net = o_r.sdf_network
    eager = U.oracle_point_adjoint(net, x, *cot)
    net.double()
    ref = U.oracle_point_adjoint(net, x, *cot)
    net.float()
    d_pts, ws_rays = _geo_backward(p_r, x, cot, rays=True)
    _check(f"d_pts, n = {n}", d_pts, ref, eager)
    # the rows the weight gradients read are those of the plain call, bit for bit
    _, ws_plain = _geo_backward(p_r, x, cot, rays=False)
    assert torch.equal(ws_rays, ws_plain)
    # launch to launch
    again, _ = _geo_backward(p_r, x, cot, rays=True)
    assert torch.equal(again, d_pts)
    # n_active: rows past the device count keep the sentinel, the rows below it are the full run's
    if n > 37:
        cap = (n + 7) // 8 * 8
        act = n - 37
        part, _ = _geo_backward(p_r, x, cot, rays=True, cap=cap, n_act=torch.tensor([act], dtype=torch.int64, device="cuda"))
        assert (part[act:] == SENTINEL).all()
        assert torch.equal(part[:act], d_pts[:act])


# ------------------------------------------------------------------ 2. direction adjoint of the colour network
@pytest.mark.parametrize("per", [1, 19])
def test_direction_adjoint_matches_fp64_autograd(pair, per):
    from dynhor_amd import _lib
    o_r, p_r = pair
    L, n = _lib.lib(), 513
    g = torch.Generator(device="cpu").manual_seed(per)
    feat = torch.randn(n, 13, generator=g).cuda()
    nrm = torch.randn(n, 3, generator=g).cuda()
    d = torch.nn.functional.normalize(torch.randn(n // per, 3, generator=g), dim=1).cuda()
    d_col = torch.randn(n, 3, generator=g).cuda()
    d_n0 = torch.randn(n, 3, generator=g).cuda()
    col = o_r.color_network

    def oracle(dt):
        col.to(dt)
        v = d.to(dt)[:, None, :].expand(n // per, per, 3).reshape(-1, 3).clone().requires_grad_(True)
        out = col(None, nrm.to(dt), v, feat.to(dt))
        gr = torch.autograd.grad((out * d_col.to(dt)).sum(), v)[0]
        col.float()
        return gr

    eager, ref = oracle(torch.float32), oracle(torch.float64)
    packed = p_r.store.ensure_packed()
    ws = p_r._workspace(n)
    outs = {}
    for rays in (False, True):
        d_feat, d_n = torch.empty(n, 13, device="cuda"), d_n0.clone()
        head = (_p(packed), _p(feat), _p(nrm), _p(d), _p(d_col), per, n, _p(ws), _p(d_feat), _p(d_n), None)
        if rays:
            d_dirs = torch.full((n, 3), SENTINEL, device="cuda")
            _lib.check(L.dh_hash_color_backward_rays(*head, _p(d_dirs), _lib.stream()))
        else:
            _lib.check(L.dh_hash_color_backward(*head, _lib.stream()))
        torch.cuda.synchronize()
        outs[rays] = (d_feat, d_n)
    _check(f"d_dirs_pts, n_per_ray = {per}", d_dirs, ref, eager)
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])


# ------------------------------------------------------------------ 3. packed scan with the direction adjoint
@pytest.mark.parametrize("step,cap", [(0.01, 128), (0.0025, 1024)])
def test_packed_scan_direction_adjoint_matches_oracle(step, cap):
    """The two cases of test_gpu_occgrid.test_packed_render_scan_and_adjoint_match_oracle (cap 1024: multi-trip segments)."""
    from dynhor_amd import _lib
    L = _lib.lib()
    B = 300
    o, d, near, far, u = _rays(B, seed=7)
    m = _hip_march(o, d, near, far, u, _blob_grid(64, seed=3), step, cap)
    N = m.N
    if cap > 128:
        assert (m.cnt > 128).any() and (m.cnt > 256).any()
    g = torch.Generator(device="cpu").manual_seed(1)
    sdf = (torch.randn(N, generator=g) * (0.05 if cap == 128 else 0.2) + (0.0 if cap == 128 else 0.15)).cuda()
    normals = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).cuda() * (0.7 + 0.6 * torch.rand(N, 1, generator=g).cuda())
    colors = torch.rand(N, 3, generator=g).cuda()
    inv_s = torch.tensor([35.0], device="cuda")
    car, bg = 0.3, torch.tensor([0.2, 0.5, 0.9], device="cuda")
    gc = torch.randn(B, 3, generator=g).cuda(); gw = torch.randn(B, generator=g).cuda(); gn = torch.randn(B, 3, generator=g).cuda()
    ec = torch.tensor([0.37], device="cuda")
    # the scan's forward leaves nothing the backward reads; eik_coef multiplies the relaxed (|n| - 1)^2 sum directly
    relax_sum = (torch.linalg.norm(m.pts, dim=-1) < 1.2).float().sum().double() + 1e-5

    def oracle(dt):
        dl = d.to(dt).clone().requires_grad_(True)
        ref = G.render_packed(m.pts.to(dt), sdf.to(dt), normals.to(dt), colors.to(dt), dl, m.ray_idx.long(), m.off, m.cnt.long(), float(m.step),
                              inv_s.to(dt), car, bg.to(dt))
        f = ((ref["color_fine"] * gc.to(dt)).sum() + (ref["weight_sum"][:, 0] * gw.to(dt)).sum() + (ref["normal_map"] * gn.to(dt)).sum()
             + ec.to(dt)[0] * relax_sum.to(dt) * ref["gradient_error"])
        return torch.autograd.grad(f, dl)[0]

    eager, ref = oracle(torch.float32), oracle(torch.float64)
    outs = {}
    for rays in (False, True):
        o_ = [torch.empty(N, device="cuda"), torch.empty(N, 3, device="cuda"), torch.empty(N, 3, device="cuda"), torch.empty(B, device="cuda")]
        head = (_p(o), _p(d), _p(m.t_start), _p(sdf), _p(normals), _p(colors), _p(inv_s), car, m.step, _p(bg), B, _p(m.off), _p(m.cnt), _p(gc),
                _p(gw), None, None, _p(gn), _p(ec), *[_p(t) for t in o_])
        if rays:
            d_rd = torch.full((B, 3), SENTINEL, device="cuda")
            _lib.check(L.dh_render_scan_bwd_packed_rays(*head, _p(d_rd), _lib.stream()))
        else:
            _lib.check(L.dh_render_scan_bwd_packed(*head, _lib.stream()))
        torch.cuda.synchronize()
        outs[rays] = o_
    _check(f"packed scan d_rays_d, cap {cap}", d_rd, ref, eager)
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 4. per-ray fold on packed rays
@pytest.mark.parametrize("B", [1, 5, 300])
def test_ray_adjoint_fold_matches_fp64_index_add(B):
    from dynhor_amd import _lib
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(B)
    base = [0, 1, 64, 65, 129, 300, 1024]                 # empty, one sample, around a trip of 64 lanes, above 256, the scan's limit
    cnt = torch.tensor(([300] if B == 1 else base[:B] if B <= len(base) else
                        base + torch.randint(0, 200, [B - len(base)], generator=g).tolist()), dtype=torch.int32)
    off = (torch.cumsum(cnt.long(), 0) - cnt.long())
    N = int(cnt.sum())
    ray = torch.repeat_interleave(torch.arange(B), cnt.long())
    d_pts, d_dirs = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)
    t_start = 1.5 + torch.rand(N, generator=g)
    step = float(torch.tensor(0.0135, dtype=torch.float32))
    acc0 = torch.randn(B, 3, generator=g)
    t = (t_start + torch.tensor(0.5 * step, dtype=torch.float32)).double()[:, None]
    ref_o = torch.zeros(B, 3, dtype=torch.float64).index_add_(0, ray, d_pts.double())
    terms_d = t * d_pts.double() + d_dirs.double()
    ref_d = acc0.double() + torch.zeros(B, 3, dtype=torch.float64).index_add_(0, ray, terms_d)
    abs_o = torch.zeros(B, 3, dtype=torch.float64).index_add_(0, ray, d_pts.double().abs())
    abs_d = acc0.double().abs() + torch.zeros(B, 3, dtype=torch.float64).index_add_(0, ray, (t * d_pts.double()).abs() + d_dirs.double().abs())
    dev = lambda x: x.cuda().contiguous()
    args = (dev(d_pts), dev(d_dirs), dev(t_start), step, dev(off), dev(cnt), B)
    res = []
    for _ in range(2):
        d_o, d_d = torch.full((B, 3), SENTINEL, device="cuda"), dev(acc0)
        _lib.check(L.dh_ray_adjoint_packed(*[_p(a) if torch.is_tensor(a) else a for a in args], _p(d_o), _p(d_d), _lib.stream()))
        torch.cuda.synchronize()
        res.append((d_o.cpu(), d_d.cpu()))
    d_o, d_d = res[0]
    e_o, e_d = (d_o.double() - ref_o).abs(), (d_d.double() - ref_d).abs()
    print(f"fold, B = {B}: worst |error| / sum |terms| {float((e_o / abs_o.clamp_min(1e-300)).max()):.2e} (d_rays_o), "
          f"{float((e_d / abs_d.clamp_min(1e-300)).max()):.2e} (d_rays_d); bound 1e-6")
    assert (e_o <= 1e-6 * abs_o).all() and (e_d <= 1e-6 * abs_d).all()
    empty = cnt == 0
    if empty.any():
        assert (d_o[empty] == 0).all() and torch.equal(d_d[empty], acc0[empty])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ------------------------------------------------------------------ whole step
@pytest.fixture(scope="module")
def tiny_dataset():
    from dynhor_amd.dataset import Dataset
    return Dataset.from_synthetic(n_frames=3, H=96, W=96, seed=7, device="cuda:0")


def _pose_leaves(ref, frame, px, py, K, dt):
    """(r6, tr leaves, o, d, R of `frame` through pixels px, py) in dtype dt: PoseRefiner.rays' formula."""
    from dynhor_amd.pose import rot6d_to_matrix
    r6 = ref.rot6d.detach().to(dt).clone().requires_grad_(True)
    tr = ref.trans.detach().to(dt).clone().requires_grad_(True)
    R = rot6d_to_matrix(r6[frame:frame + 1])[0].T
    pix = torch.stack([px.to(dt), py.to(dt), torch.ones(px.shape[0], dtype=dt, device=px.device)], -1)
    dc = torch.nn.functional.normalize(pix @ torch.inverse(K.double()).to(dt).T, dim=-1)
    d = dc @ R
    return r6, tr, (-(tr[frame] @ R)).expand_as(d), d, R


def _oracle_runs(mods, loss_fn, rays, R_frame, t_mid, ray_idx, pose):
    """The oracle in fp32 (eager) and fp64: with the rays and R as leaves (a pre-hook on the SDF network collects the per-point
    adjoint, as tests/test_gpu_pose_refinement.py does) and differentiated end to end w.r.t. the pose parameters.  loss_fn(o, d, R, dt)
    -> loss.  Returns {dt: dict(o, d, R, pts, dmix = d.grad - sum_k t_k pts.grad_k, r6, tr)}."""
    ref, frame, px, py, K, _ = pose
    B = rays.shape[0]
    out = {}
    for dt in (torch.float32, torch.float64):
        for m_ in mods:
            m_.to(dt); m_.zero_grad()
        r = rays.to(dt)
        o = r[:, :3].clone().requires_grad_(True); d = r[:, 3:6].clone().requires_grad_(True)
        R = R_frame.to(dt).clone().requires_grad_(True)
        seen = {"on": False}

        def grab(mod, inp):
            if "pts" not in seen:
                seen["pts"] = inp[0]
                inp[0].register_hook(lambda gr: seen.__setitem__("grad", gr.detach().clone()) if seen["on"] else None)
        hook = mods[0].register_forward_pre_hook(grab)
        loss = loss_fn(o, d, R, dt)
        hook.remove()
        seen["on"] = True
        loss.backward()
        pg = seen["grad"].reshape(-1, 3)
        fold = torch.zeros(B, 3, dtype=dt, device=rays.device).index_add_(0, ray_idx, t_mid.to(dt)[:, None] * pg)
        res = dict(o=o.grad, d=d.grad, R=R.grad, pts=pg, dmix=d.grad - fold)
        r6, tr, o_e, d_e, R_e = _pose_leaves(ref, frame, px, py, K, dt)
        loss_fn(o_e, d_e, R_e, dt).backward()
        res["r6"], res["tr"] = r6.grad[frame], tr.grad[frame]
        out[dt] = res
    for m_ in mods:
        m_.float()
    return out


def _check_step(p_r, run, rays, R_frame, normal_w, t_mid, ray_idx, oracle, pose, has_samples=None):
    """Everything the whole-step section of DESIGN_NEXT_ROWS.md section 28 lists, for one configuration."""
    ref_p, frame, px, py, K, Kinv = pose
    B = rays.shape[0]
    run(False)
    torch.cuda.synchronize()
    g_plain = p_r.store.grad_flat.clone()
    run(True)
    torch.cuda.synchronize()
    assert torch.equal(p_r.store.grad_flat, g_plain), "the _rays variants must not touch the parameter path"
    d_o, d_d, d_R = p_r.last_ray_grads
    assert p_r.last_partner_pose_grads is None
    s = p_r.last_state
    n_pts = oracle[torch.float64]["pts"].shape[0]
    d_pts = s.d_pts[:n_pts]
    e32, e64 = oracle[torch.float32], oracle[torch.float64]
    # per point, on the unmarked points of the real sample set
    bad = U.ambiguous(s.pts[:n_pts])
    share = bad.float().mean().item()
    print(f"marked share of the step's {n_pts} samples: {share:.4f}")
    assert share <= U.MAX_MARKED
    _check("d_pts (unmarked samples)", d_pts[~bad], e64["pts"][~bad], e32["pts"][~bad])
    # per ray, without the hash derivative in the way
    fold_o = torch.zeros(B, 3, dtype=torch.float64, device=rays.device).index_add_(0, ray_idx, d_pts.double())
    fold_d = torch.zeros(B, 3, dtype=torch.float64, device=rays.device).index_add_(0, ray_idx, t_mid.double()[:, None] * d_pts.double())
    a_o = U.two_errors(e32["o"], e64["o"])
    e_o = U.two_errors(d_o, fold_o)
    print(f"d_rays_o against the fp64 sum of the step's own d_pts: {e_o[0]:.2e} / {e_o[1]:.2e} (allowance {MARGIN:g} x {a_o[0]:.2e} / {a_o[1]:.2e})")
    assert e_o[0] <= MARGIN * a_o[0] and e_o[1] <= MARGIN * a_o[1]
    _check("d_rays_d - sum t d_pts (the SH and true_cos routes)", d_d.double() - fold_d, e64["dmix"], e32["dmix"])
    if normal_w > 0:
        _check("d_R", d_R.reshape(1, 9), e64["R"].reshape(1, 9), e32["R"].reshape(1, 9))
    else:
        assert d_R is None
    if has_samples is not None:
        assert (~has_samples).any() and (d_o[~has_samples] == 0).all() and (d_d[~has_samples] == 0).all()
    # the whole gradient into the 9 pose numbers, judged against the fp32 eager oracle's own deviation (it suffers the same cell flips)
    o_t, d_t, R_t = ref_p.rays(frame, px, py, Kinv)
    ref_p.opt.zero_grad()
    torch.autograd.backward([o_t, d_t] + ([R_t] if d_R is not None else []), [d_o, d_d] + ([d_R] if d_R is not None else []))
    for name, got, key in (("rot6d", ref_p.rot6d.grad[frame], "r6"), ("translation", ref_p.trans.grad[frame], "tr")):
        err = ((got.double() - e64[key]).norm() / e64[key].norm()).item()
        own = ((e32[key].double() - e64[key]).norm() / e64[key].norm()).item()
        print(f"pose gradient end to end, {name}: rel {err:.2e}; the fp32 eager oracle's own {own:.2e}; ratio {err / own:.2f} (margin {MARGIN:g})")
        assert err <= MARGIN * own, name
    ref_p.rot6d.grad = None; ref_p.trans.grad = None


@pytest.mark.parametrize("B,normal_w", [(67, 0.0), (67, 0.05), (96, 0.0), (96, 0.05)])
def test_hierarchical_step_ray_adjoints_match_oracle(tiny_dataset, B, normal_w):
    from dynhor_amd.pose import PoseRefiner
    ds = tiny_dataset
    o_r, p_r = make_hash_pair(seed=61)
    frame, car = 1, 0.4
    g = torch.Generator(device="cpu").manual_seed(B)
    px = torch.randint(0, ds.W, [B], generator=g).cuda(); py = torch.randint(0, ds.H, [B], generator=g).cuda()
    rays = ds.gen_rays_at_pixels(frame, px, py)
    near, far = ds._last_near_far
    z = o_r.sample_z(rays[:, :3], rays[:, 3:6], near, far, t_rand=torch.rand(B, 1, generator=g).cuda())
    n = z.shape[1]
    dz = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 2.0 / 16)], -1)
    t_mid = (z + 0.5 * dz).reshape(-1)
    ray_idx = torch.arange(B, device="cuda").repeat_interleave(n)
    mods = (o_r.sdf_network, o_r.deviation_network, o_r.color_network)

    def loss_fn(o, d, R, dt):
        out = o_r.render(o, d, near.to(dt), far.to(dt), cos_anneal_ratio=car, z_vals=z.to(dt))
        r = rays.to(dt)
        return O.neus_losses(out, r[:, 6:9], r[:, 9:10], r[:, 10:11], 0.1, 0.1, normal_w, r[:, 11:14], R)["loss"]

    pose = (PoseRefiner(ds.R, ds.T).cuda(), frame, px, py, ds.K, ds.Kinv)
    oracle = _oracle_runs(mods, loss_fn, rays, ds.R[frame], t_mid, ray_idx, pose)
    p_r.sample_z = lambda *a, **k: z
    run = lambda rg: p_r.train_step_core(rays, near, far, ds.R[frame], car, 0.1, 0.1, normal_w, ray_grads=rg)
    _check_step(p_r, run, rays, ds.R[frame], normal_w, t_mid, ray_idx, oracle, pose)


def _occ_conf(refine=True, **train):
    return {"seq_name": "occpose", "exp_name": "e", "data_info": {"synthetic": {"n_frames": 6, "H": 96, "W": 96, "seed": 11}},
            "train": dict({"batch_size": 512, "normal_weight": 0.05, "learning_rate": 5e-3, "report_freq": 10 ** 9, "save_freq": 10 ** 9,
                           "val_freq": 0, "warm_up_end": 20, "end_iter": 2000, "refine_poses": refine}, **train),
            "model": {"family": "hash", "hash_renderer": {"sampler": "occgrid", "march_samples_per_ray": 256, "grid_res": 64,
                                                         "grid_update_every": 8}}}


@pytest.mark.parametrize("normal_w", [0.0, 0.05])
def test_occgrid_step_ray_adjoints_match_oracle(tmp_path, normal_w):
    """test_gpu_occgrid._occ_runner's shapes with the renderer built with ray_grads=True; the oracle's march supplies the samples."""
    from dynhor_amd.runner import Runner
    r = Runner(conf=_occ_conf(), device="cuda:0", exp_root=str(tmp_path))
    ren, ds = r.renderer, r.dataset
    assert ren.ray_grads
    dev = torch.device("cuda:0")
    gj = torch.Generator(device=dev); gj.manual_seed(17)
    with torch.no_grad():                                 # (as the packed-step test: the initialisation leaves the encoding without signal)
        r.sdf_network.lin0.weight_v.add_(0.05 * torch.randn(r.sdf_network.lin0.weight_v.shape, device=dev, generator=gj))
        r.sdf_network.encoding.table.add_(0.005 * torch.randn(r.sdf_network.encoding.table.shape, device=dev, generator=gj))
    r.store.bump()
    o_sdf, o_col, o_var = _oracle_hash_models(r, dev)
    g = torch.Generator(device=dev); g.manual_seed(3)
    ren.update_grid(jitter=torch.rand(ren.grid.res ** 3, 3, device=dev, generator=g))
    B, frame, car = 512, 2, 0.2
    gc = torch.Generator(device="cpu").manual_seed(4)
    px = torch.randint(0, ds.W, [B], generator=gc).cuda(); py = torch.randint(0, ds.H, [B], generator=gc).cuda()
    rays = ds.gen_rays_at_pixels(frame, px, py)
    near, far = ds._last_near_far
    u = torch.rand(B, 1, device=dev, generator=g)
    og = G.OccupancyGrid(res=ren.grid.res, radius=1.0, device=dev)
    og.binary = ren.grid.binary.bool().clone()
    step = float(torch.tensor(ren.march_step, dtype=torch.float32))
    mo = G.march(rays[:, :3].contiguous(), rays[:, 3:6].contiguous(), near.reshape(-1), far.reshape(-1), u.reshape(-1), og, step,
                 max_samples=ren._cap_ladder[0])
    ray_idx, off, cnt = mo["ray_idx"], mo["off"], mo["cnt"]
    t_mid = mo["t_start"] + float(torch.tensor(0.5 * ren.march_step, dtype=torch.float32))
    mods = (o_sdf, o_var, o_col)

    def loss_fn(o, d, R, dt):
        pts = o[ray_idx] + d[ray_idx] * t_mid.to(dt)[:, None]
        out = o_sdf(pts)
        nrm = o_sdf.gradient(pts).reshape(-1, 3)
        colr = o_col(pts, nrm, d[ray_idx], out[:, 1:])
        inv_s = o_var(torch.zeros(1, 3, device=dev, dtype=dt))[:, :1].clip(1e-6, 1e6).reshape(())
        ro = G.render_packed(pts, out[:, 0], nrm, colr, d, ray_idx, off, cnt, step, inv_s, car)
        rd = {"color_fine": ro["color_fine"], "weight_sum": ro["weight_sum"], "gradient_error": ro["gradient_error"],
              "gradients": ro["normal_map"][:, None, :], "weights": torch.ones(B, 1, dtype=dt, device=dev)}
        rr = rays.to(dt)
        return O.neus_losses(rd, rr[:, 6:9], rr[:, 9:10], rr[:, 10:11], 0.1, 0.1, normal_w, rr[:, 11:14], R)["loss"]

    from dynhor_amd.pose import PoseRefiner
    pose = (PoseRefiner(ds.R, ds.T).cuda(), frame, px, py, ds.K, ds.Kinv)
    oracle = _oracle_runs(mods, loss_fn, rays, ds.R[frame], t_mid, ray_idx, pose)

    def run(rg):
        ren._march_iter = 1                               # no grid update inside the step
        ren.train_step_core(rays, near, far, ds.R[frame], car, 0.1, 0.1, normal_w, t_rand=u, ray_grads=rg)

    run(True)
    m = ren.last_state.m
    assert torch.equal(m.cnt.long(), cnt) and torch.equal(m.t_start[:int(cnt.sum())], mo["t_start"]), "the marcher selects the oracle's samples"
    _check_step(ren, run, rays, ds.R[frame], normal_w, t_mid, ray_idx, oracle, pose, has_samples=cnt > 0)


# ------------------------------------------------------------------ Runner
@pytest.mark.parametrize("sampler", ["hierarchical", "occgrid"])
def test_runner_refines_poses_of_the_hash_family_and_checkpoints_them(tmp_path, sampler):
    """The body of tests/test_gpu_pose_refinement.test_runner_refines_poses_and_checkpoints_them for family: hash; pose_start_iter 4
    launches the `_rays` entries only from iteration 4."""
    from dynhor_amd.runner import Runner
    conf = {"seq_name": "hpose", "exp_name": sampler, "data_info": {"synthetic": {"n_frames": 4, "H": 64, "W": 64, "seed": 5}},
            "train": {"batch_size": 256, "normal_weight": 0.05, "refine_poses": True, "pose_lr": 1e-3, "pose_start_iter": 4,
                      "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "warm_up_end": 10, "end_iter": 100},
            "model": {"family": "hash",
                      "hash_renderer": {"sampler": sampler, "march_samples_per_ray": 256, "grid_res": 64, "grid_update_every": 8}}}
    r = Runner(conf=conf, device="cuda:0", exp_root=str(tmp_path))
    R0, T0 = r.dataset.R.clone(), r.dataset.T.clone()
    tm = r.renderer.timer
    tm.enabled = True
    r.train(4)
    torch.cuda.synchronize()
    assert torch.equal(r.dataset.T, T0) and torch.equal(r.dataset.R, R0), "no pose moves before pose_start_iter"
    tags = tm.summary()
    assert tags["hash_geo_backward"][1] == 4 and "hash_geo_backward_rays" not in tags and "hash_color_backward_rays" not in tags
    r.train(8)
    torch.cuda.synchronize()
    tags = tm.summary()
    assert tags["hash_geo_backward"][1] == 4 and tags["hash_geo_backward_rays"][1] == 8 and tags["hash_color_backward_rays"][1] == 8
    assert ("ray_adjoint_packed" in tags) == (sampler == "occgrid")
    tm.enabled = False
    assert torch.isfinite(r.dataset.R).all() and torch.isfinite(r.store.flat).all()
    moved = (r.dataset.T - T0).abs().amax(dim=1)
    assert (moved > 0).all() and moved.max().item() < 0.05, "every visited frame's pose moved, by a small step"
    assert ((r.dataset.R @ r.dataset.R.transpose(1, 2)) - torch.eye(3, device="cuda")).abs().max().item() < 1e-5
    path = r.save_checkpoint()
    ck = torch.load(path, weights_only=False)
    assert "pose_refiner" in ck
    r2 = Runner(conf=conf, device="cuda:0", exp_root=str(tmp_path), is_continue=True)
    assert torch.allclose(r2.dataset.R, r.dataset.R, atol=1e-6) and torch.allclose(r2.dataset.T, r.dataset.T)


def test_occgrid_ray_grads_need_the_keyword_and_the_correspondence_term_stays_out(tmp_path):
    from dynhor_amd.runner import Runner
    r = Runner(conf=_occ_conf(refine=False), device="cuda:0", exp_root=str(tmp_path))
    assert not r.renderer.ray_grads
    r.train_iteration()
    with pytest.raises(ValueError, match="ray_grads=True"):
        r.renderer.train_step_core(r._last_rays, *r.dataset._last_near_far, r.dataset.R[0], 0.1, ray_grads=True)
    with pytest.raises(ValueError, match="correspondence term"):
        r.renderer.train_step_core(r._last_rays, *r.dataset._last_near_far, r.dataset.R[0], 0.1, corr=torch.zeros(512, 4, device="cuda"))
    with pytest.raises(ValueError, match="corr_weight.*occgrid.*refine_poses"):
        Runner(conf=_occ_conf(refine=True, corr_weight=0.5), device="cuda:0", exp_root=str(tmp_path))
