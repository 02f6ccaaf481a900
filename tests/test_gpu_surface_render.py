"""The sphere tracer's HIP kernels (csrc/trace.hip) and dynhor_amd/surface_render.py on the GPU: rays against dh_gen_rays, one step of
the state machine in lock-step with the fp32 restatement (tests/trace_util.py), the order-preserving compaction, the tracer end to end
on analytic fields and on trained networks of both families against the fp64 oracles, the image buffers, Runner.render_views and the
CLI.  The end-to-end bounds are the specification's: |s| <= eps at a hit, depth to eps / cos(theta), no crossing lost."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import trace_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SIZES = [1, 63, 64, 65, 257, 1000]
P = U.PARAMS


def _ordered(x):
    """fp32 -> integers in the order of the floats (ulp distances are differences of these)."""
    i = x.contiguous().view(torch.int32).long()
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps(a, b):
    return (_ordered(a) - _ordered(b)).abs()


# ------------------------------------------------------------------------------------------------ 1. rays
@pytest.mark.parametrize("H,W", [(5, 7), (33, 47)])
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("views", [[2], [0, 1, 2]])
def test_rays_equal_gen_rays_and_bounds_match_fp64(H, W, level, views):
    from dynhor_amd import surface_render as sr
    from dynhor_amd.dataset import Dataset
    ds = Dataset.from_synthetic(n_frames=3, H=H, W=W, seed=11, device=DEV)
    R, T = ds.R[views].reshape(-1, 9).contiguous(), ds.T[views].reshape(-1, 3).contiguous()
    a = sr._init(R, T, ds.Kinv.reshape(9).contiguous(), len(views), H, W, level, 1.0)
    assert (a.h, a.w) == ((H + level - 1) // level, (W + level - 1) // level) and a.N == len(views) * a.h * a.w
    for k, f in enumerate(views):
        rays, h, w = ds.gen_rays_at(f, level)
        assert (h, w) == (a.h, a.w)
        sl = slice(k * h * w, (k + 1) * h * w)
        assert torch.equal(a.d[sl], rays[:, 3:6])
        assert torch.equal(a.o[k].expand(h * w, 3), rays[:, :3])
    o = a.o.repeat_interleave(a.rays_per_view, dim=0)
    near, far, disc = U.sphere_bounds(o, a.d, 1.0)
    use = disc.abs() >= 1e-4
    assert int((~use).sum()) < 0.05 * a.N
    miss = (disc <= 0) | (far <= 0)
    assert torch.equal((a.state == sr.MISS)[use], miss[use]) and torch.equal((a.state == sr.MARCH)[use], ~miss[use])
    ok = use & ~miss
    t_ref = near.clamp(min=0.0)
    assert bool(((a.t.double() - t_ref).abs()[ok] <= 1e-5 * (1 + t_ref[ok])).all())
    assert bool(((a.t_far.double() - far).abs()[ok] <= 1e-5 * (1 + far[ok])).all())
    # the fp64 restatement from the poses gives the same rays
    ref = U.trace_init_ref(ds.R[views], ds.T[views], ds.K, H, W, level, device=DEV)
    assert float((ref["d"] - a.d.double()).abs().max()) < 1e-6 and float((ref["o"] - a.o.double()).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ 2. one step
def _upload(ref):
    """The restatement's fp32 arrays (CPU) as the namespace surface_render's wrappers take."""
    f = lambda k: ref[k].to(DEV).contiguous()
    return SimpleNamespace(N=ref["t"].numel(), rays_per_view=ref["rays_per_view"], o=f("o"), d=f("d"), t=f("t"), t_far=f("t_far"),
                           t_lo=f("t_lo"), s_lo=f("s_lo"), t_hi=f("t_hi"), s_hi=f("s_hi"), state=ref["state"].to(torch.uint8).to(DEV),
                           nq=(ref["nq"] - 65536 * (ref["nq"] >= 32768)).to(torch.int16).to(DEV),      # u16 bits in an int16 tensor
                           nref=ref["nref"].to(torch.uint8).to(DEV), flags=ref["flags"].to(torch.uint8).to(DEV))


def _random_state(N, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g)
    a = U.new_arrays(N, torch.float32)
    a["rays_per_view"] = (N + 1) // 2
    a["o"] = torch.randn(2, 3, generator=g)
    a["d"] = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=1)
    a["t_lo"] = 2.0 * rnd(N)
    a["t_hi"] = a["t_lo"] + 0.2 * rnd(N) ** 4 + 1e-5                              # some brackets narrower than eps
    a["t"] = a["t_lo"] + (a["t_hi"] - a["t_lo"]) * rnd(N)
    a["t_far"] = a["t"] + 0.12 * rnd(N)                                          # some steps pass t_far
    a["s_lo"] = 0.1 * rnd(N) + 3e-4
    a["s_hi"] = -0.1 * rnd(N) - 3e-4
    a["state"] = torch.randint(0, 5, (N,), generator=g)
    a["nq"] = torch.tensor([0, 1, 7, 65535])[torch.randint(0, 4, (N,), generator=g)]
    a["nref"] = torch.randint(0, 9, (N,), generator=g)
    a["flags"] = torch.randint(0, 8, (N,), generator=g)
    s = 0.2 * torch.randn(N, generator=g)
    kind = torch.randint(0, 10, (N,), generator=g)
    s = torch.where(kind == 0, 4e-4 * (rnd(N) - 0.5), s)                         # around +-eps
    s = torch.where(kind == 1, torch.full_like(s, float("nan")), s)
    s = torch.where(kind == 2, torch.full_like(s, float("inf")) * torch.sign(s), s)
    return a, s


def _step_both(ref, s, idx, count=None, params=P):
    from dynhor_amd import surface_render as sr
    dev = _upload(ref)
    n = idx.numel()
    pts = torch.full((n, 3), float("nan"), device=DEV)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
    sr.trace_step(dev, idx.to(torch.int32).to(DEV), cnt, s.to(DEV).contiguous(), pts, n, **params)
    m = n if count is None else min(count, n)
    tie = U.trace_step_ref(ref, idx[:m], s[:m], **params)
    torch.cuda.synchronize()
    return dev, pts, tie, m


def _compare_step(ref, dev, idx, pts, tie, m):
    nq = dev.nq.to(torch.int32).cpu() & 0xFFFF
    sure = torch.ones(ref["t"].numel(), dtype=torch.bool)
    sure[idx[:m][tie]] = False
    for k, got in (("state", dev.state), ("flags", dev.flags), ("nref", dev.nref), ("nq", nq)):
        assert torch.equal(got.cpu().long()[sure], ref[k][sure]), k
    for k, got in (("t", dev.t), ("t_lo", dev.t_lo), ("t_hi", dev.t_hi)):
        u = _ulps(got.cpu(), ref[k])[sure]
        assert int(u.max()) <= 2, (k, int(u.max()))
    for k, got in (("s_lo", dev.s_lo), ("s_hi", dev.s_hi)):
        assert torch.equal(got.cpu()[sure], ref[k][sure]), k
    # the next query points, in list order
    r = idx[:m]
    want = ref["o"][r // ref["rays_per_view"]].double() + dev.t.cpu()[r, None].double() * ref["d"][r].double()
    got = pts[:m].cpu().double()
    keep = sure[r]
    assert bool(((got - want).abs()[keep] <= 1e-6 * (1 + want.abs()[keep])).all())
    assert bool(torch.isnan(pts[m:]).all())                                       # entries past the device count stay untouched


@pytest.mark.parametrize("N", SIZES)
def test_one_step_in_lock_step_with_the_restatement(N):
    ref, s = _random_state(N, seed=N)
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(N + 1))
    before = {k: v.clone() for k, v in ref.items() if isinstance(v, torch.Tensor)}
    dev, pts, tie, m = _step_both(ref, s, idx)
    assert int(tie.sum()) <= 0.01 * N
    _compare_step(ref, dev, idx, pts, tie, m)
    # dh_trace_points gives the same points bit for bit, whatever the rays' states
    from dynhor_amd import surface_render as sr
    assert torch.equal(sr.trace_points(dev, idx.to(DEV)), pts) and sr.trace_points(dev, idx[:0].to(DEV)).shape == (0, 3)
    # rays that were not live are untouched
    dead = before["state"] >= U.HIT
    assert torch.equal(dev.t.cpu()[dead], before["t"][dead]) and torch.equal(dev.state.cpu().long()[dead], before["state"][dead])
    if N >= 63:                                                                   # a device count below the launch size
        ref2, s2 = _random_state(N, seed=N + 100)
        dev, pts, tie, m = _step_both(ref2, s2, idx, count=N // 2)
        assert int(tie.sum()) <= 0.01 * N
        _compare_step(ref2, dev, idx, pts, tie, m)


def test_one_step_exact_edge_cases():
    """Every operand is representable, so no case may count as a tie: s = +-eps and 0, a negative first sample, NaN, +-inf, t' exactly
    t_far, a REFINE at its last allowed step, a bracket of width exactly eps."""
    eps = float(torch.tensor(P["eps"], dtype=torch.float32))
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    far_tie = float(f32(1.0) + f32(P["max_step"]))                                # t = 1, s = 1: the step clamps to max_step
    cases = [  # state, nq, nref, t, t_far, t_lo, s_lo, t_hi, s_hi, s -> state, flags, t (None: unchanged)
        (U.MARCH, 3, 0, 1.0, 2.0, 0.9, 0.1, 0.0, 0.0, eps, U.HIT, 0, None),
        (U.MARCH, 3, 0, 1.0, 2.0, 0.9, 0.1, 0.0, 0.0, -eps, U.HIT, 0, None),
        (U.MARCH, 0, 0, 1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, U.HIT, 0, None),
        (U.REFINE, 5, 2, 1.0, 2.0, 0.9, 0.1, 1.1, -0.1, eps, U.HIT, 0, None),
        (U.MARCH, 0, 0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, -0.25, U.HIT, U.INSIDE, None),
        (U.MARCH, 1, 0, 1.0, 2.0, 0.5, 0.25, 0.0, 0.0, -0.25, U.REFINE, 0, 0.75),  # the secant point of (0.5, 0.25), (1, -0.25)
        (U.MARCH, 2, 0, 1.0, 2.0, 0.9, 0.1, 0.0, 0.0, float("nan"), U.FAIL, 0, None),
        (U.MARCH, 2, 0, 1.0, 2.0, 0.9, 0.1, 0.0, 0.0, float("inf"), U.FAIL, 0, None),
        (U.REFINE, 2, 1, 1.0, 2.0, 0.9, 0.1, 1.1, -0.1, float("-inf"), U.FAIL, 0, None),
        (U.MARCH, 2, 0, 1.0, far_tie, 0.9, 0.1, 0.0, 0.0, 1.0, U.MARCH, 0, far_tie),  # t' == t_far is not beyond it
        (U.MARCH, 2, 0, 1.0, 1.0625, 0.9, 0.1, 0.0, 0.0, 1.0, U.MISS, 0, None),           # t' = 1.1 is beyond t_far: t stays
        (U.REFINE, 9, P["refine_steps"] - 1, 1.0, 2.0, 0.5, 0.25, 1.5, -0.25, 0.125, U.HIT, U.CAPPED, None),
        (U.REFINE, 9, P["refine_steps"] - 2, 1.0, 2.0, 0.5, 0.25, 1.5, -0.25, 0.125, U.REFINE, 0, 1.0 + 0.5 * (0.125 / 0.375)),
        (U.REFINE, 4, 1, eps, 2.0, 0.0, 0.25, 1.0, -0.25, -0.125, U.HIT, 0, None),  # the bracket becomes [0, eps]: width == eps
        (U.MARCH, 2, 0, 1.0, 2.0, 0.9, 0.1, 0.0, 0.0, 2.0 ** -12, U.MARCH, 0, 1.0 + P["min_step"]),  # relax s below min_step
    ]
    n = len(cases)
    ref = U.new_arrays(n, torch.float32)
    col = lambda j, dt=torch.float32: torch.tensor([c[j] for c in cases], dtype=dt)
    ref["state"], ref["nq"], ref["nref"] = col(0, torch.int64), col(1, torch.int64), col(2, torch.int64)
    for j, k in enumerate(("t", "t_far", "t_lo", "s_lo", "t_hi", "s_hi")):
        ref[k] = col(3 + j)
    ref["rays_per_view"], ref["o"] = n, torch.zeros(1, 3)
    ref["d"] = torch.tensor([[0.0, 0.0, 1.0]]).repeat(n, 1)
    t_before = ref["t"].clone()
    idx = torch.arange(n)
    dev, pts, tie, m = _step_both(ref, col(9), idx)
    assert not bool(tie.any())
    _compare_step(ref, dev, idx, pts, tie, m)
    # ... and both do what the specification says
    assert dev.state.cpu().tolist() == [c[10] for c in cases]
    assert dev.flags.cpu().tolist() == [c[11] for c in cases]
    want_t = torch.tensor([float(t_before[k]) if c[12] is None else c[12] for k, c in enumerate(cases)], dtype=torch.float32)
    assert int(_ulps(dev.t.cpu(), want_t).max()) <= 2


# ------------------------------------------------------------------------------------------------ 3. compaction
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "random"])
def test_compaction_keeps_the_list_order(N, pattern):
    from dynhor_amd import surface_render as sr
    g = torch.Generator().manual_seed(N)
    live = {"none": torch.zeros(N, dtype=torch.bool), "all": torch.ones(N, dtype=torch.bool),
            "alternating": torch.arange(N) % 2 == 0, "random": torch.rand(N, generator=g) < 0.4}[pattern]
    state = torch.where(live, torch.arange(N) % 2, 2 + torch.arange(N) % 3)       # MARCH / REFINE survive; HIT / MISS / FAIL do not
    ref, _ = _random_state(N, seed=N + 7)
    ref["state"] = state
    dev = _upload(ref)
    perm = torch.randperm(N, generator=g)
    for idx, count in ((None, None), (perm, None), (perm, max(N // 3, 1))):
        n_in = N if count is None else count
        order = torch.arange(N) if idx is None else idx
        want = order[:n_in][live[order[:n_in]]]
        outs = []
        for _ in range(2):
            idx_out = torch.full((N,), -7, dtype=torch.int32, device=DEV)
            pts_out = torch.full((N, 3), float("nan"), device=DEV)
            cnt_out = torch.full((1,), -1, dtype=torch.int32, device=DEV)
            sr.trace_compact(dev, None if idx is None else idx.to(torch.int32).to(DEV),
                             None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV), N, idx_out, cnt_out, pts_out)
            outs.append((idx_out.cpu(), pts_out.cpu(), int(cnt_out.item())))
        i0, p0, c0 = outs[0]
        assert c0 == want.numel()
        assert torch.equal(i0[:c0].long(), want) and bool((i0[c0:] == -7).all())
        pw = ref["o"][want // ref["rays_per_view"]].double() + ref["t"][want, None].double() * ref["d"][want].double()
        assert bool(((p0[:c0].double() - pw).abs() <= 1e-6 * (1 + pw.abs())).all()) and bool(torch.isnan(p0[c0:]).all())
        i1, p1, c1 = outs[1]
        assert c1 == c0 and torch.equal(i0, i1) and torch.equal(p0[:c0], p1[:c0])


def test_compaction_of_an_empty_list_writes_a_zero_count():
    from dynhor_amd import surface_render as sr
    ref, _ = _random_state(4, seed=1)
    dev = _upload(ref)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    sr.trace_compact(dev, None, None, 0, torch.empty(1, dtype=torch.int32, device=DEV), cnt, torch.empty(1, 3, device=DEV))
    assert int(cnt.item()) == 0


# ------------------------------------------------------------------------------------------------ 4. analytic fields end to end
def _camera(H, W):
    R, T, K = U.reference_camera(H=H, W=W)
    return R.to(DEV), T.to(DEV), K.to(DEV)


def test_trace_of_a_sphere_hits_the_closed_form_depth():
    from dynhor_amd import surface_render as sr
    H, W = 33, 47
    R, T, K = _camera(H, W)
    # (the field in fp64 at the fp32 query point: what is measured is the tracer, not the rounding of |p| - r in fp32)
    a, st = sr.trace(lambda p: (p.double().norm(dim=-1) - 0.5).float()[:, None], R, T, K, H, W)
    o = a.o.repeat_interleave(a.rays_per_view, dim=0).double()
    hits, left, worst = U.check_sphere_depth(o, a.d.double(), a.t.double(), a.state.long(), 0.5, P["eps"])
    print(f"sphere on the GPU: {hits} hits, {left} left out, worst {worst:.3f} of eps / cos; {st}")
    assert st["hit"] == hits and st["hit"] + st["miss"] == a.N and st["inside"] == 0
    assert 5 < st["queries_mean"] < 40 and st["queries_max"] < 400


def test_trace_of_the_analytic_scene_loses_no_crossing():
    from dynhor_amd import surface_render as sr
    from dynhor_amd.scene import scene_sdf
    H, W = 33, 47
    R, T, K = _camera(H, W)
    f = lambda p: scene_sdf(p)[:, None]
    a, st = sr.trace(f, R, T, K, H, W)
    hit = a.state == sr.HIT
    o = a.o.repeat_interleave(a.rays_per_view, dim=0)
    s = scene_sdf((o + a.t[:, None] * a.d)[hit])
    capped = (a.flags[hit] & sr.FLAG_CAPPED) != 0
    print(f"scene on the GPU: {st}; largest |s| at a hit that is not capped {float(s[~capped].abs().max()):.3e}")
    assert st["hit"] > 80 and st["fail"] == 0
    assert bool(((s.abs() <= P["eps"]) | capped).all())
    assert int(capped.sum()) <= 0.01 * int(hit.sum())
    near, far, disc = U.sphere_bounds(o, a.d, 1.0)
    ins = disc > 1e-9
    missed, earlier = U.dense_check(lambda p: scene_sdf(p), o[ins].double(), a.d[ins].double(), near[ins].clamp(min=0.0), far[ins],
                                    a.state[ins].long(), a.t[ins].double())
    assert int(missed.sum()) == 0 and int(earlier.sum()) == 0
    # finished rays riding along between compactions change nothing
    b, st4 = sr.trace(f, R, T, K, H, W, compact_every=4)
    assert torch.equal(a.state, b.state) and float((a.t - b.t).abs().max()) <= 1e-6
    assert st4["count_reads"] < st["count_reads"]
    # a tracer cut short falls back on the chord scan and still loses nothing
    c, st_c = sr.trace(f, R, T, K, H, W, max_steps=6)
    assert st_c["scanned"] > st["scanned"] and st_c["fail"] == 0
    missed, earlier = U.dense_check(lambda p: scene_sdf(p), o[ins].double(), a.d[ins].double(), near[ins].clamp(min=0.0), far[ins],
                                    c.state[ins].long(), c.t[ins].double())
    assert int(missed.sum()) == 0 and int(earlier.sum()) == 0
    with pytest.raises(sr._lib.DynhorHipError, match="non-finite"):
        sr.trace(lambda p: torch.full((p.shape[0], 1), float("nan"), device=p.device), R, T, K, H, W)


# ------------------------------------------------------------------------------------------------ 5. networks end to end
def _conf(family, name="e"):
    return {"seq_name": "n1", "exp_name": name, "data_info": {"synthetic": {"n_frames": 4, "H": 64, "W": 64, "seed": 17}},
            "train": {"batch_size": 512, "normal_weight": 0.05, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0,
                      "warm_up_end": 10, "end_iter": 1000, "anneal_end": 200}, "model": {"family": family}}


# (family, iterations, fewest hits the 4 x 64 x 64 rays must give.  MI355X: the MLP family has 3,852 hits at its geometric initialisation
# -- a sphere of radius 0.5 --, none from 20 to 120 iterations (the mask loss empties the sphere before the object grows: the case of
# test_network_without_a_surface_gives_no_hit), 435 / 709 / 921 at 200 / 300 / 400; the hash family 4,188 / 2,894 / 222 / 245 / 643 at
# 0 / 20 / 60 / 120 / 200)
NETWORKS = [("neus", 300, 400), ("hash", 60, 100), ("neus", 0, 3000), ("hash", 0, 3000)]


@pytest.fixture(scope="module", params=NETWORKS, ids=["neus-300", "hash-60", "neus-init", "hash-init"])
def trained(request, tmp_path_factory):
    """tests/test_gpu_validate_parity.py's _runner (4 frames of 64 x 64) for either family, its surface render of every frame and the fp64
    oracle networks with the same weights; every case has a surface inside the unit sphere and the tests assert its hits."""
    from dynhor_amd import surface_render as sr
    from dynhor_amd.runner import Runner
    from oracle import hashgrid_oracle as HO
    from oracle import neus_oracle as O
    family, iters, min_hits = request.param
    r = Runner(conf=_conf(family), device=DEV, exp_root=str(tmp_path_factory.mktemp(family)))
    for _ in range(iters):
        r.train_iteration()
    ds = r.dataset
    out = sr.render_surface(r.renderer, ds.R, ds.T, ds.K, ds.H, ds.W, return_arrays=True)
    if family == "neus":
        o_sdf, o_col, _ = O.build_models(seed=1, device=r.device)
    else:
        o_sdf, o_col = HO.build_models(seed=1, device=r.device)
    o_sdf.load_state_dict(r.sdf_network.state_dict())
    o_col.load_state_dict(r.color_network.state_dict())
    print(f"{family} after {iters} iterations: {out['stats']}")
    assert out["stats"]["hit"] >= min_hits, out["stats"]
    return SimpleNamespace(family=family, iters=iters, min_hits=min_hits, r=r, out=out, a=out["arrays"][0], o_sdf=o_sdf, o_col=o_col)


def test_network_hits_lie_on_the_surface(trained):
    from dynhor_amd import surface_render as sr
    r, a, st = trained.r, trained.a, trained.out["stats"]
    hit = (a.state == sr.HIT).nonzero().reshape(-1)
    s = r.renderer.sdf(a.hit_points).reshape(-1)
    capped = (a.flags[hit] & sr.FLAG_CAPPED) != 0
    print(f"{trained.family}: {hit.numel()} hits, {int(capped.sum())} capped; largest |sdf| at a hit that is not capped "
          f"{float(s[~capped].abs().max()) if int((~capped).sum()) else 0.0:.3e}")
    assert st["fail"] == 0 and st["hit"] + st["miss"] == a.N and st["hit"] == hit.numel()
    assert hit.numel() >= trained.min_hits
    assert bool(((s.abs() <= P["eps"]) | capped).all())
    # nothing in front of the hit: 512 samples from the ray's start to t - scan_step on 256 random hit rays
    g = torch.Generator().manual_seed(3)
    sel = hit[torch.randperm(hit.numel(), generator=g)[:256].to(DEV)]
    o = a.o[sel // a.rays_per_view]
    near, _, _ = U.sphere_bounds(o, a.d[sel], 1.0)
    t0 = near.clamp(min=0.0).float()
    t1 = (a.t[sel] - 0.01).clamp(min=t0)
    ts = t0[:, None] + (t1 - t0)[:, None] * torch.linspace(0, 1, 512, device=DEV)[None]
    sv = r.renderer.sdf((o[:, None] + ts[..., None] * a.d[sel][:, None]).reshape(-1, 3).contiguous())
    assert bool((sv > 0).all()), float(sv.min())


def _oracle_at(trained, pts, dirs, dtype):
    o_sdf, o_col = trained.o_sdf, trained.o_col
    o_sdf.to(dtype); o_col.to(dtype)
    p = pts.to(dtype).clone()
    feat = o_sdf(p)[:, 1:].detach()
    grad = o_sdf.gradient(p).squeeze(1).detach()
    col = o_col(p.detach(), grad, dirs.to(dtype), feat).detach()
    o_sdf.float(); o_col.float()
    return grad, col


def test_network_normals_and_colours_match_the_oracle(trained):
    a = trained.a
    d = a.d[(a.state == 2).nonzero().reshape(-1)]
    assert d.shape[0] >= trained.min_hits and a.hit_points.shape[0] == d.shape[0]
    n64, c64 = _oracle_at(trained, a.hit_points, d, torch.float64)
    n32, c32 = _oracle_at(trained, a.hit_points, d, torch.float32)
    for name, got, r64, r32 in (("normals", a.normals, n64, n32), ("colours", a.colors, c64, c32)):
        e = float((got.double() - r64).abs().max())
        e32 = float((r32.double() - r64).abs().max())
        print(f"{trained.family} {name}: |hip-f64| {e:.3e}  |torch32-f64| {e32:.3e}")
        assert e < 2e-5 or e < 10 * e32, (name, e, e32)


def test_network_depth_matches_the_oracle_traced_in_fp64(trained):
    r, a = trained.r, trained.a
    ds = r.dataset
    trained.o_sdf.double()
    try:
        with torch.no_grad():
            ref = U.trace_ref(lambda p: trained.o_sdf(p)[:, 0], ds.R, ds.T, ds.K, ds.H, ds.W, device=DEV)
            hit_r = ref["state"] == U.HIT
            idx = hit_r.nonzero().reshape(-1)
        pr = U.points(ref, idx)
        n = trained.o_sdf.gradient(pr).squeeze(1).detach()
    finally:
        trained.o_sdf.float()
    hit_g = a.state == 2
    cos = torch.zeros(a.N, dtype=torch.float64, device=DEV)
    cos[idx] = (torch.nn.functional.normalize(n, dim=1) * ref["d"][idx]).sum(-1).abs()
    both = hit_g & hit_r & (cos >= 0.2)
    err = (a.t.double() - ref["t"])[both].abs() * cos[both] / (2 * P["eps"])
    one = hit_g ^ hit_r
    worst = float(err.max())
    print(f"{trained.family}: {int(hit_g.sum())} hits, the oracle's {int(hit_r.sum())}; {int(both.sum())} rays hit in both runs, worst depth "
          f"difference {worst:.3f} of 2 eps / cos; {int(one.sum())} rays hit in one run only")
    assert int(both.sum()) >= 0.8 * trained.min_hits
    assert worst <= 1.0
    # a ray that hits in one run only lies within one pixel of the other run's silhouette
    pool = lambda m: torch.nn.functional.max_pool2d(m.view(a.F, 1, a.h, a.w).float(), 3, 1, 1).view(-1) > 0
    assert bool(pool(hit_r)[hit_g & ~hit_r].all()) and bool(pool(hit_g)[hit_r & ~hit_g].all())


# ------------------------------------------------------------------------------------------------ 6. compose
def _compose_ref(a, background, frame_rgb=None):
    """dh_trace_compose as tensor expressions, every product rounded on its own.  Returns rgb / normal as floats before the u8
    conversion (so that values next to a rounding boundary can be told), depth, hit."""
    N = a.N
    hit = (a.state == 2) & (a.slot >= 0)
    R = a.R[torch.arange(N, device=DEV) // a.rays_per_view]
    d = a.d
    dz = (R[:, 6] * d[:, 0] + R[:, 7] * d[:, 1]) + R[:, 8] * d[:, 2]
    depth = torch.where(hit, a.t * dz, torch.full_like(a.t, float("inf")))
    sl = a.slot.clamp(min=0).long()
    n, c = a.normals[sl], a.colors[sl]
    nc = torch.stack([(R[:, 3 * k] * n[:, 0] + R[:, 3 * k + 1] * n[:, 1]) + R[:, 3 * k + 2] * n[:, 2] for k in range(3)], -1)
    ln = ((nc[:, 0] * nc[:, 0] + nc[:, 1] * nc[:, 1]) + nc[:, 2] * nc[:, 2]).sqrt() + 1e-6
    nv = ((nc / ln[:, None]) * 0.5 + 0.5).clamp(0, 1) * 255.0
    cv = c.clamp(0, 1) * 255.0
    if background == "frame":
        bg = frame_rgb[:, ::a.level, ::a.level].reshape(N, 3).float()
    else:
        bg = torch.full((N, 3), 255.0 if background == "white" else 0.0, device=DEV)
    return torch.where(hit[:, None], cv, bg), torch.where(hit[:, None], nv, torch.full_like(nv, 127.0)), depth, hit


@pytest.mark.parametrize("background", ["white", "black", "frame"])
def test_compose_matches_the_tensor_restatement(trained, background):
    from dynhor_amd import surface_render as sr
    a, ds = trained.a, trained.r.dataset
    frames = list(range(ds.n_images))[::-1]                                       # a view's background need not be its own frame
    rgb, depth, normal, hit = sr.compose(a, a.slot, a.normals, a.colors, background, ds.rgb, frames)
    cv, nv, dref, href = _compose_ref(a, background, ds.rgb[frames])
    N = a.N
    assert torch.equal(hit.view(N) > 0, href) and int(href.sum()) >= trained.min_hits
    assert torch.equal(depth.view(N), dref)
    got = rgb.view(N, 3).float()
    off = (got != cv.round()) & ((cv - cv.floor() - 0.5).abs() > 1e-4)
    assert not bool(off.any()), int(off.sum())
    gotn = normal.view(N, 3).float()
    offn = (gotn != nv.floor()) & ((nv - nv.round()).abs() > 1e-4)
    assert not bool(offn.any()), int(offn.sum())
    if background == "frame":
        assert torch.equal(rgb.view(N, 3)[~href], ds.rgb[frames].reshape(N, 3)[~href])
    if background == "white":                                                     # render_surface's own images are these
        assert torch.equal(rgb, trained.out["rgb"]) and torch.equal(depth, trained.out["depth"])
        assert torch.equal(normal, trained.out["normal"]) and torch.equal(hit, trained.out["hit"])


def test_network_without_a_surface_gives_no_hit(tmp_path):
    """The MLP family after 60 iterations of _runner's schedule has no surface inside the unit sphere: the tracer and the fp64 oracle
    traced by the restatement must both say so (no hit, no ray left unfinished, nothing scanned into a hit), and the images are all
    background."""
    from dynhor_amd import surface_render as sr
    from dynhor_amd.runner import Runner
    from oracle import neus_oracle as O
    r = Runner(conf=_conf("neus"), device=DEV, exp_root=str(tmp_path))
    for _ in range(60):
        r.train_iteration()
    ds = r.dataset
    out = sr.render_surface(r.renderer, ds.R, ds.T, ds.K, ds.H, ds.W, background="black")
    o_sdf, _, _ = O.build_models(seed=1, device=r.device)
    o_sdf.load_state_dict(r.sdf_network.state_dict())
    o_sdf.double()
    with torch.no_grad():
        ref = U.trace_ref(lambda p: o_sdf(p)[:, 0], ds.R, ds.T, ds.K, ds.H, ds.W, device=DEV)
    st = out["stats"]
    print(f"neus after 60 iterations: {st}; the oracle's hits {int((ref['state'] == U.HIT).sum())}")
    assert int((ref["state"] == U.HIT).sum()) == 0 and st["hit"] == 0 and st["fail"] == 0 and st["miss"] == st["rays"]
    assert st["rays_in_sphere"] == int((ref["disc"] > 0).sum()) > 10000
    assert not bool(out["hit"].any()) and not bool(out["rgb"].any()) and bool(torch.isinf(out["depth"]).all())


@pytest.fixture(scope="module")
def fresh_renderer(tmp_path_factory):
    from dynhor_amd.runner import Runner
    return Runner(conf=_conf("neus", "fresh"), device=DEV, exp_root=str(tmp_path_factory.mktemp("fresh")))


def test_view_chunks_and_levels_give_the_same_pixels(fresh_renderer, monkeypatch):
    """Views traced in chunks (MAX_RAYS) equal the views traced at once for an analytic field, and level 2 is every second pixel.  The
    geometry is bitwise the same; the network's colours and normals at the same points may round differently in another batch."""
    from dynhor_amd import surface_render as sr
    from dynhor_amd.scene import scene_sdf
    r, ds = fresh_renderer, fresh_renderer.dataset
    f = lambda p: scene_sdf(p)[:, None]
    full = sr.render_surface(r.renderer, ds.R, ds.T, ds.K, ds.H, ds.W, sdf_fn=f)
    assert full["stats"]["hit"] > 1000
    monkeypatch.setattr(sr, "MAX_RAYS", 2 * ds.H * ds.W - 1)                      # one view per chunk
    parts = sr.render_surface(r.renderer, ds.R, ds.T, ds.K, ds.H, ds.W, sdf_fn=f)
    assert torch.equal(full["hit"], parts["hit"]) and torch.equal(full["depth"], parts["depth"])
    for k in ("rgb", "normal"):
        assert int((full[k].int() - parts[k].int()).abs().max()) <= 1, k
    assert parts["stats"]["hit"] == full["stats"]["hit"] and parts["stats"]["rays"] == full["stats"]["rays"]
    half = sr.render_surface(r.renderer, ds.R, ds.T, ds.K, ds.H, ds.W, level=2, sdf_fn=f)
    assert torch.equal(half["hit"], full["hit"][:, ::2, ::2]) and torch.equal(half["depth"], full["depth"][:, ::2, ::2])
    for k in ("rgb", "normal"):
        assert int((half[k].int() - full[k][:, ::2, ::2].int()).abs().max()) <= 1, k


# ------------------------------------------------------------------------------------------------ 7. Runner and CLI
def test_runner_render_views_writes_its_files(trained):
    r = trained.r
    ds = r.dataset
    res = r.render_views("frames")
    d = res["dir"]
    assert d == os.path.join(r.base_exp_dir, "novel_views", "{:0>8d}".format(r.iter_step))
    for k in range(ds.n_images):
        name = "{:04d}".format(k)
        for suffix in (".png", "_normal.png", "_depth.npy"):
            assert os.path.exists(os.path.join(d, name + suffix)), name + suffix
    assert os.path.exists(os.path.join(d, "views.gif"))
    assert np.array_equal(np.load(os.path.join(d, "0001_depth.npy")), res["depth"][1].cpu().numpy())
    from PIL import Image
    assert np.array_equal(np.array(Image.open(os.path.join(d, "0002.png"))), res["rgb"][2].cpu().numpy())
    js = json.load(open(os.path.join(d, "views.json")))
    assert js["method"] == "surface" and js["level"] == 1 and len(js["psnr"]) == len(js["iou"]) == ds.n_images
    assert len(js["worst_psnr"]) == min(5, ds.n_images) and js["worst_psnr"][0]["psnr"] == min(js["psnr"])
    # PSNR with validate_image's mask and formula, recomputed from the returned image
    for k in range(ds.n_images):
        rays, h, w = ds.gen_rays_at(k, 1)
        rays = rays.view(h, w, 14)
        m = rays[..., 9:10] * rays[..., 10:11]
        mse = (((res["rgb"][k].to(DEV).float() / 255.0 - rays[..., 6:9]) ** 2) * m).sum() / (m.sum() * 3.0 + 1e-5)
        assert abs(float(20.0 * torch.log10(1.0 / mse.sqrt())) - js["psnr"][k]) < 1e-4
        lab = ds.label[k]
        keep, hb = lab >= 0, res["hit"][k].to(DEV) > 0
        iou = float(((hb & (lab > 0) & keep).sum()).double() / (((hb | (lab > 0)) & keep).sum()).double().clamp(min=1))
        assert abs(iou - js["iou"][k]) < 1e-9
    assert abs(js["psnr_mean"] - float(np.mean(js["psnr"]))) < 1e-9 and 0.0 < js["iou_mean"] <= 1.0
    assert int(res["hit"].sum()) == trained.out["stats"]["hit"] and js["stats"]["hit"] == trained.out["stats"]["hit"]
    assert os.path.isdir(os.path.join(r.base_exp_dir, "board"))
    # interpolate: ratio 0 is frame 0's pose, so its picture is the frame-0 render; there and back
    it = r.render_views("interpolate:0:1:3", save=False)
    assert it["rgb"].shape[0] == 5 and it["dir"] is None
    assert torch.equal(it["rgb"][0], res["rgb"][0]) and torch.equal(it["depth"][0], res["depth"][0])
    # (the turning point is frame 1's pose and the way back ends at frame 0's: the same silhouettes up to the rays on their rim)
    assert float((it["hit"][2] == res["hit"][1]).float().mean()) > 0.995 and float((it["hit"][4] == it["hit"][0]).float().mean()) > 0.995
    ob = r.render_views("orbit:2", level=2, background="black", save=False)
    assert ob["rgb"].shape == (2, 32, 32, 3) and int(ob["hit"][1].sum()) > trained.min_hits // 40
    assert bool((ob["rgb"][1][ob["hit"][1] == 0] == 0).all())
    # the volume renderer draws the same view: the two pictures agree on the object
    vol = r.render_views("interpolate:0:1:1", method="volume", level=2, save=False)
    assert vol["rgb"].shape == (1, 32, 32, 3) and "depth" not in vol
    with pytest.raises(ValueError):
        r.render_views("frames", method="volume", background="frame")
    with pytest.raises(ValueError):
        r.render_views("orbit:3", background="frame")


def test_cli_interpolate_mode_runs_in_a_child_process(tmp_path):
    import yaml
    from dynhor_amd.runner import Runner
    conf = _conf("neus", "cli")
    r = Runner(conf=conf, device=DEV, exp_root=str(tmp_path))
    for _ in range(3):
        r.train_iteration()
    r.save_checkpoint()
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--mode", "interpolate_0_1", "--view_method",
                        "surface", "--is_continue", "--exp_root", str(tmp_path)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    js = json.loads(lines[0])
    assert js["dir"] == os.path.join(r.base_exp_dir, "novel_views", "{:0>8d}".format(r.iter_step))
    assert js["views"] == "interpolate:0:1:60" and js["level"] == 2 and js["method"] == "surface"
    assert os.path.exists(os.path.join(js["dir"], "views.gif")) and os.path.exists(os.path.join(js["dir"], "0118_depth.npy"))
    assert not os.path.exists(os.path.join(js["dir"], "0119.png"))
