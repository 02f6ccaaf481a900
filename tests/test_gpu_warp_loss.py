"""GPU: dh_ray_depth, dh_warp_loss and dh_ray_depth_bwd (csrc/warp_loss.hip) against the fp64 restatement of their rule
(tests/warp_loss_util.py, licensed by tests/test_cpu_warp_loss.py).

Criterion (the project's standing one, tests/ray_kernels_util.py:ErrorLedger): max |kernel - fp64| <= 4 x max(the fp32 restatement's own
error on the same inputs, one fp32 ulp of the largest reference element), and a relative L2 error below 1e-4.  Discrete outcomes (flags,
valid neighbours, chosen count, chosen bitmask) must be equal except on the rays the fp64 restatement marks as lying within rounding of
a gate (warp_loss_util.TOL_*): those are left out of every comparison and may be at most 2 % of a case; the share is printed.

A ray's outputs depend on that ray's inputs alone, so the batch of one ray is the first ray of the batch of 77 and must give its bits,
and the batch of 256 cut into two calls must give the bits of the whole."""
import ctypes

import pytest
import torch

from tests import mvs_util as VU
from tests import warp_loss_util as U
from tests.ray_kernels_util import Canary, ErrorLedger, hip

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
DEV = "cuda:0"
NF = 9
SRC = 4                                    # the source frame of the grid: neighbours on both sides up to +-4
CELLS = [(P, Nn) for P in (1, 5, 7) for Nn in (1, 4, 8)]
BAD_ARG, UNSUPPORTED = -1, -2
# the seed of a cell's 77-ray batch, picked on the CPU with the two restatements so that at most 2 % of its rays lie within rounding of a
# gate (default 100 P + Nn; at P = 7 with 8 neighbours two of that batch's 77 rays have two l_j closer than 1e-5 at the top-1 boundary)
SEEDS = {(7, 8): 2708}


def _ws(B):
    from dynhor_amd import _lib
    return torch.empty(max(16, int(_lib.lib().dh_warp_loss_workspace(B))), dtype=torch.uint8, device=DEV)


_SCENES = {}


def scene(P):
    """48 x 64 for the two smaller patches, 96 x 96 for P = 7; built once and left unchanged."""
    hw = (96, 96) if P == 7 else (48, 64)
    if hw not in _SCENES:
        c = U.plane_case(hw[0], hw[1], NF, seed=0)
        c["dev"] = {k: c[k].to(DEV).contiguous() for k in ("gray", "valid", "R", "T", "K", "Kinv")}
        _SCENES[hw] = c
    return _SCENES[hw]


def nbr_for(Nn):
    nbr = torch.from_numpy(VU.kernel_nbr(NF, Nn)).clone()
    if Nn >= 4:
        nbr[SRC, 1] = -1                    # a hole among the entries
    if Nn == 8:
        nbr[SRC, 6] = NF + 3                # and one outside [0, F)
    return nbr.int().contiguous()


def run_warp(c, nbr, frame, pix, z, w, n, st, weight=0.0):
    d = c["dev"]
    B = pix.shape[0]
    F, H, W = c["gray"].shape
    cn = Canary(DEV)
    out_f, stats = cn.out("out_f", B, 8), cn.out("stats", 8)
    out_i = cn.out("out_i", B, 4)
    hip("dh_warp_loss", d["gray"], d["valid"], F, H, W, d["R"], d["T"], d["K"], d["Kinv"], nbr.to(DEV), int(nbr.shape[1]), int(frame),
        pix.to(DEV), z.to(DEV), w.to(DEV), n.to(DEV), B, st.patch, st.min_va, st.min_vb, st.topk, st.min_views, st.min_cos, st.min_wsum,
        float(weight), out_f, out_i, stats, _ws(B))
    cn.check()
    return out_f.cpu(), out_i.view(torch.int32).cpu(), stats.cpu()


def _stats_of(r, keep):
    """(L, count, mean score, rays with flag 1, 2, 8, 16) of a restatement's result over the rays `keep`, in fp64."""
    k = keep & r["counts"]
    cnt = max(int(k.sum()), 1)
    fl = r["flags"][keep]
    return torch.tensor([float(r["l"][k].double().sum()) / cnt, float(k.sum()), float(r["score"][k].double().sum()) / cnt]
                        + [float((fl & b).ne(0).sum()) for b in (1, 2, 8, 16)], dtype=F64)


def compare(led, c, nbr, frame, pix, z, w, n, st, got, case, unpooled=None):
    """Judge one call against the two restatements; returns (r64, kept rays).  unpooled (bool [B]): rays whose values are judged by the
    caller and stay out of the ledger's arrays (their discrete outcomes are compared here like everybody's)."""
    out_f, out_i, stats = got
    r64, r32 = U.both_forms(c["gray"], c["valid"], c["R"], c["T"], c["K"], c["Kinv"], nbr, frame, pix, z, w, n, st)
    amb = r64["amb"]
    share = float(amb.float().mean())
    keep = ~amb
    assert share <= 0.02, f"{case}: {share:.3f} of the rays lie within rounding of a gate"
    assert bool(U.discrete_equal(r64, r32)[keep].all()), f"{case}: the two restatements disagree on a ray outside the ambiguous set"
    got_d = {"valid_n": out_i[:, 0].long(), "chosen_n": out_i[:, 1].long(), "flags": out_i[:, 2].long(), "mask": out_i[:, 3].long()}
    bad = (~U.discrete_equal(r64, got_d)) & keep
    assert not bool(bad.any()), f"{case}: discrete outcomes differ on rays {bad.nonzero()[:8, 0].tolist()}: " \
                                f"kernel {out_i[bad][:4].tolist()}, flags64 {r64['flags'][bad][:4].tolist()}"
    k = keep & r64["counts"] & (~unpooled if unpooled is not None else True)
    print(f"{case}: {int(r64['counts'].sum())} of {pix.shape[0]} rays count, ambiguous share {share:.4f}")
    if bool(k.any()):
        led.add("l", out_f[k, 0], r64["l"][k], r32["l"][k], case)
        led.add("g_z", out_f[k, 1], r64["g_z"][k], r32["g_z"][k], case)
        led.add("g_n", out_f[k, 2:5], r64["g_n"][k], r32["g_n"][k], case)
        led.add("score", out_f[k, 5], r64["score"][k], r32["score"][k], case)
        led.add("best", out_f[k, 6], r64["best"][k], r32["best"][k], case)
    dead = keep & ~r64["counts"]
    want = torch.tensor([0, 0, 0, 0, 0, U.NONE, U.NONE, 0], dtype=F32)
    assert bool((out_f[dead] == want).all()), f"{case}: a ray that does not count has outputs"
    assert bool((out_f[:, 7] == 0).all())
    # stats: of the whole batch when no ray is ambiguous; else of a second call on the kept rays alone (a ray's outputs are its own, so
    # that call's per-ray outputs are the first call's), against the reference sums over the kept rays
    if bool(amb.any()):
        sub = run_warp(c, nbr, frame, pix[keep].contiguous(), z[keep].contiguous(), w[keep].contiguous(), n[keep].contiguous(), st)
        assert torch.equal(sub[0].view(torch.int32), out_f[keep].view(torch.int32)) and torch.equal(sub[1], out_i[keep])
        stats = sub[2]
    led.add("stats", stats[[0, 1, 2, 4, 5, 6, 7]], _stats_of(r64, keep), _stats_of(r32, keep).float(), case)
    return r64, keep


@pytest.mark.parametrize("P,Nn", CELLS)
def test_values_gradients_and_discrete_outcomes(P, Nn):
    c, nbr = scene(P), nbr_for(Nn)
    led = ErrorLedger()
    seed = SEEDS.get((P, Nn), 100 * P + Nn)
    for topk, mv in ((1, 1), (4, 1), (1, 2), (4, 2)):
        st = U.settings(patch=P, topk=topk, min_views=mv)
        pix, z, w, n = U.random_rays(c, SRC, 77, seed, margin=max(P - 1, 0))
        got = run_warp(c, nbr, SRC, pix, z, w, n, st, weight=0.5)
        r64, keep = compare(led, c, nbr, SRC, pix, z, w, n, st, got, f"P={P} Nn={Nn} topk={topk} min_views={mv} B=77")
        assert abs(float(got[2][3]) - 0.5 * float(got[2][0])) <= 1e-7 * max(1.0, abs(float(got[2][0])))
        if mv == 1:
            assert int(r64["counts"].sum()) >= 10, "the case must hold rays that count"
            if Nn > 1 and topk == 4:
                assert bool((r64["valid_n"][r64["counts"]] < topk).any()), "topk above the valid neighbours must occur"
        # the batch of one ray: the first ray of the batch, bit for bit; its stats are that ray's
        one = run_warp(c, nbr, SRC, pix[:1], z[:1], w[:1], n[:1], st, weight=0.5)
        assert torch.equal(one[0].view(torch.int32), got[0][:1].view(torch.int32)) and torch.equal(one[1], got[1][:1])
        cnt = 1.0 if int(one[1][0, 2]) == 0 else 0.0
        assert float(one[2][1]) == cnt and float(one[2][0]) == float(one[0][0, 0]) * cnt
    # 256 rays, and the same cut into two calls
    st = U.settings(patch=P, topk=4, min_views=1 if Nn == 1 else 2)
    pix, z, w, n = U.random_rays(c, SRC, 256, 100 * P + Nn + 7, margin=max(P - 1, 0))
    whole = run_warp(c, nbr, SRC, pix, z, w, n, st)
    compare(led, c, nbr, SRC, pix, z, w, n, st, whole, f"P={P} Nn={Nn} B=256")
    again = run_warp(c, nbr, SRC, pix, z, w, n, st)
    for a, b in zip(whole, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two launches differ"
    cut = 100
    lo = run_warp(c, nbr, SRC, pix[:cut].contiguous(), z[:cut].contiguous(), w[:cut].contiguous(), n[:cut].contiguous(), st)
    hi = run_warp(c, nbr, SRC, pix[cut:].contiguous(), z[cut:].contiguous(), w[cut:].contiguous(), n[cut:].contiguous(), st)
    assert torch.equal(torch.cat([lo[0], hi[0]]).view(torch.int32), whole[0].view(torch.int32)), "out_f of the parts differs from the whole"
    assert torch.equal(torch.cat([lo[1], hi[1]]), whole[1]), "out_i of the parts differs from the whole"
    assert float(lo[2][1]) + float(hi[2][1]) == float(whole[2][1])
    led.report(f"dh_warp_loss P={P} Nn={Nn}")


def _bwd(c_rays, R, z, t, wsum, out_f, stats, sample_dist, weight, acc, dw, dn, packed=None):
    B = c_rays.shape[0]
    if packed is None:
        hip("dh_ray_depth_bwd", c_rays, R, z, t, wsum, out_f, stats, B, int(z.shape[1]), float(sample_dist), float(weight), int(acc), dw, dn)
    else:
        off, cnt, ms = packed
        hip("dh_ray_depth_bwd_packed", c_rays, R, z, t, wsum, out_f, stats, B, off, cnt, int(ms), float(sample_dist), float(weight),
            int(acc), dw, dn)


def test_planted_rays():
    """One ray of every kind that must not count, among rays that do; none of them reaches stats or the adjoints."""
    P, Nn, frame = 5, 4, 2
    c = U.plane_case(96, 96, NF, seed=0)
    c["dev"] = {k: c[k].to(DEV).contiguous() for k in ("gray", "valid", "R", "T", "K", "Kinv")}
    nbr = torch.from_numpy(VU.kernel_nbr(NF, Nn)).int().contiguous()
    st = U.settings(patch=P, topk=4, min_views=2)
    pix, z, w, n = U.random_rays(c, frame, 24, seed=11, margin=30)
    good = (60, 30)                                                      # a textured pixel away from the border, the hand and the flat block
    plant = {"border": (2, 40), "hand": (42, 66), "flat": (37, 13), "z_inf": good, "z_neg": good, "z_zero": good,
             "away": good, "wsum": good, "scale_1": good, "scale_up": good, "scale_down": good}
    names = list(plant)
    for i, k in enumerate(names):
        x, y = plant[k]
        pix[i, 0], pix[i, 1] = x, y
        z[i] = c["z"][frame][y, x] + 0.004
        n[i] = c["n_obj"][frame] + torch.tensor([0.03, -0.02, 0.0])
        w[i] = 0.9
    at = {k: i for i, k in enumerate(names)}
    z[at["z_inf"]] = float("inf"); z[at["z_neg"]] = -0.5; z[at["z_zero"]] = 0.0
    n[at["away"]] = -n[at["away"]]
    w[at["wsum"]] = 0.3
    n[at["scale_up"]] = n[at["scale_1"]] * 1e3
    n[at["scale_down"]] = n[at["scale_1"]] * 1e-3
    assert int(c["valid"][frame][66, 42]) == 1 and int(c["valid"][frame][66, 37]) == 0, "the hand ray's own pixel is valid; its patch is not"
    out_f, out_i, stats = run_warp(c, nbr, frame, pix, z, w, n, st, weight=0.25)
    led = ErrorLedger()
    # the two scaled copies of a ray stay out of the ledger: g_n of one of them is 1e3 times everybody else's, and the relative L2 of
    # the array would be a statement about that one ray; they are judged against the unscaled ray below
    scaled = torch.zeros(pix.shape[0], dtype=torch.bool)
    scaled[at["scale_up"]] = scaled[at["scale_down"]] = True
    r64, keep = compare(led, c, nbr, frame, pix, z, w, n, st, (out_f, out_i, stats), "planted", unpooled=scaled)
    fl = out_i[:, 2]
    for k, want in (("border", 1), ("hand", 1), ("flat", 1), ("z_inf", 8), ("z_neg", 8), ("z_zero", 8), ("away", 8), ("wsum", 16)):
        assert int(fl[at[k]]) == want, (k, int(fl[at[k]]))
        assert int(out_i[at[k], 1]) == 0 and bool((out_f[at[k], :5] == 0).all())
    assert int(fl[at["scale_1"]]) == 0, "the reference ray of the scale test must count"
    # the rule does not see the normal's length: the same loss, g_z; g_n scales inversely
    a, up, dn_ = out_f[at["scale_1"]], out_f[at["scale_up"]], out_f[at["scale_down"]]
    e32 = max(led.worst["l"][2], led.worst["l"][3])
    assert abs(float(up[0] - a[0])) <= 8 * e32 and abs(float(dn_[0] - a[0])) <= 8 * e32           # each within 4 x of the reference
    eg = max(led.worst["g_z"][2], led.worst["g_z"][3])
    assert abs(float(up[1] - a[1])) <= 8 * eg and abs(float(dn_[1] - a[1])) <= 8 * eg
    en = max(led.worst["g_n"][2], led.worst["g_n"][3])
    assert float((up[2:5] * 1e3 - a[2:5]).abs().max()) <= 8 * en and float((dn_[2:5] * 1e-3 - a[2:5]).abs().max()) <= 8 * en
    assert out_i[at["scale_up"]].tolist() == out_i[at["scale_1"]].tolist() == out_i[at["scale_down"]].tolist()
    # stats: only the counted rays
    counted = fl == 0
    assert float(stats[1]) == float(counted.sum())
    assert abs(float(stats[0]) - float(out_f[counted, 0].double().mean())) <= 1e-6
    assert float(stats[4]) == float((fl & 1).ne(0).sum()) and float(stats[6]) == float((fl & 8).ne(0).sum())
    assert float(stats[7]) == float((fl & 16).ne(0).sum()) and float(stats[5]) == float((fl & 2).ne(0).sum())
    # a frame whose neighbours are all -1: every ray that has a source and a plane gets flag 2
    last = NF - 1
    pix2, z2, w2, n2 = U.random_rays(c, last, 16, seed=12, margin=30)
    f2, i2, s2 = run_warp(c, nbr, last, pix2, z2, w2, n2, st, weight=0.25)
    assert bool(((i2[:, 2] == 2) | ((i2[:, 2] & 1) != 0)).all()) and int((i2[:, 2] == 2).sum()) >= 4
    assert float(s2[1]) == 0.0 and float(s2[0]) == 0.0 and float(s2[3]) == 0.0 and bool((f2[:, :5] == 0).all())
    # the adjoints: rows of rays that do not count are exact zeros when written and untouched when added to
    B, ns = pix.shape[0], 16
    g = torch.Generator().manual_seed(5)
    rays = torch.zeros(B, 14)
    rays[:, 3:6] = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1)
    zs = torch.sort(torch.rand(B, ns, generator=g) + 0.5, dim=1).values
    t = (zs.mean(1)).contiguous()
    R = c["R"][frame].contiguous()
    dev = lambda x: x.to(DEV).contiguous()
    cn = Canary(DEV)
    dw, dnm = cn.out("dw", B, ns), cn.out("dn", B, 3)
    _bwd(dev(rays), dev(R), dev(zs), dev(t), dev(w), dev(out_f), dev(stats), 0.03, 0.25, 0, dw, dnm)
    cn.check()
    assert bool((dw.cpu()[~counted] == 0).all()) and bool((dnm.cpu()[~counted] == 0).all())
    assert bool((dw.cpu()[counted].abs().sum(1) > 0).all())
    prior_w, prior_n = torch.randn(B, ns, generator=g), torch.randn(B, 3, generator=g)
    dw2, dn2 = dev(prior_w), dev(prior_n)
    _bwd(dev(rays), dev(R), dev(zs), dev(t), dev(w), dev(out_f), dev(stats), 0.03, 0.25, 3, dw2, dn2)
    assert torch.equal(dw2.cpu()[~counted], prior_w[~counted]) and torch.equal(dn2.cpu()[~counted], prior_n[~counted])
    assert torch.equal(dw2.cpu(), prior_w + dw.cpu()) and torch.equal(dn2.cpu(), prior_n + dnm.cpu())
    led.report("dh_warp_loss planted rays")


def _depth_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    rays = torch.zeros(B, 14)
    rays[:, 3:6] = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1)
    R = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64)).Q.float().reshape(9).contiguous()
    out_f = torch.zeros(B, 8)
    out_f[:, 1:5] = torch.randn(B, 4, generator=g)
    out_f[::5, 1:5] = 0.0                                                # rays that do not count
    stats = torch.zeros(8)
    stats[1] = float(max(B - (B + 4) // 5, 0))
    return g, rays, R, out_f, stats


def _judge_bwd(led, case, dw, dn, w64, zc64_of, w32, zc32_of, out_f, stats, weight, rays):
    """d_weights, d_nmap of the kernel against fp64 autograd of sum_r s g_z,r zc_r(w) with s = weight / max(count, 1)."""
    s = weight / max(float(stats[1]), 1.0)
    refs = []
    for wv, fn, D in ((w64, zc64_of, F64), (w32, zc32_of, F32)):
        wv = wv.detach().clone().requires_grad_(True)
        zc = fn(wv)
        coef = (s * out_f[:, 1].to(F64)).to(D)
        (gw,) = torch.autograd.grad((coef * torch.nan_to_num(zc)).sum(), wv)
        refs.append(gw)
    led.add("d_weights", dw, refs[0], refs[1], case)
    n64 = s * out_f[:, 2:5].double()
    led.add("d_nmap", dn, n64, n64.float(), case)


@pytest.mark.parametrize("n", [16, 128])
def test_ray_depth_dense(n):
    B, sd, weight = 37, 0.03, 0.7
    g, rays, R, out_f, stats = _depth_inputs(B, 40 + n)
    z = torch.sort(torch.rand(B, n, generator=g) * 2 + 0.5, dim=1).values.contiguous()
    wts = (torch.rand(B, n, generator=g) ** 4).contiguous()
    wts[3] *= 1e-3                                                       # a nearly transparent ray
    dev = lambda x: x.to(DEV).contiguous()
    cn = Canary(DEV)
    t, W, zc = cn.out("t", B), cn.out("W", B), cn.out("zc", B)
    hip("dh_ray_depth", dev(rays), dev(R), dev(z), dev(wts), B, n, sd, t, W, zc)
    cn.check()
    led = ErrorLedger()
    r64 = U.ray_depth_dense(rays, R, z, wts, sd, F64)
    r32 = U.ray_depth_dense(rays, R, z, wts, sd, F32)
    for name, got, a, b in zip(("t", "W", "zc"), (t, W, zc), r64, r32):
        led.add(name, got.cpu(), a, b, f"dense n={n}")
    cn = Canary(DEV)
    dw, dn = cn.out("dw", B, n), cn.out("dn", B, 3)
    _bwd(dev(rays), dev(R), dev(z), t, W, dev(out_f), dev(stats), sd, weight, 0, dw, dn)
    cn.check()
    _judge_bwd(led, f"dense n={n}", dw.cpu(), dn.cpu(), wts.double(), lambda wv: U.ray_depth_dense(rays, R, z, wv, sd, F64)[2], wts.clone(),
               lambda wv: U.ray_depth_dense(rays, R, z, wv, sd, F32)[2], out_f, stats, weight, rays)
    assert bool((dw.cpu()[::5] == 0).all()) and bool((dn.cpu()[::5] == 0).all())
    for acc in (1, 2, 3):
        pw, pn = torch.randn(B, n, generator=g), torch.randn(B, 3, generator=g)
        dw2, dn2 = dev(pw), dev(pn)
        _bwd(dev(rays), dev(R), dev(z), t, W, dev(out_f), dev(stats), sd, weight, acc, dw2, dn2)
        assert torch.equal(dw2.cpu(), pw + dw.cpu() if acc & 1 else dw.cpu()), f"accumulate {acc}: d_weights"
        assert torch.equal(dn2.cpu(), pn + dn.cpu() if acc & 2 else dn.cpu()), f"accumulate {acc}: d_nmap"
    # either output may be absent
    dw3 = dev(torch.zeros(B, n))
    _bwd(dev(rays), dev(R), dev(z), t, W, dev(out_f), dev(stats), sd, weight, 0, dw3, None)
    assert torch.equal(dw3.cpu(), dw.cpu())
    led.report(f"dh_ray_depth dense n={n}")


def test_ray_depth_packed():
    cnt = torch.tensor([0, 1, 5, 64, 65, 130, 0, 200, 33, 7], dtype=torch.int32)
    B, step, weight, ms = cnt.numel(), 1.0 / 128, 0.7, 160                 # the cap cuts the ray of 200 samples
    g, rays, R, out_f, stats = _depth_inputs(B, 77)
    out_f[:, 1:5] = torch.randn(B, 4, generator=g)
    out_f[2, 1:5] = 0.0
    off = (torch.cumsum(cnt.long(), 0) - cnt.long()).contiguous()
    N = int(cnt.sum())
    t_start = torch.cat([torch.arange(int(k)) * step + 0.4 + 0.01 * i for i, k in enumerate(cnt)]).float().contiguous()
    wts = (torch.rand(N, generator=g) ** 3).contiguous()
    dev = lambda x: x.to(DEV).contiguous()
    cn = Canary(DEV)
    t, W, zc = cn.out("t", B), cn.out("W", B), cn.out("zc", B)
    hip("dh_ray_depth_packed", dev(rays), dev(R), dev(t_start), dev(wts), B, dev(off), dev(cnt), ms, step, t, W, zc)
    cn.check()
    led = ErrorLedger()
    r64 = U.ray_depth_packed(rays, R, t_start, wts, off, cnt, ms, step, F64)
    r32 = U.ray_depth_packed(rays, R, t_start, wts, off, cnt, ms, step, F32)
    for name, got, a, b in zip(("t", "W", "zc"), (t, W, zc), r64, r32):
        led.add(name, got.cpu(), a, b, "packed")
    empty = cnt == 0
    assert bool((t.cpu()[empty] == 0).all()) and bool((W.cpu()[empty] == 0).all()) and bool((zc.cpu()[empty] == 0).all())
    prior = torch.randn(N, generator=g)
    dw = dev(prior)
    cn = Canary(DEV)
    dn = cn.out("dn", B, 3)
    _bwd(dev(rays), dev(R), dev(t_start), t, W, dev(out_f), dev(stats), step, weight, 0, dw, dn, packed=(dev(off), dev(cnt), ms))
    cn.check()
    covered = torch.zeros(N, dtype=torch.bool)
    for r in range(B):
        covered[int(off[r]):int(off[r]) + min(int(cnt[r]), ms)] = True
    assert torch.equal(dw.cpu()[~covered], prior[~covered]), "samples past the cap were written"
    got = torch.where(covered, dw.cpu(), torch.zeros(N))
    _judge_bwd(led, "packed", got, dn.cpu(), wts.double(),
               lambda wv: U.ray_depth_packed(rays, R, t_start, wv, off, cnt, ms, step, F64)[2], wts.clone(),
               lambda wv: U.ray_depth_packed(rays, R, t_start, wv, off, cnt, ms, step, F32)[2], out_f, stats, weight, rays)
    dw2, dn2 = dev(prior), dev(torch.ones(B, 3))
    _bwd(dev(rays), dev(R), dev(t_start), t, W, dev(out_f), dev(stats), step, weight, 3, dw2, dn2, packed=(dev(off), dev(cnt), ms))
    assert torch.equal(dw2.cpu(), torch.where(covered, prior + got, prior)) and torch.equal(dn2.cpu(), 1.0 + dn.cpu())
    led.report("dh_ray_depth_packed")


def test_arguments():
    from dynhor_amd import _lib
    L = _lib.lib()
    P, Nn = 5, 4
    c, nbr = scene(P), nbr_for(Nn).to(DEV)
    d = c["dev"]
    F, H, W = c["gray"].shape
    st = U.settings(patch=P)
    pix, z, w, n = (x.to(DEV) for x in U.random_rays(c, SRC, 8, 1, margin=4))
    out_f, out_i = torch.zeros(8, 8, device=DEV), torch.zeros(8, 4, dtype=torch.int32, device=DEV)
    stats, ws = torch.zeros(8, device=DEV), _ws(8)
    p = _lib.ptr
    null = ctypes.c_void_p(0)

    def warp(**kw):
        a = dict(gray=p(d["gray"]), valid=p(d["valid"]), F=F, H=H, W=W, R=p(d["R"]), T=p(d["T"]), K=p(d["K"]), Kinv=p(d["Kinv"]), nbr=p(nbr),
                 Nn=Nn, frame=SRC, pix=p(pix), z=p(z), w=p(w), n=p(n), B=8, P=P, min_va=st.min_va, min_vb=st.min_vb, topk=4, min_views=2,
                 min_cos=0.1, min_wsum=0.5, weight=0.5, out_f=p(out_f), out_i=p(out_i), stats=p(stats), ws=p(ws))
        a.update(kw)
        return L.dh_warp_loss(*a.values(), _lib.stream())

    assert warp() == 0
    nan = float("nan")
    for kw in (dict(gray=null), dict(valid=null), dict(R=null), dict(nbr=null), dict(pix=null), dict(z=null), dict(n=null), dict(out_f=null),
               dict(out_i=null), dict(stats=null), dict(ws=null), dict(P=0), dict(P=8), dict(Nn=0), dict(Nn=9), dict(topk=0), dict(topk=9),
               dict(min_views=0), dict(min_views=9), dict(min_cos=nan), dict(min_cos=1.5), dict(min_wsum=nan), dict(min_vb=nan),
               dict(min_vb=0.0), dict(min_va=0), dict(weight=nan), dict(weight=-1.0), dict(B=-1), dict(frame=-1), dict(frame=F), dict(H=0),
               dict(z=ctypes.c_void_p(p(z).value + 2)), dict(out_f=ctypes.c_void_p(p(out_f).value + 1)),
               dict(ws=ctypes.c_void_p(p(ws).value + 8))):
        assert warp(**kw) == BAD_ARG, kw
    assert warp(B=1 << 31) == UNSUPPORTED and warp(H=(1 << 24) + 1) == UNSUPPORTED
    # B == 0 writes nothing, whatever the pointers
    cn = Canary(DEV)
    of, st8 = cn.out("out_f", 8, 8), cn.out("stats", 8)
    assert warp(B=0, out_f=p(of), stats=p(st8)) == 0 and warp(B=0, gray=null, out_f=null, stats=null, ws=null) == 0
    torch.cuda.synchronize()
    cn.check(untouched=("out_f", "stats"))
    # the ray-depth entries
    rays, R = torch.zeros(4, 14, device=DEV), torch.eye(3, device=DEV).reshape(9)
    zz, wt = torch.rand(4, 16, device=DEV), torch.rand(4, 16, device=DEV)
    t, Ws, zc = (torch.zeros(4, device=DEV) for _ in range(3))
    s = _lib.stream()
    assert L.dh_ray_depth(p(rays), p(R), p(zz), p(wt), 4, 16, 0.03, p(t), p(Ws), p(zc), s) == 0
    assert L.dh_ray_depth(p(rays), p(R), p(zz), p(wt), 4, 0, 0.03, p(t), p(Ws), p(zc), s) == BAD_ARG
    assert L.dh_ray_depth(p(rays), p(R), p(zz), p(wt), -1, 16, 0.03, p(t), p(Ws), p(zc), s) == BAD_ARG
    assert L.dh_ray_depth(null, p(R), p(zz), p(wt), 4, 16, 0.03, p(t), p(Ws), p(zc), s) == BAD_ARG
    assert L.dh_ray_depth(p(rays), p(R), p(zz), p(wt), 4, 16, 0.03, p(t), null, p(zc), s) == BAD_ARG
    assert L.dh_ray_depth(p(rays), p(R), p(zz), p(wt), 4, 16, nan, p(t), p(Ws), p(zc), s) == BAD_ARG
    assert L.dh_ray_depth(null, null, null, null, 0, 16, 0.03, null, null, null, s) == 0
    off, cnt = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    assert L.dh_ray_depth_packed(p(rays), p(R), p(zz), p(wt), 4, p(off), p(cnt), 64, 0.01, p(t), p(Ws), p(zc), s) == 0
    assert L.dh_ray_depth_packed(p(rays), p(R), p(zz), p(wt), 4, null, p(cnt), 64, 0.01, p(t), p(Ws), p(zc), s) == BAD_ARG
    assert L.dh_ray_depth_packed(p(rays), p(R), p(zz), p(wt), 4, p(off), p(cnt), -1, 0.01, p(t), p(Ws), p(zc), s) == BAD_ARG
    assert L.dh_ray_depth_packed(p(rays), p(R), p(zz), p(wt), 4, p(off), p(cnt), 1025, 0.01, p(t), p(Ws), p(zc), s) == UNSUPPORTED
    rf, dw, dn = torch.zeros(4, 8, device=DEV), torch.zeros(4, 16, device=DEV), torch.zeros(4, 3, device=DEV)
    bwd = lambda **k: L.dh_ray_depth_bwd(p(rays), p(R), p(zz), p(t), p(Ws), k.get("rf", p(rf)), k.get("st", p(stats)), k.get("B", 4),
                                         k.get("n", 16), 0.03, k.get("w", 0.5), k.get("acc", 0), p(dw), p(dn), s)
    assert bwd() == 0 and bwd(B=0) == 0
    for kw in (dict(rf=null), dict(st=null), dict(n=0), dict(w=nan), dict(w=-1.0), dict(acc=4), dict(acc=-1), dict(B=-2)):
        assert bwd(**kw) == BAD_ARG, kw
    assert L.dh_ray_depth_bwd_packed(p(rays), p(R), p(zz), p(t), p(Ws), p(rf), p(stats), 4, p(off), p(cnt), 64, 0.01, 0.5, 0, p(dw), p(dn), s) == 0
    assert L.dh_ray_depth_bwd_packed(p(rays), p(R), p(zz), p(t), p(Ws), p(rf), p(stats), 4, p(off), null, 64, 0.01, 0.5, 0, p(dw), p(dn),
                                     s) == BAD_ARG
    assert L.dh_ray_depth_bwd_packed(p(rays), p(R), p(zz), p(t), p(Ws), p(rf), p(stats), 4, p(off), p(cnt), 2000, 0.01, 0.5, 0, p(dw), p(dn),
                                     s) == UNSUPPORTED
    assert int(L.dh_warp_loss_workspace(-1)) == BAD_ARG and int(L.dh_warp_loss_workspace(0)) > 0
    torch.cuda.synchronize()
