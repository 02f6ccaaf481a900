"""GPU: dh_prior_loss and dh_prior_loss_packed (csrc/prior_loss.hip) against the fp64 restatement of their rule
(tests/prior_loss_util.py, licensed by tests/test_cpu_prior_loss.py).

Criterion (the project's standing one, tests/ray_kernels_util.py:ErrorLedger): max |kernel - fp64| <= 4 x max(the fp32 restatement's own
error on the same inputs, one fp32 ulp of the largest reference element), and a relative L2 error below 1e-4.

t^ is not an output of the entries.  It is checked where it is all an output holds: in a batch of one counted ray stats[2] (1 + 1e-5)
is |t^ c_z - prior|, so the (1, 1) shape judges t^ alone, and every d_weights row is rho'(e(t^)) c_z m_k.

A batch of B rays holds ray kinds KINDS[(i + seed) % 8]; eight seeds per shape give every kind to every shape, also to the shapes of
fewer than eight rays, and make some single-ray batches hold no valid ray at all."""
import pytest
import torch

from tests import prior_loss_util as P
from tests.ray_kernels_util import ErrorLedger, Canary, hip

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
DEV = "cuda:0"


def _ws(B):
    from dynhor_amd import _lib
    return torch.empty(max(16, int(_lib.lib().dh_prior_loss_workspace(B))), dtype=torch.uint8, device=DEV)


def run_dense(x, depth_w, normal_w, accumulate=0, d_weights=None, with_normal=True, with_prior=True):
    g = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in x.items()}
    B, n = x["z"].shape
    c = Canary(DEV)
    stats = c.out("stats", 8)
    dw = c.out("d_weights", B, n) if d_weights is None else c.inout("d_weights", d_weights.to(DEV))
    dn = c.out("d_nmap", B, 3)
    hip("dh_prior_loss", g["rays"], g["R"], g["z"], g["weights"], g["nmap"] if with_normal else None, g["prior"] if with_prior else None,
        B, n, float(x["sample_dist"]), float(depth_w), P.DELTA, float(normal_w), int(accumulate), stats, dw, dn, _ws(B))
    untouched = (() if with_normal and normal_w > 0 else ("d_nmap",)) + (() if with_prior else ("d_weights",))
    c.check(untouched=untouched)
    return stats.cpu(), dw.cpu(), dn.cpu()


def run_packed(x, depth_w, normal_w, max_samples=1024):
    g = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in x.items()}
    B, N = x["rays"].shape[0], x["t_start"].shape[0]
    c = Canary(DEV)
    stats, dn = c.out("stats", 8), c.out("d_nmap", B, 3)
    # samples past a cap below the counts are not written: only the pads are watched then
    dw = c.out("d_weights", N) if max_samples >= int(x["cnt"].max()) else c.inout("d_weights", torch.zeros(N))
    hip("dh_prior_loss_packed", g["rays"], g["R"], g["t_start"], g["weights"], g["nmap"], g["prior"], B, g["off"], g["cnt"],
        int(max_samples), x["step"], float(depth_w), P.DELTA, float(normal_w), 0, stats, dw, dn, _ws(B))
    c.check(untouched=() if normal_w > 0 else ("d_nmap",))
    return stats.cpu(), dw.cpu(), dn.cpu()


def reference(x, mid, weights, depth_w, normal_w, dtype, has_sample=None):
    d = P.depth_term(x["rays"], x["R"], mid, weights, x["prior"], P.DELTA, dtype, has_sample)
    nr = P.normal_term(x["rays"], x["R"], x["nmap"], dtype)
    return (P.stats_ref(d, nr, depth_w, normal_w), P.depth_adjoint(d, mid, depth_w, P.DELTA, dtype),
            P.normal_adjoint(x["rays"], x["R"], x["nmap"], normal_w, dtype), d)


@pytest.mark.parametrize("B,n", [(1, 1), (3, 5), (4, 64), (5, 128), (131, 96), (300, 128)])
def test_dense_kernel_matches_fp64(B, n):
    led = ErrorLedger()
    kinds, branches, empty_batches = set(), [0, 0], 0
    for seed in range(8):
        x = P.dense_inputs(B, n, seed, grey_every=3)
        mid64 = P.midpoints(x["z"].double(), x["sample_dist"])
        mid32 = P.midpoints(x["z"], torch.tensor(x["sample_dist"], dtype=F32))
        mg = P.margins(x, mid64, x["weights"])
        assert mg["delta"] > 0.1 and mg["zero"] > 0.1 and mg["prior"] > 1e-4 and mg["normal"] > 0.2, mg
        kinds |= {P.KINDS[k] for k in x["kind"].tolist()}
        branches[0] += mg["inliers"]; branches[1] += mg["outliers"]
        dw_, nw_ = 0.7, 0.3
        s64, w64, n64, d64 = reference(x, mid64, x["weights"], dw_, nw_, F64)
        s32, w32, n32, _ = reference(x, mid32, x["weights"], dw_, nw_, F32)
        stats, dw, dn = run_dense(x, dw_, nw_)
        case = f"B={B} n={n} seed={seed}"
        print(case, "stats", stats.tolist(), "fp64", s64.tolist())
        v = d64["v"]
        if int(v.sum()) == 0:
            empty_batches += 1
            assert stats[0].item() == 0.0 and stats[1].item() == 0.0 and stats[2].item() == 0.0 and stats[3].item() == 0.0
            assert bool((dw == 0).all())
        if B == 1 and int(v.sum()) == 1:
            # one counted ray: stats[2] (1 + 1e-5) = |t^ c_z - prior|, t^'s own check (against the fp32 restatement's |e|)
            e64 = d64["e"].abs()
            e32 = P.depth_term(x["rays"], x["R"], mid32, x["weights"], x["prior"], P.DELTA, F32)["e"].abs()
            led.add("t_hat", stats[2:3] * (1.0 + 1e-5), e64, e32, case, pool=True)
        # the depth statistics, the normal statistics and the adjoints are judged apart: their sizes differ by orders of magnitude.
        # Batches of at most 5 rays are pooled over the shape's eight seeds (ray_kernels_util.pooled: "4 x the fp32 restatement's error"
        # is a statement about a sample).  That holds for d_weights at any n: a row is ONE rounding-sensitive number, rho'(e) with e
        # what is left of z^ - prior (0.2 .. 0.7 delta of a depth near 2), times the exact m_k -- a few coefficients a batch, and the
        # fp32 restatement's z^ of two rays can be right to 1e-8 by luck.
        pool = B <= 5
        for name, sl in (("L_d", slice(0, 1)), ("sum_v", slice(1, 2)), ("abs_e", slice(2, 3)), ("w_L_d", slice(3, 4)), ("L_n", slice(4, 5)),
                         ("sum_q", slice(5, 6)), ("w_L_n", slice(6, 7))):
            led.add(name, stats[sl], s64[sl], s32[sl], case, pool=pool)
        assert stats[7].item() == 0.0
        led.add("d_weights", dw, w64, w32, case, pool=pool)
        led.add("d_nmap", dn, n64, n32, case, pool=pool)
        assert bool((dw[~v] == 0).all()), "rays that do not count get exact zeros"
        assert bool((dn[P.normal_term(x["rays"], x["R"], x["nmap"], F64)["q"] == 0] == 0).all())
        stats2, dw2, dn2 = run_dense(x, dw_, nw_)
        assert torch.equal(stats, stats2) and torch.equal(dw, dw2) and torch.equal(dn, dn2), "two launches must agree bit for bit"
    led.flush(f"B={B} n={n}, eight seeds pooled")
    led.report(f"dh_prior_loss B={B} n={n}")
    assert kinds == set(P.KINDS), f"the shape's batches must hold every kind of ray, got {sorted(kinds)}"
    assert branches[0] > 0 and branches[1] > 0, "both Huber branches"
    if B == 1:
        assert empty_batches >= 4, "single-ray batches of an invalid kind hold no valid ray"


def test_batch_without_a_valid_ray():
    x = P.dense_inputs(37, 16, 2, grey_every=2)
    x["prior"][0::2] = float("nan")
    x["prior"][1::2] = 0.0
    stats, dw, _ = run_dense(x, 0.5, 0.0)
    assert stats[0].item() == 0.0 and stats[1].item() == 0.0 and stats[3].item() == 0.0 and bool((dw == 0).all())
    # a null prior_depth is the same statement, and neither reads nor writes d_weights
    stats0, _, _ = run_dense(x, 0.5, 0.0, with_prior=False)
    assert torch.equal(stats0[:4], torch.zeros(4)) and stats0[4].item() == stats[4].item()


def test_accumulate_stacks_on_the_correspondence_adjoint():
    from tests.test_gpu_correspondence import _random_case
    B, n = 131, 96
    o, d, z, w, corr, R_all, T_all, K = _random_case(B, n, seed=9)
    x = P.dense_inputs(B, n, 1)
    x["z"], x["weights"] = z.cpu(), w.cpu()
    x["rays"][:, 0:3], x["rays"][:, 3:6] = o.cpu(), d.cpu()
    mid = P.midpoints(x["z"].double(), x["sample_dist"])
    d64 = P.depth_term(x["rays"], x["R"], mid, x["weights"], torch.ones(B), P.DELTA, F64)
    x["prior"] = P.make_prior(d64["t_hat"] * d64["c_z"], x["kind"], P._gen(5))
    st, res, dwc = torch.empty(4, device=DEV), torch.empty(B, device=DEV), torch.empty(B, n, device=DEV)
    hip("dh_corr_loss", o, d, z, w, corr, R_all, T_all, R_all.shape[0], K, B, n, float(x["sample_dist"]), 4.0, 0.3, st, res, dwc, None)
    assert float(dwc.abs().max()) > 0
    _, alone, _ = run_dense(x, 0.7, 0.0)
    assert float(alone.abs().max()) > 0
    _, both, _ = run_dense(x, 0.7, 0.0, accumulate=1, d_weights=dwc)
    want = dwc.cpu().double() + alone.double()
    big = torch.maximum(dwc.cpu().abs(), alone.abs()).double()
    assert bool(((both.double() - want).abs() <= 2.0 ** -23 * big).all()), "one fp32 rounding of the larger addend"
    _, kept, _ = run_dense(x, 0.0, 0.0, accumulate=1, d_weights=dwc)
    assert torch.equal(kept.view(torch.int32), dwc.cpu().view(torch.int32)), "depth_weight 0 must leave the buffer bit for bit"
    neg = torch.full((B, n), -0.0)
    _, kept, _ = run_dense(x, 0.0, 0.0, accumulate=1, d_weights=neg)
    assert torch.equal(kept.view(torch.int32), neg.view(torch.int32))


PACKED_COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 1024, 0, 5, 129, 64, 1, 1024, 63, 2]


def test_packed_kernel_matches_fp64():
    led = ErrorLedger()
    kinds = set()
    for seed in range(8):
        x = P.packed_inputs(PACKED_COUNTS, seed)
        has = x["cnt"] > 0
        mg = P.margins(x, x["mid_pad"], x["w_pad"], has)
        assert mg["delta"] > 0.1 and mg["zero"] > 0.1 and mg["prior"] > 1e-4 and mg["inliers"] > 0 and mg["outliers"] > 0, mg
        kinds |= {P.KINDS[k] for k in x["kind"].tolist()}
        live = x["live"]
        step32 = torch.tensor(x["step"], dtype=F32)
        t_pad = torch.zeros(live.shape, dtype=F32); t_pad[live] = x["t_start"]
        mid32 = torch.where(live, t_pad + 0.5 * step32, torch.zeros_like(t_pad))
        s64, w64, _, d64 = reference(x, x["mid_pad"], x["w_pad"], 0.7, 0.3, F64, has)
        s32, w32, _, _ = reference(x, mid32, x["w_pad"], 0.7, 0.3, F32, has)
        stats, dw, _ = run_packed(x, 0.7, 0.3)
        case = f"packed seed={seed}"
        print(case, "stats", stats.tolist(), "fp64", s64.tolist())
        for name, i in (("L_d", 0), ("sum_v", 1), ("abs_e", 2), ("w_L_d", 3), ("L_n", 4), ("sum_q", 5), ("w_L_n", 6)):
            led.add(name, stats[i:i + 1], s64[i:i + 1], s32[i:i + 1], case)
        led.add("d_weights", dw, w64[live], w32[live], case)
        # a ray without samples counts nowhere although it has a prior and obj = keep = 1
        none = ~has
        assert bool(P.has_prior(x["prior"])[none].all()) and not bool(d64["v"][none].any())
        assert stats[1].item() == float(d64["v"].sum())
        rows = torch.zeros(live.shape, dtype=F32); rows[live] = dw
        assert bool((rows[~d64["v"]] == 0).all())
        stats2, dw2, _ = run_packed(x, 0.7, 0.3)
        assert torch.equal(stats, stats2) and torch.equal(dw, dw2)
    led.report("dh_prior_loss_packed")
    assert kinds == set(P.KINDS)


def test_packed_cap_and_error_returns():
    from dynhor_amd import _lib
    L = _lib.lib()
    x = P.packed_inputs([5, 70, 3], 0)
    # max_samples caps a ray as the march's cap does: the second ray's samples past 64 are not read
    keep = x["live"].clone(); keep[:, 64:] = False
    stats, dw, _ = run_packed(x, 0.7, 0.0, max_samples=64)
    w_cap = torch.where(keep, x["w_pad"], torch.zeros_like(x["w_pad"]))
    d = P.depth_term(x["rays"], x["R"], x["mid_pad"], w_cap, x["prior"], P.DELTA, F64, x["cnt"] > 0)
    assert abs(stats[2].item() - d["abs"].item()) < 1e-5
    g = {k: v.to(DEV) for k, v in x.items() if torch.is_tensor(v)}
    st, ws = torch.empty(8, device=DEV), _ws(3)
    dwb = torch.empty(78, device=DEV)
    p = _lib.ptr
    null = None

    def packed(B=3, max_samples=1024, delta=0.02, dw=0.5, nw=0.0, rays=g["rays"], off=g["off"], ws_=ws):
        return L.dh_prior_loss_packed(p(rays) if rays is not None else null, p(g["R"]), p(g["t_start"]), p(g["weights"]), null, p(g["prior"]),
                                      B, p(off) if off is not None else null, p(g["cnt"]), max_samples, x["step"], dw, delta, nw, 0, p(st),
                                      p(dwb), null, p(ws_) if ws_ is not None else null, _lib.stream())

    def dense(B=3, n=5, delta=0.02, dw=0.5, nw=0.0, z=g["t_start"]):
        return L.dh_prior_loss(p(g["rays"]), p(g["R"]), p(z) if z is not None else null, p(g["weights"]), null, p(g["prior"]), B, n, 0.03, dw,
                               delta, nw, 0, p(st), p(dwb), null, p(ws), _lib.stream())
    assert packed() == 0 and dense() == 0
    assert packed(B=0) == 0 and dense(B=0) == 0, "B == 0 is a no-op"
    assert packed(max_samples=1025) == -2, "DH_ERR_UNSUPPORTED"
    for rc in (packed(B=-1), packed(max_samples=-1), packed(delta=0.0), packed(delta=float("nan")), packed(dw=-1.0), packed(dw=float("nan")),
               packed(nw=-0.5), packed(nw=float("nan")), packed(rays=None), packed(off=None), packed(ws_=None), dense(B=-1), dense(n=0),
               dense(delta=-1.0), dense(dw=float("nan")), dense(z=None)):
        assert rc == -1, "DH_ERR_BAD_ARG"
    torch.cuda.synchronize()


def _neus_inputs(B, seed, grey_every):
    x = P.dense_inputs(B, 8, seed, grey_every=grey_every)
    g = P._gen(seed + 100)
    x["color"] = torch.rand(B, 3, generator=g)
    x["wsum"] = 0.05 + 0.9 * torch.rand(B, generator=g)
    x["eik"] = torch.rand(B, 2, generator=g)
    return x


def _neus_loss(x, normal_w):
    B = x["rays"].shape[0]
    g = {k: v.to(DEV) for k, v in x.items() if torch.is_tensor(v)}
    stats, dc, dws, dn, ec = (torch.empty(s, device=DEV) for s in ((8,), (B, 3), (B,), (B, 3), (1,)))
    hip("dh_neus_loss", g["color"], g["wsum"], g["nmap"], g["eik"], g["rays"], g["R"], B, 0.1, 0.1, float(normal_w), stats, dc, dws, dn, ec)
    return stats.cpu(), dn.cpu()


@pytest.mark.parametrize("B", [5, 300, 1500])
def test_masked_normal_term_equals_the_loss_kernels_when_every_ray_has_a_normal(B):
    x = _neus_inputs(B, 3, grey_every=0)
    assert bool(P.has_normal(x["rays"]).all())
    ns, ndn = _neus_loss(x, 0.3)
    stats, _, dn = run_dense(x, 0.0, 0.3)
    rel = lambda a, b: (a.double() - b.double()).abs().max().item() / b.double().abs().max().item()
    print(f"B={B}: normal loss {stats[4].item():.7f} vs dh_neus_loss {ns[4].item():.7f}; d_nmap rel {rel(dn, ndn):.2e}")
    assert abs(stats[4].item() - ns[4].item()) <= 1e-6 * abs(ns[4].item())
    assert abs(stats[6].item() - 0.3 * ns[4].item()) <= 1e-6 * abs(0.3 * ns[4].item())
    assert stats[5].item() == float((x["rays"][:, 9] * x["rays"][:, 10]).sum())
    assert rel(dn, ndn) <= 1e-6


def test_masked_normal_term_skips_grey_pixels():
    B = 301
    x = _neus_inputs(B, 4, grey_every=2)
    has = P.has_normal(x["rays"])
    assert 0.4 < has.float().mean().item() < 0.6
    led = ErrorLedger()
    stats, _, dn = run_dense(x, 0.0, 0.3)
    n64, n32 = P.normal_term(x["rays"], x["R"], x["nmap"], F64), P.normal_term(x["rays"], x["R"], x["nmap"], F32)
    led.add("L_n", stats[4:5], n64["L"].view(1), n32["L"].view(1), "half grey")
    led.add("d_nmap", dn, P.normal_adjoint(x["rays"], x["R"], x["nmap"], 0.3, F64), P.normal_adjoint(x["rays"], x["R"], x["nmap"], 0.3, F32),
            "half grey")
    led.report("masked normal term, half the rays at grey 128")
    assert bool((dn[~has] == 0).all()), "rays without a normal get an exactly-zero adjoint"
    m = x["rays"][:, 9] * x["rays"][:, 10] > 0
    assert stats[5].item() == float((has & m).sum()), "the ray count is the number of normals"
    assert bool((dn[has & m].abs().sum(-1) > 0).all())
    # dh_neus_loss on the same rays pulls the grey ones too: that is what the mask removes
    ns, ndn = _neus_loss(x, 0.3)
    assert bool((ndn[~has & m].abs().sum(-1) > 0).all()) and abs(ns[4].item() - stats[4].item()) > 1e-3
    # stats are computed at weight 0 too, and d_normal_map is then left alone
    stats0, _, _ = run_dense(x, 0.0, 0.0)
    assert stats0[4].item() == stats[4].item() and stats0[6].item() == 0.0
