"""CPU: tests/ray_kernels_util.py licensed before the GPU tests rely on it (tests/test_gpu_ray_sampling.py, test_gpu_ray_scan.py,
test_gpu_loss_adam.py).  Nothing here touches a kernel: the criteria are shown to accept the oracle's own result and to reject a
result that is wrong in the way a kernel would be wrong, and the input builders are shown to keep every branched-on quantity off
its switch by the stated margin, with both sides of every switch populated -- on exactly the inputs the GPU tests use."""
import pytest
import torch

from tests import ray_kernels_util as U

F32, F64 = U.F32, U.F64


# ------------------------------------------------------------------------------------------------ canary
def test_canary_sees_missing_and_out_of_range_writes():
    c = U.Canary("cpu")
    a, b = c.out("a", 5, 3), c.out("b", 7)
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all())
    a.fill_(1.0); b.fill_(2.0)
    c.check()
    with pytest.raises(AssertionError, match="must stay untouched"):
        c.check(untouched=("b",))
    b[3] = torch.tensor([U.CANARY_BITS], dtype=torch.int32).view(F32)[0]          # one word never written
    with pytest.raises(AssertionError, match="1 of 7 output words were never written"):
        c.check()
    b.fill_(2.0)
    raw = c.items[1][1]
    raw[U.PAD + 7] = 0                                                            # the first word behind the payload
    with pytest.raises(AssertionError, match="outside the buffer"):
        c.check()
    raw[U.PAD + 7] = U.CANARY_BITS
    raw[U.PAD - 1] = 0                                                            # the last word before it
    with pytest.raises(AssertionError, match="outside the buffer"):
        c.check()
    c2 = U.Canary("cpu")
    p = c2.inout("p", torch.arange(6.0))
    assert torch.equal(p, torch.arange(6.0))
    c2.check()                                                                    # an in-place buffer: only the pads are watched
    c3 = U.Canary("cpu")
    c3.out("never", 4)
    c3.check(untouched=("never",))


# ------------------------------------------------------------------------------------------------ up-sampling
def _fp64_sampler(o, d, z, sdf, k, inv_s):
    return U.oracle_upsample(o, d, z, sdf, k, inv_s, F64)[0], None


def test_upsample_criteria_accept_the_fp64_oracle_on_every_case_and_the_cap_holds():
    """Every case of the GPU test: the radius margin, tol < 0.25 / n_new on the reference alone, and the fp64 oracle passing range,
    order, CDF space and z space.  All four families occur in every case."""
    worst = {}
    for case in U.upsample_cases():
        B, n, k, inv_s, seeds = case
        fams = set()
        for seed in seeds:
            fams |= set(U.upsample_inputs(B, n, seed)[4].tolist())
        assert fams == {0, 1, 2, 3}, case
        m = U.check_upsample_case(case, _fp64_sampler)
        assert m["res"] < 1e-9 and m["dz"] == 0.0
        worst[k] = max(worst.get(k, 0.0), m["tol"] / m["cap"])
    print("largest tol / cap per n_new (fp32 oracle residual x 4 against 0.25 / n_new):", {k: f"{v:.3f}" for k, v in worst.items()})
    assert len(U.upsample_cases()) == 9 * 4 * 4 + 3 * 9


def test_upsample_families_are_what_they_say():
    o, d, z, sdf, fam = U.upsample_inputs(257, 64, 0)
    assert bool((z[:, 1:] > z[:, :-1]).all())
    assert bool((sdf[fam == 2] > 0).all()), "rays that miss: all sdf > 0"
    assert bool((sdf[fam == 0].min(-1)[0] < 0).all()) and bool((sdf[fam == 1].min(-1)[0] < 0).any())
    # thin slab: most sections of the ray are empty
    assert ((sdf[fam == 1] < 0).sum(-1).float().mean().item()) < 6
    # opaque in its first section: the fp64 oracle at inv_s = 512 puts most of the new samples into section 0, and the second slope
    # is steeper than the first (so that lane 0's "previous cosine = 0" matters)
    f3 = fam == 3
    zn, cdf = U.oracle_upsample(o, d, z, sdf, 16, 512.0, F64)
    assert bool((cdf[f3][:, 1] > 0.7).all()) and bool((zn[f3][:, :11] <= z[f3][:, 1:2].double()).all())
    c0 = (sdf[f3, 1] - sdf[f3, 0]) / (z[f3, 1] - z[f3, 0]); c1 = (sdf[f3, 2] - sdf[f3, 1]) / (z[f3, 2] - z[f3, 1])
    assert bool((c1 < c0).all()) and bool((c0 < 0).all())
    r = U.radius64(o, d, z)
    assert bool((r < 1).any()) and bool((r > 1).any()), "both sides of the unit sphere"
    assert bool((r[f3][:, :2] < 1).all())


def test_upsample_criteria_reject_a_sample_in_the_neighbouring_populated_section():
    case = (257, 64, 16, 64.0, (0,))

    def moved(o, d, z, sdf, k, inv_s):
        zn = U.oracle_upsample(o, d, z, sdf, k, inv_s, F64)[0].clone()
        zn[8, 5] = zn[8, 6]                      # ray 8 (bumpy sphere), sample 5 sits where sample 6 belongs: still ordered
        return zn, None
    with pytest.raises(AssertionError, match="CDF-space residual"):
        U.check_upsample_case(case, moved)

    def one_ulp_back(o, d, z, sdf, k, inv_s):
        zn = U.oracle_upsample(o, d, z, sdf, k, inv_s, F64)[0].to(F32)
        zn[8, 6] = torch.nextafter(zn[8, 5], torch.tensor(0.0))
        return zn, None
    with pytest.raises(AssertionError, match="not ascending"):
        U.check_upsample_case(case, one_ulp_back)

    def outside(o, d, z, sdf, k, inv_s):
        zn = U.oracle_upsample(o, d, z, sdf, k, inv_s, F64)[0].to(F32)
        zn[3, -1] = torch.nextafter(z[3, -1], torch.tensor(9.0))
        return zn, None
    with pytest.raises(AssertionError, match="outside"):
        U.check_upsample_case(case, outside)

    def fp32(o, d, z, sdf, k, inv_s):            # the fp32 oracle is, by construction, within the bounds derived from it
        zn = U.oracle_upsample(o, d, z, sdf, k, inv_s, F32)[0]
        return zn, (o[:, None, :] + d[:, None, :] * zn[..., None]).reshape(-1, 3)
    U.check_upsample_case(case, fp32)

    def bad_points(o, d, z, sdf, k, inv_s):
        zn, pts = fp32(o, d, z, sdf, k, inv_s)
        pts = pts.clone(); pts[7, 1] += 4e-6
        return zn, pts
    with pytest.raises(AssertionError, match="pts_new"):
        U.check_upsample_case(case, bad_points)


# ------------------------------------------------------------------------------------------------ merge
def test_merge_reference_and_swapped_ties():
    z, zn, s, sn = U.merge_inputs(5, 64, 16, "ties")
    zz, ss = U.merge_reference(z, zn, s, sn)
    assert bool((zz[:, 1:] >= zz[:, :-1]).all())
    cross = (z[:, :, None] == zn[:, None, :]).any()
    assert bool(cross) and bool((z[:, 1:] == z[:, :-1]).any()) and bool((zn[:, 1:] == zn[:, :-1]).any())
    # stable: among equal depths the old samples come first, each list in its own order
    b = 0
    v = zn[b, 0]
    where = (zz[b] == v).nonzero().reshape(-1)
    n_old = int((z[b] == v).sum())
    assert torch.equal(ss[b, where[:n_old]], s[b][z[b] == v]) and torch.equal(ss[b, where[n_old:]], sn[b][zn[b] == v])
    # two swapped ties: the depths still agree, the gathered sdf does not
    i = int(where[0]); assert zz[b, i] == zz[b, i + 1]
    bad = ss.clone(); bad[b, i], bad[b, i + 1] = ss[b, i + 1], ss[b, i]
    assert ss[b, i] != ss[b, i + 1], "tied depths carry distinguishable sdf values, or a swap could not be seen"
    assert U.merge_matches(zz, ss, zz, ss) and U.merge_matches(zz, None, zz, ss)
    assert not U.merge_matches(zz, bad, zz, ss), "the criterion of the GPU test rejects two swapped ties"
    for mode, first in (("before", "new"), ("after", "old")):
        z, zn, s, sn = U.merge_inputs(3, 65, 16, mode)
        zz, ss = U.merge_reference(z, zn, s, sn)
        assert torch.equal(zz, torch.cat([zn, z] if first == "new" else [z, zn], -1))


# ------------------------------------------------------------------------------------------------ coarse samples / mid-points
def test_coarse_and_midpoint_references():
    o, d, near, far, t = U.coarse_inputs(5)
    z = U.coarse_reference(o, d, near, far, t, 8)
    lin = torch.arange(8, dtype=F64) / 7
    want = near.double()[:, None] + (far.double() - near.double())[:, None] * lin[None, :] + (t.double()[:, None] - 0.5) * 2.0 / 8
    assert (z - want).abs().max().item() < 1e-14 and z.abs().max().item() < 4.0
    assert torch.equal(U.coarse_reference(o, d, near, far, None, 1), near.double()[:, None])
    z32 = z.to(F32)
    p = U.midpoints_reference(o, d, z32, 0.25)
    mid = torch.cat([0.5 * (z32[:, 1:].double() + z32[:, :-1].double()), z32[:, -1:].double() + 0.125], -1)
    assert (p.view(5, 8, 3) - (o.double()[:, None] + d.double()[:, None] * mid[..., None])).abs().max().item() < 1e-14
    p0 = U.midpoints_reference(o, d, z32, 0.0)
    assert (p0 - p).view(5, 8, 3)[:, -1].abs().max().item() > 0.05, "the last section uses sample_dist"


# ------------------------------------------------------------------------------------------------ dense scan
@pytest.mark.parametrize("n", U.SCAN_N)
def test_scan_builder_margins_and_both_sides_of_every_switch(n):
    total, zeros = {}, 0
    for B in U.SCAN_B:
        for seed in U.scan_seeds(B):
            x = U.scan_inputs(B, n, seed)
            for car in U.SCAN_CAR:
                mg = U.scan_margins(x, car)
                U.assert_scan_margins(mg, (n, B, seed, car))
                U.add_sides(total, mg["sides"])
            zeros += mg["zero_normals"]
    missing = [k for k in U.scan_required_sides(n) if total.get(k, 0) == 0]
    assert not missing and zeros > 0, (missing, zeros)
    # the largest batch populates every side on its own
    big = U.scan_margins(U.scan_inputs(130, n, 0), 0.37)
    assert all(big["sides"][k] > 0 for k in U.scan_required_sides(n))


def test_scan_reference_conventions_and_ledger():
    B, n = 5, 64
    x = U.scan_inputs(B, n, 0)
    cot = U.scan_cotangents(B, n, 0)
    bg = torch.tensor([0.2, 0.5, 0.9])
    f64, g64 = U.scan_reference(x, 0.37, bg, cot, U.COT_OPTIONAL, F64)
    f32, g32 = U.scan_reference(x, 0.37, bg, cot, U.COT_OPTIONAL, F32)
    for g in g64.values():
        assert bool(torch.isfinite(g).all())
    zero = (x["normals"] == 0).all(-1)
    assert int(zero.sum()) > 0
    # a zero normal: no eikonal gradient (the kernel's nn > 0 guard) and a finite one everywhere else
    cot0 = dict(cot, ec=torch.zeros(1))
    g_noeik = U.scan_reference(x, 0.37, bg, cot0, U.COT_OPTIONAL, F64)[1]["d_normals"]
    assert torch.equal(g_noeik[zero], g64["d_normals"][zero]) and (g_noeik[~zero] - g64["d_normals"][~zero]).abs().max().item() > 1e-3
    # a clipped sample (alpha_raw < 0) carries no weight and no gradient
    mg = U.scan_margins(x, 0.37)
    assert mg["sides"]["alpha_raw<0"] > 0
    assert int((f64["weights"] == 0).sum()) == mg["sides"]["alpha_raw<0"]
    assert bool((g64["d_sdf"][f64["weights"].reshape(-1) == 0] == 0).all())
    # the mid-points the oracle evaluated are the ones scan_margins measured
    pn = f64["pts"].norm(dim=-1).view(B, n)
    assert torch.equal((pn < 1.0).double(), f64["inside"])
    # the ledger: the oracle's own results pass; a relative 1e-3 error in a few elements does not
    led = U.ErrorLedger()
    for k in ("weights", "color", "wsum", "wmax", "cdf", "eik", "nmap"):
        led.add(k, f32[k], f64[k], f32[k])
        led.add(k, f64[k], f64[k], f32[k])
    for k in g64:
        led.add(k, g32[k].reshape(g64[k].shape), g64[k], g32[k].reshape(g64[k].shape))
    bad = g32["d_sdf"].clone(); bad[::7] *= 1.001
    with pytest.raises(AssertionError, match="d_sdf"):
        led.add("d_sdf", bad, g64["d_sdf"], g32["d_sdf"])
    # each optional cotangent changes the reference: none of the six configurations is a duplicate of another
    seen = []
    for use in U.COT_CONFIGS:
        gr = U.scan_reference(x, 0.37, bg, cot, use, F64)[1]
        seen.append(torch.cat([gr["d_sdf"], gr["d_normals"].reshape(-1)]))
    for i in range(len(seen)):
        for j in range(i):
            assert (seen[i] - seen[j]).abs().max().item() > 1e-3


# ------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("B", (1, 2, 1023, 1024, 1025, 2048, 5000))
def test_loss_inputs_populate_every_branch(B):
    sides = {}
    for mode in ("hand", "background", "mixed"):
        for seed in range(10 if B <= 2 else 1):
            x = U.loss_inputs(B, mode, seed)
            assert U.loss_margin(x) >= U.LOSS_CLIP_MARGIN
            ws = x["wsum"].double()
            e = x["color"] - x["rays"][:, 6:9]
            for k, v in (("ws below", ws < 1e-3), ("ws inside", (ws > 1e-3) & (ws < 1 - 1e-3)), ("ws above", ws > 1 - 1e-3),
                         ("e == 0", e == 0), ("e > 0", e > 0), ("e < 0", e < 0), ("zero nmap row", (x["nmap"] == 0).all(-1)),
                         ("object", x["rays"][:, 9] * x["rays"][:, 10] > 0), ("hand", x["rays"][:, 10] == 0),
                         ("background", (x["rays"][:, 9] == 0) & (x["rays"][:, 10] > 0))):
                sides[k] = sides.get(k, 0) + int(v.sum())
            ref = U.loss_reference(x, 0.1, 0.1, 0.05)
            assert bool(torch.isfinite(ref["d_color"]).all()) and bool(torch.isfinite(ref["d_wsum"]).all()) and bool(torch.isfinite(ref["d_nmap"]).all())
            assert bool(torch.isfinite(ref["stats"][:5]).all())
            gate = ((ws >= 1e-3) & (ws <= 1 - 1e-3))
            assert bool((ref["d_wsum"][~gate] == 0).all()), "the clipped BCE passes no gradient outside the clip"
            assert bool((ref["d_color"][e == 0] == 0).all())
    need = ["ws below", "ws inside", "ws above", "e == 0", "object", "hand", "background"] + (["zero nmap row", "e > 0", "e < 0"] if B > 2 else [])
    assert all(sides[k] > 0 for k in need), sides


# ------------------------------------------------------------------------------------------------ Adam
def test_adam_reference_is_torch_adam():
    g = torch.Generator().manual_seed(3)
    n = 1000
    p0 = torch.randn(n, generator=g)
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([p], lr=float(torch.tensor(1e-3, dtype=F32)), betas=(float(torch.tensor(0.9, dtype=F32)), float(torch.tensor(0.999, dtype=F32))),
                           eps=float(torch.tensor(1e-8, dtype=F32)))
    q, m, v = p0.double().clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in range(1, 6):
        grad = torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 3, (n,), generator=g).float()
        p.grad = grad.double() * float(torch.tensor(1.0 / 3.0, dtype=F32))
        opt.step()
        q, m, v, upd, scale = U.adam_reference(q, grad, m, v, 1e-3, 0.9, 0.999, 1e-8, step, 1.0 / 3.0)
        assert (p.detach() - q).abs().max().item() < 1e-15
        assert bool((scale >= upd.abs() * (1 - 1e-12)).all())
    q2 = U.adam_reference(q, torch.zeros(n), torch.zeros(n), torch.zeros(n), 1e-3, 0.9, 0.999, 1e-8, 7, 1.0)[0]
    assert torch.equal(q2, q), "zero gradient and zero moments: the eps path leaves the parameter alone"
