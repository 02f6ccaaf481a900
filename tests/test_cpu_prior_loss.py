"""CPU: what licenses tests/prior_loss_util.py as the reference of the depth / masked normal priors (dh_prior_loss), and the pieces of
the feature that need no GPU: the validity rule of the normal maps, the settings, the analytic depth maps of the synthetic scene."""
import pytest
import torch

from tests import prior_loss_util as P

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("B,n,seed", [(8, 5, 0), (37, 16, 3), (64, 128, 5)])
def test_restated_adjoints_equal_autograd(B, n, seed):
    x = P.dense_inputs(B, n, seed, grey_every=3)
    mid = P.midpoints(x["z"].double(), x["sample_dist"])
    mg = P.margins(x, mid, x["weights"])
    assert mg["inliers"] > 0 and mg["outliers"] > 0, "both Huber branches must occur"
    assert mg["delta"] > 0.1 and mg["zero"] > 0.1 and mg["prior"] > 1e-4 and mg["normal"] > 0.2, mg
    kinds = {P.KINDS[k] for k in x["kind"].tolist()}
    assert kinds == set(P.KINDS), "every kind of ray: inf, NaN, 0, negative, obj * keep = 0, all-zero weights, both branches"
    dw, nw = 0.7, 0.3
    w = x["weights"].double().requires_grad_(True)
    nm = x["nmap"].double().requires_grad_(True)
    d = P.depth_term(x["rays"], x["R"], mid, w, x["prior"], P.DELTA, F64)
    nr = P.normal_term(x["rays"], x["R"], nm, F64)
    (dw * d["L"] + nw * nr["L"]).backward()
    got_w = P.depth_adjoint(d, mid, dw, P.DELTA, F64).detach()
    got_n = P.normal_adjoint(x["rays"], x["R"], x["nmap"], nw, F64)
    assert torch.allclose(got_w, w.grad, rtol=1e-12, atol=1e-15)
    assert torch.allclose(got_n, nm.grad, rtol=1e-10, atol=1e-14)
    # rays that do not count carry exact zeros, and the counted ones are the valid kinds alone
    v = d["v"]
    assert bool((got_w[~v] == 0).all()) and bool((got_n[nr["q"] == 0] == 0).all())
    valid = torch.tensor([P.KINDS[k] in ("inlier", "outlier", "empty") for k in x["kind"].tolist()])
    assert torch.equal(v, valid)
    assert int(nr["rays"]) == int((P.has_normal(x["rays"]) & (x["rays"][:, 9] * x["rays"][:, 10] > 0)).sum())


def test_a_batch_without_a_valid_ray_scores_zero():
    x = P.dense_inputs(6, 4, 0)
    x["prior"][:] = float("inf")
    d = P.depth_term(x["rays"], x["R"], P.midpoints(x["z"].double(), x["sample_dist"]), x["weights"], x["prior"], P.DELTA, F64)
    assert d["L"].item() == 0.0 and d["rays"].item() == 0.0 and d["abs"].item() == 0.0


def test_quarter_rule_separates_grey_from_every_encoded_unit_normal():
    """Grey 128 decodes to a squared norm of 4.6e-5; a unit normal's bytes decode to at least (1 - sqrt(3)/255)^2 = 0.986: each
    component moves by at most 1/255 (half a byte step of 2/255), so the norm by at most sqrt(3)/255.  Dense sample of the sphere: a
    Fibonacci lattice of 200,000 points plus the axes, the diagonals and their neighbours."""
    n = 200_000
    i = torch.arange(n, dtype=F64) + 0.5
    phi = torch.pi * (1.0 + 5.0 ** 0.5) * i
    zc = 1.0 - 2.0 * i / n
    rad = (1.0 - zc * zc).sqrt()
    pts = torch.stack([rad * torch.cos(phi), rad * torch.sin(phi), zc], -1)
    special = torch.tensor([[sx * a, sy * b, sz * c] for a, b, c in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1),
                                                                  (1, 1e-3, 0), (1, 1, 1e-3))
                            for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], dtype=F64)
    pts = torch.cat([pts, torch.nn.functional.normalize(special, dim=-1)])
    dec = P.encode_normal(pts)
    n2 = (dec * dec).sum(-1)
    assert n2.min().item() >= (1.0 - 3.0 ** 0.5 / 255.0) ** 2 - 1e-6
    rays = torch.zeros(pts.shape[0] + 1, 14)
    rays[:-1, 11:14] = dec
    rays[-1, 11:14] = P.GREY
    has = P.has_normal(rays)
    assert bool(has[:-1].all()) and not bool(has[-1])
    assert abs((P.GREY * P.GREY).sum().item() - 4.6e-5) < 1e-6


def test_settings_parse_and_reject_unknown_keys():
    from dynhor_amd.runner import DEFAULT_CONF
    from dynhor_amd.settings import PRIOR_DEFAULTS, prior_settings
    assert PRIOR_DEFAULTS == {"depth_weight": 0.0, "depth_delta": 0.02, "depth_start_iter": 0, "normal_skip_missing": False}
    assert prior_settings(DEFAULT_CONF["train"]) == PRIOR_DEFAULTS
    assert prior_settings({"learning_rate": 1e-3}) == PRIOR_DEFAULTS          # a config written before the keys existed
    got = prior_settings({"depth_weight": 0.1, "depth_delta": 0.05, "depth_start_iter": 500, "normal_skip_missing": True})
    assert got == {"depth_weight": 0.1, "depth_delta": 0.05, "depth_start_iter": 500, "normal_skip_missing": True}
    for bad in ({"depth_wieght": 0.1}, {"normal_skip_mising": True}, {"depth_weight": -1.0}, {"depth_weight": float("nan")},
                {"depth_delta": 0.0}, {"depth_start_iter": -1}, {"depth_start_iter": 1.5}, {"normal_skip_missing": 1}):
        with pytest.raises(ValueError):
            prior_settings(bad)
    with pytest.raises(ValueError, match="depth_wieght"):
        prior_settings({"depth_wieght": 0.1})


def test_analytic_depth_maps_lie_on_the_surface_and_nowhere_else():
    """Every finite pixel: |scene_sdf(o + t d)| <= 1e-5 at the depth the map holds (fp32 storage of z: 2.5 x 6e-8 x 1 / c_z), and it is the
    FIRST zero (the SDF is positive on the ray before it).  inf exactly off the object: every pixel that is not labelled object, and of
    the labelled ones those whose ray misses the analytic surface (the fp32 labelling counts a ray that passes within 5e-4)."""
    from dynhor_amd.scene import make_depth_maps, make_sequence, scene_sdf
    frames = make_sequence(3, 48, 40, seed=11, device="cpu")
    depth = make_depth_maps(frames)
    F_, H, W = frames["label"].shape
    assert depth.shape == (F_, H, W) and depth.dtype == F32
    Kinv = torch.inverse(frames["K"].double())
    on_object = 0
    for f in range(F_):
        lab = frames["label"][f].reshape(-1)
        z = depth[f].reshape(-1).double()
        idx = torch.arange(H * W)
        pix = torch.stack([(idx % W).double(), (idx // W).double(), torch.ones(H * W, dtype=F64)], -1)
        dc = torch.nn.functional.normalize(pix @ Kinv.T, dim=-1)
        R, T = frames["R"][f].double(), frames["T"][f].double()
        d, o = dc @ R, (-(T @ R)).expand(H * W, 3)
        fin = torch.isfinite(z)
        assert bool((lab[fin] == 1).all()), "a depth off the object"
        t = z[fin] / dc[fin, 2]
        assert scene_sdf(o[fin] + d[fin] * t[:, None]).abs().max().item() <= 1e-5
        before = torch.linspace(0.0, 1.0, 400, dtype=F64)[None, :-1] * (t[:, None] - 1e-4)
        assert bool((scene_sdf(o[fin, None, :] + d[fin, None, :] * before[..., None]) > 0).all()), "not the first zero"
        miss = (lab == 1) & ~fin
        ts = torch.linspace(1.0, 4.0, 6001, dtype=F64)
        assert bool((scene_sdf(o[miss, None, :] + d[miss, None, :] * ts[None, :, None]) > 0).all()), "an object pixel without its depth"
        assert int(miss.sum()) <= 0.02 * int((lab == 1).sum()) + 2
        on_object += int(fin.sum())
    assert on_object > 100
