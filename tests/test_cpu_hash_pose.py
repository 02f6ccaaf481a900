"""CPU: the rules of the hash family's pose-refinement adjoints (include/dynhor_hip.h dh_hash_geo_backward_rays,
dh_hash_color_backward_rays) restated in tests/hash_pose_util.py against autograd on oracle/hashgrid_oracle.py in fp64, and the share
of points the comparisons leave out."""
import torch

from oracle import hashgrid_oracle as HO
from tests import hash_pose_util as U


def _net64(seed=3, table_scale=0.3):
    net, col = HO.build_models(seed=seed, device="cpu", dtype=torch.float64)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    with torch.no_grad():
        net.encoding.table.copy_((torch.rand(net.encoding.table.shape, generator=g, dtype=torch.float64) * 2 - 1) * table_scale)
        net.lin0.weight_v.add_(0.02 * torch.randn(net.lin0.weight_v.shape, generator=g, dtype=torch.float64))      # encoding columns matter
    return net, col


def test_point_adjoint_rule_equals_autograd_on_the_oracle():
    net, _ = _net64()
    x, share = U.unmarked_points(96, seed=5)
    assert share <= U.MAX_MARKED
    d_sdf, d_feat, d_grad = U.geo_cotangents(96, seed=6)
    ref = U.oracle_point_adjoint(net, x, d_sdf, d_feat, d_grad)
    got = U.point_adjoint_rule(net, x, d_sdf, d_feat, d_grad)
    rel, worst = U.two_errors(got, ref)
    print(f"point-adjoint rule vs fp64 autograd: rel {rel:.2e}, worst point {worst:.2e}")
    assert ref.norm().item() > 0 and rel < 1e-10 and worst < 1e-10


def test_sh_gradient_rule_equals_autograd_on_the_oracle():
    g = torch.Generator(device="cpu").manual_seed(2)
    d = (torch.randn(257, 3, generator=g, dtype=torch.float64) * 1.3).requires_grad_(True)      # not normalised: plain polynomials
    dy = torch.randn(257, 16, generator=g, dtype=torch.float64)
    ref = torch.autograd.grad((HO.sh4(d) * dy).sum(), d)[0]
    got = U.sh4_grad_rule(d.detach(), dy)
    assert (got - ref).abs().max().item() < 1e-12 * ref.abs().max().item()


def test_marked_share_of_the_test_point_sets_is_below_the_cap():
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(100000, 3, generator=g)
    x = (x / x.norm(dim=1, keepdim=True) * torch.rand(100000, 1, generator=g) ** (1 / 3) * 0.9).float()
    share = U.ambiguous(x).float().mean().item()
    print(f"marked share of 100,000 points uniform in the ball of radius 0.9: {share:.4f}")
    assert 0.02 < share <= U.MAX_MARKED
    for n in (1, 255, 257, 4099):
        pts, s = U.unmarked_points(n, seed=n)
        assert pts.shape == (n, 3) and s <= U.MAX_MARKED and not U.ambiguous(pts).any()
    # a point on a cell face of level 0 (pos = x01 * 15 + 0.5 integral) is marked, also when only a shifted evaluation lands there
    on_face = torch.tensor([[(2.5 / 15) * 2 - 1, 0.123, -0.456]])
    assert U.ambiguous(on_face).all() and U.ambiguous(on_face + torch.tensor([[1e-3, 0.0, 0.0]])).all()
