"""GPU: every forward through the network hooks takes the workspace (NeuSRenderer.net_state stamps it), so a backward whose saved tiles a
later forward has overwritten raises instead of computing on them -- also when that later forward is eval_points (vertex colours, surface
rendering), which used to write the workspace without a stamp."""
import pytest
import torch

from tests.test_gpu_render_forward import make_pair, make_rays

pytestmark = pytest.mark.gpu


def _renderer(family):
    if family == "neus":
        return make_pair(seed=5, n_samples=16, n_importance=16, up_sample_steps=2)[1]
    from tests.test_gpu_hash_family import make_hash_pair
    return make_hash_pair(seed=3)[1]


@pytest.mark.parametrize("family", ["neus", "hash"])
def test_eval_points_between_a_forward_and_its_backward_makes_the_backward_raise(family):
    ren = _renderer(family)
    B = 77                                            # 77 x 32 points: 38.5 tiles of 64
    o, d, near, far, t_rand = make_rays(B, seed=4)
    z = ren.sample_z(o, d, near, far, t_rand=t_rand)
    # adjoints of the size a training step's have (a mean over the rays, the eikonal term a mean over the points at weight 0.1): the hash
    # family's fixed-point table scatter answers NaN to contributions beyond its range
    adj = (torch.full((B, 3), 1.0 / B, device=o.device), torch.zeros(B, 1, device=o.device), None, None, None,
           torch.full((1,), 0.1 / (B * 32), device=o.device))
    s = ren._forward_core(o, d, z, 0.5, None, want_nmap=False)
    normals, colors = ren.eval_points(o[:50] * 0.2, d[:50], "test")
    assert normals.shape == colors.shape == (50, 3) and bool(torch.isfinite(colors).all())
    with pytest.raises(RuntimeError, match="workspace was overwritten"):
        ren._backward_core(s, *adj)
    s = ren._forward_core(o, d, z, 0.5, None, want_nmap=False)
    grad = ren._backward_core(s, *adj)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()) and grad.abs().max().item() > 0
    with pytest.raises(RuntimeError, match="infer_only"):
        ren._backward_core(ren._forward_core(o, d, z, 0.5, None, want_nmap=False, infer_only=True), *adj)
