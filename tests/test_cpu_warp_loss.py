"""CPU: what licenses tests/warp_loss_util.py as the reference of the multi-view photometric term (dh_warp_loss, DESIGN_NEXT_ROWS.md
section 30) -- its fp64 autograd gradient equals central differences of itself -- the term's behaviour on the analytic scene, the settings
and the source-level no-host-read guard of the new step code."""
import inspect
import re

import pytest
import torch

from tests import mvs_util as VU
from tests import warp_loss_util as U

F64 = torch.float64


def _args(c, nbr, frame, pix, z, w, n, st):
    return (c["gray"], c["valid"], c["R"], c["T"], c["K"], c["Kinv"], nbr, frame, pix, z, w, n, st)


def test_fp64_autograd_equals_central_differences():
    """On rays whose taps all lie at least 0.05 px from a cell boundary, so that the differences see one smooth piece: d l / d z and
    d l / d n by autograd against central differences with steps that move a tap by about 0.01 px (the cells and the choice stay fixed)."""
    c = U.plane_case(48, 64, 5, seed=0)
    nbr = torch.from_numpy(VU.kernel_nbr(5, 2))
    st = U.settings(patch=2, topk=2, min_views=1)
    pix, z, w, n = U.random_rays(c, 2, 300, seed=5, margin=3)
    r64, r32 = U.both_forms(*_args(c, nbr, 2, pix, z, w, n, st))
    sel = (r64["counts"] & (r64["margin"] > 0.05) & ~r64["amb"] & (r64["valid_n"] == 2)).nonzero()[:, 0][:12]
    assert sel.numel() >= 6, sel.numel()
    pix, z, w, n = pix[sel], z[sel], w[sel], n[sel]
    r32 = U.warp_eval(*_args(c, nbr, 2, pix, z, w, n, st), dtype=torch.float32)
    cells = r32["cells"]
    base = U.warp_eval(*_args(c, nbr, 2, pix, z, w, n, st), dtype=F64, cells=cells)
    assert bool(base["counts"].all())
    f = lambda zz, nn_: U.warp_rule(*_args(c, nbr, 2, pix, zz, w, nn_, st), dtype=F64, cells=cells)["l"]
    z64, n64 = z.double(), n.double()
    hz, hn = 2e-5, 2e-5
    fd_z = (f(z64 + hz, n64) - f(z64 - hz, n64)) / (2 * hz)
    err_z = float((fd_z - base["g_z"]).abs().max() / base["g_z"].abs().max())
    errs_n = []
    for k in range(3):
        d = torch.zeros(3, dtype=F64)
        d[k] = hn
        fd = (f(z64, n64 + d) - f(z64, n64 - d)) / (2 * hn)
        errs_n.append(float((fd - base["g_n"][:, k]).abs().max() / base["g_n"].abs().max()))
    print(f"autograd vs central differences: d/dz rel {err_z:.2e}, d/dn rel {max(errs_n):.2e} over {sel.numel()} rays; "
          f"|g_z| max {float(base['g_z'].abs().max()):.3g}, |g_n| max {float(base['g_n'].abs().max()):.3g}")
    # central differences of a smooth function: truncation h^2 f''' / 6 and rounding 1e-16 / h, both far below 1e-5 relative here
    assert err_z < 1e-5 and max(errs_n) < 1e-5
    # g_n is orthogonal to n: the rule does not see the normal's length
    assert float((base["g_n"] * n64).sum(1).abs().max()) < 1e-12 * float(base["g_n"].abs().max() + 1)


def _analytic_scene():
    from dynhor_amd import scene
    fr = scene.make_sequence(n_frames=6, H=96, W=96, seed=4321, device="cpu", hand=True)
    depth = scene.make_depth_maps(fr)
    rgb = fr["rgb"].double()
    gray = torch.floor(0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2] + 0.5).clamp(0, 255).to(torch.uint8)
    obj = (fr["label"] == 1).float()[:, None]
    valid = (-torch.nn.functional.max_pool2d(-obj, 3, 1, 1))[:, 0].to(torch.uint8)       # eroded by one pixel
    gray = torch.where(valid != 0, gray, torch.zeros_like(gray))
    K = fr["K"].float()
    Kinv = torch.inverse(K.double()).float()
    return fr, depth, gray, valid, K.reshape(9), Kinv.reshape(9)


def test_true_surface_scores_higher_than_a_moved_one():
    """On the analytic scene's true depth and normal the median chosen score is high; moving z by +-0.02 lowers it.  Every frame is a
    source in turn and the rays are pooled.  The module's defaults, but for two settings the scene forces: its six cameras stand 60
    degrees apart, so a ray rarely has more than one usable neighbour (min_views 1), and the object is some 32 px wide, so a 7 x 7 patch
    (P 3) is the largest that the eroded mask and the hand leave more than a hundred rays for.  Recorded (CPU, fp64 restatement):
    true 0.9772 (125 rays), z - 0.02 0.9220 (78), z + 0.02 0.9590 (210).  Only the ordering is asserted."""
    from dynhor_amd import scene
    from dynhor_amd.mvs import neighbours
    fr, depth, gray, valid, K, Kinv = _analytic_scene()
    P = 3
    st = U.settings(patch=P, topk=4, min_views=1)
    nbr = neighbours(6, (1, 2))
    R, T = fr["R"].float(), fr["T"].float()
    scores = {0.0: [], -0.02: [], 0.02: []}
    for frame in range(6):
        ok = torch.isfinite(depth[frame]) & (valid[frame] != 0)
        py, px = ok.nonzero(as_tuple=True)
        z = depth[frame][py, px].float()
        p = torch.stack([px.double(), py.double(), torch.ones_like(px, dtype=F64)], 1)
        Xc = z.double()[:, None] * (p @ Kinv.double().reshape(3, 3).T)
        Xo = (Xc - T[frame].double()) @ R[frame].double()                                 # R^T (Xc - T)
        n = scene._normal(Xo).float()
        pix = torch.stack([px, py], 1).int()
        for dz in scores:
            r = U.warp_eval(gray, valid, R, T, K, Kinv, nbr, frame, pix, z + dz, torch.ones(px.numel()), n, st, dtype=F64, grad=False)
            scores[dz].append(r["score"][r["counts"]])
    med = {}
    for dz, v in scores.items():
        v = torch.cat(v)
        assert v.numel() >= 40, (dz, v.numel())
        med[dz] = (float(v.median()), v.numel())
    print(f"median chosen score on the analytic scene (6 frames of 96 x 96, P {P}): true {med[0.0][0]:.4f} ({med[0.0][1]} rays), "
          f"z - 0.02 {med[-0.02][0]:.4f} ({med[-0.02][1]}), z + 0.02 {med[0.02][0]:.4f} ({med[0.02][1]})")
    assert med[0.0][0] > med[-0.02][0] and med[0.0][0] > med[0.02][0]


def test_warp_settings_accepts_and_rejects():
    from dynhor_amd.settings import prior_settings, warp_settings
    from dynhor_amd.warp_loss import DEFAULTS, check_settings
    s = warp_settings({"learning_rate": 1e-3, "depth_weight": 0.1})
    assert s["weight"] == 0.0 and s["patch"] == 5 and s["offsets"] == (1, 2, 4, 8) and s["topk"] == 4 and s["min_views"] == 2
    assert s["min_cos"] == 0.1 and s["min_wsum"] == 0.5 and s["sigma"] == 1.0 and s["a_min"] == 0.5 and s["erode_px"] == 1 and s["start_iter"] == 0
    s = warp_settings({"warp_weight": 0.5, "warp_patch": 3, "warp_offsets": [1, 3], "warp_start_iter": 100})
    assert s["weight"] == 0.5 and s["patch"] == 3 and s["offsets"] == (1, 3) and s["start_iter"] == 100
    for bad in ({"warp_wieght": 0.1}, {"warp_weight": -1.0}, {"warp_weight": float("nan")}, {"warp_patch": 8}, {"warp_patch": 0},
                {"warp_topk": 9}, {"warp_min_views": 0}, {"warp_offsets": [1, 2, 3, 4, 5]}, {"warp_offsets": [0]}, {"warp_min_cos": 2.0},
                {"warp_min_wsum": float("nan")}, {"warp_weight": True}):
        with pytest.raises(ValueError):
            warp_settings(bad)
    with pytest.raises(ValueError, match="unknown"):
        check_settings({"patchh": 3})
    # the two blocks do not look at each other's keys
    assert prior_settings({"warp_weight": 0.5, "warp_patch": 3})["depth_weight"] == 0.0
    assert set(DEFAULTS) >= {"patch", "offsets", "topk", "min_views", "min_cos", "min_wsum", "sigma", "a_min", "erode_px", "start_iter"}


def test_neighbour_table_drops_held_out_frames():
    from dynhor_amd.warp_loss import neighbour_table
    nbr = neighbour_table(10, [f for f in range(10) if f % 4 != 0], (1, 2))
    assert nbr.shape == (10, 4) and nbr.dtype == torch.int32
    assert not any(int(v) in (0, 4, 8) for v in nbr.reshape(-1))
    assert nbr[5].tolist() == [-1, 6, 3, 7] and nbr[0].tolist() == [-1, 1, -1, 2]


def test_the_step_source_reads_nothing_back():
    """The source-level guard of tests/test_cpu_no_host_sync.py for what a step with the term runs."""
    from dynhor_amd import warp_loss
    from tests.test_cpu_no_host_sync import FORBIDDEN
    for fn in (warp_loss.ray_depth, warp_loss.warp_loss, warp_loss.ray_depth_bwd, warp_loss.warp_term, warp_loss.step_input):
        src = re.sub(r'"""[\s\S]*?"""', "", inspect.getsource(fn))
        src = "\n".join(ln.split("#")[0] for ln in src.splitlines())
        for pat in FORBIDDEN:
            assert not re.search(pat, src), f"{fn.__qualname__} contains {pat}"
