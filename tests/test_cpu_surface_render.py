"""CPU: the sphere tracer's restatement (tests/trace_util.py) against closed forms and against a dense first-crossing check on the
analytic scene, interpolate_pose, and the argument validation of dynhor_amd/surface_render.py and of the CLI's --mode / --views.
The HIP kernels themselves are compared with the restatement in tests/test_gpu_surface_render.py."""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import trace_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 96


def _sphere(r):
    return lambda p: p.norm(dim=-1) - r


def test_restatement_hits_a_sphere_at_the_closed_form_depth():
    R, T, K = U.reference_camera(H=H, W=W)
    a = U.trace_ref(_sphere(0.5), R, T, K, H, W)
    o = a["o"].repeat_interleave(a["rays_per_view"], dim=0)
    assert not bool((a["flags"] & U.INSIDE).any())
    hits, left, worst = U.check_sphere_depth(o, a["d"], a["t"], a["state"], 0.5, U.PARAMS["eps"])
    in_sphere = a["disc"] > 0
    print(f"sphere: {hits} hits, {left} grazing rays left out, worst depth error {worst:.3f} of eps / cos; "
          f"{float((a['nq'] + a['scan_q'])[in_sphere].double().mean()):.1f} queries per ray in the unit sphere")
    assert hits > 500 and set(a["state"].tolist()) <= {U.HIT, U.MISS}


@pytest.mark.parametrize("scale", [1.0, 2.75])
def test_restatement_loses_no_crossing_of_the_analytic_scene(scale):
    from dynhor_amd.scene import scene_sdf
    f = lambda p: scale * scene_sdf(p)
    R, T, K = U.reference_camera(H=H, W=W)
    a = U.trace_ref(f, R, T, K, H, W)
    ins = a["disc"] > 0
    o = a["o"].repeat_interleave(a["rays_per_view"], dim=0)
    missed, earlier = U.dense_check(f, o[ins], a["d"][ins], a["near"][ins].clamp(min=0.0), a["far"][ins], a["state"][ins], a["t"][ins])
    q = (a["nq"] + a["scan_q"])[ins].double()
    print(f"scene x {scale}: {int((a['state'] == U.HIT).sum())} hits of {int(ins.sum())} rays in the sphere, {q.mean():.1f} queries per ray "
          f"(max {int(q.max())}), {int((a['flags'] & U.SCANNED != 0).sum())} scanned, {int((a['flags'] & U.CAPPED != 0).sum())} capped; "
          f"missed {int(missed.sum())}, earlier {int(earlier.sum())}")
    assert int((a["state"] == U.HIT).sum()) > 500
    assert int(missed.sum()) == 0 and int(earlier.sum()) == 0
    hit = a["state"] == U.HIT
    s = f(U.points(a, hit.nonzero().reshape(-1)))
    capped = (a["flags"][hit] & U.CAPPED) != 0
    assert bool(((s.abs() <= scale * U.PARAMS["eps"] * (1 + 1e-9)) | capped).all())


def test_interpolate_pose():
    from dynhor_amd.scene import look_at_pose
    from dynhor_amd.surface_render import interpolate_pose
    R0, T0 = look_at_pose(torch.tensor([2.0, 0.9, 0.7], dtype=torch.float64))
    R1, T1 = look_at_pose(torch.tensor([-0.4, 2.1, -0.8], dtype=torch.float64))
    Ra, Ta = interpolate_pose(R0, T0, R1, T1, 0.0)
    Rb, Tb = interpolate_pose(R0, T0, R1, T1, 1.0)
    assert torch.equal(Ra, R0) and torch.equal(Ta, T0) and torch.equal(Rb, R1) and torch.equal(Tb, T1)
    Rm, Tm = interpolate_pose(R0, T0, R1, T1, 0.5)
    assert float((Rm @ Rm.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12 and abs(float(torch.linalg.det(Rm)) - 1.0) < 1e-12
    ang = lambda A, B: math.acos(max(-1.0, min(1.0, (float(torch.trace(A.T @ B)) - 1.0) / 2.0)))
    full = ang(R0, R1)
    assert full > 1.0
    assert abs(ang(R0, Rm) - 0.5 * full) < 1e-9 and abs(ang(Rm, R1) - 0.5 * full) < 1e-9
    assert torch.allclose(Tm, 0.5 * (T0 + T1), rtol=0, atol=1e-15)
    # fp32 inputs (the dataset's poses) are taken as they are
    Rf, _ = interpolate_pose(R0.float(), T0.float(), R1.float(), T1.float(), 0.0)
    assert torch.equal(Rf, R0.float().double())
    # identical rotations: no axis to turn about
    Rs, _ = interpolate_pose(R0, T0, R0, T1, 0.3)
    assert torch.equal(Rs, R0)


def test_public_functions_validate_their_arguments():
    from dynhor_amd import surface_render as sr
    R, T, K = U.reference_camera()
    f = _sphere(0.5)
    with pytest.raises(TypeError):
        sr.trace(None, R, T, K, 8, 8)
    with pytest.raises(TypeError):
        sr.trace(f, R.numpy(), T, K, 8, 8)
    for bad in (dict(H=0), dict(W=-1), dict(level=0), dict(level=1.5), dict(bound=0.0), dict(eps=-1e-4), dict(relax=float("nan")),
                dict(min_step=0.2, max_step=0.1), dict(refine_steps=0), dict(refine_steps=256), dict(max_steps=0), dict(scan_step=0),
                dict(compact_every=0), dict(compact_every=True)):
        kw = dict(H=8, W=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            sr.trace(f, R, T, K, **kw)
    with pytest.raises(ValueError):
        sr.trace(f, R[0, :2], T, K, 8, 8)
    with pytest.raises(ValueError):
        sr.trace(f, R, T[:, :2], K, 8, 8)
    with pytest.raises(ValueError):
        sr.trace(f, R, T, K[:2], 8, 8)
    with pytest.raises(ValueError):
        sr.trace(f, R * float("nan"), T, K, 8, 8)
    with pytest.raises(ValueError, match="GPU"):
        sr.trace(f, R, T, K, 8, 8)                      # host tensors: the tracer runs on the device only (no CPU fallback)
    with pytest.raises(ValueError):
        sr.volume_rays(R, T, K, 8, 0)
    with pytest.raises(ValueError, match="GPU"):
        sr.volume_rays(R, T, K, 8, 8)
    with pytest.raises(ValueError):
        sr.render_surface(None, R, T, K, 8, 8, background="green")
    with pytest.raises(ValueError):
        sr.render_surface(None, R, T, K, 8, 8, level=0)
    with pytest.raises(ValueError, match="GPU"):
        sr.render_surface(None, R, T, K, 8, 8)
    eye = torch.eye(3, dtype=torch.float64)
    z = torch.zeros(3, dtype=torch.float64)
    for args in ((eye[:2], z, eye, z, 0.5), (eye, z[:2], eye, z, 0.5), (eye, z, 2 * eye, z, 0.5), (eye, z, eye, z, float("inf")),
                 (eye, z, eye, z, "half"), (eye, z, -eye, z, 0.5), (eye * float("nan"), z, eye, z, 0.5)):
        with pytest.raises(ValueError):
            sr.interpolate_pose(*args)


def test_view_spec_parser():
    from dynhor_amd.surface_render import parse_views, view_poses
    assert parse_views("frames", 8) == ("frames",)
    assert parse_views("interpolate:3:7:5", 8) == ("interpolate", 3, 7, 5)
    assert parse_views("orbit:4", 8) == ("orbit", 4)
    for bad in ("interpolate:3", "interpolate:3:8:5", "interpolate:-1:2:5", "interpolate:3:7:0", "orbit:0", "orbit", "orbit:x", "frames:2",
                "turntable:4", "", 7):
        with pytest.raises(ValueError):
            parse_views(bad, 8)
    from dynhor_amd.scene import look_at_pose
    poses = [look_at_pose(torch.tensor(p)) for p in ([2.0, 0.9, 0.7], [0.3, 2.2, -0.5], [-1.9, 0.2, 1.0])]
    R, T = torch.stack([p[0] for p in poses]), torch.stack([p[1] for p in poses])
    names, Rv, Tv, fr = view_poses(("interpolate", 0, 2, 3), R, T)
    assert len(names) == 5 and fr is None                                     # there and back, the turning point once
    assert torch.equal(Rv[0], R[0].double()) and torch.equal(Rv[2], R[2].double()) and torch.equal(Rv[4], R[0].double())
    assert torch.equal(Rv[1], Rv[3])
    names, Rv, Tv, fr = view_poses(("orbit", 4), R, T)
    assert len(names) == 4 and torch.equal(Rv[0], R[0].double()) and torch.equal(Tv[2], T[0].double())
    # the object turns about ITS z axis: the camera's distance and the axis' image stay
    assert torch.allclose(Rv[2][:, 2], R[0].double()[:, 2]) and torch.allclose(Rv[2][:, 0], -R[0].double()[:, 0])
    names, Rv, Tv, fr = view_poses(("frames",), R, T)
    assert fr == [0, 1, 2] and torch.equal(Rv, R.double())


def test_cli_rejects_an_unknown_mode_with_status_2():
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", "none.yaml", "--mode", "interpolate_3"],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 2 and "invalid choice" in p.stderr
    from dynhor_amd.run import MODES, mode_arg
    assert mode_arg("interpolate_0_38") == "interpolate_0_38" and mode_arg("render_views") == "render_views"
    assert {"train", "validate_image", "validate_mesh", "evaluate_mesh", "visualize_mesh", "refine_poses", "export_poses",
            "init_poses"} <= set(MODES)
    import argparse
    for bad in ("interpolate", "interpolate_a_b", "interpolate_1_2_3", "Train", ""):
        with pytest.raises(argparse.ArgumentTypeError):
            mode_arg(bad)


def test_surface_render_defaults_and_config_block(tmp_path):
    """SURFACE_RENDER_DEFAULTS carries the issue's parameters; a config's surface_render: block overrides them and is validated."""
    from dynhor_amd.runner import SURFACE_RENDER_DEFAULTS, Runner
    from dynhor_amd.surface_render import TRACE_DEFAULTS
    assert {k: SURFACE_RENDER_DEFAULTS[k] for k in TRACE_DEFAULTS} == TRACE_DEFAULTS
    assert TRACE_DEFAULTS == {"eps": 2e-4, "relax": 0.8, "min_step": 1e-3, "max_step": 0.1, "refine_steps": 8, "max_steps": 48,
                              "scan_step": 0.01, "compact_every": 1}
    r = Runner.__new__(Runner)
    r.conf = {"surface_render": {"level": 2, "background": "black"}}
    c = r._surface_conf(method="volume")
    assert (c["level"], c["background"], c["method"], c["eps"]) == (2, "black", "volume", 2e-4)
    for conf, kw in (({"surface_render": {"levle": 2}}, {}), ({}, {"method": "raster"}), ({}, {"background": "sky"}), ({}, {"level": 0}),
                     ({}, {"method": "volume", "background": "frame"})):
        r.conf = conf
        with pytest.raises(ValueError):
            r._surface_conf(**kw)
