"""Mesh alignment without a GPU: the closed forms (Umeyama from moment sums, the point-to-plane Gauss-Newton step), the rotation seed
set and its covering radius, argument validation of the flags and of the two HIP entry points, and the fp64 restatement of
tests/mesh_align_util.py recovering the three-box fixture's transforms at reduced size (what licenses it as the GPU tests' yardstick)."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import mesh_align_util as U
from tests.mesh_eval_util import icosphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def point_moments(p, q, d, origin_src, origin_tgt):
    """The point-to-point layout of dh_icp_moments (include/dynhor_hip.h) from the pairs themselves, fp64."""
    pc, qc = p.double() - origin_src, q.double() - origin_tgt
    return torch.cat([torch.tensor([float(p.shape[0])], dtype=torch.float64), pc.sum(0), qc.sum(0), (qc[:, :, None] * pc[:, None, :]).sum(0).reshape(-1),
                      pc.pow(2).sum().reshape(1), qc.pow(2).sum().reshape(1), d.double().sum().reshape(1)])


def plane_moments(x, q, n, origin_tgt):
    """The point-to-plane layout of dh_icp_moments from transformed points x, their targets q and the targets' normals n, fp64."""
    y, qc = x.double() - origin_tgt, q.double() - origin_tgt
    J = torch.cat([torch.linalg.cross(y, n.double()), n.double(), (n.double() * y).sum(dim=1, keepdim=True)], dim=1)
    b = -(n.double() * (y - qc)).sum(dim=1)
    N = J.T @ J
    iu = torch.triu_indices(7, 7)
    return torch.cat([N[iu[0], iu[1]], J.T @ b, torch.tensor([float(x.shape[0])], dtype=torch.float64)])


def _random_rotation(g, max_deg=180.0):
    ax = torch.randn(3, generator=g, dtype=torch.float64)
    return U.axis_angle(ax.tolist(), float(torch.rand(1, generator=g, dtype=torch.float64)) * max_deg)


def test_umeyama_from_moments_recovers_random_similarities():
    from dynhor_amd.mesh_align import umeyama_from_moments
    g = torch.Generator().manual_seed(3)
    worst = 0.0
    for trial in range(40):
        R = _random_rotation(g) if trial else U.axis_angle((1.0, 2.0, -0.5), 180.0)          # a half turn among them
        s = 10.0 ** float(torch.rand(1, generator=g, dtype=torch.float64) * 2 - 1)           # 0.1 ... 10
        t = torch.randn(3, generator=g, dtype=torch.float64) * 3
        p = torch.randn(200, 3, generator=g, dtype=torch.float64) * 0.3 + torch.randn(3, generator=g, dtype=torch.float64)
        q = s * (p @ R.T) + t
        os_, ot = p.mean(0), q.mean(0)
        mom = point_moments(p, q, torch.zeros(200), os_, ot)
        s1, R1, t1 = umeyama_from_moments(mom, os_, ot, with_scale=True)
        err = max(abs(float(s1) - s) / s, float((R1 - R).abs().max()), float((t1 - t).abs().max()))
        worst = max(worst, err)
        assert float(torch.linalg.det(R1)) > 0
        # rigid mode: the scale is 1 exactly, the rotation the same
        s2, R2, _ = umeyama_from_moments(mom, os_, ot, with_scale=False)
        assert float(s2) == 1.0 and float((R2 - R).abs().max()) < 1e-10
    print(f"umeyama_from_moments: worst error over 40 random similarities {worst:.2e}")
    assert worst < 1e-10
    # a mirrored cloud: the best PROPER rotation is returned, never the reflection
    p = torch.randn(100, 3, generator=g, dtype=torch.float64)
    q = p * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64)
    mom = torch.stack([point_moments(p, q, torch.zeros(100), p.mean(0), q.mean(0))] * 2)
    s3, R3, _ = umeyama_from_moments(mom, p.mean(0), q.mean(0))
    assert R3.shape == (2, 3, 3) and torch.allclose(torch.linalg.det(R3), torch.ones(2, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(R3 @ R3.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(2, 3, 3), atol=1e-12)


def test_umeyama_from_moments_names_degenerate_input():
    from dynhor_amd.mesh_align import umeyama_from_moments
    g = torch.Generator().manual_seed(4)
    p = torch.randn(2, 3, generator=g, dtype=torch.float64)
    with pytest.raises(ValueError, match="fewer than 3 inliers"):
        umeyama_from_moments(point_moments(p, p + 1, torch.zeros(2), p.mean(0), p.mean(0)), p.mean(0), p.mean(0))
    line = torch.linspace(-1, 1, 50, dtype=torch.float64)[:, None] * torch.tensor([[0.3, -0.2, 0.9]], dtype=torch.float64) + 0.5
    with pytest.raises(ValueError, match="collinear"):
        umeyama_from_moments(point_moments(line, 2 * line, torch.zeros(50), line.mean(0), 2 * line.mean(0)), line.mean(0), 2 * line.mean(0))


def test_plane_update_from_moments_is_a_gauss_newton_step():
    """Exact correspondences on an icosphere-free shape (random points with random unit normals): no residual gives no update; a small
    similarity away, one step undoes it to second order; rigid mode leaves the scale alone."""
    from dynhor_amd.mesh_align import plane_update_from_moments
    g = torch.Generator().manual_seed(6)
    q = torch.randn(500, 3, generator=g, dtype=torch.float64) * 0.3
    n = torch.randn(500, 3, generator=g, dtype=torch.float64)
    n = n / n.norm(dim=1, keepdim=True)
    ot = q.mean(0)
    one, eye, zero = torch.ones(1, dtype=torch.float64), torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3, dtype=torch.float64)
    s, R, t = plane_update_from_moments(plane_moments(q, q, n, ot)[None], one, eye, zero, ot)
    assert float(s) == 1.0 and float((R - eye).abs().max()) < 1e-14 and float(t.abs().max()) < 1e-14
    # the source is the target moved by a small similarity D; the step must return nearly D^-1
    Rd, sd, td = U.axis_angle((0.2, 1.0, -0.4), 0.5), 1.004, torch.tensor([0.002, -0.001, 0.003], dtype=torch.float64)
    x = sd * (q @ Rd.T) + td
    s, R, t = plane_update_from_moments(plane_moments(x, q, n, ot)[None], one, eye, zero, ot)
    back = float(s) * (x @ R[0].T) + t[0]
    # what a linearised step leaves is of second order in the motion: at most (|w| + |l|)^2 times the cloud's radius
    second_order = (math.radians(0.5) + math.log(sd)) ** 2 * float((q - ot).norm(dim=1).max())
    left = float((back - q).norm(dim=1).max())
    print(f"plane step: residual motion {left:.2e} of {float((x - q).norm(dim=1).max()):.2e}, second-order bound {second_order:.2e}")
    assert left < second_order
    s, R, t = plane_update_from_moments(plane_moments(x, q, n, ot)[None], one, eye, zero, ot, with_scale=False)
    assert float(s) == 1.0
    with pytest.raises(ValueError, match="fewer than 7 inliers"):
        plane_update_from_moments(plane_moments(x[:5], q[:5], n[:5], ot)[None], one, eye, zero, ot)


def test_rotation_seeds_are_proper_deterministic_and_cover_so3():
    """The design relies on a 40-degree basin of the coarse level (dynhor_amd/mesh_align.py ALIGN_DEFAULTS says where the number comes
    from): the largest angle from any rotation to its nearest seed must stay below it."""
    from dynhor_amd.mesh_align import ALIGN_DEFAULTS, quat_to_matrix, rotation_seeds
    n = ALIGN_DEFAULTS["n_seeds"]
    S = rotation_seeds(n)
    assert S.shape == (n, 3, 3) and S.dtype == torch.float64
    assert torch.equal(S, rotation_seeds(n))
    assert torch.allclose(torch.linalg.det(S), torch.ones(n, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(S @ S.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(n, 3, 3), atol=1e-12)
    g = torch.Generator().manual_seed(0)
    rnd = quat_to_matrix(torch.randn(10_000, 4, generator=g, dtype=torch.float64))          # normalised Gaussian quaternions: Haar
    tr = torch.einsum("aij,bij->ab", rnd, S)
    nearest = torch.rad2deg(torch.acos(((tr - 1) / 2).clamp(-1, 1))).min(dim=1).values
    print(f"rotation_seeds({n}): covering radius {float(nearest.max()):.2f} deg, mean distance {float(nearest.mean()):.2f} deg "
          "(10^4 random rotations)")
    assert float(nearest.max()) < 40.0
    with pytest.raises(ValueError):
        rotation_seeds(0)


def test_flags_are_validated():
    from dynhor_amd.metrics import check_align_args, mesh_metrics
    from dynhor_amd.mesh_align import align_clouds
    v, f = icosphere(0.5, 1)
    with pytest.raises(ValueError, match="gt_align must be"):
        mesh_metrics(v, f, v, f, gt_align="icp")
    with pytest.raises(ValueError, match="gt_align_init must be"):
        mesh_metrics(v, f, v, f, gt_align="rigid", gt_align_init="random")
    with pytest.raises(ValueError, match="gt_align must be"):
        check_align_args("evaluate_mesh", "affine", "identity")                                # the eval: block goes through this
    for ok in ("none", "rigid", "similarity"):
        for init in ("identity", "global"):
            check_align_args("evaluate_mesh", ok, init)
    with pytest.raises(ValueError, match="mode must be"):
        align_clouds(v, v, None, mode="none")
    with pytest.raises(ValueError, match="unknown options"):
        align_clouds(v, v, None, mode="rigid", n_seed=4)
    # the CLI refuses a mode it does not know before anything else runs
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", "none.yaml", "--mode", "evaluate_mesh", "--gt_align",
                        "affine"], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--gt_align" in p.stderr


def test_device_functions_refuse_cpu_tensors():
    from dynhor_amd import _lib
    from dynhor_amd.mesh_align import icp_correspond, icp_moments
    z = torch.zeros(4, 3)
    with pytest.raises(_lib.DynhorHipError, match="no CPU fallback"):
        icp_correspond(z, z, torch.zeros(1, 12))
    with pytest.raises(_lib.DynhorHipError, match="no CPU fallback"):
        icp_moments(z, z, None, torch.zeros(1, 12), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4), torch.zeros(1), torch.zeros(3),
                    torch.zeros(3))


def test_icp_entry_points_declared_bound_and_checked(hiplib):
    from dynhor_amd import _lib
    header = open(os.path.join(ROOT, "include", "dynhor_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("dh_icp_correspond", "dh_icp_correspond_workspace", "dh_icp_moments", "dh_icp_moments_workspace", "dh_icp_moments_sums"):
        assert s + "(" in header and hasattr(raw, s) and s in _lib.SIGNATURES
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(0x7f0000000000)       # fake: non-null, aligned, never dereferenced by a refused call
    L = hiplib
    assert L.dh_icp_correspond(null, 0, null, 10, null, 3, null, null, null, null) == 0              # N == 0: no-op
    assert L.dh_icp_correspond(null, 5, null, 10, null, 0, null, null, null, null) == 0              # H == 0: no-op
    assert L.dh_icp_correspond(null, 5, null, 10, null, 3, null, null, null, null) == -1             # null pointers
    assert L.dh_icp_correspond(fake, 5, fake, 10, fake, 3, fake, null, null, null) == -1             # idx is required
    assert L.dh_icp_correspond(fake, 5, fake, 0, fake, 3, fake, fake, null, null) == -1              # M == 0 with work to do
    assert L.dh_icp_correspond(fake, -1, fake, 10, fake, 3, fake, fake, null, null) == -1
    assert L.dh_icp_correspond(fake, 5, fake, 10, fake, -3, fake, fake, null, null) == -1
    assert L.dh_icp_correspond(fake, 5, fake, 1 << 31, fake, 3, fake, fake, null, null) == -2        # int32 indices
    assert L.dh_icp_correspond(fake, 5, fake, 10, fake, 1 << 16, fake, fake, null, null) == -2       # grid.z
    assert L.dh_icp_correspond(fake, 5, fake, 10, fake, 3, fake, fake, ctypes.c_void_p(0x7f0000000004), null) == -1   # misaligned ws
    assert L.dh_icp_correspond_workspace(-1, 5, 1) == -1 and L.dh_icp_correspond_workspace(5, 5, -1) == -1
    # slab split: with one hypothesis exactly the plan of dh_nearest_sqdist; hypotheses count as query blocks
    assert L.dh_icp_correspond_workspace(37, 10 ** 6, 1) == L.dh_nearest_sqdist_workspace(37, 10 ** 6) > 0
    assert L.dh_icp_correspond_workspace(10 ** 7, 10 ** 6, 2) == 0 and L.dh_icp_correspond_workspace(1024, 4096, 256) == 0
    few, many = L.dh_icp_correspond_workspace(100_000, 100_000, 1), L.dh_icp_correspond_workspace(100_000, 100_000, 4)
    assert few > 0 and many > 0 and many // (4 * 100_000 * 8) < few // (100_000 * 8)                 # fewer slabs per hypothesis
    assert L.dh_icp_moments_sums(0) == 19 and L.dh_icp_moments_sums(1) == 36
    assert L.dh_icp_moments_workspace(100_000, 3, 0) == 3 * 128 * 19 * 8 and L.dh_icp_moments_workspace(1000, 2, 1) == 2 * 4 * 36 * 8
    assert L.dh_icp_moments_workspace(-1, 1, 0) == -1
    args = [fake] * 9 + [5, 10, 3, fake, fake, null]
    for k in (0, 1, 3, 4, 5, 6, 7, 8, 12, 13):                                                       # every required pointer (2: normals, optional)
        bad = list(args)
        bad[k] = null
        assert L.dh_icp_moments(*bad) == -1, k
    assert L.dh_icp_moments(*([null] * 9 + [5, 10, 0, null, null, null])) == 0                       # H == 0: no-op
    assert L.dh_icp_moments(*([fake] * 9 + [-5, 10, 3, fake, fake, null])) == -1
    assert L.dh_icp_moments(*([fake] * 9 + [5, 1 << 31, 3, fake, fake, null])) == -2


# ---- the restatement recovers the fixture's transforms at reduced size -------------------------------------------------------------
N_SMALL = 4000
MOVE_S, MOVE_T = 7.3, (2.0, -3.0, 1.5)                  # the translation: several object sizes (the fixture is 0.5 long)


@pytest.fixture(scope="module")
def boxes():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return U.three_box_mesh(64), U.three_box_mesh(80)


def _score(pv, pf, gv, gf, aligned_v, s_total):
    spacing = math.sqrt(U.mesh_area(pv, pf) / N_SMALL)
    c_al, c_un = U.ref_chamfer_l1(pv, pf, aligned_v, gf, N_SMALL), U.ref_chamfer_l1(pv, pf, gv, gf, N_SMALL)
    print(f"  chamfer_l1 aligned {c_al:.6f}, ground truth left in place {c_un:.6f}, sample spacing {spacing:.6f}, total scale x 7.3 = "
          f"{s_total * MOVE_S:.5f}")
    assert abs(c_al - c_un) < spacing
    assert abs(s_total * MOVE_S - 1.0) < 0.01


@pytest.mark.parametrize("method", ["plane", "point"])
def test_restatement_recovers_the_local_case(boxes, method):
    """15 degrees off, started from the reference normalisation (the identity in that frame), default parameters."""
    from dynhor_amd.mesh_align import ALIGN_DEFAULTS as D
    from dynhor_amd.metrics import normalize_like_reference, sample_surface
    (pv, pf), (gv, gf) = boxes
    Rm = U.axis_angle((0.3, -0.5, 0.8), 15.0)
    mv = U.moved(gv, MOVE_S, Rm, torch.tensor(MOVE_T, dtype=torch.float64))
    nv, _, sc = normalize_like_reference(mv)
    g = torch.Generator().manual_seed(0)
    tgt, tn = sample_surface(pv, pf, N_SMALL, g)
    src, _ = sample_surface(nv, gf, N_SMALL, g)
    s, R, t, st = U.ref_icp(src, tgt, tn, 1.0, torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), True, method,
                            D["trim"], D["max_iters"], D["tol"])
    print(f"restatement, local, {method}: {st}, rotation error {U.angle_deg(R, Rm.T):.3f} deg")
    assert U.angle_deg(R, Rm.T) < 1.0
    _score(pv, pf, gv, gf, (s * (nv.double() @ R.T) + t).float(), s * sc)


def test_restatement_recovers_the_global_case(boxes):
    """130 degrees about a skew axis, nothing known: centroid / RMS start, 64 seeds and a 512 x 2048 coarse level of 20 iterations
    (reduced from the defaults for the CPU's sake), the best four refined with the default method."""
    from dynhor_amd.mesh_align import ALIGN_DEFAULTS as D, rotation_seeds
    from dynhor_amd.metrics import sample_surface
    (pv, pf), (gv, gf) = boxes
    Rm = U.axis_angle((0.3, -0.5, 0.8), 130.0)
    mv = U.moved(gv, MOVE_S, Rm, torch.tensor(MOVE_T, dtype=torch.float64))
    g = torch.Generator().manual_seed(0)
    tgt, tn = sample_surface(pv, pf, N_SMALL, g)
    src, _ = sample_surface(mv, gf, N_SMALL, g)
    s, R, t, st = U.ref_align_global(src, tgt, tn, rotation_seeds(64), True, D["method"], D["trim"], (512, 2048), 20, D["n_refine"],
                                     D["max_iters"], D["tol"], D["second_min_deg"])
    print(f"restatement, global: rotation error {U.angle_deg(R, Rm.T):.3f} deg, two-sided residual {st['residual_two_sided']:.5f}, "
          f"runner-up {st['residual_second']}, refined {[round(c['two_sided'], 5) for c in st['refined']]}")
    assert U.angle_deg(R, Rm.T) < 1.0
    assert st["residual_second"] is not None and st["residual_second"] >= 2 * st["residual_two_sided"]
    _score(pv, pf, gv, gf, (s * (mv.double() @ R.T) + t).float(), s)
