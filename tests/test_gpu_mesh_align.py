"""Mesh alignment on the GPU: dh_icp_correspond bit for bit against dh_nearest_sqdist on clouds transformed by the documented fp32
formula, dh_icp_moments against fp64 torch sums, local and global registration of the three-box fixture against the fp64 restatement
(tests/mesh_align_util.py) and against the metrics of the ground truth left in place, the synthetic scene (recorded, not asserted),
Runner.evaluate_mesh / the CLI end to end, and evaluate_mesh without the flags unchanged."""
import ctypes
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import mesh_align_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
MOVE_S, MOVE_T = 7.3, (2.0, -3.0, 1.5)                  # the translation: several object sizes (the fixture is 0.5 long)


def _transforms(h, seed):
    """h similarity transforms as the kernels take them ([h,12] fp32 on the device) and in fp64 (s, R, t)."""
    from dynhor_amd.mesh_align import pack_transforms, quat_to_matrix
    g = torch.Generator().manual_seed(seed)
    R = quat_to_matrix(torch.randn(h, 4, generator=g, dtype=torch.float64))
    s = 0.5 + torch.rand(h, generator=g, dtype=torch.float64)
    t = torch.randn(h, 3, generator=g, dtype=torch.float64) * 0.1
    return pack_transforms(s, R, t).to(DEV), (s, R, t)


def _clouds(n, m, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return ((torch.rand(n, 3, device=DEV, generator=g) - 0.5) * 1.2).contiguous(), ((torch.rand(m, 3, device=DEV, generator=g) - 0.5) * 1.2).contiguous()


def _raw_correspond(src, tgt, xf, ws, stream=None):
    from dynhor_amd import _lib
    h, n = xf.shape[0], src.shape[0]
    d2 = torch.empty(h, n, device=DEV)
    idx = torch.empty(h, n, dtype=torch.int32, device=DEV)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    _lib.check(_lib.lib().dh_icp_correspond(_lib.ptr(src), n, _lib.ptr(tgt), tgt.shape[0], _lib.ptr(xf), h, _lib.ptr(d2), _lib.ptr(idx),
                                            _lib.ptr(ws) if ws is not None else None, st))
    return d2, idx


@pytest.mark.parametrize("n,m,slabs", [(5000, 300_000, True), (3000, 5000, False)])
def test_correspond_equals_nearest_sqdist_on_transformed_clouds(n, m, slabs):
    from dynhor_amd import _lib
    from dynhor_amd.metrics import nearest_sqdist
    src, tgt = _clouds(n, m, seed=n + m)
    xf, _ = _transforms(3, seed=1)
    # a tie across slabs: two target points at the same place, a source point of hypothesis 1 landing exactly there
    x1 = U.transform32(src, xf[1])
    tgt[m // 3] = x1[0]
    tgt[m - 2] = x1[0]
    nbytes = _lib.lib().dh_icp_correspond_workspace(n, m, 3)
    assert (nbytes > 0) == slabs
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes > 0 else None
    a = _raw_correspond(src, tgt, xf, ws)
    b = _raw_correspond(src, tgt, xf, ws)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = _raw_correspond(src, tgt, xf, ws, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    one = _raw_correspond(src, tgt, xf, None)                    # the one-slab sweep
    for other in (b, c, one):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
    for h in range(3):
        d2, idx = nearest_sqdist(U.transform32(src, xf[h]), tgt, return_index=True)
        assert torch.equal(a[0][h], d2), f"hypothesis {h}: distances differ from dh_nearest_sqdist on the transformed cloud"
        assert torch.equal(a[1][h].long(), idx), f"hypothesis {h}: indices differ"
    assert float(a[0][1][0]) == 0.0 and int(a[1][1][0]) == m // 3, "duplicated targets: the smallest index wins"


@pytest.mark.parametrize("plane", [False, True])
def test_moments_match_fp64_sums_and_are_reproducible(plane):
    """Every entry within 1e-9 x the sum of the absolute values of its terms (only the order of fp64 additions differs: N 2^-53 ~ 1e-10
    at N = 10^6), and two launches give the same bits."""
    from dynhor_amd.mesh_align import icp_correspond, icp_moments
    n, m, H = 1_000_000, 50_000, 3
    src, tgt = _clouds(n, m, seed=17)
    g = torch.Generator(device=DEV).manual_seed(2)
    nrm = torch.randn(m, 3, device=DEV, generator=g)
    nrm = (nrm / nrm.norm(dim=1, keepdim=True)).contiguous()
    xf, _ = _transforms(H, seed=5)
    d2, idx = icp_correspond(src, tgt, xf)
    thr = torch.kthvalue(d2, int(0.9 * n), dim=1).values
    o_src, o_tgt = src.mean(0), tgt.mean(0)
    out = icp_moments(src, tgt, nrm if plane else None, xf, idx, d2, thr, o_src, o_tgt)
    again = icp_moments(src, tgt, nrm if plane else None, xf, idx, d2, thr, o_src, o_tgt)
    assert torch.equal(out, again)
    assert out.shape == (H, 36 if plane else 19) and out.dtype == torch.float64
    worst = 0.0
    for h in range(H):
        keep = d2[h] <= thr[h]
        p = src[keep].double()
        q = tgt[idx[h][keep].long()].double() - o_tgt.double()
        if plane:
            A, t = xf[h, :9].double().reshape(3, 3), xf[h, 9:].double()
            y = p @ A.T + t - o_tgt.double()
            nv = nrm[idx[h][keep].long()].double()
            J = torch.cat([torch.linalg.cross(y, nv), nv, (nv * y).sum(dim=1, keepdim=True)], dim=1)
            b = -(nv * (y - q)).sum(dim=1)
            iu = torch.triu_indices(7, 7)
            terms = torch.cat([J[:, iu[0]] * J[:, iu[1]], J * b[:, None], torch.ones_like(b)[:, None]], dim=1)
        else:
            pc = p - o_src.double()
            terms = torch.cat([torch.ones(p.shape[0], 1, dtype=torch.float64, device=DEV), pc, q,
                               (q[:, :, None] * pc[:, None, :]).reshape(-1, 9), pc.pow(2).sum(dim=1, keepdim=True),
                               q.pow(2).sum(dim=1, keepdim=True), d2[h][keep].double().sqrt()[:, None]], dim=1)
        ref, mag = terms.sum(dim=0), terms.abs().sum(dim=0)
        rel = ((out[h] - ref).abs() / mag.clamp(min=1e-300)).max()
        worst = max(worst, float(rel))
        assert bool(((out[h] - ref).abs() <= 1e-9 * mag).all()), (h, float(rel))
        assert float(out[h][35 if plane else 0]) == float(keep.sum())
    print(f"dh_icp_moments ({'plane' if plane else 'point'}): worst |error| / sum |terms| = {worst:.2e}")


# ---- the three-box fixture ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def boxes():
    (pv, pf), (gv, gf) = U.three_box_mesh(128, DEV), U.three_box_mesh(192, DEV)
    return (pv, pf), (gv.cpu(), gf.cpu())


def _samples(pv, pf, sv, sf, n, seed=0):
    """The samples align_meshes draws (prediction first, one generator)."""
    from dynhor_amd.metrics import sample_surface
    g = torch.Generator(device=DEV).manual_seed(seed)
    tgt, tn = sample_surface(pv.to(DEV, torch.float32), pf, n, g)
    src, _ = sample_surface(sv.to(DEV, torch.float32), sf, n, g)
    return src, tgt, tn


def _check_against_restatement(tag, hip, ref, src, tgt, tol):
    """(a): the two registrations, from the same samples and start, end within each other's last-iteration step.  A run stops when a
    step is below tol x the target's bounding radius, so neither transform is defined more finely than that: the bound is the sum of
    the two last steps, and never below that resolution."""
    (s1, R1, t1, st1), (s2, R2, t2, st2) = hip, ref
    c = src.double().mean(0).cpu()
    r_src = float((src.double().cpu() - c).norm(dim=1).max())
    r_tgt = float((tgt.double() - tgt.double().mean(0)).norm(dim=1).max())
    gap = U.transform_gap((s1, R1, t1), (s2, R2, t2), c, r_src)
    bound = max(st1["last_step"] + st2["last_step"], tol * r_tgt)
    print(f"{tag}: HIP {st1['iters']} iterations (converged {st1['converged']}, last step {st1['last_step']:.3e}), restatement "
          f"{st2['iters']} (converged {st2['converged']}, last step {st2['last_step']:.3e}); gap between the two {gap:.3e}, bound {bound:.3e}; "
          f"rotation apart {U.angle_deg(R1, R2):.5f} deg, scale ratio {float(s1) / float(s2):.8f}")
    assert gap <= bound, (gap, bound)


def _check_metrics(tag, pv, pf, gv, gf, moved_v, n_samples=200_000, **kw):
    """(b): the metrics are what they would be without the move, gt_scale is the move's; without gt_align the frame error shows."""
    from dynhor_amd.metrics import mesh_metrics
    spacing = math.sqrt(U.mesh_area(pv, pf) / n_samples)
    base = mesh_metrics(pv, pf, gv, gf, n_samples=n_samples, device=DEV)
    al = mesh_metrics(pv, pf, moved_v, gf, n_samples=n_samples, device=DEV, **kw)
    print(f"{tag}: chamfer_l1 aligned {al['chamfer_l1']:.6f}, ground truth left in the canonical frame {base['chamfer_l1']:.6f}, sample "
          f"spacing {spacing:.6f}; gt_scale {al['gt_scale']:.5f}; " + json.dumps({k: v for k, v in al.items() if k.startswith('align_')}))
    assert abs(al["chamfer_l1"] - base["chamfer_l1"]) < spacing
    assert abs(al["gt_scale"] / MOVE_S - 1.0) < 0.01
    off = mesh_metrics(pv, pf, moved_v, gf, n_samples=n_samples, device=DEV, **{k: v for k, v in kw.items() if k == "gt_normalize"})
    print(f"{tag}: without gt_align chamfer_l1 {off['chamfer_l1']:.5f}")
    assert off["chamfer_l1"] > 0.05
    return al


@pytest.mark.parametrize("method", ["plane", "point"])
def test_local_alignment_of_the_three_box_fixture(boxes, method):
    """15 degrees off, scale 7.3, far away: init "identity" after gt_normalize "reference"."""
    from dynhor_amd.mesh_align import ALIGN_DEFAULTS as D, align_clouds
    from dynhor_amd.metrics import normalize_like_reference
    (pv, pf), (gv, gf) = boxes
    Rm = U.axis_angle((0.3, -0.5, 0.8), 15.0)
    mv = U.moved(gv, MOVE_S, Rm, torch.tensor(MOVE_T, dtype=torch.float64))
    nv, _, _ = normalize_like_reference(mv)
    src, tgt, tn = _samples(pv, pf, nv, gf, 20_000)
    s, R, t, st = align_clouds(src, tgt, tn, mode="similarity", init="identity", method=method)
    ref = U.ref_icp(src, tgt, tn, 1.0, torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), True, method, D["trim"],
                    D["max_iters"], D["tol"])
    print(f"local {method}: rotation error {U.angle_deg(R, Rm.T):.4f} deg (restatement {U.angle_deg(ref[1], Rm.T):.4f})")
    _check_against_restatement(f"local {method}", (s, R, t, st), ref, src, tgt, D["tol"])
    al = _check_metrics(f"local {method}", pv, pf, gv, gf, mv, gt_normalize="reference", gt_align="similarity", gt_align_init="identity",
                        align_opts={"method": method})
    assert al["gt_align"] == "similarity" and al["gt_align_init"] == "identity" and al["align_method"] == method


def test_global_alignment_of_the_three_box_fixture(boxes):
    """130 degrees about a skew axis, nothing known about the frame: init "global"."""
    from dynhor_amd.mesh_align import ALIGN_DEFAULTS as D, align_clouds, rotation_seeds
    (pv, pf), (gv, gf) = boxes
    Rm = U.axis_angle((0.3, -0.5, 0.8), 130.0)
    mv = U.moved(gv, MOVE_S, Rm, torch.tensor(MOVE_T, dtype=torch.float64))
    src, tgt, tn = _samples(pv, pf, mv, gf, 20_000)
    s, R, t, st = align_clouds(src, tgt, tn, mode="similarity", init="global")
    rs, rR, rt, rst = U.ref_align_global(src, tgt, tn, rotation_seeds(D["n_seeds"]), True, D["method"], D["trim"],
                                         (D["coarse_src"], D["coarse_tgt"]), D["coarse_iters"], D["n_refine"], D["max_iters"], D["tol"],
                                         D["second_min_deg"])
    print(f"global: rotation error {U.angle_deg(R, Rm.T):.4f} deg (restatement {U.angle_deg(rR, Rm.T):.4f}); two-sided residual "
          f"{st['residual_two_sided']:.6f} (restatement {rst['residual_two_sided']:.6f}), runner-up {st['residual_second']} "
          f"(restatement {rst['residual_second']})")
    _check_against_restatement("global", (s, R, t, st), (rs, rR, rt, rst), src, tgt, D["tol"])
    al = _check_metrics("global", pv, pf, gv, gf, mv, gt_align="similarity", gt_align_init="global")
    assert al["align_seeds"] == D["n_seeds"] and al["align_n_align"] == D["n_align"]
    assert al["align_residual_second"] is not None and al["align_residual_second"] >= 2 * al["align_residual_two_sided"]


def test_synthetic_scene_is_recorded():
    """The project's own scene (a sphere with a box half inside it: nearly symmetric, smooth), 15 degrees off, both methods: iterations,
    final rotation error and `converged` are printed for DESIGN_NEXT_ROWS.md section 12 -- recorded, not asserted."""
    from dynhor_amd.mesh_align import align_clouds
    from dynhor_amd.metrics import normalize_like_reference
    from dynhor_amd.scene import scene_sdf
    pv, pf = U.sdf_mesh(scene_sdf, 128, DEV, bound=0.55)
    gv, gf = U.sdf_mesh(scene_sdf, 192, DEV, bound=0.55)
    Rm = U.axis_angle((0.3, -0.5, 0.8), 15.0)
    mv = U.moved(gv, MOVE_S, Rm, torch.tensor(MOVE_T, dtype=torch.float64))
    nv, _, sc = normalize_like_reference(mv)
    src, tgt, tn = _samples(pv, pf, nv, gf.cpu(), 100_000)
    for method in ("point", "plane"):
        s, R, t, st = align_clouds(src, tgt, tn, mode="similarity", init="identity", method=method)
        print(f"synthetic scene, 15 deg off, {method}: iterations {st['iters']}, converged {st['converged']}, final rotation error "
              f"{U.angle_deg(R, Rm.T):.3f} deg, total scale x 7.3 = {s * sc * MOVE_S:.5f}, residual {st['residual']:.6f}")
        assert math.isfinite(s)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _synthetic_conf(name, **extra):
    return {"seq_name": "malign", "exp_name": name,
            "data_info": {"synthetic": {"n_frames": 3, "H": 64, "W": 64, "seed": 5}},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100}, **extra}


def _moved_fixture_file(tmp_path):
    from dynhor_amd.mesh import write_ply
    gv, gf = U.three_box_mesh(96, DEV)
    mv = U.moved(gv, MOVE_S, U.axis_angle((0.3, -0.5, 0.8), 15.0), torch.tensor(MOVE_T, dtype=torch.float64))
    path = str(tmp_path / "scan.ply")
    write_ply(path, mv, gf.cpu())
    return path


def test_evaluate_mesh_with_alignment_end_to_end(tmp_path):
    """Plumbing: a geometric-init network is only a rough sphere, so no pose is asserted."""
    from dynhor_amd.metrics import load_mesh, normalize_like_reference
    from dynhor_amd.runner import Runner
    scan = _moved_fixture_file(tmp_path)
    r = Runner(conf=_synthetic_conf("e2e"), device="cuda:0", exp_root=str(tmp_path))
    n = 50_000
    m = r.evaluate_mesh(gt_mesh=scan, gt_align="similarity", gt_normalize="reference", resolution=96, n_samples=n,
                        align_opts={"n_align": 20_000})
    stem = os.path.join(r.base_exp_dir, "meshes", "{:0>8d}".format(r.iter_step))
    saved = json.load(open(stem + "_eval.json"))
    keys = {"gt_align", "gt_align_init", "align_scale", "align_R", "align_t", "align_residual", "align_residual_two_sided", "align_iters",
            "align_inliers", "align_n_align", "align_seeds", "align_converged", "align_residual_second", "gt_scale", "chamfer_l1"}
    assert keys <= set(saved) and saved == json.loads(json.dumps(m))
    assert m["gt_align"] == "similarity" and m["gt_align_init"] == "identity" and m["align_n_align"] == 20_000 and m["align_seeds"] == 1
    for k in ("align_scale", "align_residual", "align_residual_two_sided", "gt_scale", "chamfer_l1", "accuracy", "completeness"):
        assert math.isfinite(m[k]), (k, m[k])
    R = torch.tensor(m["align_R"], dtype=torch.float64).reshape(3, 3)
    assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-9 and abs(float(torch.linalg.det(R)) - 1.0) < 1e-9
    file_v, file_f = load_mesh(scan)
    got_v, got_f = load_mesh(stem + "_gt_aligned.ply")
    nv, _, sc = normalize_like_reference(file_v)
    want = (m["align_scale"] * (nv.double() @ R.T) + torch.tensor(m["align_t"], dtype=torch.float64)).float()
    assert torch.equal(got_f, file_f) and torch.allclose(got_v, want, atol=1e-6)
    assert abs(m["gt_scale"] * m["align_scale"] * sc - 1.0) < 1e-12
    blob = b"".join(open(os.path.join(r.base_exp_dir, "board", fn), "rb").read() for fn in os.listdir(os.path.join(r.base_exp_dir, "board")))
    r.close()
    assert b"eval/align_residual" in blob

    # the analytic ground truth is aligned already: the rigid registration must return (nearly) the identity, or say it did not converge
    e = r.evaluate_mesh(resolution=96, gt_resolution=128, n_samples=n, gt_align="rigid", align_opts={"n_align": 20_000}, save=False)
    assert e["gt"] == "scene_sdf@128" and e["align_scale"] == 1.0
    gv, gf = r._scene_gt_mesh(128)
    Re, te = torch.tensor(e["align_R"], dtype=torch.float64).reshape(3, 3), torch.tensor(e["align_t"], dtype=torch.float64)
    disp = float(((gv.double().cpu() @ Re.T + te) - gv.double().cpu()).norm(dim=1).max())
    spacing = math.sqrt(U.mesh_area(gv.cpu(), gf.cpu()) / 20_000)
    print(f"analytic ground truth, rigid: largest vertex displacement {disp:.5f} (sample spacing {spacing:.5f}), converged "
          f"{e['align_converged']}, iterations {e['align_iters']}")
    assert disp < spacing or e["align_converged"] is False


def test_cli_evaluate_mesh_with_alignment(tmp_path):
    from dynhor_amd.runner import Runner
    scan = _moved_fixture_file(tmp_path)
    conf = _synthetic_conf("cli", eval={"n_samples": 50_000, "gt_mesh": scan, "gt_normalize": "reference", "gt_align_init": "identity",
                                        "align_opts": {"n_align": 20_000}})
    r = Runner(conf=conf, device="cuda:0", exp_root=str(tmp_path))
    r.train(2)
    r.save_checkpoint()
    import yaml
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--mode", "evaluate_mesh", "--is_continue",
                        "--exp_root", str(tmp_path), "--mesh_resolution", "64", "--gt_align", "similarity"], cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["gt_align"] == "similarity" and out["gt_align_init"] == "identity" and out["align_n_align"] == 20_000
    assert math.isfinite(out["align_residual"]) and math.isfinite(out["chamfer_l1"]) and len(out["align_R"]) == 9
    # a mode the eval: block does not know is refused
    bad = Runner(conf=_synthetic_conf("bad", eval={"gt_align": "affine"}), device="cuda:0", exp_root=str(tmp_path))
    with pytest.raises(ValueError, match="gt_align must be"):
        bad.evaluate_mesh(resolution=32, n_samples=1000, save=False)


def test_mesh_metrics_without_the_flags_is_unchanged():
    """gt_align "none" (the default) against the code path as it was before the flags existed, restated here: same keys, same values."""
    from dynhor_amd.metrics import distance_metrics, mesh_metrics, nearest_sqdist, normalize_like_reference, sample_surface
    from tests.mesh_eval_util import icosphere
    pv, pf = icosphere(0.45, 4)
    gv, gf = icosphere(0.5, 4)
    gv = gv * 3 + 1
    n = 50_000
    for kw in ({}, {"gt_align": "none", "gt_align_init": "global"}):
        got = mesh_metrics(pv, pf, gv, gf, n_samples=n, seed=3, gt_normalize="reference", device=DEV, **kw)
        g_v, _, scale = normalize_like_reference(gv.to(DEV, torch.float32))
        g = torch.Generator(device=DEV).manual_seed(3)
        p, pn = sample_surface(pv.to(DEV, torch.float32), pf, n, g)
        q, qn = sample_surface(g_v, gf, n, g)
        d2_pg, i_pg = nearest_sqdist(p, q, return_index=True)
        d2_gp, i_gp = nearest_sqdist(q, p, return_index=True)
        want = distance_metrics(d2_pg, d2_gp, (0.005, 0.01, 0.02))
        want["normal_consistency"] = 0.5 * (float((pn * qn[i_pg]).sum(dim=1).abs().double().mean())
                                            + float((qn * pn[i_gp]).sum(dim=1).abs().double().mean()))
        want.update(n_samples=n, n_pred_faces=int(pf.shape[0]), n_gt_faces=int(gf.shape[0]), gt_scale=1.0 / scale)
        assert list(got) == list(want) and got == want
