"""CPU: the fp64 restatement of the silhouette pose loss (tests/pose_sil_util.py) is licensed first -- coverage against a hand-written
inside test, the halo's three defining properties, its gradient against central differences, the smoothness term from moments against
the direct mean -- and shown to recover perturbed poses on a small scene.  Then the parts of the feature that need no GPU: argument
validation of the three entry points through ctypes, the wrappers' refusal of CPU tensors, the frame selection, the CLI flags, the
config block, and export_poses -> Dataset._load_from_disk with and without obj_scale."""
import ctypes
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pose_sil_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------ the restatement
def _inside_by_angles(tri, p):
    """A pixel centre lies in a triangle (edges included) when it is a vertex, lies on an edge, or the signed angles it subtends with the
    three edges add up to +-2 pi.  Nothing in common with the edge-function test of the restatement."""
    out = torch.zeros(p.shape[0], dtype=torch.bool)
    for k in range(p.shape[0]):
        tot, on = 0.0, False
        for i in range(3):
            a, b = tri[i] - p[k], tri[(i + 1) % 3] - p[k]
            cr, dt = float(a[0] * b[1] - a[1] * b[0]), float(a[0] * b[0] + a[1] * b[1])
            if abs(cr) < 1e-12 and dt <= 1e-12:
                on = True
            tot += math.atan2(cr, dt)
        out[k] = on or abs(abs(tot) - 2.0 * math.pi) < 1e-6
    return out


def test_restatement_d2_is_zero_exactly_on_the_covered_pixels():
    H, W = 24, 31
    p = U.pixel_grid(H, W)
    tris = torch.tensor([[[3.2, 2.1], [25.7, 6.4], [11.3, 20.9]],            # general position
                         [[4.0, 4.0], [20.0, 4.0], [4.0, 16.0]],             # vertices and two edges on pixel centres
                         [[18.0, 22.0], [29.5, 12.0], [22.0, 3.0]],          # the other winding
                         [[5.5, 5.5], [5.9, 5.6], [5.6, 5.9]]], dtype=F64)   # sub-pixel: covers no centre
    ok = torch.ones(1, dtype=torch.bool)
    for k in range(tris.shape[0]):
        d2 = U.face_d2(tris[k:k + 1], ok, p)[:, 0]
        inside = _inside_by_angles(tris[k], p)
        assert torch.equal(d2 == 0, inside), k
        assert bool((d2[~inside] > 0).all())
    assert int((U.face_d2(tris[3:4], ok, p) == 0).sum()) == 0 and int((U.face_d2(tris[1:2], ok, p) == 0).sum()) > 80
    # outside, d2 is the squared distance to the nearest point of the outline: checked against a dense sampling of the three edges
    t = torch.linspace(0.0, 1.0, 4001, dtype=F64)[:, None]
    tri = tris[0]
    samples = torch.cat([tri[i] + t * (tri[(i + 1) % 3] - tri[i]) for i in range(3)])
    d2 = U.face_d2(tris[0:1], ok, p)[:, 0]
    brute = (torch.cdist(p, samples) ** 2).min(dim=1).values
    out = d2 > 0
    assert torch.allclose(d2[out], brute[out], rtol=0.0, atol=2e-2) and bool((d2[out] <= brute[out] + 1e-12).all())
    # a skipped face reports inf; the smallest face index wins a tie
    assert bool(torch.isinf(U.face_d2(tris[0:1], torch.zeros(1, dtype=torch.bool), p)).all())
    verts = torch.tensor([[-0.2, -0.2, 0.0], [0.2, -0.2, 0.0], [0.0, 0.2, 0.0]], dtype=F64)
    faces = torch.tensor([[0, 1, 2], [0, 1, 2], [0, 1, 2]])
    K = torch.tensor([[40.0, 0.0, 15.0], [0.0, 40.0, 12.0], [0.0, 0.0, 1.0]], dtype=F64)
    d2, face = U.nearest(verts, faces, torch.eye(3, dtype=F64), torch.tensor([0.0, 0.0, 1.0], dtype=F64), K, H, W)
    assert int((d2 == 0).sum()) > 20 and bool((face == 0).all())


def test_restatement_halo_is_one_at_zero_continuous_at_the_cut_and_zero_beyond():
    for sigma, cut in ((4.0, 3.0), (1.5, 3.0), (2.0, 2.0)):
        cs2 = U.halo_consts(sigma, cut)[0]
        x = torch.tensor([0.0, cs2 * (1 - 1e-9), cs2, cs2 * (1 + 1e-9), 4 * cs2, float("inf")], dtype=F64)
        h = U.halo(x, sigma, cut)
        assert float(h[0]) == 1.0
        assert 0.0 <= float(h[1]) < 1e-6 and 0.0 <= float(h[2]) < 1e-6            # continuous: no jump where it is cut off
        assert float(h[3]) == 0.0 and float(h[4]) == 0.0 and float(h[5]) == 0.0
        xs = torch.linspace(0.0, cs2, 200, dtype=F64)
        hs = U.halo(xs, sigma, cut)
        assert bool((hs[1:] <= hs[:-1]).all()) and bool((hs >= 0).all())


def test_restatement_gradient_agrees_with_central_differences():
    sc = U.small_scene(n_frames=2, H=48, W=48, seed=11, n_lat=5, n_lon=8)
    v, f, K, lab = sc["verts"], sc["faces"], sc["K"], sc["label"]
    rot6d = U.matrix_to_rot6d(sc["R0"]).requires_grad_(True)
    trans = sc["T0"].clone().requires_grad_(True)
    sigma = 2.5
    M, w = U.target_and_weight(lab, sigma, 3.0, 0.5)
    loss, _ = U.sil_loss(v, f, rot6d, trans, K, lab, sigma, M=M, w=w)
    g_rot, g_tr = torch.autograd.grad(loss, (rot6d, trans))
    assert float(g_rot.norm()) > 0 and float(g_tr.norm()) > 0
    eps = 1e-6
    worst = 0.0
    for p, g in ((rot6d, g_rot), (trans, g_tr)):
        flat = p.detach().reshape(-1)
        num = torch.zeros_like(flat)
        for k in range(flat.numel()):
            vals = []
            for s in (+1.0, -1.0):
                q = flat.clone()
                q[k] += s * eps
                args = (q.view_as(p), trans.detach()) if p is rot6d else (rot6d.detach(), q.view_as(p))
                vals.append(float(U.sil_loss(v, f, args[0], args[1], K, lab, sigma, M=M, w=w)[0]))
            num[k] = (vals[0] - vals[1]) / (2 * eps)
        err = float((num - g.reshape(-1)).norm() / g.norm())
        worst = max(worst, err)
    # fp64 central differences with a 1e-6 step: truncation ~1e-12 relative, cancellation ~1e-16 / 1e-6 / |g|; a switch of the winning
    # face or segment inside the step would show as an error of order one
    assert worst < 1e-5, worst


def test_restatement_smoothness_from_moments_equals_the_direct_mean():
    g = torch.Generator().manual_seed(2)
    verts = torch.randn(57, 3, generator=g, dtype=F64) * 0.3 + 0.1
    rot6d = torch.randn(5, 3, 2, generator=g, dtype=F64).requires_grad_(True)
    trans = torch.randn(5, 3, generator=g, dtype=F64).requires_grad_(True)
    R, T = U.poses_of(rot6d, trans)
    a, b = U.smooth_direct(verts, R, T), U.smooth_moments(verts, R, T)
    assert abs(float(a.detach()) - float(b.detach())) <= 1e-12 * abs(float(a.detach()))
    ga, gb = torch.autograd.grad(a, (rot6d, trans), retain_graph=True), torch.autograd.grad(b, (rot6d, trans))
    for x, y in zip(ga, gb):
        assert float((x - y).norm()) <= 1e-12 * float(x.norm())


def test_restatement_recovers_perturbed_poses_on_a_small_scene():
    """4 frames of 96^2, the 288-face bent ellipsoid, a hand rectangle over the outline, poses off by 8 degrees about random axes and
    0.06-0.12 in translation; sigma 4 -> 1.5 over 60 iterations, lr 5e-3.  Measured here: mean IoU 0.776 -> 0.990 (min 0.720 -> 0.984),
    mean reprojection error of the vertices 4.92 -> 1.22 px (one frame keeps 4.2 px: a rotation its outline barely shows)."""
    sc = U.small_scene()
    v, f, K, lab = sc["verts"], sc["faces"], sc["K"], sc["label"]
    assert f.shape[0] <= 400 and lab.shape == (4, 96, 96) and int((lab == -1).sum()) > 0
    c0 = U.sil_terms(v, f, sc["R0"], sc["T0"], K, lab, 1.0)[2]
    rp0 = U.reprojection_error(v, sc["R0"], sc["T0"], sc["R_true"], sc["T_true"], K)
    R, T, curve = U.refine(v, f, sc["R0"], sc["T0"], K, lab, iters=60, lr=5e-3, sigma_px=4.0, sigma_end_px=1.5)
    c1 = U.sil_terms(v, f, R, T, K, lab, 1.0)[2]
    rp1 = U.reprojection_error(v, R, T, sc["R_true"], sc["T_true"], K)
    i0, i1 = U.iou(c0), U.iou(c1)
    print(f"restatement: IoU {i0.tolist()} -> {i1.tolist()}; reprojection {rp0.tolist()} -> {rp1.tolist()} px; "
          f"L_sil {curve[0][2]:.3e} -> {curve[-1][2]:.3e}")
    assert float(i1.mean()) > float(i0.mean()) + 0.1 and float(i1.min()) > float(i0.min())
    assert float(rp1.mean()) < 0.5 * float(rp0.mean())
    assert curve[-1][2] < 0.1 * curve[0][2]


# ------------------------------------------------------------------------------------------------------------ the C ABI
ENTRY_POINTS = ("dh_label_edt", "dh_sil_nearest", "dh_sil_nearest_workspace", "dh_sil_loss_grad", "dh_sil_loss_grad_workspace",
                "dh_sil_loss_sums")


def test_entry_points_are_declared_exported_and_bound():
    from dynhor_amd import _lib
    header = open(os.path.join(ROOT, "include", "dynhor_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ENTRY_POINTS:
        assert s + "(" in header and hasattr(raw, s) and s in _lib.SIGNATURES, s


def test_argument_validation_without_gpu(hiplib):
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    L = hiplib
    # dh_label_edt(label, n_frames, H, W, value, rmax, tmp, out, stream)
    assert L.dh_label_edt(null, 0, 4, 4, 1, 3, null, null, null) == 0                      # n_frames == 0: a no-op
    assert L.dh_label_edt(null, 2, 4, 4, 1, 3, null, null, null) == -1                     # null pointers
    assert L.dh_label_edt(some, 2, 4, 4, 1, 3, null, some, null) == -1
    assert L.dh_label_edt(some, -1, 4, 4, 1, 3, some, some, null) == -1
    assert L.dh_label_edt(some, 2, 0, 4, 1, 3, some, some, null) == -1
    assert L.dh_label_edt(some, 2, 4, 4, 1, -1, some, some, null) == -1
    assert L.dh_label_edt(some, 2, 4, 4, 300, 3, some, some, null) == -1
    assert L.dh_label_edt(some, 2, 4, 4, 1, 2897, some, some, null) == -2                   # 2 rmax^2 must stay below 2^24
    assert L.dh_label_edt(some, 1 << 30, 4, 4, 1, 3, some, some, null) == -2
    # dh_sil_nearest(verts, nv, faces, nf, R, T, K, n_frames, H, W, rmax_px, near, ws, stream)
    assert L.dh_sil_nearest_workspace(3, 33, 17) == (3 * 3 * 2 + 15) // 16 * 16 and L.dh_sil_nearest_workspace(-1, 4, 4) == -1
    assert L.dh_sil_nearest(null, 0, null, 0, null, null, null, 0, 8, 8, 2.0, null, null, null) == 0
    assert L.dh_sil_nearest(null, 5, null, 0, null, null, null, 3, 8, 8, 2.0, null, null, null) == 0          # no faces: a no-op
    assert L.dh_sil_nearest(null, 5, null, 4, null, null, null, 3, 8, 8, 2.0, null, null, null) == -1
    assert L.dh_sil_nearest(some, 5, some, 4, some, some, some, 3, 8, 8, 2.0, some, null, null) == -1         # ws is required
    assert L.dh_sil_nearest(some, 5, some, 4, some, some, some, 3, 8, 8, -1.0, some, some, null) == -1
    assert L.dh_sil_nearest(some, 5, some, 4, some, some, some, 3, 8, 8, float("nan"), some, some, null) == -1
    assert L.dh_sil_nearest(some, 5, some, 4, some, some, some, -3, 8, 8, 2.0, some, some, null) == -1
    assert L.dh_sil_nearest(some, 5, some, 4, some, some, some, 3, 0, 8, 2.0, some, some, null) == -1
    assert L.dh_sil_nearest(some, 5, some, 1 << 32, some, some, some, 3, 8, 8, 2.0, some, some, null) == -2
    # dh_sil_loss_grad(near, verts, nv, faces, nf, R, T, K, d2_obj, d2_hand, label, n_frames, H, W, sigma, cut, edge_offset, out, ws, stream)
    assert L.dh_sil_loss_sums() == 17
    assert L.dh_sil_loss_grad_workspace(3, 10, 10) == 3 * 1 * 17 * 8 and L.dh_sil_loss_grad_workspace(2, 1080, 1920) == 2 * 64 * 17 * 8
    assert L.dh_sil_loss_grad_workspace(2, 0, 4) == -1
    tail = lambda **k: (k.get("sigma", 2.0), k.get("cut", 3.0), k.get("off", 0.5), k.get("out", some), k.get("ws", some), null)
    head = (some, some, 5, some, 4, some, some, some, some, some, some)
    assert L.dh_sil_loss_grad(*([null] * 2 + [0, null, 0] + [null] * 6), 0, 8, 8, *tail(out=null, ws=null)) == 0   # n_frames == 0
    assert L.dh_sil_loss_grad(*([null] * 2 + [0, null, 0] + [null] * 6), 2, 8, 8, *tail()) == -1
    assert L.dh_sil_loss_grad(*head, 2, 8, 8, *tail(ws=null)) == -1
    assert L.dh_sil_loss_grad(*head, 2, 8, 8, *tail(ws=ctypes.c_void_p(4100))) == -1                           # misaligned workspace
    assert L.dh_sil_loss_grad(*head, 2, 8, 8, *tail(sigma=0.0)) == -1
    assert L.dh_sil_loss_grad(*head, 2, 8, 8, *tail(cut=float("nan"))) == -1
    assert L.dh_sil_loss_grad(*head, 2, 8, 8, *tail(off=-0.5)) == -1
    assert L.dh_sil_loss_grad(*head, -2, 8, 8, *tail()) == -1
    assert L.dh_sil_loss_grad(*head, 70000, 8, 8, *tail()) == -2


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from dynhor_amd import _lib, pose_sil
    lab = torch.zeros(1, 4, 4, dtype=torch.int8)
    with pytest.raises(_lib.DynhorHipError):
        pose_sil.label_edt(lab, 1, 2)
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    with pytest.raises(_lib.DynhorHipError):
        pose_sil.nearest_faces(v, f, torch.eye(3)[None], torch.zeros(1, 3), torch.eye(3), 4, 4, 2.0)
    with pytest.raises(_lib.DynhorHipError):
        pose_sil.silhouette_loss_grad(v, f, torch.zeros(1, 4, 4, dtype=torch.int64), torch.eye(3)[None], torch.zeros(1, 3), torch.eye(3),
                                      torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), lab, 2.0)
    with pytest.raises(_lib.DynhorHipError):
        pose_sil.SilhouettePoseOptimizer(v, f, lab, torch.eye(3)[None], torch.zeros(1, 3), torch.eye(3))


def test_frame_selection_and_schedule():
    from dynhor_amd.pose_sil import halo_radius, select_frames, sigma_at
    stems = ["a", "b", "c", "d"]
    iou = [0.9, 0.2, None, 0.5]
    assert select_frames(None, stems, iou) == [0, 1, 2, 3] and select_frames("all", stems, iou) == [0, 1, 2, 3]
    assert select_frames("worst:2", stems, iou) == [1, 3] and select_frames("worst:9", stems, iou) == [0, 1, 3]
    assert select_frames("d,a", stems, iou) == [0, 3] and select_frames([2, "b"], stems, iou) == [1, 2]
    for bad in ("worst:0", "worst:x", "nope", [7], ""):
        with pytest.raises(ValueError):
            select_frames(bad, stems, iou)
    assert sigma_at(0, 10, 8.0, 1.0) == 8.0 and abs(sigma_at(9, 10, 8.0, 1.0) - 1.0) < 1e-12 and sigma_at(0, 1, 8.0, 1.0) == 8.0
    assert abs(sigma_at(3, 7, 8.0, 1.0) / sigma_at(2, 7, 8.0, 1.0) - sigma_at(5, 7, 8.0, 1.0) / sigma_at(4, 7, 8.0, 1.0)) < 1e-12
    assert 3.0 * 2.0 < halo_radius(2.0, 3.0) < 3.0 * 2.0 * 1.01
    assert all(sigma_at(k, 9, 6.0, 1.5) == U.sigma_at(k, 9, 6.0, 1.5) for k in range(9))


# ------------------------------------------------------------------------------------------------------------ config, CLI, poses out
def test_config_block_defaults():
    import yaml
    from dynhor_amd.pose_sil import DEFAULTS
    from dynhor_amd.runner import DEFAULT_CONF, _merge
    assert set(DEFAULTS) == {"iters", "lr", "rot_lr_mult", "sigma_px", "sigma_end_px", "cut", "edge_offset_px", "lw_sil", "lw_smooth",
                             "resolution", "frame_chunk", "report_freq"}
    assert DEFAULTS["rot_lr_mult"] == 10.0 and DEFAULTS["cut"] == 3.0 and DEFAULTS["edge_offset_px"] == 0.5
    assert DEFAULTS["resolution"] == 128 and DEFAULTS["lw_smooth"] == 0.0 and DEFAULTS["sigma_end_px"] <= DEFAULTS["sigma_px"]
    assert DEFAULT_CONF["pose_sil"] == DEFAULTS
    conf = _merge(DEFAULT_CONF, yaml.safe_load(open(os.path.join(ROOT, "configs", "synthetic.yaml"))))
    assert conf["pose_sil"] == DEFAULTS
    over = _merge(DEFAULT_CONF, {"pose_sil": {"iters": 7}})
    assert over["pose_sil"]["iters"] == 7 and over["pose_sil"]["lr"] == DEFAULTS["lr"]


def test_cli_knows_the_new_modes_and_flags():
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--help"], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    for word in ("refine_poses", "export_poses", "--pose_frames", "--pose_dir", "--vis_mesh", "--mesh_resolution"):
        assert word in p.stdout, word
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", "x.yaml", "--mode", "refine_pose"], cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "invalid choice" in p.stderr


def _write_frames(root, stems, H, W, rng):
    from PIL import Image
    for sub in ("rgb", "sam_seg"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for s in stems:
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, "rgb", s + ".jpg"))
        m = np.zeros((H, W, 3), np.uint8)
        m[..., 1][rng.random((H, W)) > 0.6] = 255
        Image.fromarray(m).save(os.path.join(root, "sam_seg", s + ".png"))


@pytest.mark.parametrize("folder", ["obj_infos_ref", "obj_infos_scaled"])
def test_export_poses_round_trips_through_the_loader(tmp_path, folder):
    """Runner.export_poses needs nothing of a Runner but its dataset, directory and iteration: the poses of a tiny on-disk sequence
    (with and without obj_scale) are moved, exported and read back by Dataset._load_from_disk."""
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.runner import Runner
    src = os.path.join(GOLD, folder)
    stems = sorted(f[:-4] for f in os.listdir(src) if f.endswith(".npz") and not f.startswith("_"))
    root = str(tmp_path / "seq")
    _write_frames(root, stems, 16, 20, np.random.default_rng(3))
    ds = Dataset({"dataroot": root, "obj_infos": src}, device="cpu")
    scaled = folder == "obj_infos_scaled"
    assert (float(ds.obj_scale[0]) == 2.0) == scaled
    with torch.no_grad():                                               # poses that are not the ones on disk
        ds.T += torch.tensor([0.01, -0.02, 0.03])
        ds.R.copy_(ds.R @ U.axis_angle((0.2, 1.0, -0.3), 3.0).float())
    stub = SimpleNamespace(dataset=ds, base_exp_dir=str(tmp_path / "exp"), iter_step=42, rank=0, last_pose_dir=None)
    d = Runner.export_poses(stub)
    assert d == os.path.join(str(tmp_path / "exp"), "poses", "00000042", "obj_infos") and stub.last_pose_dir == d
    assert sorted(os.listdir(d)) == [s + ".npz" for s in stems]
    for k, s in enumerate(stems):
        z = np.load(os.path.join(d, s + ".npz"))
        assert sorted(z.files) == (["K", "R", "T", "obj_scale"] if scaled else ["K", "R", "T"])
        assert z["R"].shape == (3, 3) and z["T"].shape == (1, 3) and z["K"].shape == (3, 3)                 # run.py:172-176
        assert z["R"].dtype == z["T"].dtype == z["K"].dtype == np.float32
        if scaled:
            sk = float(ds.obj_scale[k])
            assert sk != 1.0 and float(z["obj_scale"]) == sk and np.allclose(z["T"][0], sk * ds.T[k].numpy(), atol=1e-6)
    back = Dataset._load_from_disk({"dataroot": root, "obj_infos": d})
    assert back["stems"] == stems
    assert np.allclose(back["R"].numpy(), ds.R.numpy(), atol=1e-6) and np.allclose(back["T"].numpy(), ds.T.numpy(), atol=1e-6)
    assert np.array_equal(back["K"].numpy(), ds.K.numpy()) and np.allclose(back["obj_scale"].numpy(), ds.obj_scale.numpy())
    d2 = Runner.export_poses(stub, str(tmp_path / "elsewhere"))
    assert d2 == str(tmp_path / "elsewhere") and len(os.listdir(d2)) == len(stems)
