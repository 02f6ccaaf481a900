"""The photometric pose term on the GPU: dh_image_blur and dh_photo_loss_grad against the fp64 restatement (tests/pose_photo_util.py,
licensed by tests/test_cpu_pose_photo.py), reproducibility across launches and frame splits, a step that reads nothing back, the
rotation of a textured sphere that no silhouette can recover, and the Runner / CLI round trip."""
import functools
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_texture_util as TU
from tests import pose_photo_util as U
from tests import pose_sil_util as SU
from tests.test_cpu_pose_photo import K30_FINAL_DEG_RECORDED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
SETTINGS = dict(depth_eps=0.01, min_cos=0.2, a_min=0.5, delta=0.1)


# ------------------------------------------------------------------------------------------------------------ blur
def _blur_input(F, H, W):
    from dynhor_amd.mesh_color import usable_map
    rgb = TU.smooth_noisy_frames(F, H, W, seed=F + H)
    label = torch.ones(F, H, W, dtype=torch.int8)
    label[:, :, 40:44] = -1                                # a hand band
    label[:, H // 3:H // 3 + 2, :] = 0
    label[:, :, W - 9:] = 0
    usable = usable_map(label.to(DEV), 1)
    assert torch.equal(usable.cpu(), TU.erode_object(label, 1))
    return rgb, usable.cpu()


@pytest.mark.parametrize("F,H,W", [(3, 64, 96), (1, 5, 70), (2, 33, 257)])
def test_blur_agrees_with_the_fp64_restatement_and_is_bitwise_reproducible(F, H, W):
    """Allowed: four times the deviation of the restatement run in float32 from the one in float64 on the same input (the rule of
    DESIGN_NEXT_ROWS.md section 18), for the colour and for a separately; the prints are what section 19 records."""
    from dynhor_amd.pose_photo import blur_frames
    rgb, usable = _blur_input(F, H, W)
    rgb_d, us_d = rgb.to(DEV), usable.to(DEV)
    for radius in (0, 1, 3, 12):
        sigma = radius / 3.0
        g, r = U.taps(sigma)
        assert r == radius
        want = U.blur(rgb, usable, g, torch.float64)
        w32 = U.blur(rgb, usable, g, torch.float32).double()
        got = blur_frames(rgb_d, us_d, sigma)
        assert got.shape == (F, H, W, 4) and got.dtype == torch.float32
        g64 = got.cpu().double()
        for name, sl in (("colour", slice(0, 3)), ("a", slice(3, 4))):
            allowed = 4.0 * float((w32[..., sl] - want[..., sl]).abs().max())
            err = float((g64[..., sl] - want[..., sl]).abs().max())
            print(f"blur {F}x{H}x{W} radius {radius} {name}: measured {err:.3e}, allowed {allowed:.3e}")
            assert err <= allowed, (radius, name, err, allowed)
        zero = want[..., 3] == 0
        assert torch.equal(g64[..., 3] == 0, zero) and float(g64[zero].abs().max() if bool(zero.any()) else 0.0) == 0.0
        if radius == 0:
            assert torch.equal(got.cpu(), torch.cat([rgb.float() / 255.0 * usable[..., None], usable[..., None].float()], -1))
        assert torch.equal(blur_frames(rgb_d, us_d, sigma), got)                                  # a second launch
        for chunk in sorted({1, 2, F}):
            parts = [blur_frames(rgb_d[s:s + chunk].contiguous(), us_d[s:s + chunk].contiguous(), sigma) for s in range(0, F, chunk)]
            assert torch.equal(torch.cat(parts), got), (radius, chunk)


# ------------------------------------------------------------------------------------------------------------ loss sums
@functools.lru_cache(maxsize=None)
def _loss_fixture():
    """The bake scene on the device, its own z-buffer, its frames blurred by the kernel at radius 0 and 3, and 4,001 clear points of
    the mesh with the restatement's sums (computed once, on the CPU, from the device's z-buffer and blur)."""
    from dynhor_amd.mesh_color import raster_depth, usable_map
    from dynhor_amd.pose_photo import blur_frames, surface_points
    verts, faces, ds = TU.bake_scene()
    g = torch.Generator().manual_seed(5)
    pts, nrm, _ = surface_points(verts, faces, 4200, 17, vertex_colors=torch.rand(verts.shape[0], 3, generator=g))
    col = torch.rand(4200, 3, generator=g)
    zbuf = raster_depth(verts.to(DEV), faces.to(DEV), ds.R.to(DEV), ds.T.to(DEV), ds.K.to(DEV), ds.H, ds.W)
    usable = usable_map(ds.label.to(DEV), 1)
    imgs = {r: blur_frames(ds.rgb.to(DEV), usable, r / 3.0) for r in (0, 3)}
    zc = zbuf.cpu()
    amb = torch.zeros(4200, dtype=torch.bool)
    for r in (0, 3):
        amb |= U.ambiguous(pts, nrm, imgs[r].cpu(), zc, ds.R, ds.T, ds.K, SETTINGS["depth_eps"], SETTINGS["min_cos"], SETTINGS["a_min"])
    share = float(amb.double().mean())
    print(f"loss fixture: {int(amb.sum())} of 4200 points ambiguous ({100 * share:.3f} %)")
    assert share < U.AMBIGUOUS_CAP
    keep = (~amb).nonzero().reshape(-1)[:4001]
    assert keep.shape[0] == 4001
    pts, nrm, col = pts[keep].contiguous(), nrm[keep].contiguous(), col[keep].contiguous()
    return SimpleNamespace(ds=ds, pts=pts, nrm=nrm, col=col, zbuf=zbuf, zc=zc, imgs=imgs,
                           dev=[t.to(DEV) for t in (pts, nrm, col)], cams=[t.to(DEV) for t in (ds.R, ds.T, ds.K)])


@pytest.mark.parametrize("radius", [0, 3])
@pytest.mark.parametrize("n", [1, 63, 257, 4001])
def test_loss_sums_and_gradient_agree_with_the_fp64_restatement(n, radius):
    """Counts equal; every float sum within 1e-9 of the sum of |terms| of that sum (both sides add at most 2e4 fp64 terms built from the
    same fp32 inputs: N 2^-53 ~ 2e-12, three decades left for the device's sqrt and divide)."""
    from dynhor_amd.pose_photo import photo_sums
    fx = _loss_fixture()
    ds = fx.ds
    want, absum = U.all_sums(fx.pts[:n], fx.nrm[:n], fx.col[:n], fx.imgs[radius].cpu(), fx.zc, ds.R, ds.T, ds.K, **SETTINGS)
    p, nr, c = (t[:n].contiguous() for t in fx.dev)
    R, T, K = fx.cams
    got = photo_sums(p, nr, c, fx.imgs[radius], fx.zbuf, R, T, K, **SETTINGS)
    assert got.shape == (5, 16) and got.dtype == torch.float64
    gc = got.cpu()
    print(f"photo sums n {n} radius {radius}: pairs {[int(x) for x in gc[:, 14]]} inliers {[int(x) for x in gc[:, 15]]}, worst "
          f"|got - want| / sum |terms| {float(((gc[:, :14] - want[:, :14]).abs() / absum.clamp(min=1e-300)).max()):.3e}")
    assert torch.equal(gc[:, 14:], want[:, 14:])
    assert bool(((gc[:, :14] - want[:, :14]).abs() <= 1e-9 * absum).all())
    if n == 4001:
        assert int(gc[:4, 14].min()) > 0 and float(gc[:4, 2:14].abs().sum(1).min()) > 0    # (the camera inside sees back faces only)
        assert int((gc[:, 14] < n).sum()) == 5                                            # and every frame drops some
    assert torch.equal(photo_sums(p, nr, c, fx.imgs[radius], fx.zbuf, R, T, K, **SETTINGS), got)           # a second launch
    for chunk in (1, 2, 5):
        parts = [photo_sums(p, nr, c, fx.imgs[radius][s:s + chunk].contiguous(), fx.zbuf[s:s + chunk].contiguous(),
                            R[s:s + chunk].contiguous(), T[s:s + chunk].contiguous(), K, **SETTINGS) for s in range(0, 5, chunk)]
        assert torch.equal(torch.cat(parts), got), chunk


def test_no_points_zero_the_sums():
    from dynhor_amd.pose_photo import photo_sums
    fx = _loss_fixture()
    R, T, K = fx.cams
    e = torch.zeros(0, 3, device=DEV)
    got = photo_sums(e, e, e, fx.imgs[0], fx.zbuf, R, T, K, **SETTINGS)
    assert got.shape == (5, 16) and float(got.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ the step
def test_step_with_the_term_reads_nothing_back_to_the_host():
    from dynhor_amd.mesh_color import usable_map
    from dynhor_amd.pose_photo import PhotometricTerm, surface_points
    from dynhor_amd.pose_sil import SilhouettePoseOptimizer
    sc = SU.small_scene()
    f32 = lambda t: t.to(DEV, torch.float32).contiguous()
    verts, faces, label = f32(sc["verts"]), sc["faces"].to(DEV), sc["label"].to(DEV)
    g = torch.Generator().manual_seed(1)
    pts, nrm, col = surface_points(verts, faces, 1000, 3, vertex_colors=torch.rand(verts.shape[0], 3, generator=g).to(DEV))
    rgb = TU.smooth_noisy_frames(4, sc["H"], sc["W"], seed=8, device=DEV)
    term = PhotometricTerm(pts, nrm, col, rgb, usable_map(label, 1), levels=(1.0, 0.0))
    opt = SilhouettePoseOptimizer(verts, faces, label, f32(sc["R0"]), f32(sc["T0"]), f32(sc["K"]), sigma_px=4.0, lw_smooth=0.1,
                                  frame_chunk=3, photo=term, lw_photo=1.0)
    term.set_level(1.0)
    opt.step(4.0)                                                       # first use: library load, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step(4.0)
        opt.step(3.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    st = opt.stats()
    assert st["iter"] == 3 and np.isfinite(st["loss"]) and np.isfinite(st["loss_photo"]) and st["loss_photo"] > 0
    assert len(st["photo_pairs"]) == 4 and min(st["photo_pairs"]) > 0 and 0.0 <= st["photo_inliers"] <= 1.0
    # without the term the step's arithmetic is what it was: the same poses as an optimiser that never heard of it
    a = SilhouettePoseOptimizer(verts, faces, label, f32(sc["R0"]), f32(sc["T0"]), f32(sc["K"]), sigma_px=4.0, lw_smooth=0.1)
    b = SilhouettePoseOptimizer(verts, faces, label, f32(sc["R0"]), f32(sc["T0"]), f32(sc["K"]), sigma_px=4.0, lw_smooth=0.1, photo=None,
                                lw_photo=3.0)
    for s in (4.0, 3.0):
        a.step(s); b.step(s)
    assert torch.equal(a.rot6d, b.rot6d) and torch.equal(a.trans, b.trans) and "loss_photo" not in a.stats()


# ------------------------------------------------------------------------------------------------------------ what a silhouette cannot do
def test_the_term_recovers_a_rotation_the_outline_of_a_sphere_does_not_show():
    """The k = 30 sphere scene (5 frames of 96 x 128, every rotation 10 degrees off), the N = 20 marching-cubes sphere as the mesh,
    4,000 points with their analytic colours, levels (4, 2, 1, 0), 160 iterations at the default lw_photo.
    (a) with the term every frame ends within twice the restatement's largest final angle (tests/test_cpu_pose_photo.py);
    (b) without it, from the same start, every frame keeps at least half of its 10 degrees;
    (c) the mean silhouette IoU with the term is not lower than without it by more than 0.0057 (DESIGN_NEXT_ROWS.md section 13).

    Measured on an MI355X at the default lw_photo = 0.25 (DESIGN_NEXT_ROWS.md section 19): (a) final angles 0.150, 0.085, 0.157, 0.272,
    0.195 degrees against the bound 2 x 0.2737 = 0.547; (b) without the term the frames end 7.9 to 29.2 degrees off; (c) IoU 0.9967
    with, 0.9887 without.  The last iterate of Adam at a constant rate jitters (in the CPU restatement the largest angle moves between
    0.27 and 0.48 degrees over the last eleven iterations), and at lw_photo = 1 this run ends at 0.593 degrees and misses (a)."""
    from dynhor_amd.pose_photo import DEFAULTS, PhotometricTerm
    from dynhor_amd.pose_sil import refine_poses
    sc = U.photo_scene(30, 10.0)
    verts, faces = TU.sphere_mesh((0.0, 0.0, 0.0), TU.SPHERE_R, N=20)
    verts, faces = verts.to(DEV), faces.to(DEV)
    f32 = lambda t: t.to(DEV, torch.float32).contiguous()
    rgb, label = sc["rgb"].to(DEV), sc["label"].to(DEV)

    def dataset():
        return SimpleNamespace(label=label, rgb=rgb, R=f32(sc["R0"]), T=f32(sc["T0"]), K=f32(sc["K"]), H=sc["H"], W=sc["W"], n_images=5,
                               stems=None)
    out = {}
    for with_term in (True, False):
        ds = dataset()
        term = PhotometricTerm(f32(sc["pts"]), f32(sc["normals"]), f32(sc["colors"]), rgb, sc["usable"].to(DEV),
                               levels=(4.0, 2.0, 1.0, 0.0)) if with_term else None
        torch.cuda.synchronize()
        t0 = time.time()
        res = refine_poses(verts, faces, ds, iters=160, lr=5e-3, photo=term)
        torch.cuda.synchronize()
        ang = U.angles_deg(ds.R.cpu(), sc["R_true"])
        out[with_term] = (ang, res["iou_mean_after"])
        print(f"sphere k = 30, term {with_term}: {time.time() - t0:.2f} s wall; final angles {[round(float(a), 4) for a in ang]} deg "
              f"(restatement's largest {K30_FINAL_DEG_RECORDED}), |dT| {[round(float(x), 4) for x in (ds.T.cpu().double() - sc['T_true']).norm(dim=1)]}, "
              f"IoU {res['iou_mean_before']:.4f} -> {res['iou_mean_after']:.4f}"
              + (f", pairs {res['photo_pairs']}, lw_photo {res['settings']['photo']['lw_photo']}, loss_photo "
                 f"{[round(c['loss_photo'], 5) for c in res['curve']]}" if with_term else ""))
        if with_term:
            assert res["settings"]["photo"]["lw_photo"] == DEFAULTS["lw_photo"] and min(res["photo_pairs"]) > 500
            assert [c["blur_sigma"] for c in res["curve"]][0] == 4.0 and res["curve"][-1]["blur_sigma"] == 0.0
    assert float(out[True][0].max()) <= 2.0 * K30_FINAL_DEG_RECORDED, out[True][0]
    assert float(out[False][0].min()) >= 5.0, out[False][0]
    assert out[True][1] >= out[False][1] - 0.0057, (out[True][1], out[False][1])


# ------------------------------------------------------------------------------------------------------------ Runner, CLI
def test_cli_refines_with_the_term_and_none_changes_nothing(tmp_path):
    import yaml
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.scene import make_sequence
    from tests.test_gpu_pose_sil import _write_sequence
    conf = {"seq_name": "pphoto", "exp_name": "cli",
            "data_info": {"synthetic": {"n_frames": 8, "H": 96, "W": 96, "seed": 5}},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 3, "val_freq": 0, "end_iter": 100},
            "pose_sil": {"iters": 20, "sigma_px": 3.0, "sigma_end_px": 1.5, "report_freq": 5, "resolution": 48},
            "pose_photo": {"points": 4000}}
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--exp_root", str(tmp_path)] + list(a),
                                    cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    p = run("--mode", "train", "--iters", "3")
    assert p.returncode == 0, p.stderr[-3000:]
    stems = ["{:04d}".format(i) for i in range(8)]

    def refine(*flags):
        p = run("--mode", "refine_poses", "--is_continue", *flags)
        assert p.returncode == 0, p.stderr[-3000:]
        res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
        d = res["dir"]
        files = {}                                           # the arrays' bytes (an .npz carries the time it was written)
        for s in stems:
            z = np.load(os.path.join(d, "obj_infos", s + ".npz"))
            files[s] = [(k, str(z[k].dtype), z[k].shape, z[k].tobytes()) for k in sorted(z.files)]
        return res, open(os.path.join(d, "refine.json"), "rb").read(), files

    res, js_bytes, files = refine("--pose_photo", "views")
    js = json.loads(js_bytes)
    assert js["photo"] == "views" and js["settings"]["photo"]["points"] == 4000 and js["settings"]["iters"] == 20
    assert len(js["curve"]) >= 4 and all("loss_photo" in c and np.isfinite(c["loss_photo"]) for c in js["curve"])
    assert len(js["photo_pairs"]) == 8 and min(js["photo_pairs"]) > 0, js["photo_pairs"]
    from dynhor_amd.tb_events import read_scalars
    board = os.path.join(os.path.dirname(os.path.dirname(res["dir"])), "board")
    tags = {tag for fn in os.listdir(board) for _, tag, _ in read_scalars(os.path.join(board, fn))}
    assert "pose/loss_photo" in tags and "pose_sil/loss_sil" in tags, tags
    # the poses round-trip through a Dataset
    root = str(tmp_path / "seq")
    _write_sequence(root, make_sequence(8, 96, 96, 5, device="cpu"), stems)
    ds = Dataset({"dataroot": root, "obj_infos": os.path.join(res["dir"], "obj_infos")}, device=DEV)
    for k, s in enumerate(stems):
        z = np.load(os.path.join(res["dir"], "obj_infos", s + ".npz"))
        assert np.allclose(ds.R[k].cpu().numpy(), z["R"], atol=1e-6) and np.allclose(ds.T[k].cpu().numpy(), z["T"][0], atol=1e-6)
    # "none" is a run without the flag, bit for bit
    _, js_none, files_none = refine("--pose_photo", "none")
    _, js_plain, files_plain = refine()
    assert js_none == js_plain and files_none == files_plain
    assert b"photo" not in js_plain and files_plain != files
