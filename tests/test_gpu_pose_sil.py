"""Silhouette pose refinement on the GPU: the distance transform against a brute-force window search, the nearest-face buffer against
raster_depth's coverage and the fp64 restatement (tests/pose_sil_util.py; a coarse mesh with faces larger than 32 px and a fine one
with sub-pixel faces), the loss sums and pose gradient against the restatement's autograd, the counts against mesh_vis.shade,
reproducibility across launches and frame chunkings, recovery of perturbed poses on the synthetic sequence, frame selection, the
smoothness term, and the Runner / CLI round trip through obj_infos/*.npz."""
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pose_sil_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _dev(sc):
    """The small scene's tensors as the kernels take them (float32 / int64 / int8 on the device)."""
    f32 = lambda t: t.to(DEV, torch.float32).contiguous()
    return SimpleNamespace(verts=f32(sc["verts"]), faces=sc["faces"].to(DEV).contiguous(), K=f32(sc["K"]), label=sc["label"].to(DEV),
                           R0=f32(sc["R0"]), T0=f32(sc["T0"]), R_true=f32(sc["R_true"]), T_true=f32(sc["T_true"]), H=sc["H"], W=sc["W"])


def _d2(near):
    """float32 d2 of a nearest_faces buffer (inf where empty)."""
    d = (near >> 32).to(torch.int32).view(torch.float32)
    return torch.where(near == -1, torch.full_like(d, float("inf")), d)


# ------------------------------------------------------------------------------------------------------------ distance transform
@pytest.mark.parametrize("rmax", [0, 1, 25])
def test_label_edt_equals_the_brute_force_window_search(rmax):
    from dynhor_amd.pose_sil import label_edt
    g = torch.Generator().manual_seed(5)
    F, H, W = 4, 37, 53
    lab = torch.zeros(F, H, W, dtype=torch.int8)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for f in range(F - 1):                                              # the last frame has neither object nor hand
        cx, cy = 10 + 30 * float(torch.rand((), generator=g)), 8 + 20 * float(torch.rand((), generator=g))
        lab[f][((xx - cx) / 9.0) ** 2 + ((yy - cy) / 6.0) ** 2 < 1.0] = 1
        lab[f][(xx > cx + 4) & (xx < cx + 15) & (yy > cy - 3) & (yy < cy + 2) & (lab[f] == 0)] = -1
        lab[f][torch.rand(H, W, generator=g) < 0.002] = 1               # isolated pixels
    lab[1, 0, 0] = 1
    lab[1, H - 1, W - 1] = -1
    for value in (1, -1):
        got = label_edt(lab.to(DEV), value, rmax).cpu()
        want = U.edt_window(lab, value, rmax)
        assert got.dtype == torch.float32 and torch.equal(got, want), (value, rmax, (got != want).sum())
        assert torch.isinf(got[F - 1]).all()
        # every result <= rmax^2 is the image's exact distance transform
        exact = U.edt_exact(lab, value).to(torch.float32)
        near = got <= rmax * rmax
        assert torch.equal(got[near], exact[near]) and bool((exact[~near] > rmax * rmax).all())


# ------------------------------------------------------------------------------------------------------------ nearest faces
def _nearest_case(kind):
    if kind == "coarse":                                                # 36 faces over a 256^2 image: wider than the 32 px of the per-lane path
        sc = U.small_scene(n_frames=16, H=256, W=256, seed=4, n_lat=4, n_lon=6, hand=False)
    else:                                                               # 5,616 faces over ~1,200 pixels: sub-pixel faces
        sc = U.small_scene(n_frames=16, H=64, W=64, seed=4, n_lat=40, n_lon=72, hand=False)
    return sc, _dev(sc)


# measured on MI355X: the largest |d2_fp32 - d2_fp64| / (1 + sqrt(d2_fp64)) over the uncovered pixels within rmax_px, three frames of
# each case: coarse 2.026e-05, fine 7.735e-06 (the reported face's own fp64 distance exceeds the fp64 minimum by at most 5.5e-07 on the
# same scale); the tolerance is 4 x the larger one
NEAREST_MEASURED = (2.026e-05, 7.735e-06)
NEAREST_TOL = 4 * max(NEAREST_MEASURED)


@pytest.mark.parametrize("kind", ["coarse", "fine"])
def test_nearest_faces_against_coverage_and_the_restatement(kind):
    from dynhor_amd.mesh_color import raster_depth
    from dynhor_amd.pose_sil import nearest_faces
    sc, d = _nearest_case(kind)
    rmax = 12.0
    R, T = d.R0, d.T0
    near = nearest_faces(d.verts, d.faces, R, T, d.K, d.H, d.W, rmax)
    assert near.dtype == torch.int64 and near.shape == (16, d.H, d.W)
    assert torch.equal(near, nearest_faces(d.verts, d.faces, R, T, d.K, d.H, d.W, rmax))          # a second launch
    for chunk in (1, 5, 16):
        parts = [nearest_faces(d.verts, d.faces, R[s:s + chunk].contiguous(), T[s:s + chunk].contiguous(), d.K, d.H, d.W, rmax)
                 for s in range(0, 16, chunk)]
        assert torch.equal(torch.cat(parts), near), chunk
    zbuf = raster_depth(d.verts, d.faces, R, T, d.K, d.H, d.W)
    covered = zbuf != -1
    assert torch.equal(((near >> 32) == 0) & (near != -1), covered)
    assert int(covered.sum()) > 0 and int((~covered & (near != -1)).sum()) > 0
    uv0 = U.project(sc["verts"], sc["R0"][0], sc["T0"][0], sc["K"])[0][sc["faces"]]                 # [nf,3,2]
    extent = float((uv0.max(dim=1).values - uv0.min(dim=1).values).max(dim=1).values.max())
    assert extent > 40.0 if kind == "coarse" else extent < 3.0, extent
    d2_gpu = _d2(near).cpu().double()
    face_gpu = (near & 0xFFFFFFFF).cpu()
    v64, K64 = d.verts.cpu().double(), d.K.cpu().double()
    worst = 0.0
    for f in range(3):
        R64, T64 = R[f].cpu().double(), T[f].cpu().double()
        d2, _ = U.nearest(v64, sc["faces"], R64, T64, K64, d.H, d.W)
        unc = ~covered[f].cpu()
        inside = unc & (d2 <= (rmax - 0.01) ** 2) & (d2 > 0)
        outside = unc & (d2 > (rmax + 0.01) ** 2)
        assert bool(torch.isfinite(d2_gpu[f][inside]).all()) and bool(torch.isinf(d2_gpu[f][outside]).all())
        err = (d2_gpu[f][inside] - d2[inside]).abs() / (1.0 + d2[inside].sqrt())
        worst = max(worst, float(err.max()))
        # the reported face attains the fp64 minimum within the tolerance
        uv, _ = U.project(v64, R64, T64, K64)
        tri = uv[sc["faces"][face_gpu[f][inside]]]
        p = U.pixel_grid(d.H, d.W)[inside.reshape(-1)]
        own = torch.stack([U.seg_d2(tri[:, 0], tri[:, 1], p), U.seg_d2(tri[:, 1], tri[:, 2], p), U.seg_d2(tri[:, 2], tri[:, 0], p)],
                          -1).min(dim=-1).values
        slack = (own - d2[inside]) / (1.0 + d2[inside].sqrt())
        print(f"nearest_faces {kind} frame {f}: {int(inside.sum())} band pixels, worst |d2 error| / (1 + d) = {float(err.max()):.3e}, "
              f"worst face slack {float(slack.max()):.3e}")
        assert float(err.max()) <= NEAREST_TOL and float(slack.max()) <= NEAREST_TOL
    print(f"nearest_faces {kind}: worst over the frames {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------ loss and gradient
# measured on MI355X (4 frames of 96^2, the 288-face bent ellipsoid, poses off by 8 degrees / 0.06-0.12), at sigma 4 and 1.5: the largest
# |numerator error| / numerator 1.227e-10 and the largest |gradient error| / |frame gradient| 3.823e-07, both in the one frame where
# a pixel's fp32 search and the fp64 search pick different faces at nearly the same distance (the other seven stay below 1e-15); the
# tolerances are 4 x those
LOSS_MEASURED = (1.227e-10, 3.823e-07)
LOSS_NUM_TOL = 4 * LOSS_MEASURED[0]
LOSS_GRAD_TOL = 4 * LOSS_MEASURED[1]


def test_loss_sums_and_gradient_against_the_restatement():
    from dynhor_amd.mesh_color import raster_depth
    from dynhor_amd.mesh_vis import shade
    from dynhor_amd.pose_sil import halo_radius, label_edt, nearest_faces, silhouette_loss_grad
    sc = U.small_scene()
    d = _dev(sc)
    cut, delta = 3.0, 0.5
    v64, K64 = d.verts.cpu().double(), d.K.cpu().double()
    worst_num, worst_grad = 0.0, 0.0
    for sigma in (4.0, 1.5):
        rmax = int(math.ceil(cut * sigma + delta)) + 1
        d2o, d2h = label_edt(d.label, 1, rmax), label_edt(d.label, -1, rmax)
        near = nearest_faces(d.verts, d.faces, d.R0, d.T0, d.K, d.H, d.W, halo_radius(sigma, cut))
        num, wt, dR, dT, counts = silhouette_loss_grad(d.verts, d.faces, near, d.R0, d.T0, d.K, d2o, d2h, d.label, sigma, cut, delta)
        assert num.dtype == torch.float64 and counts.dtype == torch.int64 and dR.shape == (4, 3, 3) and dT.shape == (4, 3)
        # bitwise the same from a second launch and frame by frame
        again = silhouette_loss_grad(d.verts, d.faces, near, d.R0, d.T0, d.K, d2o, d2h, d.label, sigma, cut, delta)
        assert all(torch.equal(a, b) for a, b in zip((num, wt, dR, dT, counts), again))
        for f in range(4):
            one = silhouette_loss_grad(d.verts, d.faces, near[f:f + 1].contiguous(), d.R0[f:f + 1].contiguous(),
                                       d.T0[f:f + 1].contiguous(), d.K, d2o[f:f + 1].contiguous(), d2h[f:f + 1].contiguous(),
                                       d.label[f:f + 1].contiguous(), sigma, cut, delta)
            assert all(torch.equal(a[0], b[f]) for a, b in zip(one, (num, wt, dR, dT, counts))), f
        # the counts are mesh_vis.shade's
        zbuf = raster_depth(d.verts, d.faces, d.R0, d.T0, d.K, d.H, d.W)
        assert torch.equal(counts, shade(d.verts, d.faces, zbuf, d.R0, d.T0, d.K, label=d.label)[1])
        # the restatement's autograd, on the same fp32 inputs
        R64 = d.R0.cpu().double().requires_grad_(True)
        T64 = d.T0.cpu().double().requires_grad_(True)
        rnum, rwt, rcounts = U.sil_terms(v64, sc["faces"], R64, T64, K64, sc["label"], sigma, cut, delta)
        assert torch.equal(wt.cpu(), rwt) and torch.equal(counts.cpu(), rcounts)
        for f in range(4):
            gR, gT = torch.autograd.grad(rnum[f], (R64, T64), retain_graph=True)
            want = torch.cat([gR[f].reshape(-1), gT[f].reshape(-1)])
            got = torch.cat([dR[f].reshape(-1), dT[f].reshape(-1)]).cpu()
            e_num = abs(float(num[f]) - float(rnum[f].detach())) / float(rnum[f].detach())
            e_grad = float((got - want).norm() / want.norm())
            print(f"silhouette_loss_grad sigma {sigma} frame {f}: numerator {float(num[f]):.6f} (restatement {float(rnum[f]):.6f}, "
                  f"rel {e_num:.3e}), weight {int(wt[f])}, |gradient| {float(want.norm()):.4e}, gradient rel {e_grad:.3e}")
            worst_num, worst_grad = max(worst_num, e_num), max(worst_grad, e_grad)
            assert float(want.norm()) > 0
    print(f"silhouette_loss_grad: worst numerator rel {worst_num:.3e}, worst gradient rel {worst_grad:.3e}")
    assert worst_num <= LOSS_NUM_TOL and worst_grad <= LOSS_GRAD_TOL


def test_loss_sums_are_bitwise_the_same_for_every_frame_chunking():
    from dynhor_amd.pose_sil import halo_radius, label_edt, nearest_faces, silhouette_loss_grad
    d = _dev(U.small_scene(n_frames=16, H=61, W=75, seed=6, n_lat=6, n_lon=10))
    sigma, cut, delta = 3.0, 3.0, 0.5
    d2o, d2h = label_edt(d.label, 1, 11), label_edt(d.label, -1, 11)
    near = nearest_faces(d.verts, d.faces, d.R0, d.T0, d.K, d.H, d.W, halo_radius(sigma, cut))
    whole = silhouette_loss_grad(d.verts, d.faces, near, d.R0, d.T0, d.K, d2o, d2h, d.label, sigma, cut, delta)
    assert float(whole[0].min()) > 0 and float(whole[2].abs().sum(dim=(1, 2)).min()) > 0
    for chunk in (1, 5, 16):
        parts = [silhouette_loss_grad(d.verts, d.faces, near[s:s + chunk].contiguous(), d.R0[s:s + chunk].contiguous(),
                                      d.T0[s:s + chunk].contiguous(), d.K, d2o[s:s + chunk].contiguous(), d2h[s:s + chunk].contiguous(),
                                      d.label[s:s + chunk].contiguous(), sigma, cut, delta) for s in range(0, 16, chunk)]
        for k in range(5):
            assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), (chunk, k)


def test_step_reads_nothing_back_to_the_host():
    from dynhor_amd.pose_sil import SilhouettePoseOptimizer
    d = _dev(U.small_scene())
    opt = SilhouettePoseOptimizer(d.verts, d.faces, d.label, d.R0, d.T0, d.K, sigma_px=4.0, lw_smooth=0.1, frame_chunk=3)
    opt.step(4.0)                                                       # first use: library load, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step(4.0)
        opt.step(3.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    st = opt.stats()
    assert st["iter"] == 3 and math.isfinite(st["loss"]) and 0.0 < st["iou_mean"] <= 1.0


# ------------------------------------------------------------------------------------------------------------ end to end
# Margins (ISSUE "numbers"): the fp64 restatement on a reduced copy of this test (4 frames of 96^2 of the same synthetic sequence, the
# analytic scene mesh at resolution 24, one frame shifted by 0.1 and one rotated by 10 degrees, sigma 3 -> 1.5, 60 iterations, lr 5e-3)
# took the shifted frame's IoU 0.658 -> 0.968 and the rotated one's 0.895 -> 0.982 (true poses: 0.994, 0.983) and left every frame, the
# two unperturbed ones included, within E2E_SHORTFALL = 0.0278 of its IoU at the true pose (mean reprojection error of the perturbed
# frames 5.46 / 1.71 -> 2.05 / 0.59 px); the margin is twice that (one factor for fp32, one for the larger images).
E2E_SHORTFALL = 0.0278
E2E_MARGIN = 2 * E2E_SHORTFALL
E2E = dict(iters=120, lr=5e-3, sigma_px=6.0, sigma_end_px=1.5)          # cut sigma = 18 px > the 12-15 px of the shifts
SHIFTED, ROTATED = (3, 11), (6, 14)


def _perturbed_synthetic():
    from dynhor_amd.dataset import Dataset
    ds = Dataset.from_synthetic(n_frames=16, H=256, W=256, seed=21, device=DEV, hand=True)
    R_true, T_true = ds.R.clone(), ds.T.clone()
    for f in SHIFTED:
        ds.T[f, 0] += 0.1
    for k, f in enumerate(ROTATED):
        dR = U.axis_angle((0.3, 1.0, 0.5) if k == 0 else (1.0, -0.4, 0.2), 10.0).to(DEV, torch.float32)
        ds.R[f] = ds.R[f] @ dR
    return ds, R_true, T_true


def _score(verts, faces, ds):
    from dynhor_amd.mesh_vis import overlay_frames
    c = overlay_frames(verts, faces, ds).cpu().double()
    return c[:, 0] / c.sum(dim=1)


def test_refine_poses_recovers_perturbed_frames_of_the_synthetic_sequence():
    from dynhor_amd.pose_sil import refine_poses
    from dynhor_amd.runner import Runner
    stub = SimpleNamespace(device=DEV)
    score_mesh = Runner._scene_gt_mesh(stub, 256)
    refine_mesh = Runner._scene_gt_mesh(stub, 64)
    ds, R_true, T_true = _perturbed_synthetic()
    R_bad, T_bad = ds.R.clone(), ds.T.clone()
    bad = _score(*score_mesh, ds)
    ds.R.copy_(R_true); ds.T.copy_(T_true)
    good = _score(*score_mesh, ds)
    ds.R.copy_(R_bad); ds.T.copy_(T_bad)
    torch.cuda.synchronize()
    import time
    t0 = time.time()
    res = refine_poses(*refine_mesh, ds, **E2E)
    torch.cuda.synchronize()
    wall = time.time() - t0
    after = _score(*score_mesh, ds)
    assert torch.equal(ds.R, res["R"]) and torch.equal(ds.T, res["T"])
    v64 = refine_mesh[0].cpu().double()
    rp0 = U.reprojection_error(v64, R_bad.cpu().double(), T_bad.cpu().double(), R_true.cpu().double(), T_true.cpu().double(),
                               ds.K.cpu().double())
    rp1 = U.reprojection_error(v64, ds.R.cpu().double(), ds.T.cpu().double(), R_true.cpu().double(), T_true.cpu().double(),
                               ds.K.cpu().double())
    pert = SHIFTED + ROTATED
    print(f"refine_poses 16 x 256^2, {refine_mesh[1].shape[0]} faces, {E2E}: {wall:.2f} s wall; IoU (scene mesh at 256) of the perturbed "
          f"frames {pert}: true {[round(float(good[f]), 4) for f in pert]} perturbed {[round(float(bad[f]), 4) for f in pert]} refined "
          f"{[round(float(after[f]), 4) for f in pert]}; largest drop of any frame {float((good - after).max()):.4f}; mean reprojection "
          f"error {float(rp0.mean()):.3f} -> {float(rp1.mean()):.3f} px (perturbed frames {[round(float(rp0[f]), 2) for f in pert]} -> "
          f"{[round(float(rp1[f]), 2) for f in pert]}); loss curve {[round(c['loss_sil'], 6) for c in res['curve']]}")
    for f in range(16):
        assert float(after[f]) >= float(good[f]) - E2E_MARGIN, (f, float(good[f]), float(after[f]))
    for f in pert:
        assert float(after[f]) - float(bad[f]) >= 0.5 * (float(good[f]) - float(bad[f])), (f, float(good[f]), float(bad[f]), float(after[f]))
    assert float(rp1.mean()) < float(rp0.mean())
    assert res["iou_mean_after"] > res["iou_mean_before"] and len(res["iou_before"]) == 16 and res["frames"] == list(range(16))
    # the same run again: the same bits
    ds.R.copy_(R_bad); ds.T.copy_(T_bad)
    res2 = refine_poses(*refine_mesh, ds, **E2E)
    assert torch.equal(res2["R"], res["R"]) and torch.equal(res2["T"], res["T"])


def test_worst_frames_selection_moves_only_those_frames():
    from dynhor_amd.pose_sil import refine_poses
    from dynhor_amd.runner import Runner
    mesh = Runner._scene_gt_mesh(SimpleNamespace(device=DEV), 64)
    ds, _, _ = _perturbed_synthetic()
    R_bad, T_bad = ds.R.clone(), ds.T.clone()
    res = refine_poses(*mesh, ds, iters=20, lr=5e-3, sigma_px=6.0, sigma_end_px=3.0, frames="worst:2", lw_smooth=0.05)
    assert sorted(res["frames"]) == sorted(SHIFTED), res["frames"]         # a 0.1 shift costs far more IoU than a 10 degree turn
    others = [f for f in range(16) if f not in SHIFTED]
    assert torch.equal(ds.R[others], R_bad[others]) and torch.equal(ds.T[others], T_bad[others])
    for f in SHIFTED:
        assert not torch.equal(ds.T[f], T_bad[f])
        assert res["iou_after"][f] > res["iou_before"][f]
    with pytest.raises(ValueError):
        refine_poses(*mesh, ds, iters=1, frames="worst:0")
    with pytest.raises(ValueError):
        refine_poses(*mesh, ds, iters=1, frames="no_such_frame")


def test_smoothness_weight_lowers_the_smoothness_term():
    from dynhor_amd.pose_sil import refine_poses
    d = _dev(U.small_scene(n_frames=4, seed=9, rot_deg=4.0, shift=(0.03, 0.06)))       # per-frame jitter about a smooth arc
    out = {}
    for lw in (0.0, 1.0):
        ds = SimpleNamespace(label=d.label, R=d.R0.clone(), T=d.T0.clone(), K=d.K, H=d.H, W=d.W, n_images=4, stems=None,
                             rgb=torch.zeros(4, d.H, d.W, 3, dtype=torch.uint8, device=DEV))
        res = refine_poses(d.verts, d.faces, ds, iters=40, lr=5e-3, sigma_px=4.0, sigma_end_px=1.5, lw_smooth=lw)
        out[lw] = U.smooth_direct(d.verts.cpu().double(), ds.R.cpu().double(), ds.T.cpu().double())
        assert math.isfinite(res["curve"][-1]["loss_smooth"])
    print(f"L_smooth after 40 iterations: lw_smooth 0 -> {float(out[0.0]):.6f}, lw_smooth 1 -> {float(out[1.0]):.6f}")
    assert float(out[1.0]) < float(out[0.0])


# ------------------------------------------------------------------------------------------------------------ Runner, CLI
def _conf(name, n_frames=4, HW=64, **train):
    return {"seq_name": "psil", "exp_name": name,
            "data_info": {"synthetic": {"n_frames": n_frames, "H": HW, "W": HW, "seed": 5}},
            "train": dict({"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100}, **train),
            "pose_sil": {"iters": 12, "sigma_px": 3.0, "sigma_end_px": 1.5, "report_freq": 4, "resolution": 48}}


def _check_pose_dir(d, stems, R, T, K):
    for k, s in enumerate(stems):
        z = np.load(os.path.join(d, s + ".npz"))
        assert sorted(z.files) == ["K", "R", "T"]
        assert z["R"].shape == (3, 3) and z["T"].shape == (1, 3) and z["K"].shape == (3, 3)
        assert z["R"].dtype == np.float32 and z["T"].dtype == np.float32 and z["K"].dtype == np.float32
        assert np.allclose(z["R"], R[k].cpu().numpy(), atol=1e-6) and np.allclose(z["T"][0], T[k].cpu().numpy(), atol=1e-6)
        assert np.array_equal(z["K"], K.cpu().numpy())


def test_runner_refine_poses_writes_poses_a_dataset_reads_back(tmp_path):
    from dynhor_amd.runner import Runner
    from dynhor_amd.tb_events import read_scalars
    r = Runner(conf=_conf("run", refine_poses=True), device="cuda:0", exp_root=str(tmp_path))
    r.train(3)
    with torch.no_grad():
        r.dataset.T[1, 0] += 0.05
    T_before = r.dataset.T.clone()
    res = r.refine_poses_silhouette()
    assert os.path.exists(res["checkpoint"])                            # the re-seeded PoseRefiner is checkpointed
    d = os.path.join(r.base_exp_dir, "poses", "00000003")
    assert res["dir"] == d and res["mesh"] == "reconstruction@48"
    stems = ["{:04d}".format(i) for i in range(4)]
    _check_pose_dir(os.path.join(d, "obj_infos"), stems, r.dataset.R, r.dataset.T, r.dataset.K)
    js = json.load(open(os.path.join(d, "refine.json")))
    assert js["iter"] == 3 and len(js["iou_before"]) == 4 and len(js["iou_after"]) == 4 and js["settings"]["iters"] == 12
    assert len(js["curve"]) >= 3 and js["mesh"] == "reconstruction@48"
    # the PoseRefiner was re-seeded: its poses are the refined ones, so the next checkpoint carries them
    Rp, Tp = r.pose_refiner.poses()
    assert torch.allclose(Rp, r.dataset.R, atol=1e-6) and torch.allclose(Tp, r.dataset.T, atol=1e-6)
    r.close()
    board = os.path.join(r.base_exp_dir, "board")
    tags = {tag for fn in os.listdir(board) for _, tag, _ in read_scalars(os.path.join(board, fn))}
    assert {"pose_sil/loss_sil", "pose_sil/iou_mean", "pose_sil/iou_min"} <= tags, tags
    # export_poses writes the same layout for the current poses
    d2 = r.export_poses(str(tmp_path / "exported"))
    _check_pose_dir(d2, stems, r.dataset.R, r.dataset.T, r.dataset.K)
    # a second Runner whose data_info.obj_infos points at either folder loads the refined poses
    from dynhor_amd.scene import make_sequence
    root = str(tmp_path / "seq")
    _write_sequence(root, make_sequence(4, 64, 64, 5, device="cpu"), stems)
    for k, folder in enumerate((os.path.join(d, "obj_infos"), d2)):
        conf = dict(_conf(f"reload{k}"), data_info={"dataroot": root, "obj_infos": folder})
        r2 = Runner(conf=conf, device="cuda:0", exp_root=str(tmp_path))
        assert r2.dataset.n_images == 4
        assert torch.allclose(r2.dataset.R, r.dataset.R, atol=1e-6) and torch.allclose(r2.dataset.T, r.dataset.T, atol=1e-6)
        assert not torch.allclose(r2.dataset.T, T_before, atol=1e-6)


def _write_sequence(root, frames, stems):
    from PIL import Image
    for sub in ("rgb", "sam_seg", "monocular_normal"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for k, s in enumerate(stems):
        Image.fromarray(frames["rgb"][k].cpu().numpy()).save(os.path.join(root, "rgb", s + ".png"))
        lab = frames["label"][k].cpu().numpy()
        m = np.zeros(lab.shape + (3,), dtype=np.uint8)
        m[..., 1][lab == 1] = 255
        m[..., 2][lab == -1] = 255
        Image.fromarray(m).save(os.path.join(root, "sam_seg", s + ".png"))
        Image.fromarray(frames["normal"][k].cpu().numpy()).save(os.path.join(root, "monocular_normal", s + ".png"))


def test_cli_refine_and_export_poses_round_trip_through_a_dataset(tmp_path):
    import yaml
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.scene import make_sequence
    conf = _conf("cli", n_frames=3, save_freq=3, refine_poses=True)     # the checkpoint --is_continue picks up carries a PoseRefiner
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--exp_root", str(tmp_path)] + list(a),
                                    cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    p = run("--mode", "train", "--iters", "3")
    assert p.returncode == 0, p.stderr[-3000:]
    stems = ["{:04d}".format(i) for i in range(3)]
    load = lambda d: {s: dict(np.load(os.path.join(d, s + ".npz"))) for s in stems}
    p = run("--mode", "export_poses", "--is_continue", "--pose_dir", str(tmp_path / "before"))
    assert p.returncode == 0, p.stderr[-3000:]
    before = load(str(tmp_path / "before"))
    p = run("--mode", "refine_poses", "--is_continue", "--pose_frames", "all")
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert "iou_mean_before" in res and "iou_mean_after" in res and os.path.isdir(os.path.join(res["dir"], "obj_infos"))
    assert os.path.exists(os.path.join(res["dir"], "refine.json")) and os.path.exists(res["checkpoint"])
    refined = load(os.path.join(res["dir"], "obj_infos"))
    assert any(not np.allclose(refined[s]["T"], before[s]["T"], atol=1e-7) for s in stems)        # the poses did move
    # a fresh process that continues from the checkpoint holds the refined poses, not the ones of the checkpoint before
    p = run("--mode", "export_poses", "--is_continue", "--pose_dir", str(tmp_path / "after"))
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert out["frames"] == 3 and out["dir"] == str(tmp_path / "after") and sorted(os.listdir(out["dir"])) == [s + ".npz" for s in stems]
    after = load(out["dir"])
    for s in stems:
        for k in ("R", "T", "K"):
            assert after[s][k].shape == refined[s][k].shape and np.allclose(after[s][k], refined[s][k], atol=1e-6), (s, k)
    # a Dataset whose obj_infos points at the written folder loads the refined poses
    root = str(tmp_path / "seq")
    _write_sequence(root, make_sequence(3, 64, 64, 5, device="cpu"), stems)
    ds = Dataset({"dataroot": root, "obj_infos": os.path.join(res["dir"], "obj_infos")}, device=DEV)
    for k, s in enumerate(stems):
        assert np.allclose(ds.R[k].cpu().numpy(), refined[s]["R"], atol=1e-6)
        assert np.allclose(ds.T[k].cpu().numpy(), refined[s]["T"][0], atol=1e-6)
