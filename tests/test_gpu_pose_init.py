"""Pose initialisation on the GPU: the three integer kernels of csrc/pose_init.hip against the restatement tests/pose_init_util.py bit
for bit (boxes, crop and pack, bank scores, for every chunking and on a second launch), the view bank against the restatement applied
to raster_depth's own coverage, retrieval (indices, IoUs, the recall bound), the whole pipeline from unknown poses, and the Runner /
CLI round trip through obj_infos/*.npz."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pose_init_util as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ boxes
def test_label_boxes_at_the_borders_and_without_an_object():
    from dynhor_amd.pose_init import label_boxes
    H, W = 37, 53
    lab = torch.zeros(6, H, W, dtype=torch.int8)
    lab[0, 0, 5] = 1; lab[0, 11, 0] = 1; lab[0, H - 1, 30] = 1; lab[0, 20, W - 1] = 1      # touches each border
    lab[1, 17, 41] = 1                                                                      # a single pixel
    lab[3, 4:9, 7:30] = -1                                                                  # hand pixels only (frame 2 stays empty)
    lab[4] = 1                                                                              # a full frame
    lab[5, 3:20, 9:44] = 1; lab[5, 10:30, 2:12] = -1; lab[5, 25, 50] = 1                    # object, hand, a stray pixel
    want = P.boxes(lab)
    assert want.tolist() == [[0, 0, W - 1, H - 1], [41, 17, 41, 17], [W, H, -1, -1], [W, H, -1, -1], [0, 0, W - 1, H - 1], [9, 3, 50, 25]]
    got = label_boxes(lab.to(DEV))
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    assert torch.equal(label_boxes(lab.to(DEV)).cpu(), want)                                # a second launch: the same bits
    assert torch.equal(label_boxes(lab[2:5].to(DEV)).cpu(), want[2:5])                      # a split of the frames
    # more than one workgroup per image (8192 pixels each): the extremes lie in different chunks
    g = torch.Generator().manual_seed(1)
    big = (torch.rand(3, 130, 131, generator=g) < 0.001).to(torch.int8)
    big[1] = 0
    big[1, 2, 100] = 1; big[1, 127, 3] = 1
    big[2][torch.rand(130, 131, generator=g) < 0.3] = -1
    assert torch.equal(label_boxes(big.to(DEV)).cpu(), P.boxes(big))
    assert tuple(label_boxes(torch.zeros(0, 4, 4, dtype=torch.int8, device=DEV)).shape) == (0, 4)


# ------------------------------------------------------------------------------------------------------------ crop and pack
def _random_labels(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 3, (n, H, W), generator=g) - 1).to(torch.int8)                # -1, 0, 1


@pytest.mark.parametrize("S", [8, 16, 24])
def test_crop_pack_on_dyadic_squares_equals_the_restatement(S):
    """Squares whose (x0, y0, step) are multiples of 1/8 with a dyadic step: (c + 0.5) step + x0 and the + 0.5 are exact in fp32, so the
    kernel and the restatement must agree on every bit."""
    from dynhor_amd.pose_init import sil_crop_pack
    H, W = 37, 53
    lab = _random_labels(8, H, W, 3)
    sq = torch.tensor([[-6.5, 3.25, 1.0],                      # partly left of the image
                       [10.0, -9.125, 1.5],                    # partly above it
                       [30.0, 20.0, 2.0],                      # beyond the right and lower border
                       [-20.0, -20.0, 6.0],                    # on every side at once
                       [12.0, 9.0, 0.125],                     # b < S: every pixel is read several times
                       [0.5, 0.25, 4.5 if S == 8 else 2.25],   # b >> S
                       [0.0, 0.0, 0.0],                        # the mark of an empty box
                       [20.0, 10.0, 0.5]], dtype=torch.float32)
    wo, wk = P.crop(lab, sq, S)
    assert bool(wo[:6].any(dim=(1, 2)).all()) and not bool(wk[6].any()) and not bool(wk[0].all()) and not bool(wk[2].all())
    o, k = sil_crop_pack(lab.to(DEV), sq.to(DEV), S)
    assert o.dtype == torch.int64 and tuple(o.shape) == (8, S * S // 64)
    assert torch.equal(o.cpu(), P.pack(wo)) and torch.equal(k.cpu(), P.pack(wk))
    o2, k2 = sil_crop_pack(lab[3:7].to(DEV), sq[3:7].to(DEV), S)                            # a split, a second launch
    assert torch.equal(o2, o[3:7]) and torch.equal(k2, k[3:7])
    with pytest.raises(ValueError):
        sil_crop_pack(lab.to(DEV), sq.to(DEV), 12)


def test_crop_pack_on_random_squares_equals_the_restatement_away_from_pixel_boundaries():
    """64 squares from random tight boxes (the host's rule, not dyadic).  A sample is left out only where its fp64 coordinate lies within
    1e-4 px of a pixel boundary (fp32 rounds coordinates of a few hundred pixels to 3e-5); more than 0.1 % left out fails.  A box whose
    edge makes (c + 0.5 - S / 2) step an integer puts whole columns of samples exactly on a boundary (about one seed in ten has no such
    box among its 64: 3, 30, 39 of the first 40); the seed is chosen so that this set has none."""
    from dynhor_amd.pose_init import crop_squares, sil_crop_pack
    H, W, S, n = 97, 131, 24, 64
    lab = _random_labels(n, H, W, 8)
    g = torch.Generator().manual_seed(3)
    lo = torch.stack([torch.randint(0, W - 8, (n,), generator=g), torch.randint(0, H - 8, (n,), generator=g)], 1)
    ext = torch.randint(1, 80, (n, 2), generator=g)
    bx = torch.cat([lo, torch.minimum(lo + ext, torch.tensor([W - 1, H - 1]))], 1).to(torch.int32)
    sq = crop_squares(bx, S)
    assert torch.equal(sq, P.squares(bx, S))
    _, _, ex, ey = P.sample_pixels(sq, S)
    near = lambda e: ((e + 0.5) - torch.floor(e + 0.5 + 0.5)).abs() < 1e-4          # distance of e + 0.5 to the nearest integer
    skip = near(ey)[:, :, None] | near(ex)[:, None, :]
    frac = float(skip.double().mean())
    assert frac <= 1e-3, frac
    wo, wk = P.crop(lab, sq, S)
    o, k = sil_crop_pack(lab.to(DEV), sq.to(DEV), S)
    go, gk = P.unpack(o.cpu()).view(n, S, S), P.unpack(k.cpu()).view(n, S, S)
    assert torch.equal(go | skip, wo | skip) and torch.equal(gk | skip, wk | skip)
    print(f"random squares: {int(skip.sum())} of {skip.numel()} samples within 1e-4 px of a pixel boundary; "
          f"{int((go != wo).sum()) + int((gk != wk).sum())} bits differ there")


# ------------------------------------------------------------------------------------------------------------ score
@pytest.mark.parametrize("Wd", [1, 4, 9])
def test_bank_score_equals_the_restatement_for_every_chunking(Wd):
    from dynhor_amd.pose_init import iou_from_counts, sil_bank_score
    F, V = 3, 130
    g = torch.Generator().manual_seed(Wd)
    rnd = lambda *s: torch.randint(-2 ** 63, 2 ** 63 - 1, s, generator=g, dtype=torch.int64)
    fo, fk, bo = rnd(F, Wd), rnd(F, Wd), rnd(V, Wd)
    fk[0] = 0                                                  # nothing kept: the union is 0
    fo[1] = -1; fk[1] = -1                                     # all ones
    bo[5] = fo[2]                                              # the frame itself: inter == union
    bo[7] = 0                                                  # an empty view
    bo[129] = -1
    want = P.score(P.unpack(fo), P.unpack(fk), P.unpack(bo))
    assert want[0].abs().sum() == 0 and want[2, 5, 0] == want[2, 5, 1] and want[1, 7].tolist() == [0, 64 * Wd]
    assert want[1, 129].tolist() == [64 * Wd, 64 * Wd]
    d = lambda t: t.to(DEV)
    got = sil_bank_score(d(fo), d(fk), d(bo))
    assert got.dtype == torch.int32 and tuple(got.shape) == (F, V, 2)
    assert torch.equal(got.cpu(), want)
    for chunk in (1, 7, 130):
        assert torch.equal(sil_bank_score(d(fo), d(fk), d(bo), view_chunk=chunk), got)
    assert torch.equal(sil_bank_score(d(fo), d(fk), d(bo)), got)                            # a second launch
    assert torch.equal(sil_bank_score(d(fo[1:]), d(fk[1:]), d(bo)), got[1:])                # a split of the frames
    assert torch.equal(iou_from_counts(got.cpu()), P.iou(want)) and float(P.iou(want)[0].max()) == 0.0


def test_bank_score_more_frames_than_one_tile_and_more_words_than_one_chunk():
    """17 frames (a frame tile holds 16), 70 views (a view tile holds 64), 36 and 40 words (the kernel stages 32 at a time)."""
    from dynhor_amd.pose_init import sil_bank_score
    g = torch.Generator().manual_seed(40)
    for Wd in (36, 40):
        rnd = lambda *s: torch.randint(-2 ** 63, 2 ** 63 - 1, s, generator=g, dtype=torch.int64)
        fo, fk, bo = rnd(17, Wd), rnd(17, Wd), rnd(70, Wd)
        got = sil_bank_score(fo.to(DEV), fk.to(DEV), bo.to(DEV))
        assert torch.equal(got.cpu(), P.score(P.unpack(fo), P.unpack(fk), P.unpack(bo)))


# ------------------------------------------------------------------------------------------------------------ bank
def _bank_coverage(verts, faces, bank):
    from dynhor_amd.mesh_color import raster_depth
    n = bank["R"].shape[0]
    rs = bank["settings"]["render_size"]
    R = bank["R"].to(DEV, torch.float32).contiguous()
    cov = []
    for v0 in range(0, n, 256):
        Rc = R[v0:v0 + 256].contiguous()
        cov.append((raster_depth(verts, faces, Rc, bank["T"][None].expand(Rc.shape[0], 3).contiguous(), bank["K"], rs, rs) != -1).cpu())
    return torch.cat(cov)


@pytest.mark.parametrize("kind", ["coarse", "fine"])
def test_view_bank_equals_the_restatement_on_raster_depths_coverage(kind):
    from dynhor_amd.pose_init import arvo_rotations, build_view_bank
    n_lat, n_lon, rs = (4, 6, 96) if kind == "coarse" else (40, 72, 64)       # faces wider than 32 px / sub-pixel faces
    v, f = P.U.bent_ellipsoid(n_lat, n_lon)
    verts, faces = v.to(DEV, torch.float32).contiguous(), f.to(DEV).contiguous()
    bank = build_view_bank(verts, faces, n_views=70, seed=5, render_size=rs, crop_size=48, view_chunk=32)      # three chunks
    assert torch.equal(bank["R"], arvo_rotations(70, 5)) and tuple(bank["obj"].shape) == (70, 36)
    Kw, Tw = P.bank_camera(v, rs, 3.5)
    assert torch.allclose(bank["K"].cpu().double(), Kw, atol=1e-5) and torch.allclose(bank["T"].cpu().double(), Tw, atol=1e-6)
    cov = _bank_coverage(verts, faces, bank)
    assert int(cov.sum(dim=(1, 2)).min()) > 0.05 * rs * rs                   # every view shows the template, about a tenth of the image
    wo, _, wb, _ = P.pack_label(cov.to(torch.int8), 48)
    assert torch.equal(bank["obj"].cpu(), wo) and torch.equal(bank["boxes"], wb)
    again = build_view_bank(verts, faces, n_views=70, seed=5, render_size=rs, crop_size=48, view_chunk=70)
    assert torch.equal(again["obj"], bank["obj"])


# ------------------------------------------------------------------------------------------------------------ retrieval
RECALL_GAP_BOUND = 10.0          # the issue's; tests/test_cpu_pose_init.py measured 3.73 degrees on the fp64 restatement


def _recall_bank():
    from dynhor_amd.pose_init import build_view_bank
    fx, c = P.recall_scene(), P.RECALL
    verts = fx["scene"]["verts"].to(DEV, torch.float32).contiguous()
    faces = fx["scene"]["faces"].to(DEV).contiguous()
    bank = build_view_bank(verts, faces, n_views=c["n_views"], seed=c["bank_seed"], render_size=c["render_size"],
                           crop_size=c["crop_size"], distance_scale=c["distance_scale"])
    return fx, verts, faces, bank


def test_retrieval_equals_the_restatement_and_recalls_a_view_near_the_truth():
    from dynhor_amd.pose_init import retrieve
    fx, verts, faces, bank = _recall_bank()
    r = P.retrieval(_bank_coverage(verts, faces, bank), fx)
    assert torch.equal(bank["obj"].cpu(), r["bank_obj"])
    got = retrieve(fx["scene"]["label"].to(DEV), bank, P.RECALL["candidates"])
    assert torch.equal(got["boxes"], fx["frame_boxes"])
    assert torch.equal(got["index"], r["index"]) and torch.equal(got["iou"], r["iou"]) and torch.equal(got["iou_all"], r["iou_all"])
    gap = r["best_deg"] - r["near_deg"]
    print(f"nearest bank view {[round(float(x), 1) for x in r['near_deg']]}, best of the top 32 "
          f"{[round(float(x), 1) for x in r['best_deg']]} (largest gap {float(gap.max()):.2f}), argmax "
          f"{[round(float(x), 1) for x in r['argmax_deg']]} degrees")
    assert float(gap.max()) <= RECALL_GAP_BOUND


# ------------------------------------------------------------------------------------------------------------ end to end
# gap = the mean IoU that refine_poses reaches from the fixture's own perturbed start (8 degrees, 0.06-0.12 off: the parent's behaviour;
# tests/test_gpu_pose_sil.py's E2E_SHORTFALL is its recorded measure) minus the mean final IoU after init_poses from R = I, both in the
# same test run.  The first run on an MI355X measured 0.9925 against 0.9926: E2E_GAP_MEASURED = -0.0001, init_poses ends one or two
# pixels AHEAD (a pixel of one frame is 7e-5 of the mean).  The allowed gap is twice the measured shortfall (ISSUE "End to end"); a
# negative shortfall counts as none, so init_poses may not end behind the perturbed start at all.  Both runs are bitwise reproducible.
# Per frame on that run (view, rank among the 32, the view's angle to the truth, IoU bank / fit / final, final angle to the truth):
#   0: 1367, 24, 25.0, 0.8726 / 0.9912 / 0.9926, 0.4      4:  562, 30, 37.2, 0.8815 / 0.9947 / 0.9942, 2.1
#   1:  773, 29, 16.7, 0.8735 / 0.9926 / 0.9895, 0.9      5:  105,  5,  7.5, 0.9253 / 0.9916 / 0.9916, 1.4
#   2:  773,  4, 10.9, 0.9371 / 0.9935 / 0.9899, 0.3      6: 1297,  0, 26.8, 0.9320 / 0.9975 / 0.9956, 0.3
#   3:  105,  2, 24.7, 0.9399 / 0.9924 / 0.9930, 2.5      7: 1346,  3, 15.9, 0.9171 / 0.9945 / 0.9945, 1.0
E2E_GAP_MEASURED = -0.0001
E2E_GAP_ALLOWED = 2 * max(E2E_GAP_MEASURED, 0.0)
E2E_MAX_DEG = 45.0               # the wrong basins of this fixture sit at 150-180 degrees


def test_init_poses_from_unknown_poses_ends_near_the_truth():
    from dynhor_amd.pose_init import init_poses, rotation_angle_deg
    from dynhor_amd.pose_sil import refine_poses
    fx, verts, faces, bank = _recall_bank()
    sc, c = fx["scene"], P.RECALL
    F, H, W = c["n_frames"], c["H"], c["W"]
    f32 = lambda t: t.to(DEV, torch.float32).contiguous()
    mk = lambda R, T: SimpleNamespace(label=sc["label"].to(DEV), R=f32(R), T=f32(T), K=f32(sc["K"]), H=H, W=W, n_images=F, stems=None,
                                      rgb=torch.zeros(F, H, W, 3, dtype=torch.uint8, device=DEV))
    base = mk(sc["R0"], sc["T0"])
    ref = refine_poses(verts, faces, base)
    ds = mk(torch.eye(3, dtype=torch.float64).expand(F, 3, 3), torch.tensor([0.0, 0.0, 1.75], dtype=torch.float64).expand(F, 3))
    res = init_poses(verts, faces, ds, bank=bank)
    assert torch.equal(ds.R, res["R"]) and torch.equal(ds.T, res["T"])
    ang = rotation_angle_deg(ds.R.cpu().double(), sc["R_true"])
    true_ang = P.angle_deg(sc["R_true"][:, None], fx["R"][None, :])
    rows = [(k, fr["view"], fr["rank"], round(float(true_ang[k, fr["view"]]), 1), round(fr["iou_bank"], 4), round(fr["iou_fit"], 4),
             round(fr["iou_final"], 4), round(float(ang[k]), 1)) for k, fr in enumerate(res["frames"])]
    gap = ref["iou_mean_after"] - res["iou_final_mean"]
    print("frame, view, rank, view's angle to the truth, IoU bank / fit / final, final angle to the truth:")
    for r in rows:
        print("  ", r)
    print(f"mean final IoU {res['iou_final_mean']:.4f}; refine_poses from the perturbed start reaches {ref['iou_mean_after']:.4f}: "
          f"gap {gap:.6f}; angles to the truth {[round(float(a), 1) for a in ang]}")
    keys = {"stem", "view", "rank", "iou_bank", "iou_fit", "iou_final", "angle_prev_deg", "filled_from"}
    assert all(set(fr) == keys for fr in res["frames"]) and res["frames"][0]["angle_prev_deg"] is None
    assert float(ang.max()) <= E2E_MAX_DEG, [round(float(a), 1) for a in ang]
    assert gap <= E2E_GAP_ALLOWED, (gap, E2E_GAP_ALLOWED)


def test_init_poses_fills_a_frame_without_an_object_from_its_neighbour():
    from dynhor_amd.pose_init import build_view_bank, init_poses
    sc = P.U.small_scene(n_frames=3, H=64, W=64, seed=3, hand=False)
    verts, faces = sc["verts"].to(DEV, torch.float32).contiguous(), sc["faces"].to(DEV).contiguous()
    label = sc["label"].clone()
    label[1] = 0
    bank = build_view_bank(verts, faces, n_views=64, seed=1, render_size=64, crop_size=32)
    f32 = lambda t: t.to(DEV, torch.float32).contiguous()
    ds = SimpleNamespace(label=label.to(DEV), R=f32(sc["R0"]), T=f32(sc["T0"]), K=f32(sc["K"]), H=64, W=64, n_images=3, stems=None)
    res = init_poses(verts, faces, ds, bank=bank, candidates=4, hyp_iters=4, final_refine=False)
    assert res["frames"][1]["view"] is None and res["frames"][1]["filled_from"] == "0000"
    assert torch.equal(ds.R[1], ds.R[0]) and torch.equal(ds.T[1], ds.T[0]) and res["refine"] is None
    ds.label = torch.zeros_like(ds.label)
    with pytest.raises(ValueError):
        init_poses(verts, faces, ds, bank=bank, candidates=4, hyp_iters=4, final_refine=False)
    with pytest.raises(ValueError):
        init_poses(verts, faces, ds, bank=bank, no_such_setting=1)


# ------------------------------------------------------------------------------------------------------------ Runner, CLI
def test_cli_init_poses_writes_poses_a_dataset_reads_back(tmp_path):
    import yaml
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.runner import Runner
    from dynhor_amd.scene import make_sequence, write_sequence_to_disk
    from dynhor_amd.tb_events import read_scalars
    root = str(tmp_path / "seq")
    frames = make_sequence(4, 64, 64, 5, device="cpu")
    write_sequence_to_disk(frames, root, pose_dir=str(tmp_path / "true_poses"))            # the dataroot holds no pose file
    assert not os.path.exists(os.path.join(root, "obj_infos"))
    with pytest.raises(FileNotFoundError):
        Dataset({"dataroot": root}, device=DEV)                                            # every other mode keeps today's error
    v, f = Runner._scene_gt_mesh(SimpleNamespace(device=DEV), 32)
    template = str(tmp_path / "template.obj")
    with open(template, "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(r) for r in v.cpu().tolist()))
        fh.write("".join("f %d %d %d\n" % tuple(i + 1 for i in r) for r in f.cpu().tolist()))
    conf = {"seq_name": "pinit", "exp_name": "cli",
            "data_info": {"dataroot": root, "obj_path": template, "normalize_mesh": False, "K": frames["K"].tolist()},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100},
            "pose_sil": {"iters": 8, "sigma_px": 3.0, "sigma_end_px": 1.5, "report_freq": 4},
            "pose_init": {"n_views": 128, "render_size": 64, "crop_size": 32, "candidates": 4, "hyp_iters": 6, "hyp_sigma_px": 4.0}}
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--exp_root", str(tmp_path), "--mode", "init_poses"],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    d = os.path.join(str(tmp_path), "pinit", "cli", "poses", "init")
    assert res["dir"] == d and res["mesh"] == template and res["settings"]["n_views"] == 128 and res["settings"]["candidates"] == 4
    js = json.load(open(os.path.join(d, "init.json")))
    assert len(js["frames"]) == 4 and js["refine"]["settings"]["iters"] == 8
    for fr in js["frames"]:
        assert {"view", "rank", "iou_bank", "iou_fit", "iou_final", "angle_prev_deg"} <= set(fr)
    stems = ["%04d" % i for i in range(4)]
    assert sorted(os.listdir(os.path.join(d, "obj_infos"))) == [s + ".npz" for s in stems]
    ds = Dataset({"dataroot": root, "obj_infos": os.path.join(d, "obj_infos")}, device=DEV)
    assert ds.n_images == 4 and list(ds.stems) == stems
    for k, s in enumerate(stems):
        z = np.load(os.path.join(d, "obj_infos", s + ".npz"))
        assert sorted(z.files) == ["K", "R", "T"] and z["R"].dtype == np.float32 and z["T"].shape == (1, 3)
        assert np.allclose(ds.R[k].cpu().numpy(), z["R"], atol=1e-6) and np.allclose(ds.T[k].cpu().numpy(), z["T"][0], atol=1e-6)
        assert np.allclose(z["K"], frames["K"].numpy(), atol=1e-6)
        assert abs(float(np.linalg.det(z["R"])) - 1.0) < 1e-4 and float(z["T"][0, 2]) > 0.0
    board = os.path.join(str(tmp_path), "pinit", "cli", "board")
    tags = {tag for fn in os.listdir(board) for _, tag, _ in read_scalars(os.path.join(board, fn))}
    assert {"init/iou_bank", "init/iou_fit", "init/iou_final", "init/iou_final_mean"} <= tags, tags
    # without pose files and without a K in the config the loader falls back on the reference's guess
    ds0 = Dataset({"dataroot": root}, device=DEV, poses=False)
    focal = float(np.float32(1.2 * 64))
    assert ds0.K.cpu().tolist() == [[focal, 0.0, 32.0], [0.0, focal, 32.0], [0.0, 0.0, 1.0]]
    assert torch.equal(ds0.R.cpu(), torch.eye(3).expand(4, 3, 3)) and ds0.T.cpu().tolist() == [[0.0, 0.0, 1.75]] * 4
