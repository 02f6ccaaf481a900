"""GPU: dh_mvs_sweep and dh_mvs_check against the numpy restatement (tests/mvs_util.py, licensed by tests/test_cpu_mvs.py), their
reproducibility, mvs.depth_maps end to end on the textured sphere with a guide 5 % too small, with a hand, and Runner.mvs_depth."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import match_util as MU
from tests import mesh_texture_util as TU
from tests import mvs_util as V
from tests import pose_photo_util as PU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_sweep(args):
    from dynhor_amd import mvs
    gray, valid, R, T, K, Ki, pix, guide, nbr, D, step, P, min_va, min_vb, min_views, min_cos = args
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(DEV)
    # the wrapper inverts K itself: the restatement is given the same float32 inverse
    assert np.array_equal(mvs._kinv(t(K.reshape(3, 3), torch.float32)).cpu().numpy(), Ki)
    of, oi = mvs.sweep(t(gray, torch.uint8), t(valid, torch.uint8), t(R.reshape(-1, 3, 3), torch.float32), t(T, torch.float32),
                       t(K.reshape(3, 3), torch.float32), t(pix, torch.int32), t(guide, torch.float32), t(nbr, torch.int32), D, float(step), P,
                       min_va, float(min_vb), min_views, float(min_cos))
    return of, oi


@functools.lru_cache(maxsize=None)
def _refs(case):
    kc = V.kernel_case(case)
    return kc, V.sweep_ref(*kc["args"], dtype=np.float64), V.sweep_ref(*kc["args"], dtype=np.float32, ambiguity=False)


# ------------------------------------------------------------------------------------------------ the kernels against the restatement
@pytest.mark.parametrize("case", V.CASES)
def test_sweep_agrees_with_the_restatement(case):
    """5 frames of 40 x 48 (mvs_util.plane_scene: a hole, a ragged strip and a single pixel invalid, a flat block), pixels on every image
    border, guides with NaN / inf / tiny z0, a sweep crossing 1e-3, grazing, averted, zero and NaN normals, a frame without neighbours
    and frames with fewer than min_views.  Flags and views equal the fp64 restatement's outside its ambiguous pixels (at most 2 %);
    c_best and z within four times the float32 restatement's own deviation from fp64."""
    kc, r64, r32 = _refs(case)
    of, oi = (t.cpu().numpy() for t in _gpu_sweep(kc["args"]))
    live = (r64["c"] > -1.5) & (r32["c"] > -1.5)
    dev_c = float(np.abs(r64["c"] - r32["c"].astype(np.float64))[live].max())
    amb = r64["amb"] | V.argmax_ambiguous(r64["c"], 8 * dev_c)
    clear = ~amb
    assert amb.mean() <= V.AMBIGUOUS_CAP
    res = clear & (r64["out_i"][:, 2] & 11 == 0)                       # pixels with a result (flag 4 alone still has one)
    dev_z = float(np.abs(r64["out_f"][res, 0] - r32["out_f"][res, 0].astype(np.float64)).max())
    dev_b = float(np.abs(r64["out_f"][res, 1] - r32["out_f"][res, 1].astype(np.float64)).max())
    err_z = float(np.abs(of[res, 0].astype(np.float64) - r64["out_f"][res, 0]).max())
    err_b = float(np.abs(of[res, 1].astype(np.float64) - r64["out_f"][res, 1]).max())
    bits = int((of.view(np.int32) != r32["out_f"].view(np.int32)).any(1).sum())
    print(f"case {case}: n {kc['n']}, ambiguous {amb.mean():.4f}, with a result {int(res.sum())}, flags "
          f"{np.bincount(r64['out_i'][:, 2], minlength=9).tolist()}; float32 restatement vs fp64: c_best {dev_b:.3e}, z {dev_z:.3e}; kernel vs "
          f"fp64: c_best {err_b:.3e}, z {err_z:.3e}; rows that differ from the float32 restatement in a bit: {bits}")
    assert np.array_equal(oi[clear, 2], r64["out_i"][clear, 2]) and np.array_equal(oi[clear, 1], r64["out_i"][clear, 1])
    assert np.array_equal(oi[clear, 0], r64["out_i"][clear, 0]) and np.array_equal(oi[clear, 3], r64["out_i"][clear, 3])
    assert set(np.unique(r64["out_i"][:, 2])) >= {0, 1, 2, 8}
    assert err_b <= 4 * dev_b and err_z <= 4 * dev_z
    none = clear & (r64["out_i"][:, 2] & 11 != 0)
    assert (of[none] == np.array([0, V.NONE, V.NONE, 0], np.float32)).all() and (oi[none][:, [0, 1, 3]] == 0).all()
    assert np.abs(of[res, 2].astype(np.float64) - r64["out_f"][res, 2]).max() <= 4 * dev_c                  # c_second


def test_sweep_of_one_pixel_and_of_none():
    kc, r64, _ = _refs(V.CASES[2])
    a = list(kc["args"])
    i = int(np.nonzero(r64["out_i"][:, 2] == 0)[0][0])
    whole = _gpu_sweep(kc["args"])
    a[6], a[7] = kc["args"][6][i:i + 1], kc["args"][7][i:i + 1]
    of, oi = _gpu_sweep(a)
    assert torch.equal(of, whole[0][i:i + 1]) and torch.equal(oi, whole[1][i:i + 1])
    a[6], a[7] = kc["args"][6][:0], kc["args"][7][:0]
    of, oi = _gpu_sweep(a)
    assert of.shape == (0, 4) and oi.shape == (0, 4)


@pytest.mark.parametrize("case", (V.CASES[0], V.CASES[2]))
def test_sweep_is_reproducible_across_orders_and_splits(case):
    """The same pixels shuffled, split into three calls and run one pixel per call give the same bits (a wave holds 16 pixels at D = 3
    and one at D = 33: a pixel's slot must not matter)."""
    kc, _, _ = _refs(case)
    a = list(kc["args"])
    pix, guide = kc["args"][6], kc["args"][7]
    of, oi = _gpu_sweep(kc["args"])
    of2, oi2 = _gpu_sweep(kc["args"])
    assert torch.equal(of, of2) and torch.equal(oi, oi2)
    perm = np.random.default_rng(5).permutation(len(pix))
    a[6], a[7] = pix[perm], guide[perm]
    ofp, oip = _gpu_sweep(a)
    assert torch.equal(ofp.cpu(), of.cpu()[perm]) and torch.equal(oip.cpu(), oi.cpu()[perm])
    cuts = [0, 7, len(pix) // 2 + 1, len(pix)]
    parts = []
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        a[6], a[7] = pix[c0:c1], guide[c0:c1]
        parts.append(_gpu_sweep(a))
    assert torch.equal(torch.cat([p[0] for p in parts]), of) and torch.equal(torch.cat([p[1] for p in parts]), oi)
    singles = []
    for i in range(0, len(pix), 5):                                     # every fifth pixel alone in its call
        a[6], a[7] = pix[i:i + 1], guide[i:i + 1]
        singles.append(_gpu_sweep(a))
    assert torch.equal(torch.cat([p[0] for p in singles]), of[::5]) and torch.equal(torch.cat([p[1] for p in singles]), oi[::5])


@pytest.mark.parametrize("offsets", V.CHECK_OFFSETS)
def test_check_equals_the_restatement(offsets):
    """mvs_util.check_case: the counts equal the restatement's outside the pixels it marks as ambiguous (a projection within 1e-3 px of
    a rounding boundary, a depth ratio within 1e-6 of depth_rel: at most 1 %)."""
    from dynhor_amd import mvs
    depth, R32, T32, K32, Ki32, nbr = V.check_case(offsets)
    want, amb = V.check_ref(depth, R32, T32, K32, Ki32, nbr, np.float32(0.01))
    t = lambda a: torch.as_tensor(a).to(DEV)
    got = mvs.check(t(depth), t(R32), t(T32), t(K32), t(nbr), 0.01).cpu().numpy()
    print(f"check {offsets}: counts {np.bincount(want.ravel(), minlength=3).tolist()}, ambiguous {amb.mean():.4f}, differ "
          f"{(got != want).sum()} (outside the ambiguous: {((got != want) & ~amb).sum()})")
    assert amb.mean() <= V.CHECK_AMBIGUOUS_CAP and want.max() == 2 * len(offsets)
    assert np.array_equal(got[~amb], want[~amb]) and (got[~np.isfinite(depth)] == 0).all()
    again = mvs.check(t(depth), t(R32), t(T32), t(K32), t(nbr), 0.01).cpu().numpy()
    assert np.array_equal(got, again)
    none = mvs.check(t(depth), t(R32), t(T32), t(K32), t(np.full((len(depth), 1), -1, np.int32)), 0.01)
    assert int(none.max()) == 0


# ------------------------------------------------------------------------------------------------ end to end
def _dataset(sc):
    return SimpleNamespace(rgb=sc["rgb"].to(DEV), label=sc["label"].to(DEV), R=sc["R"].float().to(DEV), T=sc["T"].float().to(DEV),
                           K=sc["K"].float().to(DEV))


# peak_margin 0: on this smooth texture the score two steps from the peak lies 0.001 .. 0.004 below it, so the default gate of 0.02
# measures the main lobe's own curvature and loses 313 of the 314 pixels that pass the other gates (the fp64 restatement,
# tests/test_cpu_mvs.py); the gate is for a second lobe, which this scene does not have
E2E = {"step_px": V.E2E_STEP_PX, "peak_margin": 0.0}


@functools.lru_cache(maxsize=None)
def _e2e():
    """mvs.depth_maps on the device and the fp64 restatement of the same passes from the device's own grey frames and guide: the sphere
    at five poses 6 degrees apart, pattern(36), an icosphere 5 % too small as the guide, frames 1 .. 3 on a grid of 4 px."""
    from dynhor_amd import mvs
    from dynhor_amd.match import gray_frames, usable_sources
    from dynhor_amd.mesh_color import usable_map
    sc = V.e2e_scene()
    ds = _dataset(sc)
    verts, faces = V.icosphere(0.95 * V.SPHERE_E2E_R, 3)
    out = mvs.depth_maps(ds, verts.to(DEV), faces.to(DEV), frames=V.E2E_FRAMES, **E2E)
    gray, valid = gray_frames(ds.rgb, usable_map(ds.label, 1), 1.0, 0.5)
    src_ok = usable_sources(gray, valid, 4).cpu().numpy()
    guide = mvs.guide_from_mesh(verts.to(DEV), faces.to(DEV), ds.R, ds.T, ds.K, sc["H"], sc["W"]).cpu().numpy()
    Rf, Tf, Kf, Kif = V.f32_inputs(sc)
    ref = V.depth_maps_ref(gray.cpu().numpy(), valid.cpu().numpy(), src_ok, guide, Rf, Tf, Kf, Kif, V.neighbours_ref(len(sc["R"])),
                           V.E2E_FRAMES, step_px=V.E2E_STEP_PX, peak_margin=0.0)
    z_true = PU.sphere_hits(sc["R"], sc["T"], sc["K"], sc["H"], sc["W"])[2].numpy()
    return sc, out, ref, guide, z_true


def test_depth_maps_improve_on_a_guide_that_is_too_small():
    sc, out, ref, guide, z_true = _e2e()
    mid = len(sc["R"]) // 2
    k, kr = out["kept"][mid].cpu().numpy(), ref["kept"][mid]
    z = out["depth"][mid].cpu().numpy().astype(np.float64)
    err, err_ref = np.median(np.abs(z[k] - z_true[mid][k])), np.median(np.abs(ref["depth"][mid][kr] - z_true[mid][kr]))
    err_guide = np.median(np.abs(guide[mid][k][:, 0] - z_true[mid][k]))
    row = out["stats"]["per_frame"][1]
    swept = int(ref["swept"][mid].sum())
    print(f"middle frame: swept {row['swept']} (restatement {swept}), kept {int(k.sum())} (restatement {int(kr.sum())}), lost {row['lost']} "
          f"(restatement {np.bincount(ref['lost'][mid].ravel(), minlength=6)[1:].tolist()}); median |z - z_true| {err:.3e} (restatement "
          f"{err_ref:.3e}, guide {err_guide:.3e}); seconds {out['stats']['seconds']}")
    assert row["frame"] == mid and row["swept"] == swept and row["kept"] + sum(row["lost"].values()) == row["swept"]
    assert kr.sum() >= 100 and err_guide >= 5 * err_ref               # the restatement alone meets the factor
    assert err <= 2 * err_ref and err_guide >= 5 * err
    assert k.sum() / row["swept"] >= 0.5 * kr.sum() / swept
    assert not out["kept"][0].any() and not out["kept"][4].any()       # frames that were not asked for
    depth = out["depth"][mid].cpu().numpy()
    assert np.isnan(depth[~k]).all() and np.isfinite(depth[k]).all()


def test_margin_gate_rejects_what_the_restatement_rejects():
    """The end-to-end scene's middle frame at peak_margin 0.002, inside the scene's spread of c_best - c_second (median 0.0021), without
    the consistency check: the gate loses some pixels and keeps some, and the per-pixel verdicts are the fp64 restatement's but for the
    pixels whose margin lies within the float32 deviation of the threshold (at most 2 % of the swept, the cap on ambiguous pixels)."""
    from dynhor_amd import mvs
    from dynhor_amd.match import gray_frames, usable_sources
    from dynhor_amd.mesh_color import usable_map
    sc = V.e2e_scene()
    ds = _dataset(sc)
    mid = len(sc["R"]) // 2
    verts, faces = V.icosphere(0.95 * V.SPHERE_E2E_R, 3)
    out = mvs.depth_maps(ds, verts.to(DEV), faces.to(DEV), frames=[mid], step_px=V.E2E_STEP_PX, peak_margin=V.E2E_MARGIN, min_consistent=0)
    gray, valid = gray_frames(ds.rgb, usable_map(ds.label, 1), 1.0, 0.5)
    src_ok = usable_sources(gray, valid, 4).cpu().numpy()
    guide = mvs.guide_from_mesh(verts.to(DEV), faces.to(DEV), ds.R, ds.T, ds.K, sc["H"], sc["W"]).cpu().numpy()
    Rf, Tf, Kf, Kif = V.f32_inputs(sc)
    ref = V.depth_maps_ref(gray.cpu().numpy(), valid.cpu().numpy(), src_ok, guide, Rf, Tf, Kf, Kif, V.neighbours_ref(len(sc["R"])), [mid],
                           step_px=V.E2E_STEP_PX, peak_margin=V.E2E_MARGIN, min_consistent=0)
    lost, lost_ref = out["lost"][mid].cpu().numpy(), ref["lost"][mid]
    row = out["stats"]["per_frame"][0]
    counts = np.bincount(lost_ref.ravel(), minlength=6)[1:].tolist()
    differ = int((lost != lost_ref).sum())
    print(f"peak_margin {V.E2E_MARGIN}: swept {row['swept']}, kept {row['kept']} (restatement {int(ref['kept'][mid].sum())}), lost "
          f"{row['lost']} (restatement {counts}), verdicts that differ: {differ}")
    assert counts[2] >= 50 and ref["kept"][mid].sum() >= 50
    assert row["lost"]["margin"] == int((lost == 3).sum()) > 0 and row["kept"] > 0
    assert differ <= V.AMBIGUOUS_CAP * row["swept"]


def test_normals_of_the_depth_maps_follow_the_sphere():
    sc, out, ref, guide, z_true = _e2e()
    mid = len(sc["R"]) // 2
    Ki = np.linalg.inv(sc["K"].double().numpy())
    _, pts, _ = PU.sphere_hits(sc["R"], sc["T"], sc["K"], sc["H"], sc["W"])
    true = (pts[mid] / V.SPHERE_E2E_R).numpy() @ sc["R"][mid].double().numpy().T       # the sphere's normal in the camera frame
    inner = TU.erode_object(sc["label"], 3)[mid].numpy() != 0
    n_ref, ok_ref = V.normals_ref(np.nan_to_num(ref["depth"][mid]), ref["kept"][mid], Ki, 0.01, V.E2E_STEP_PX)
    n, ok = out["normal"][mid].cpu().numpy().astype(np.float64), out["normal_ok"][mid].cpu().numpy()
    m, mr = ok & inner, ok_ref & inner
    ang = np.degrees(np.arccos(np.clip((n[m] * true[m]).sum(-1), -1, 1)))
    ang_ref = np.degrees(np.arccos(np.clip((n_ref[mr] * true[mr]).sum(-1), -1, 1)))
    print(f"normals: {int(m.sum())} pixels (restatement {int(mr.sum())}), median angle {np.median(ang):.2f} deg (restatement "
          f"{np.median(ang_ref):.2f} deg)")
    assert mr.sum() >= 50 and m.sum() >= 0.5 * mr.sum()
    assert np.median(ang) <= 2 * np.median(ang_ref)
    assert np.abs(np.linalg.norm(n[ok], axis=-1) - 1).max() < 1e-5 and (n[~ok] == 0).all()


def test_a_hand_is_neither_kept_nor_read():
    """A hand ellipse over the sphere in frames 1 and 2: no swept or kept pixel lies on it or within a patch of it (every patch reads
    usable pixels only: the grey frames' validity map is 0 on the hand), and the gates' counts add up."""
    from dynhor_amd import mvs
    hands = [None, (150.0, 100.0, 22.0, 30.0), (118.0, 80.0, 18.0, 14.0), None, None]
    sc = MU.turned_sphere(V.E2E_DEGS, hands, k=36)
    verts, faces = V.icosphere(0.95 * V.SPHERE_E2E_R, 3)
    out = mvs.depth_maps(_dataset(sc), verts.to(DEV), faces.to(DEV), frames=V.E2E_FRAMES, **E2E)
    hand = (sc["label"] == -1)
    near = torch.nn.functional.max_pool2d(hand.float()[:, None], 9, 1, 4)[:, 0] > 0          # within the 9 x 9 patch of a hand pixel
    kept, lost = out["kept"].cpu(), out["lost"].cpu()
    assert hand[1].sum() > 500 and hand[2].sum() > 300
    assert not (kept & near).any() and not ((lost != 0) & near).any()
    for row in out["stats"]["per_frame"]:
        f = row["frame"]
        assert row["swept"] == int(((lost[f] != 0) | kept[f]).sum()) and row["kept"] + sum(row["lost"].values()) == row["swept"]
        assert row["lost"]["flags"] == int((lost[f] == 1).sum())
    clean = _e2e()[1]
    assert out["stats"]["per_frame"][0]["swept"] < clean["stats"]["per_frame"][0]["swept"]
    assert int(kept[2].sum()) > 50


# ------------------------------------------------------------------------------------------------ Runner
def _tree(d, skip=("mvs", "board")):
    out = {}
    for base, dirs, files in os.walk(d):
        dirs[:] = [x for x in dirs if not (base == d and x in skip)]
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def test_runner_writes_what_the_loader_reads(tmp_path):
    """Runner.mvs_depth on the synthetic sequence at 64 x 64 with the analytic scene's own mesh as the guide: every listed file, PNGs
    that Dataset reloads, an mvs.json that parses, board scalars; the experiment directory's other files keep their bytes.  The synthetic
    sequence's frames lie tens of degrees apart, so the stereo keeps nothing here (measured: 67 swept, all lost to flags): this run
    tests the files and that other outputs stay untouched; test_runner_output_carries_the_kept_pixels tests their content."""
    import shutil
    from dynhor_amd import mvs
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.mesh import write_ply
    from dynhor_amd.runner import Runner
    from dynhor_amd.scene import make_sequence, write_sequence_to_disk
    from dynhor_amd.tb_events import read_scalars
    frames = make_sequence(5, 64, 64, 5, device="cpu", hand=True)
    root = str(tmp_path / "seq")
    write_sequence_to_disk(frames, root)
    conf = {"seq_name": "mvs", "exp_name": "run", "data_info": {"dataroot": root},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100},
            "mvs": {"step_px": 1, "peak_margin": 0.0}}
    runner = Runner(conf=conf, mode="mvs_depth", device=DEV, exp_root=str(tmp_path))
    v, f = runner._scene_gt_mesh(64)
    mesh = str(tmp_path / "guide.ply")
    write_ply(mesh, v, f)
    with open(os.path.join(runner.base_exp_dir, "notes.txt"), "w") as fh:
        fh.write("another mode's output")
    before = _tree(runner.base_exp_dir)
    with pytest.raises(ValueError):
        runner.mvs_depth(mesh=mesh, nonsense=1)
    assert runner.mvs_depth(mesh=mesh, save=False).get("dir") is None and _tree(runner.base_exp_dir, skip=()) == before
    res = runner.mvs_depth(mesh=mesh, voxel=0.01)
    runner.close()
    d = res["dir"]
    assert d == os.path.join(runner.base_exp_dir, "mvs", "00000000") and _tree(runner.base_exp_dir) == before
    stems = runner.dataset.stems
    assert sorted(os.listdir(d)) == ["cloud.ply", "depth", "monocular_normal", "mvs.json"]
    assert sorted(os.listdir(os.path.join(d, "depth"))) == [s + ".npy" for s in stems]
    assert sorted(os.listdir(os.path.join(d, "monocular_normal"))) == [s + ".png" for s in stems]
    js = json.load(open(os.path.join(d, "mvs.json")))
    assert js["settings"]["step_px"] == 1 and js["settings"]["offsets"] == [1, 2] and js["mesh"] == mesh and js["voxel"] == 0.01
    assert len(js["per_frame"]) == 5 and len(js["lowest_kept_share"]) == 5 and set(js["per_frame"][0]["lost"]) == set(mvs.LOST)
    assert js["totals"]["kept"] == sum(r["kept"] for r in js["per_frame"]) and {"sweep", "check", "write"} <= set(js["seconds"])
    kept_total = 0
    for s in stems:
        z = np.load(os.path.join(d, "depth", s + ".npy"))
        assert z.dtype == np.float32 and z.shape == (64, 64) and not np.isnan(z).any()
        kept_total += int(np.isfinite(z).sum())
    assert kept_total == js["totals"]["kept"]
    head = open(os.path.join(d, "cloud.ply"), "rb").read(400).decode("latin1")
    assert f"element vertex {js['cloud_points']}" in head and "property float nx" in head and "property uchar red" in head
    print(f"runner: swept {js['totals']['swept']}, kept {js['totals']['kept']}, normals {js['totals']['normals']}, cloud "
          f"{js['cloud_points']}, lost {js['totals']['lost']}")
    # the loader reads the folder once the data root's monocular_normal/ is pointed at it
    shutil.rmtree(os.path.join(root, "monocular_normal"), ignore_errors=True)
    shutil.copytree(os.path.join(d, "monocular_normal"), os.path.join(root, "monocular_normal"))
    ds = Dataset({"dataroot": root}, device=DEV)
    out = mvs.depth_maps(runner.dataset, v.float().contiguous(), f.long().contiguous(), step_px=1, peak_margin=0.0)
    assert torch.equal(ds.normal, mvs.encode_normals(out["normal"], out["normal_ok"]))
    assert ((ds.normal == 128).all(-1) == ~out["normal_ok"]).all()
    board = os.path.join(runner.base_exp_dir, "board")
    tags = {tag for fn in os.listdir(board) for _, tag, _ in read_scalars(os.path.join(board, fn))}
    assert "mvs/kept_share" in tags


def test_runner_output_carries_the_kept_pixels(tmp_path):
    """Runner.mvs_depth on the end-to-end sphere written to disk (five poses 6 degrees apart, the icosphere 5 % too small as --vis_mesh,
    a grid of 4 px): pixels are kept, so the files have content.  The .npy maps are inf exactly where nothing is kept and equal
    depth_maps' depths elsewhere; the PNGs, copied to the data root's monocular_normal/, come back from Dataset as the encoded normals
    with pixels that are not 128; cloud.ply holds fuse()'s points, normals and colours record by record.  The config and the call both
    name a voxel: the call's wins."""
    import shutil
    from dynhor_amd import mvs
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.mesh import write_ply
    from dynhor_amd.runner import Runner
    from dynhor_amd.scene import write_sequence_to_disk
    sc = V.e2e_scene()
    frames = {"rgb": sc["rgb"], "label": sc["label"], "normal": torch.full_like(sc["rgb"], 128), "R": sc["R"].float(), "T": sc["T"].float(),
              "K": sc["K"]}
    root = str(tmp_path / "seq")
    write_sequence_to_disk(frames, root)
    verts, faces = V.icosphere(0.95 * V.SPHERE_E2E_R, 3)
    mesh = str(tmp_path / "guide.ply")
    write_ply(mesh, verts, faces)
    conf = {"seq_name": "mvs", "exp_name": "sphere", "data_info": {"dataroot": root},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100},
            "mvs": {"step_px": V.E2E_STEP_PX, "peak_margin": 0.0, "voxel": 0.5}}
    runner = Runner(conf=conf, mode="mvs_depth", device=DEV, exp_root=str(tmp_path))
    res = runner.mvs_depth(mesh=mesh, voxel=0.02)
    runner.close()
    d, stems, ds0 = res["dir"], runner.dataset.stems, runner.dataset
    assert res["voxel"] == 0.02 and res["totals"]["kept"] > 500 and res["totals"]["normals"] > 100
    gv, gf = verts.to(DEV), faces.to(DEV)
    out = mvs.depth_maps(ds0, gv, gf, step_px=V.E2E_STEP_PX, peak_margin=0.0)
    kept, depth = out["kept"].cpu().numpy(), out["depth"].cpu().numpy()
    assert int(kept.sum()) == res["totals"]["kept"] and int(out["normal_ok"].sum()) == res["totals"]["normals"]
    for f, s in enumerate(stems):
        z = np.load(os.path.join(d, "depth", s + ".npy"))
        assert z.dtype == np.float32 and z.shape == kept[f].shape
        assert np.array_equal(np.isfinite(z), kept[f]) and np.isposinf(z[~kept[f]]).all() and np.array_equal(z[kept[f]], depth[f][kept[f]])
    assert kept[1].sum() > 100 and kept[2].sum() > 100 and kept[3].sum() > 100
    # the loader reads the folder once the data root's monocular_normal/ is pointed at it
    shutil.rmtree(os.path.join(root, "monocular_normal"))
    shutil.copytree(os.path.join(d, "monocular_normal"), os.path.join(root, "monocular_normal"))
    ds = Dataset({"dataroot": root}, device=DEV)
    enc = mvs.encode_normals(out["normal"], out["normal_ok"])
    assert torch.equal(ds.normal, enc)
    assert torch.equal((ds.normal != 128).any(-1), out["normal_ok"]) and int(out["normal_ok"].sum()) > 100
    f, y, x = (int(v) for v in out["normal_ok"].nonzero()[0])
    n = ds.normal[f, y, x].double() / 255 * 2 - 1                      # the loader's decoding: the camera-frame normal, facing the camera
    assert float((n - out["normal"][f, y, x].double()).abs().max()) <= 1.0 / 255 + 1e-6 and float(n[2]) < 0
    # the cloud: fuse()'s records
    pts, nrm, col, idx = mvs.fuse(out["depth"], out["kept"], out["normal"], out["normal_ok"], ds0.rgb, ds0.R, ds0.T, ds0.K, 0.02)
    whole = mvs.fuse(out["depth"], out["kept"], out["normal"], out["normal_ok"], ds0.rgb, ds0.R, ds0.T, ds0.K)[0]
    raw = open(os.path.join(d, "cloud.ply"), "rb").read()
    head, body = raw[:raw.index(b"end_header\n") + 11], raw[raw.index(b"end_header\n") + 11:]
    assert f"element vertex {pts.shape[0]}\n".encode() in head and res["cloud_points"] == pts.shape[0]
    assert 50 < pts.shape[0] < whole.shape[0] == res["totals"]["normals"]          # thinned by the call's voxel, not the config's 0.5
    rec = np.frombuffer(body, dtype=[("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
    assert len(rec) == pts.shape[0]
    assert np.array_equal(rec["p"], pts.cpu().numpy()) and np.array_equal(rec["n"], nrm.cpu().numpy())
    assert np.array_equal(rec["c"], col.cpu().numpy())
    assert float((pts.double().norm(dim=1) - V.SPHERE_E2E_R).abs().median()) < 0.01     # the points lie on the true sphere, not the guide
    print(f"runner on the sphere: kept {res['totals']['kept']} of {res['totals']['swept']}, normals {res['totals']['normals']}, cloud "
          f"{pts.shape[0]} of {whole.shape[0]}, lost {res['totals']['lost']}")
