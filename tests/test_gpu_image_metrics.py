"""GPU: dh_ssim against the numpy restatement (tests/image_metrics_util.py, licensed by tests/test_cpu_image_metrics.py) -- the map bit for
bit, the integer sums exactly, the two float sums within the reordering bound --, reproducibility across launches and splits, writes
confined to their regions, image_metrics.ssim_frames, and Runner.evaluate_views with held-out frames through the CLI."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import image_metrics_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_H, TILE_W = 16, 32                     # image_metrics.hip: IM_TH, IM_TW
SIZES = [(1, 1), (7, 5), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (TILE_H - 1, TILE_W - 1), (40, 130)]
RADII = {0: None, 1: 0.5, 5: 1.5, 16: 4.0}  # radius -> sigma
W_MINS = (1, 1 << 31, 1 << 32)
MASKS = ("null", "ones", "random", "zero", "disc", "island")
IMAGES = ("random", "identical", "white", "black_white", "checker")


def _taps(radius):
    from dynhor_amd import image_metrics as im
    return [65536] if radius == 0 else im.gaussian_taps_q16(RADII[radius], radius)


def _mask(kind, H, W, rng):
    if kind == "ones":
        return np.ones((H, W), np.uint8)
    if kind == "random":
        return (rng.random((H, W)) < 0.5).astype(np.uint8)
    if kind == "zero":
        return np.zeros((H, W), np.uint8)
    if kind == "disc":
        return U.disc_mask(H, W, H // 2, W // 2, max(1, min(H, W) // 2))
    m = np.zeros((H, W), np.uint8)
    m[H // 2, W // 2] = 1
    return m


def _images(kind, H, W, rng):
    y, x = np.mgrid[0:H, 0:W]
    if kind == "random":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "identical":
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        return a, a.copy()
    if kind == "white":
        return np.full((H, W, 3), 255, np.uint8), np.full((H, W, 3), 255, np.uint8)
    if kind == "black_white":
        return np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8)
    a = (((x + y) & 1) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    return a, 255 - a


def run_ssim(a, b, usable, taps, radius, w_min, want_map=True):
    """dh_ssim on device tensors through the raw C ABI: (map f32 [F,H,W] or None, out f64 [F,6]) on the device."""
    from dynhor_amd import _lib
    L = _lib.lib()
    F, H, W, _ = a.shape
    out = torch.full((F, 6), -7.0, dtype=torch.float64, device=a.device)
    smap = torch.full((F, H, W), -7.0, dtype=torch.float32, device=a.device) if want_map else None
    ws = torch.empty(max(16, int(L.dh_ssim_workspace(F, H, W))), dtype=torch.uint8, device=a.device)
    t = (ctypes.c_int32 * len(taps))(*taps)
    _lib.check(L.dh_ssim(_lib.ptr(a), _lib.ptr(b), _lib.ptr(usable) if usable is not None else None, F, H, W, t, radius, w_min,
                         _lib.ptr(smap) if want_map else None, _lib.ptr(out), _lib.ptr(ws), _lib.stream()))
    return smap, out


def _check_against_ref(smap, out, ref, tag):
    got_map, got = smap.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(got_map, ref["map"]), f"{tag}: the map differs at {int((got_map != ref['map']).sum())} pixels"
    assert np.array_equal(got[:, 1:5], ref["out"][:, 1:5]), f"{tag}: integer sums {got[:, 1:5]} != {ref['out'][:, 1:5]}"
    n = ref["out"][:, 1]
    for k, tot in ((0, ref["abs0"]), (5, ref["abs5"])):
        err, bound = np.abs(got[:, k] - ref["out"][:, k]), n * 2.0 ** -53 * tot
        assert np.all(err <= bound), f"{tag}: sum {k} off by {err.max()} (bound {bound[err.argmax()]})"


@pytest.mark.parametrize("radius", sorted(RADII))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_matches_the_restatement(size, radius):
    """Every mask x every image pair as the frames of one call, at each w_min; then `usable` null on the same pictures."""
    H, W = size
    rng = np.random.default_rng(1000 * H + 10 * W + radius)
    taps = _taps(radius)
    A, B, M = [], [], []
    for mk in MASKS[1:]:
        for ik in IMAGES:
            a, b = _images(ik, H, W, rng)
            A.append(a), B.append(b), M.append(_mask(mk, H, W, rng))
    A, B, M = np.stack(A), np.stack(B), np.stack(M)
    M[0][M[0] == 1] = 7                                              # any non-zero byte is usable
    a, b, m = (torch.from_numpy(v).to(DEV) for v in (A, B, M))
    for w_min in W_MINS:
        ref = U.ssim_ref(A, B, M, taps, w_min)
        smap, out = run_ssim(a, b, m, taps, radius, w_min)
        _check_against_ref(smap, out, ref, f"{H}x{W} r{radius} w_min {w_min}")
        zero = slice(2 * len(IMAGES), 3 * len(IMAGES))                # the all-zero masks
        assert not smap[zero].any() and not out[zero].any()
        ident = [k for k in range(len(A)) if k % len(IMAGES) in (1, 2)]
        s = smap[ident].cpu().numpy()
        assert np.all(s[ref["counted"][ident]] == 1.0), "identical pictures must score exactly 1 on every counted pixel"
    n = len(IMAGES)
    for w_min in W_MINS:
        ref = U.ssim_ref(A[:n], B[:n], None, taps, w_min)
        smap, out = run_ssim(a[:n].contiguous(), b[:n].contiguous(), None, taps, radius, w_min)
        _check_against_ref(smap, out, ref, f"{H}x{W} r{radius} w_min {w_min} null mask")
        if w_min == 1:
            assert ref["counted"].all()
    one = run_ssim(a[:1].contiguous(), b[:1].contiguous(), m[:1].contiguous(), taps, radius, 1 << 31)
    ref = U.ssim_ref(A[:1], B[:1], M[:1], taps, 1 << 31)
    _check_against_ref(one[0], one[1], ref, f"{H}x{W} r{radius} one frame")


def test_reproducible_across_launches_splits_and_without_a_map():
    H, W, radius = 37, 70, 5
    rng = np.random.default_rng(5)
    taps = _taps(radius)
    a = torch.from_numpy(rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)).to(DEV)
    b = torch.from_numpy(rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)).to(DEV)
    m = torch.from_numpy((rng.random((3, H, W)) < 0.8).astype(np.uint8)).to(DEV)
    m1, o1 = run_ssim(a, b, m, taps, radius, 1 << 31)
    m2, o2 = run_ssim(a, b, m, taps, radius, 1 << 31)
    assert torch.equal(m1, m2) and torch.equal(o1, o2)
    ma, oa = run_ssim(a[:1].contiguous(), b[:1].contiguous(), m[:1].contiguous(), taps, radius, 1 << 31)
    mb, ob = run_ssim(a[1:].contiguous(), b[1:].contiguous(), m[1:].contiguous(), taps, radius, 1 << 31)
    assert torch.equal(torch.cat([ma, mb]), m1) and torch.equal(torch.cat([oa, ob]), o1)
    none, o3 = run_ssim(a, b, m, taps, radius, 1 << 31, want_map=False)
    assert none is None and torch.equal(o3, o1)


def test_no_write_outside_the_workspace_and_the_map():
    from dynhor_amd import _lib
    L = _lib.lib()
    F, H, W, radius = 2, 19, 45, 5
    rng = np.random.default_rng(6)
    taps = _taps(radius)
    a = torch.from_numpy(rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)).to(DEV)
    b = torch.from_numpy(rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)).to(DEV)
    nws, pad = int(L.dh_ssim_workspace(F, H, W)), 4096
    assert nws == F * 2 * 2 * 6 * 8
    ws = torch.full((nws + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
    smap = torch.full((F * H * W + 2 * pad,), 12345.0, dtype=torch.float32, device=DEV)
    out = torch.full((F * 6 + 2 * pad,), 12345.0, dtype=torch.float64, device=DEV)
    t = (ctypes.c_int32 * len(taps))(*taps)
    _lib.check(L.dh_ssim(_lib.ptr(a), _lib.ptr(b), None, F, H, W, t, radius, 1 << 31, _lib.ptr(smap[pad:]), _lib.ptr(out[pad:]),
                         _lib.ptr(ws[pad:]), _lib.stream()))
    torch.cuda.synchronize()
    assert bool((ws[:pad] == 0xA5).all()) and bool((ws[pad + nws:] == 0xA5).all())
    assert bool((smap[:pad] == 12345.0).all()) and bool((smap[pad + F * H * W:] == 12345.0).all())
    assert bool((out[:pad] == 12345.0).all()) and bool((out[pad + F * 6:] == 12345.0).all())
    ref = U.ssim_ref(a.cpu().numpy(), b.cpu().numpy(), None, taps, 1 << 31)
    _check_against_ref(smap[pad:pad + F * H * W].view(F, H, W), out[pad:pad + F * 6].view(F, 6), ref, "canary")


def test_ssim_frames_chunks_and_errors():
    from dynhor_amd import image_metrics as im
    rng = np.random.default_rng(7)
    F, H, W = 5, 33, 50
    A = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    B = np.clip(A.astype(int) + rng.integers(-30, 31, A.shape), 0, 255).astype(np.uint8)
    M = np.stack([U.disc_mask(H, W, 16, 25, 14)] * F)
    M[4] = 0
    B[3] = A[3]
    a, b, m = (torch.from_numpy(v).to(DEV) for v in (A, B, M))
    whole = im.ssim_frames(a, b, m, want_map=True, chunk=16)
    for chunk in (1, 2, 5):
        part = im.ssim_frames(a, b, m, want_map=True, chunk=chunk)
        assert torch.equal(part["sums"], whole["sums"]) and torch.equal(part["map"], whole["map"])
        assert all(part[k] == whole[k] for k in ("ssim", "ssim_std", "psnr", "l1", "counted", "usable"))
    ref = U.ssim_ref(A, B, M, im.gaussian_taps_q16(1.5, 5), 1 << 31)
    assert np.array_equal(whole["map"].cpu().numpy(), ref["map"])
    assert whole["counted"] == [int(v) for v in ref["out"][:, 1]] and whole["usable"] == [int(v) for v in ref["out"][:, 4]]
    assert whole["ssim"][3] == 1.0 and whole["ssim_std"][3] == 0.0 and whole["psnr"][3] == float("inf") and whole["l1"][3] == 0.0
    assert whole["ssim"][4] is None and whole["psnr"][4] is None and whole["l1"][4] is None and whole["usable"][4] == 0
    assert abs(whole["ssim"][0] - ref["out"][0, 0] / ref["out"][0, 1]) < 1e-12
    se = float(((A[0].astype(int) - B[0].astype(int)) ** 2 * M[0][..., None]).sum())
    assert abs(whole["psnr"][0] - 10.0 * np.log10(65025.0 * 3.0 * int(M[0].sum()) / se)) < 1e-12
    assert "map" not in im.ssim_frames(a, b, None)
    with pytest.raises(TypeError, match="b must be torch.uint8"):
        im.ssim_frames(a, b.float(), m)
    with pytest.raises(ValueError, match="usable must be"):
        im.ssim_frames(a, b, m[:, :-1])
    with pytest.raises(ValueError, match="a must be contiguous"):
        im.ssim_frames(a.permute(0, 2, 1, 3)[:, :, :, :], b.permute(0, 2, 1, 3).contiguous(), None)
    with pytest.raises(ValueError, match="chunk"):
        im.ssim_frames(a, b, m, chunk=0)
    with pytest.raises(ValueError, match="min_weight"):
        im.ssim_frames(a, b, m, min_weight=0.0)
    empty = im.ssim_frames(a[:0], b[:0], m[:0], want_map=True)
    assert empty["ssim"] == [] and empty["map"].shape == (0, H, W)


# ------------------------------------------------------------------------------------------------ the Runner and the CLI
def _conf(name, holdout=None):
    tr = {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "warm_up_end": 10, "end_iter": 1000,
          "anneal_end": 200}
    if holdout is not None:
        tr["holdout"] = holdout
    # 8 frames of 64 x 64, seed 17: with the restatement on these labels (CPU) every frame counts 0.93 to 0.98 of its usable pixels at
    # the default window and min_weight 0.5 (frame 0: 205 of 220, frame 4: 287 of 305)
    return {"seq_name": "im", "exp_name": name, "data_info": {"synthetic": {"n_frames": 8, "H": 64, "W": 64, "seed": 17}}, "train": tr,
            "model": {"family": "neus"}}


def _cli(cfg, exp_root, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--mode", "evaluate_views", "--is_continue",
                        "--exp_root", exp_root, *extra], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def held(tmp_path_factory):
    """A run with train.holdout every:4 trained for six iterations, its checkpoint, and the pictures render_views draws of it."""
    import yaml
    from types import SimpleNamespace
    from dynhor_amd.runner import Runner
    tmp = tmp_path_factory.mktemp("held")
    conf = _conf("h", "every:4")
    r = Runner(conf=conf, device=DEV, exp_root=str(tmp))
    assert r.holdout_frames == [0, 4] and r.train_frames == [1, 2, 3, 5, 6, 7]
    drawn = []
    for _ in range(6):
        drawn.append(r.frame_for_slot(r.iter_step))
        r.train_iteration()
    assert sorted(drawn) == r.train_frames
    r.save_checkpoint()
    cfg = str(tmp / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    views = r.render_views("frames", save=False)
    return SimpleNamespace(r=r, cfg=cfg, root=str(tmp), views=views)


def test_psnr_agrees_with_render_views(held):
    from dynhor_amd import image_metrics as im
    from dynhor_amd.mesh_color import usable_map
    ds = held.r.dataset
    res = im.ssim_frames(held.views["rgb"].to(DEV).contiguous(), ds.rgb.contiguous(), usable_map(ds.label.contiguous(), 0))
    assert len(res["psnr"]) == 8
    for got, want in zip(res["psnr"], held.views["psnr"]):
        print(got, want)
        assert abs(got - want) < 1e-3
    for c, u in zip(res["counted"], res["usable"]):
        assert u > 0 and c >= 0.9 * u, (c, u)


def test_evaluate_views_cli_scores_the_held_out_frames(held):
    from PIL import Image
    from dynhor_amd import image_metrics as im
    from dynhor_amd.mesh_color import usable_map
    r, ds = held.r, held.r.dataset
    d = os.path.join(r.base_exp_dir, "image_eval", "{:0>8d}".format(r.iter_step))
    js = _cli(held.cfg, held.root)
    assert js["dir"] == d and js["n_holdout"] == 2 and js["n_train"] == 0 and js["method"] == "surface"
    auto = json.load(open(os.path.join(d, "eval.json")))
    assert [x["frame"] for x in auto["frames"]] == ["0000", "0004"] and all(x["split"] == "holdout" for x in auto["frames"])
    assert auto["settings"] == {"frames": "auto", "sigma": 1.5, "radius": 5, "min_weight": 0.5, "erode_px": 0, "maps": False}
    assert auto["ssim_train"] is None and auto["ssim_holdout"] == auto["ssim_mean"]
    assert not [f for f in os.listdir(d) if f.endswith(".png")]

    js = _cli(held.cfg, held.root, "--eval_frames", "all", "--eval_maps")
    full = json.load(open(os.path.join(d, "eval.json")))
    rows = full["frames"]
    assert [x["frame"] for x in rows] == ["{:04d}".format(k) for k in range(8)]
    assert [x["split"] for x in rows] == ["holdout" if k % 4 == 0 else "train" for k in range(8)]
    want = im.ssim_frames(held.views["rgb"].to(DEV).contiguous(), ds.rgb.contiguous(), usable_map(ds.label.contiguous(), 0),
                          want_map=True)
    for k, x in enumerate(rows):
        for key in ("psnr", "ssim", "ssim_std", "l1", "counted", "usable"):
            assert x[key] == want[key][k], (k, key, x[key], want[key][k])
        assert x["usable"] > 0 and x["counted"] >= 0.9 * x["usable"]
    for x, y in zip(auto["frames"], (rows[0], rows[4])):
        assert (x["frame"], x["usable"], x["counted"]) == (y["frame"], y["usable"], y["counted"])
    for key in ("psnr", "ssim", "l1"):
        for split in ("train", "holdout"):
            v = [x[key] for x in rows if x["split"] == split]
            assert abs(full[f"{key}_{split}"] - np.mean(v)) < 1e-12
        assert abs(full[key + "_mean"] - np.mean([x[key] for x in rows])) < 1e-12
        assert js[key + "_mean"] == full[key + "_mean"]
    worst = sorted(rows, key=lambda x: x["ssim"])[:5]
    assert [w["frame"] for w in full["worst_ssim"]] == [w["frame"] for w in worst]
    grey = (want["map"].clamp(0, 1) * 255.0).round().to(torch.uint8).cpu().numpy()
    for k in range(8):
        png = np.asarray(Image.open(os.path.join(d, "{:04d}_ssim.png".format(k))))
        assert png.shape == (64, 64) and np.array_equal(png, grey[k])
    board = os.path.join(r.base_exp_dir, "board")
    assert os.path.isdir(board) and os.listdir(board)


def test_evaluate_views_selections_and_errors(held):
    r = held.r
    assert r.eval_frame_indices("auto") == [0, 4] and r.eval_frame_indices("holdout") == [0, 4]
    assert r.eval_frame_indices("train") == [1, 2, 3, 5, 6, 7] and r.eval_frame_indices("all") == list(range(8))
    assert r.eval_frame_indices("every:3:1") == [1, 4, 7] and r.eval_frame_indices("0002,0005") == [2, 5]
    with pytest.raises(ValueError, match="image_eval.frames"):
        r.eval_frame_indices("0099")
    res = r.evaluate_views(frames="0001", save=False)
    assert res["dir"] is None and [x["frame"] for x in res["frames"]] == ["0001"] and res["frames"][0]["split"] == "train"
    assert "map" not in res
    # the volume method at half resolution: the frame and the mask are subsampled as the picture is
    vol = r.evaluate_views(frames="0005", method="volume", level=2, maps=True, save=False)
    row = vol["frames"][0]
    assert vol["method"] == "volume" and vol["level"] == 2 and vol["map"].shape == (1, 32, 32)
    assert row["usable"] == int((r.dataset.label[5, ::2, ::2] == 1).sum()) and 0 < row["counted"] <= row["usable"]
    assert int((vol["map"][0] != 0).sum()) <= row["counted"] and row["psnr"] is not None and -1.0 <= row["ssim"] <= 1.0


def test_holdout_errors_and_a_checkpoint_of_another_split(held, tmp_path):
    from dynhor_amd.runner import Runner
    with pytest.raises(ValueError, match="train.holdout"):
        Runner(conf=_conf("e1", "every:1"), device=DEV, exp_root=str(tmp_path))
    with pytest.raises(ValueError, match="train.holdout"):
        Runner(conf=_conf("e2", ["0042"]), device=DEV, exp_root=str(tmp_path))
    conf = _conf("e3", "every:4")
    conf["train"]["corr_weight"] = 0.1
    with pytest.raises(ValueError, match="corr_weight"):
        Runner(conf=conf, device=DEV, exp_root=str(tmp_path))
    ck = os.path.join(held.r.base_exp_dir, "checkpoints", "ckpt_{:0>6d}.pth".format(held.r.iter_step))
    other = Runner(conf=_conf("e4"), device=DEV, exp_root=str(tmp_path))
    assert other.holdout_frames == [] and other.eval_frame_indices("auto") == list(range(8))
    with pytest.raises(ValueError, match="train.holdout"):
        other.load_checkpoint(ck)
    with pytest.raises(ValueError, match="selects no frame"):
        other.eval_frame_indices("holdout")


def test_no_holdout_trains_exactly_as_a_configuration_without_the_key(tmp_path):
    from dynhor_amd import schedules
    from dynhor_amd.runner import Runner
    plain = Runner(conf=_conf("p"), device=DEV, exp_root=str(tmp_path))
    none = Runner(conf=_conf("n", "none"), device=DEV, exp_root=str(tmp_path))
    perm = schedules.FramePermutation(8, plain.conf["train"]["ray_seed"])
    for k in range(3):
        assert plain.frame_for_slot(k) == none.frame_for_slot(k) == perm.frame(k)
        sa, sb = plain.train_iteration(), none.train_iteration()
        assert torch.equal(sa, sb)
    assert torch.equal(plain.store.flat, none.store.flat)
    a, b = plain.frame_perm.state_dict(), none.frame_perm.state_dict()
    assert set(a) == set(b) == {"gen", "perm", "epoch"} and torch.equal(a["perm"], b["perm"]) and torch.equal(a["gen"], b["gen"])
