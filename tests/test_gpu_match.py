"""The dense frame matcher on the GPU: dh_match_gray and dh_match_search bit for bit against the numpy restatement
(tests/match_util.py, licensed by tests/test_cpu_match.py), reproducibility across launches, splits and orders of the queries, the
error codes, the mesh guide against its fp64 restatement on the device's own z-buffer, and the Runner / CLI round trip."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import match_util as M
from tests import mesh_texture_util as TU
from tests.test_gpu_pose_photo import _blur_input

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ grey
@pytest.mark.parametrize("F,H,W", [(1, 5, 70), (2, 33, 257)])
def test_gray_equals_the_float32_restatement(F, H, W):
    from dynhor_amd.match import gray_frames, match_gray
    from dynhor_amd.pose_photo import blur_frames
    rgb, usable = _blur_input(F, H, W)
    seen = 0
    # the labelled input, and the same frames with every pixel usable (the 5-row image has no usable pixel left after the erosion)
    for us in (usable, torch.ones_like(usable)):
        rgb_d, us_d = rgb.to(DEV), us.to(DEV)
        for sigma in (0.0, 1.0, 2.5):
            img = blur_frames(rgb_d, us_d, sigma)
            for a_min in (0.5, 0.93):
                gray, valid = match_gray(img, a_min)
                want_g, want_v = M.gray_ref(img.cpu().numpy(), a_min)
                assert gray.dtype == torch.uint8 and gray.shape == (F, H, W) and valid.shape == (F, H, W)
                assert torch.equal(valid.cpu(), torch.from_numpy(want_v)) and torch.equal(gray.cpu(), torch.from_numpy(want_g))
                assert int((gray * (valid == 0)).max()) == 0
                seen += int(valid.sum())
            g2, v2 = gray_frames(rgb_d, us_d, sigma, 0.93, frame_chunk=1)               # frame by frame: the same bytes
            assert torch.equal(g2, gray) and torch.equal(v2, valid)
    assert seen >= 3 * F * H * W                             # the frames with every pixel usable have grey values to compare (a < 0.93 near a border)


# ------------------------------------------------------------------------------------------------------------ search
CASES = [(1, 0), (1, 3), (4, 8), (7, 32)]
N_QUERIES = 257


@functools.lru_cache(maxsize=None)
def _search_images():
    """2 x 37 x 53 random bytes with holes in `valid`, a flat block in frame 0, and a band of period 2 in frame 1 (exact ties)."""
    g = np.random.default_rng(11)
    gray = g.integers(0, 256, (2, 37, 53), dtype=np.uint8)
    valid = np.ones((2, 37, 53), np.uint8)
    gray[0, 0:17, 0:17] = 40
    gray[1, 22:37, :] = np.tile(g.integers(0, 256, (2, 2), dtype=np.uint8), (8, 27))[:15, :53]
    valid[0, 3:6, 40:44] = 0
    valid[1, 10, 10] = 0
    valid[1, 15:18, 30:33] = 0
    valid[0, 30, 25] = 0
    return gray, valid


@functools.lru_cache(maxsize=None)
def _queries():
    g = np.random.default_rng(12)
    H, W = 37, 53
    q = []
    corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    for c in corners:
        q.append((0, 1, c[0], c[1], c[0], c[1]))                                        # the source patch leaves the image
        q.append((0, 1, 26, 22, c[0], c[1]))                                            # the guess in a corner
        q.append((1, 0, 30, 9, c[0], c[1]))
    q += [(0, 1, 26, 20, -5, -5), (0, 1, 26, 20, 60, 10), (1, 0, 30, 9, 10000, -10000), (0, 1, 26, 20, -(1 << 30), 1 << 30),
          (0, 1, 26, 20, (1 << 31) - 1, -(1 << 31)), (0, 1, 26, 20, 26, 80)]                                  # guesses outside the image
    q += [(0, 1, 8, 8, 8, 8), (0, 0, 8, 8, 30, 20), (0, 1, 7, 9, 20, 20)]                                   # flat source patches
    q += [(1, 1, x, 29, x + dx, 29 + dy) for x in (9, 20, 31, 44) for dx, dy in ((0, 0), (1, 0), (-1, 1))]  # exact ties in the band
    q += [(0, 0, 30, 22, 30, 22), (1, 1, 20, 8, 21, 7), (0, 0, 44, 25, 40, 27)]                              # fi == fj
    while len(q) < N_QUERIES - 6:
        fi, fj = int(g.integers(0, 2)), int(g.integers(0, 2))
        x, y = int(g.integers(0, W)), int(g.integers(0, H))
        q.append((fi, fj, x, y, x + int(g.integers(-6, 7)), y + int(g.integers(-6, 7))))
    q += [q[0], q[13], q[40], q[40], q[100], q[27]]                                                         # duplicates
    q = np.array(q, np.int64)
    assert q.shape == (N_QUERIES, 6)
    q[[0, 33]] = q[[33, 0]]                                 # the first query (the n == 1 case) is one that searches at every (P, R)
    assert tuple(q[0]) == (0, 0, 30, 22, 30, 22)
    return q


@functools.lru_cache(maxsize=None)
def _reference(P, R):
    gray, valid = _search_images()
    return M.search_ref(gray, valid, _queries(), P, R, 2, M.default_min_va(P))


def _device_search(q, P, R):
    from dynhor_amd.match import search
    gray, valid = (torch.from_numpy(a).to(DEV) for a in _search_images())
    return search(gray, valid, torch.from_numpy(q).to(torch.int32).to(DEV), P, R, 2, M.default_min_va(P))


@pytest.mark.parametrize("n", [1, 63, N_QUERIES])
@pytest.mark.parametrize("P,R", CASES)
def test_search_equals_the_restatement_bit_for_bit(P, R, n):
    want_i, want_f = _reference(P, R)
    oi, of = _device_search(_queries()[:n], P, R)
    assert oi.shape == (n, 4) and oi.dtype == torch.int32 and of.shape == (n, 4) and of.dtype == torch.float64
    oi, of = oi.cpu().numpy(), of.cpu().numpy()
    flags = np.bincount(want_i[:n, 2], minlength=5)
    print(f"search P {P} R {R} n {n}: flags 0/1/2/4 = {flags[0]}/{flags[1]}/{flags[2]}/{flags[4]}, ties (s1 == s2) "
          f"{int((want_f[:n, 0] == want_f[:n, 1]).sum())}, rows that differ: int {int((oi != want_i[:n]).any(1).sum())}, "
          f"float bits {int((of.view(np.int64) != want_f[:n].view(np.int64)).any(1).sum())}")
    assert np.array_equal(oi, want_i[:n])
    assert np.array_equal(of.view(np.int64), want_f[:n].view(np.int64))
    if n == N_QUERIES:                                      # the fixture does hold what it is meant to hold
        assert flags[1] >= 5 and flags[2] >= 3 and flags[0] + flags[4] >= 40
        if R >= 3:
            assert int(((want_f[:, 0] == want_f[:, 1]) & (want_f[:, 0] > 0.999)).sum()) >= 8


@pytest.mark.parametrize("P,R", [(4, 8), (7, 32)])
def test_search_is_reproducible_across_launches_splits_and_orders(P, R):
    from dynhor_amd.match import search
    q = _queries()
    oi, of = _device_search(q, P, R)
    oi2, of2 = _device_search(q, P, R)
    assert torch.equal(oi, oi2) and torch.equal(of.view(torch.int64), of2.view(torch.int64))
    gray, valid = (torch.from_numpy(a).to(DEV) for a in _search_images())
    qd = torch.from_numpy(q).to(torch.int32).to(DEV)
    for chunk in (1, 7, N_QUERIES):
        parts = [search(gray, valid, qd[s:s + chunk].contiguous(), P, R, 2, M.default_min_va(P)) for s in range(0, N_QUERIES, chunk)]
        assert torch.equal(torch.cat([p[0] for p in parts]), oi), chunk
        assert torch.equal(torch.cat([p[1] for p in parts]).view(torch.int64), of.view(torch.int64)), chunk
    perm = torch.from_numpy(np.random.default_rng(3).permutation(N_QUERIES)).to(DEV)
    pi, pf = search(gray, valid, qd[perm].contiguous(), P, R, 2, M.default_min_va(P))
    assert torch.equal(pi, oi[perm]) and torch.equal(pf.view(torch.int64), of[perm].view(torch.int64))


def test_search_error_codes():
    from dynhor_amd import _lib
    L = _lib.lib()
    gray, valid = (torch.from_numpy(a).to(DEV) for a in _search_images())
    q = torch.from_numpy(_queries()[:9]).to(torch.int32).to(DEV)
    oi = torch.empty(9, 4, dtype=torch.int32, device=DEV)
    of = torch.empty(9, 4, dtype=torch.float64, device=DEV)
    null = ctypes.c_void_p(0)

    def call(gray_=gray, valid_=valid, F=2, H=37, W=53, q_=q, n=9, P=4, R=8, excl=2, min_va=1, oi_=oi, of_=of):
        p = lambda t: t if isinstance(t, ctypes.c_void_p) else _lib.ptr(t)
        return L.dh_match_search(p(gray_), p(valid_), F, H, W, p(q_), n, P, R, excl, min_va, p(oi_), p(of_), _lib.stream())
    assert call() == 0
    before = (oi.clone(), of.clone())
    assert call(n=0, q_=null, oi_=null, of_=null) == 0                                 # n == 0: a no-op
    for kw in ({"gray_": null}, {"valid_": null}, {"q_": null}, {"oi_": null}, {"of_": null}, {"n": -1}, {"P": 0}, {"P": 8}, {"R": -1},
               {"R": 33}, {"excl": -1}, {"min_va": 0}, {"H": 0}, {"W": 0}, {"F": -1}):
        assert call(**kw) == -1, kw
    assert call(n=1 << 31) == -2 and call(H=(1 << 24) + 1) == -2
    for col, val in ((0, 2), (1, 2), (0, -1), (1, -7)):                                # a frame index outside [0, F)
        bad = q.clone()
        bad[4, col] = val
        assert call(q_=bad) == -1, (col, val)
    assert call(F=1) == -1                                                             # the queries name frame 1
    assert call() == 0 and torch.equal(oi, before[0]) and torch.equal(of.view(torch.int64), before[1].view(torch.int64))


# ------------------------------------------------------------------------------------------------------------ mesh guide
def _three_cameras(H, W):
    """One camera of mesh_texture_util.cameras and the object turned by 15 and 40 degrees about match_util.AXIS before it: views that
    share a part of the sphere, so that the guide keeps some queries and drops others (hidden, facing away, outside the image)."""
    R0, T0, K = TU.cameras(1, H, W, radius=2.2, seed=3)
    R = torch.stack([(R0[0].double() @ M.SU.axis_angle(M.AXIS, d)).float() for d in (0.0, 15.0, 40.0)])
    T = T0.expand(3, 3).clone()
    T[2, 0] += 0.35                                          # the third view off-centre: part of the sphere leaves the image
    return R.contiguous(), T.contiguous(), K


def test_mesh_guide_equals_its_restatement_on_the_device_z_buffer():
    """N = 20 sphere, three views, every second pixel of every frame as a query into both other frames: the guesses and the dropped
    set equal the fp64 restatement's from the device's own z-buffer; queries within its tolerances of a decision are left out, at most
    2 % of them."""
    from dynhor_amd.match import mesh_guesses
    from dynhor_amd.mesh_color import raster_depth
    H, W = 96, 128
    R, T, K = _three_cameras(H, W)
    verts, faces = TU.sphere_mesh((0.0, 0.0, 0.0), TU.SPHERE_R, N=20)
    dv = [t.to(DEV) for t in (verts, faces, R, T, K)]
    zbuf = raster_depth(*dv, H, W)
    ys, xs = torch.meshgrid(torch.arange(0, H, 2), torch.arange(0, W, 2), indexing="ij")
    p1 = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    fi = torch.cat([torch.full((len(p1),), i) for i in range(3) for _ in range(2)])
    fj = torch.cat([torch.full((len(p1),), j) for i in range(3) for j in range(3) if j != i])
    p = p1.repeat(6, 1)
    g, keep, guide = mesh_guesses(fi.to(DEV), fj.to(DEV), p.to(DEV), zbuf, *dv)
    want_g, want_keep, amb = M.mesh_guesses_ref(fi, fj, p, zbuf.cpu(), verts, faces, R, T, K)
    clear = ~amb
    print(f"mesh guide: {len(p)} queries, {int(want_keep.sum())} kept by the restatement, {int(amb.sum())} ambiguous "
          f"({100 * float(amb.double().mean()):.3f} %)")
    assert float(amb.double().mean()) <= 0.02
    assert 1000 < int(want_keep.sum()) < int((zbuf.cpu()[fi, p[:, 1], p[:, 0]] != -1).sum())          # some kept, some dropped
    assert torch.equal(keep.cpu()[clear], want_keep[clear])
    both = clear & want_keep
    assert torch.equal(g.cpu()[both], want_g[both])
    assert float((guide.cpu()[both] - g.cpu()[both].double()).abs().max()) <= 0.5


def test_match_frames_with_a_mesh_guide_meets_the_guided_scene_caps():
    """tests/test_cpu_match.py's guided scene through match_frames(guide="mesh"): two sphere frames 12 degrees apart with a hand
    ellipse in both, the N = 20 sphere mesh, frame 1's pose 6 degrees wrong (P 4, R 8, 3 px grid).  The same caps: at least 150 kept,
    median at most 0.75 px and below a quarter of the guide's own median error, at most 10 % beyond 1.5 px.  The fp64 restatement with a
    brute-force z-buffer gives 468 searched of 470, 211 kept, median 0.493 px against the guide's 3.06 px, 5.2 % beyond 1.5 px."""
    from types import SimpleNamespace
    from dynhor_amd.match import match_frames
    from tests.test_cpu_match import HANDS, WRONG
    sc = M.turned_sphere([0.0, 12.0], HANDS)
    verts, faces = TU.sphere_mesh((0.0, 0.0, 0.0), TU.SPHERE_R, N=20)
    Rw = torch.stack([sc["R"][0], sc["R"][1] @ M.SU.axis_angle(*WRONG)]).float()
    ds = SimpleNamespace(rgb=sc["rgb"].to(DEV), label=sc["label"].to(DEV), R=Rw.to(DEV), T=sc["T"].float().to(DEV), K=sc["K"].to(DEV))
    matches, st = match_frames(ds, verts.to(DEV), faces.to(DEV), guide="mesh", offsets=(1,), range=8, step=3)
    row = st["pairs"][0]
    assert len(matches) == 1 and (matches[0]["i"], matches[0]["j"]) == (0, 1) and st["settings"]["guide"] == "mesh"
    assert 0 < row["searched"] <= row["queries"] and row["kept"] + sum(row["lost"].values()) == row["searched"]
    k0, k1 = matches[0]["kpts0"].long(), matches[0]["kpts1"].numpy()
    assert len(k1) == row["kept"] and matches[0]["conf"].shape == (row["kept"],) and 0.0 < float(matches[0]["conf"].min()) <= 1.0
    X = sc["pts"][0][k0[:, 1], k0[:, 0]]
    u, w = (t.numpy() for t in M.project(X, sc["R"][1], sc["T"][1], sc["K"]))
    gu, gw = (t.numpy() for t in M.project(X, Rw[1], sc["T"][1], sc["K"]))
    guide_med = float(np.median(np.hypot(gu - u, gw - w)))
    med, p95, far = M.error_stats(k1, u, w)
    print(f"mesh-guided 12 deg, hands: {row['queries']} queries, {row['searched']} searched, kept {row['kept']}, lost {row['lost']}, median "
          f"{med:.3f} px (guide {guide_med:.3f} px, kept matches lie {row['median_guide_px']:.3f} px from it), p95 {p95:.3f} px, "
          f"{100 * far:.2f} % beyond 1.5 px, {st['seconds']:.2f} s")
    assert row["kept"] >= 150
    assert med <= 0.75 and med < 0.25 * guide_med
    assert far <= 0.10
    assert row["median_guide_px"] > 1.0                     # the matches moved away from the wrong guide


# ------------------------------------------------------------------------------------------------------------ Runner, CLI
def _arrays(cdir):
    out = {}
    for f in sorted(os.listdir(cdir)):
        z = np.load(os.path.join(cdir, f))
        out[f] = [(k, str(z[k].dtype), z[k].shape, z[k].tobytes()) for k in sorted(z.files)]
    return out


def test_cli_round_trip(tmp_path):
    """Three sphere frames 6 degrees apart, --mode match_frames --match_guide none --match_offsets 1,2 in a child process (3 px grid,
    R 8: the setting of the CPU scene test), then Runner.match_frames() in this process on the same experiment."""
    import yaml
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.match import gray_frames
    from dynhor_amd.mesh_color import usable_map
    from dynhor_amd.runner import Runner
    from dynhor_amd.scene import write_sequence_to_disk
    from dynhor_amd.tb_events import read_scalars
    sc = M.turned_sphere([0.0, 6.0, 12.0], None)
    frames = {"rgb": sc["rgb"], "label": sc["label"], "normal": torch.full_like(sc["rgb"], 128), "R": sc["R"].float(), "T": sc["T"].float(),
              "K": sc["K"]}
    root = str(tmp_path / "seq")
    write_sequence_to_disk(frames, root)
    conf = {"seq_name": "match", "exp_name": "cli", "data_info": {"dataroot": root},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100},
            "match": {"step": 3, "range": 8}}
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--exp_root", str(tmp_path), "--mode", "match_frames",
                        "--match_guide", "none", "--match_offsets", "1,2"], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    d = line["dir"]
    cdir = os.path.join(d, "correspondence_infos")
    assert sorted(os.listdir(cdir)) == ["0000_0001.npz", "0000_0002.npz", "0001_0002.npz"]
    js = json.load(open(os.path.join(d, "match.json")))
    assert js["settings"]["guide"] == "none" and js["settings"]["offsets"] == [1, 2] and js["settings"]["range"] == 8
    assert [(r["i"], r["j"]) for r in js["pairs"]] == [(0, 1), (0, 2), (1, 2)] and js["steps"] == [3, 3, 3]
    first = _arrays(cdir)

    # the restatement's pipeline on the same frames (grey from the device: the grey kernel has its own test)
    usable = usable_map(sc["label"].to(DEV), 1)
    gray, valid = (t.cpu().numpy() for t in gray_frames(sc["rgb"].to(DEV), usable, 1.0, 0.5))
    src = M.usable_sources_ref(gray, valid, 4, M.default_min_va(4))
    pix, steps = M.select_queries_ref(src, 3, 4096)
    total = 0
    for row in js["pairs"]:
        i, j = row["i"], row["j"]
        pi = pix[pix[:, 0] == i]
        dx, dy = M.box_guess_ref(sc["label"].numpy(), i, j)
        q = np.concatenate([np.full((len(pi), 1), i), np.full((len(pi), 1), j), pi[:, 1:3], pi[:, 1:3] + np.array([dx, dy])], 1)
        res = M.match_pairs_ref(gray, valid, q, 4, 8)
        k = res["keep"]
        z = np.load(os.path.join(cdir, "%04d_%04d.npz" % (i, j)))
        assert row["queries"] == row["searched"] == len(q) and row["kept"] == int(k.sum()) == len(z["conf"])
        assert [row["lost"][name] for name in M.LOST] == np.bincount(res["lost"], minlength=5)[1:].tolist()
        assert row["kept"] + sum(row["lost"].values()) == row["searched"]
        assert np.array_equal(z["kpts0"], q[k, 2:4].astype(np.float32)) and z["kpts0"].dtype == np.float32
        assert np.array_equal(z["kpts1"], res["kpts1"][k]) and np.array_equal(z["conf"], res["conf"][k])
        total += row["kept"]
        if (i, j) == (0, 1):                                # the caps of tests/test_cpu_match.py's unguided scene
            X = sc["pts"][0][q[k, 3], q[k, 2]]
            u, w = (t.numpy() for t in M.project(X, sc["R"][1], sc["T"][1], sc["K"]))
            med, p95, far = M.error_stats(z["kpts1"], u, w)
            print(f"pair (0, 1): {len(q)} queries, kept {row['kept']} ({k.mean():.3f}), median {med:.3f} px, p95 {p95:.3f} px, "
                  f"{100 * far:.2f} % beyond 1.5 px; whole mode {js['seconds']:.2f} s")
            assert k.mean() >= 0.5 and med <= 0.5 and far <= 0.02
    assert js["totals"]["kept"] == total and js["totals"]["pairs"] == 3

    # a Dataset that is pointed at the folder loads them
    ds = Dataset({"dataroot": root, "correspondence_infos": cdir}, device=DEV)
    assert ds.corr is not None and ds.corr.shape == (total, 6) and ds.corr_dropped == 0
    assert Dataset({"dataroot": root}, device=DEV).corr is None

    # the same mode in this process: the same bytes on disk, and the dataset carries the rows
    runner = Runner(conf_path=cfg, mode="match_frames", device=DEV, exp_root=str(tmp_path))
    res = runner.match_frames(guide="none", offsets="1,2")
    runner.close()
    assert res["dir"] == d and _arrays(cdir) == first
    assert torch.equal(runner.dataset.corr.cpu(), ds.corr.cpu()) and torch.equal(runner.dataset.corr_pair.cpu(), ds.corr_pair.cpu())
    board = os.path.join(os.path.dirname(d), "board")
    tags = {tag for fn in os.listdir(board) for _, tag, _ in read_scalars(os.path.join(board, fn))}
    assert {"match/kept", "match/kept_share"} <= tags, tags
