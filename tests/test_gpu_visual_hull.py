"""Visual hull on the GPU (dynhor_amd/visual_hull.py, csrc/visual_hull.hip): the signed pixel distance bit for bit against the float32
restatement, dh_hull_accumulate against the fp64 restatement (tests/visual_hull_util.py) at every launch size and m, its independence
of the order and grouping of the frames, the hull of the synthetic scene against the analytic surface, and the Runner mode and CLI.

Observed on an MI355X (test_accumulate_against_fp64, 6 frames of 48 x 64, 23,335 points, |g| up to 2.65): the float32 restatement
deviates from fp64 by at most 8.81e-7 (tol 3.52e-6), the device by at most 8.96e-7; 0.570 % of the points are ambiguous and 0.009 %
near-ties.  test_visual_hull_of_the_synthetic_scene: the device's and the restatement's meshes have the same 11,886 vertices, scene_sdf
min -0.0318 (bound -(1.5 foot + cell) = -0.0531), mean 0.0028."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import visual_hull_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_FRAME, SHIFT = 5, (0.06, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------------------ the signed map
def _edge_labels():
    """i8 [5,37,53]: three random frames of blobs with object and hand pixels on every image edge, an all-background frame and an
    all-solid frame."""
    g = torch.Generator().manual_seed(3)
    H, W = 37, 53
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    lab = torch.zeros(5, H, W, dtype=torch.int8)
    for f in range(3):
        for value in (1, -1, 1, -1):
            cx, cy = float(torch.rand(1, generator=g)) * W, float(torch.rand(1, generator=g)) * H
            r = 3 + 7 * float(torch.rand(1, generator=g))
            lab[f][(xs - cx) ** 2 + (ys - cy) ** 2 < r * r] = value
        lab[f][torch.rand(H, W, generator=g) < 0.01] = 1                       # single pixels
        for k, value in enumerate((1, -1)):                                    # both kinds on the four edges and in two corners
            lab[f, 0, 7 + 20 * k + f], lab[f, H - 1, 11 + 20 * k + f] = value, value
            lab[f, 5 + 15 * k + f, 0], lab[f, 9 + 15 * k + f, W - 1] = value, value
        lab[f, 0, 0], lab[f, H - 1, W - 1] = 1, -1
    lab[4] = 1
    lab[4, 10:20, 10:30] = -1
    return lab


@pytest.mark.parametrize("band_px", [1, 4, 16])
def test_signed_label_distance_equals_the_float32_restatement(band_px):
    from dynhor_amd.visual_hull import signed_label_distance
    lab = _edge_labels()
    want = torch.from_numpy(U.signed_label_distance(lab, band_px, np.float32))
    got = signed_label_distance(lab.to(DEV), band_px).cpu()
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert bool((got[3] == band_px).all()) and bool((got[4] == -band_px).all())          # no outline in the window: the clamp
    assert bool(((got < 0) == (lab != 0)).all()) and float(got.abs().min()) == 0.5


# ------------------------------------------------------------------------------------------------------------ accumulate
@functools.lru_cache(maxsize=None)
def _ds6():
    from dynhor_amd.dataset import Dataset
    return Dataset.from_synthetic(n_frames=6, H=48, W=64, seed=11, hand=True, device=DEV)


def _unproject(R, T, K, f, x, y, z):
    """fp64 points [n,3] that frame f projects to pixel position (x, y) at depth z."""
    c = np.stack([(x - K[0, 2]) / K[0, 0] * z, (y - K[1, 2]) / K[1, 1] * z, z], axis=-1)
    return (c - T[f]) @ R[f]


@functools.lru_cache(maxsize=None)
def _case():
    """The shared inputs and references: points f32 [n,3] (shuffled, so that every prefix mixes the kinds), the signed map of the six
    frames from the device, per-frame values in fp64 and in float32, and the ambiguous points."""
    from dynhor_amd.visual_hull import signed_label_distance
    ds = _ds6()
    rng = np.random.default_rng(7)
    R, T, K = (U.as_np(t).astype(np.float64) for t in (ds.R, ds.T, ds.K))
    H, W = ds.H, ds.W
    parts = [rng.uniform(-0.6, 0.6, (20000, 3)), rng.uniform(-6.0, 6.0, (2000, 3))]
    for f in range(6):
        n = 100
        z = rng.uniform(1.6, 3.0, n)
        parts.append(_unproject(R, T, K, f, rng.integers(1, W - 1, n).astype(np.float64), rng.integers(1, H - 1, n).astype(np.float64), z))   # centres
        parts.append(_unproject(R, T, K, f, np.full(10, W - 1.0), rng.uniform(0, H - 1, 10), z[:10]))                           # last column
        parts.append(_unproject(R, T, K, f, rng.uniform(0, W - 1, 10), np.full(10, H - 1.0), z[:10]))                           # last row
        parts.append(_unproject(R, T, K, f, np.array([0.0, W - 1.0]), np.array([0.0, H - 1.0]), z[:2]))                          # two corners
        dz = rng.choice([-1e-3, -1e-4, 1e-4, 1e-3], n)                                               # just behind / in front of the centre
        parts.append(_unproject(R, T, K, f, K[0, 2] + rng.uniform(-15, 15, n), K[1, 2] + rng.uniform(-15, 15, n), dz))
    parts.append(np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.1, 0.1, 0.1]]))
    pts = np.concatenate(parts)
    pts = pts[rng.permutation(pts.shape[0])].astype(np.float32)
    sd = signed_label_distance(ds.label, 16)
    sd_np = U.as_np(sd).astype(np.float64)
    g64, ok64, u, w, z = U.frame_values(pts, sd_np, R, T, K, np.float64, with_uv=True)
    g32, ok32 = U.frame_values(pts, sd_np, R, T, K, np.float32)
    with np.errstate(invalid="ignore"):
        amb = ((np.abs(u) < 1e-3) | (np.abs(u - (W - 1)) < 1e-3) | (np.abs(w) < 1e-3) | (np.abs(w - (H - 1)) < 1e-3)
               | (np.abs(z) < 1e-5)).any(axis=0)
    both = ok64 & ok32 & ~amb[None]
    dev32 = float(np.abs(g32.astype(np.float64) - g64)[both].max())
    return {"pts": torch.from_numpy(pts).to(DEV), "sd": sd, "g64": g64, "ok64": ok64, "amb": amb, "dev32": dev32,
            "gmax": float(np.abs(g64[ok64]).max())}


def _fresh(n, m):
    return (torch.full((n, m), float("-inf"), device=DEV), torch.full((n,), -1, dtype=torch.int32, device=DEV),
            torch.zeros(n, dtype=torch.int32, device=DEV))


def _run(pts, sd, ds, m, chunks, frame_ids=None):
    """The state after the calls `chunks` = [(first, last)] over the rows of sd, in that order."""
    from dynhor_amd.visual_hull import hull_accumulate
    topk, arg, seen = _fresh(pts.shape[0], m)
    for a, b in chunks:
        hull_accumulate(pts, sd[a:b], ds.R[a:b], ds.T[a:b], ds.K, a if frame_ids is None else frame_ids[a], topk, arg, seen)
    return topk, arg, seen


@pytest.mark.parametrize("m", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, None])
def test_accumulate_against_fp64(n, m):
    c, ds = _case(), _ds6()
    n = c["pts"].shape[0] if n is None else n
    topk, arg, seen = (t.cpu().numpy() for t in _run(c["pts"][:n].contiguous(), c["sd"], ds, m, [(0, 6)]))
    r_topk, r_arg, r_seen = U.state_from_values(c["g64"][:, :n], c["ok64"][:, :n], max(m, 2))
    amb = c["amb"][:n]
    tol = 4.0 * c["dev32"]
    assert 0 < tol < 1e-5, tol
    assert np.array_equal(seen[~amb], r_seen[~amb])
    a, b = topk[~amb].astype(np.float64), r_topk[~amb][:, :m]
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin) and bool((a[~fin] == -np.inf).all())
    dev = float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0
    with np.errstate(invalid="ignore"):
        tie = (r_topk[:, 0] - r_topk[:, 1] <= tol) & np.isfinite(r_topk[:, 1])
    exempt = amb | tie
    print(f"n {n}, m {m}: |g| <= {c['gmax']:.3f}; float32 restatement deviates from fp64 by {c['dev32']:.3e}, the device by {dev:.3e} "
          f"(tol {tol:.3e}); ambiguous {100 * amb.mean():.3f} %, near-ties {100 * tie.mean():.3f} % of {n} points")
    assert dev <= tol
    assert np.array_equal(arg[~exempt], r_arg[~exempt])
    assert bool((topk[:, :-1] >= topk[:, 1:]).all())                                 # descending, everywhere
    assert bool(((arg >= -1) & (arg < 6)).all()) and bool(((arg == -1) == (seen == 0)).all())
    if n == c["pts"].shape[0]:
        assert exempt.mean() < 0.01
        assert int((r_seen == 0).sum()) > 500 and int((r_seen == 6).sum()) > 15000   # both kinds of point are present


@pytest.mark.parametrize("m", [1, 2])
def test_accumulate_on_a_two_by_two_image(m):
    from dynhor_amd.visual_hull import signed_label_distance
    ds = _ds6()
    K = torch.tensor([[2.4, 0.0, 1.0], [0.0, 2.4, 1.0], [0.0, 0.0, 1.0]], device=DEV)
    sd = signed_label_distance(torch.tensor([[[1, 0], [-1, 0]]] * 6, dtype=torch.int8, device=DEV), 4)
    pts = torch.from_numpy(np.random.default_rng(2).uniform(-0.6, 0.6, (3000, 3)).astype(np.float32)).to(DEV)
    me = type("D", (), {"R": ds.R, "T": ds.T, "K": K})
    topk, arg, seen = (t.cpu().numpy() for t in _run(pts, sd, me, m, [(0, 6)]))
    R, T = U.as_np(ds.R).astype(np.float64), U.as_np(ds.T).astype(np.float64)
    g64, ok64, u, w, z = U.frame_values(U.as_np(pts), U.as_np(sd), R, T, U.as_np(K), np.float64, with_uv=True)
    g32, ok32 = U.frame_values(U.as_np(pts), U.as_np(sd), R, T, U.as_np(K), np.float32)
    amb = ((np.abs(u) < 1e-3) | (np.abs(u - 1) < 1e-3) | (np.abs(w) < 1e-3) | (np.abs(w - 1) < 1e-3)).any(axis=0)
    tol = 4.0 * float(np.abs(g32.astype(np.float64) - g64)[ok64 & ok32 & ~amb[None]].max())
    r_topk, r_arg, r_seen = U.state_from_values(g64, ok64, 2)
    assert int(r_seen.max()) >= 3 and amb.mean() < 0.05      # 1e-3 px of a 1 px image: more of the points
    assert np.array_equal(seen[~amb], r_seen[~amb])
    a, b = topk[~amb].astype(np.float64), r_topk[~amb][:, :m]
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin) and float(np.abs(a[fin] - b[fin]).max()) <= tol


# ------------------------------------------------------------------------------------------------------------ order independence
def test_state_does_not_depend_on_the_order_or_grouping_of_the_frames():
    c, ds = _case(), _ds6()
    pts = c["pts"]
    for m in (2, 3):
        base = _run(pts, c["sd"], ds, m, [(0, 6)])
        again = _run(pts, c["sd"], ds, m, [(0, 6)])
        assert all(torch.equal(x, y) for x, y in zip(base, again)), "two identical launches differ"
        for chunks in ([(0, 1), (1, 6)], [(0, 2), (2, 4), (4, 6)], [(4, 6), (0, 4)], [(5, 6), (4, 5), (3, 4), (2, 3), (1, 2), (0, 1)]):
            got = _run(pts, c["sd"], ds, m, chunks)
            for name, x, y in zip(("topk", "arg", "seen"), base, got):
                assert torch.equal(x, y), (m, chunks, name)


def test_equal_values_go_to_the_lower_frame():
    """Frame 2 again as frame 3: wherever that pose and mask give the largest value, arg is 2, in either order of the calls."""
    c, ds = _case(), _ds6()
    idx = torch.tensor([0, 1, 2, 2, 4], device=DEV)
    me = type("D", (), {"R": ds.R[idx].contiguous(), "T": ds.T[idx].contiguous(), "K": ds.K})
    sd = c["sd"][idx].contiguous()
    one = _run(c["pts"], sd, me, 2, [(0, 5)])
    assert not bool((one[1] == 3).any()) and int((one[1] == 2).sum()) > 1000
    twice = one[0][one[1] == 2]
    assert torch.equal(twice[:, 0], twice[:, 1])                                    # the same value twice at the top
    for chunks in ([(3, 5), (0, 3)], [(3, 4), (2, 3), (0, 2), (4, 5)]):
        got = _run(c["pts"], sd, me, 2, chunks)
        assert all(torch.equal(x, y) for x, y in zip(one, got)), chunks


def test_hull_field_chunks_and_frame_subsets():
    from dynhor_amd.visual_hull import hull_field
    c, ds = _case(), _ds6()
    base = hull_field(c["pts"], ds)
    got = hull_field(c["pts"], ds, frame_chunk=4, point_chunk=5000)
    assert all(torch.equal(x, y) for x, y in zip(base, got))
    assert base[1].shape[1] == 2 and hull_field(c["pts"][:10].contiguous(), ds, min_carve_votes=3)[1].shape[1] == 3
    r_topk, r_arg, r_seen = U.state_from_values(c["g64"][[0, 2, 3, 5]], c["ok64"][[0, 2, 3, 5]], 2, frame_index=[0, 2, 3, 5])
    h, topk, arg, seen = hull_field(c["pts"], ds, frames=[5, 0, 3, 2], min_carve_votes=2, min_seen=0.75)
    keep = ~c["amb"]
    assert np.array_equal(seen.cpu().numpy()[keep], r_seen[keep]) and set(arg.unique().tolist()) <= {-1, 0, 2, 3, 5}
    want = U.field_from_state(r_topk, r_seen, 4, 2, 0.75, 1.0)
    assert np.array_equal((h.cpu().numpy() == 1.0)[keep], (r_seen < 3)[keep])
    judged = keep & (r_seen >= 3)
    assert float(np.abs(h.cpu().numpy()[judged] - want[judged]).max()) <= 4.0 * c["dev32"]
    with pytest.raises(ValueError, match="frames"):
        hull_field(c["pts"], ds, frames=[0, 6])


# ------------------------------------------------------------------------------------------------------------ the hull
@functools.lru_cache(maxsize=None)
def _ds16():
    from dynhor_amd.dataset import Dataset
    return Dataset.from_synthetic(n_frames=16, H=96, W=96, seed=11, hand=True, device=DEV)


def _sdf(v):
    from dynhor_amd.scene import scene_sdf
    return scene_sdf(v.double())


def test_visual_hull_of_the_synthetic_scene():
    from dynhor_amd.mesh import marching_cubes
    from dynhor_amd.visual_hull import grid_points, visual_hull
    ds = _ds16()
    verts, faces, st = visual_hull(ds, resolution=64)
    foot = (float(ds.T.norm(dim=1).max()) + 0.6) / float(ds.K[0, 0])
    cell = st["cell"]
    assert st["resolution"] == 64 and abs(cell - (st["bound_max"][0] - st["bound_min"][0]) / 63) < 1e-9 and faces.shape[0] == st["faces"] > 1000
    assert all(-1.0 <= lo < hi <= 1.0 for lo, hi in zip(st["bound_min"], st["bound_max"])) and st["bound_max"][0] - st["bound_min"][0] < 1.4
    s = _sdf(verts)
    # the restatement's field on the same grid, meshed by the same marching cubes
    pts, _ = grid_points(st["bound_min"], st["bound_max"], 64, DEV)
    topk, arg, seen = U.hull_state(pts.cpu().numpy().astype(np.float64), ds.label, ds.R, ds.T, ds.K, m=2)
    h = torch.from_numpy(U.field_from_state(topk, seen, 16).astype(np.float32)).to(DEV)
    rv, rf = marching_cubes((-h).view(64, 64, 64), 0.0, st["bound_min"], st["bound_max"])
    rs = _sdf(rv)
    print(f"hull at 64^3: cell {cell:.5f}, foot {foot:.5f}; scene_sdf over {verts.shape[0]} vertices: min {float(s.min()):.5f}, mean "
          f"{float(s.mean()):.5f}; the restatement's mesh ({rv.shape[0]} vertices): min {float(rs.min()):.5f}, mean {float(rs.mean()):.5f}; "
          f"volume {st['volume']:.5f}, radius_max {st['radius_max']:.4f}")
    assert float(s.min()) >= -(1.5 * foot + cell)
    assert float(rs.mean()) > 0 and float(s.mean()) <= 1.25 * float(rs.mean())
    assert st["touches_bound"] is False
    assert abs(st["volume"] - st["inside_cells"] * cell ** 3) < 1e-12 and 0.3 < st["radius_max"] < 0.6
    sc = st["sole_carved"]
    assert len(sc["cells"]) == len(sc["share"]) == 16 and len(sc["worst"]) == 5 and sc["share_max"] == max(sc["share"]) < 0.03
    v2, f2, st2 = visual_hull(ds, resolution=64)
    assert torch.equal(verts, v2) and torch.equal(faces, f2) and st2 == st
    # a fixed box gives the same surface where the two grids agree on the object: its volume within a few cells' worth
    v3, f3, st3 = visual_hull(ds, resolution=64, bound=0.6)
    assert st3["bound_min"] == [-0.6] * 3 and st3["touches_bound"] is False and abs(st3["volume"] - st["volume"]) < 0.1 * st["volume"]


def test_an_empty_hull_names_the_poses():
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.visual_hull import visual_hull
    src = _ds16()
    frames = {"rgb": src.rgb[:4], "label": torch.zeros_like(src.label[:4]), "normal": src.normal[:4], "R": src.R[:4], "T": src.T[:4], "K": src.K}
    with pytest.raises(ValueError, match=r"empty.*4 frames of 96 x 96.*camera distances"):
        visual_hull(Dataset(frames=frames, device=DEV), resolution=32, coarse_resolution=16)


# ------------------------------------------------------------------------------------------------------------ Runner and CLI
def _conf(name):
    return {"seq_name": "vhull", "exp_name": name,
            "data_info": {"synthetic": {"n_frames": 16, "H": 96, "W": 96, "seed": 11}},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "warm_up_end": 10, "end_iter": 1000,
                      "anneal_end": 200},
            "visual_hull": {"resolution": 64}}


def test_runner_visual_hull_end_to_end(tmp_path):
    from dynhor_amd import metrics
    from dynhor_amd.runner import Runner
    from dynhor_amd.tb_events import read_scalars
    from dynhor_amd.visual_hull import VISUAL_HULL_DEFAULTS
    r = Runner(conf=_conf("e2e"), device=DEV, exp_root=str(tmp_path))
    res = r.visual_hull(simplify="faces:3000")
    d = os.path.join(str(tmp_path), "vhull", "e2e", "hull")
    assert res["dir"] == d and res["mesh"] == os.path.join(d, "hull.ply") and res["mesh_simple"] == os.path.join(d, "hull_simple.ply")
    js = json.load(open(os.path.join(d, "hull.json")))
    assert {"settings", "stats", "silhouette", "seconds", "simplify", "iter"} <= set(js)
    assert js["settings"] == dict(VISUAL_HULL_DEFAULTS, resolution=64)
    assert {"resolution", "bound_min", "bound_max", "cell", "verts", "faces", "volume", "radius_max", "touches_bound", "sole_carved"} <= set(js["stats"])
    assert {"cells", "share", "worst", "share_max", "hull2_cells"} <= set(js["stats"]["sole_carved"])
    assert {"coarse", "fine", "fine_signed_distance", "fine_accumulate", "mesh", "simplify", "silhouette"} <= set(js["seconds"])
    assert len(js["silhouette"]["frames"]) == 16 and js["silhouette"]["iou_mean"] > 0.85
    v, f = metrics.load_mesh(res["mesh"])
    assert f.shape[0] == js["stats"]["faces"] and v.shape[0] == js["stats"]["verts"]
    assert 0 < metrics.load_mesh(res["mesh_simple"])[1].shape[0] <= 3000
    tags = {tag for fn in os.listdir(os.path.join(r.base_exp_dir, "board")) for _, tag, _ in read_scalars(os.path.join(r.base_exp_dir, "board", fn))}
    assert {"hull/iou_mean", "hull/volume", "hull/sole_carved_max"} <= tags, tags
    print(f"hull of 16 frames at 64^3: silhouette IoU mean {js['silhouette']['iou_mean']:.4f}, min {js['silhouette']['iou_min']:.4f}; "
          f"sole-carved max {100 * js['stats']['sole_carved']['share_max']:.2f} %; seconds {js['seconds']}")
    # the hull as the template of the SDF warm start
    fit = r.init_sdf(mesh=res["mesh"], iters=20, points=2048, heldout_points=2048, resolution=32)
    assert fit["heldout_after"] < fit["heldout_before"], fit
    # one frame's pose shifted by about 3 px: that frame carves alone
    r.dataset.T[BAD_FRAME] += torch.tensor(SHIFT, device=DEV)
    bad = r.visual_hull(save=False)
    sc = bad["stats"]["sole_carved"]
    names = ["{:04d}".format(i) for i in range(16)] if r.dataset.stems is None else [str(s) for s in r.dataset.stems]
    print(f"frame {BAD_FRAME} shifted: sole-carved shares {[round(100 * s, 2) for s in sc['share']]} %, worst {sc['worst']}")
    assert sc["worst"][0] == names[BAD_FRAME] and "dir" not in bad
    assert sc["share"][BAD_FRAME] >= 3.0 * sorted(sc["share"])[-2]
    r.close()


def test_cli_visual_hull_prints_its_json_line(tmp_path):
    import yaml
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(dict(_conf("cli"), mesh_simplify={"mode": "faces:2000"}), fh)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--exp_root", str(tmp_path), "--mode", "visual_hull",
                        "--hull_resolution", "48", "--hull_votes", "2"],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["settings"]["resolution"] == 48 and res["settings"]["min_carve_votes"] == 2 and res["simplify"] == "faces:2000"
    assert "frames" not in res["silhouette"] and "share" not in res["stats"]["sole_carved"] and len(res["stats"]["sole_carved"]["worst"]) == 5
    for k in ("mesh", "mesh_simple"):
        assert os.path.exists(res[k]), k
    assert os.path.exists(os.path.join(res["dir"], "hull.json"))
