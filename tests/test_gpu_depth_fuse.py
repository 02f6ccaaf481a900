"""Depth fusion on the GPU (dynhor_amd/depth_fuse.py, csrc/tsdf.hip): dh_tsdf_integrate frame by frame against the fp64 restatement
(tests/depth_fuse_util.py) at every launch size, its integer identities (any order, any split, any start), its edges, fuse_field's
chunks and bricks, the dented sphere end to end against the analytic surface, the hull and the restatement, and the Runner mode and
CLI.

The tolerance of test 1 is four times the float32 restatement's own max |q32 - q64| on the fixture, per unit of weight: 4 x 1 = 4 of
65536 (6.1e-5 of trunc), computed in the test from the restatement, not from the kernel.

Observed on an MI355X: the device deviates from fp64 by at most 1 of 65536 per unit of weight (0 at n <= 65), 0.382 % of the 96,042
pairs ambiguous.  test_fused_mesh_of_the_dented_sphere (64^3, cell 0.0189): dent median 0.01045, 95th percentile 0.01212 over 596
vertices, the restatement's mesh the same to five digits (ratios 1.000; max |field - restatement| 9.0e-6), the hull's 0.1140 and
0.2036 (10.9 x, 16.8 x); outside the dent at most 0.01295; 3,952 carved cells; frame 3 scaled by 1.03: residual median 0.0231
against at most 0.0032.  The Runner on eleven of the twelve frames: dent median 0.01045, outside the dent at most 0.0172, IoU 0.9956."""
import functools
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import depth_fuse_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the kernel
@functools.lru_cache(maxsize=None)
def _case():
    """The fixture on the device and its references (computed once, never changed)."""
    fx = U.kernel_fixture()
    r = U.fixture_references(fx)
    t = {"pts": torch.from_numpy(fx["pts"]).to(DEV), "depth": torch.from_numpy(fx["depth"]).to(DEV),
         "weight": torch.from_numpy(fx["weight"]).to(DEV), "R": torch.from_numpy(fx["R"]).float().to(DEV),
         "T": torch.from_numpy(fx["T"]).float().to(DEV), "K": torch.from_numpy(fx["K"]).float().to(DEV)}
    return fx, r, t


def _zeros(n):
    return (torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV),
            torch.zeros(n, dtype=torch.int32, device=DEV))


def _run(t, trunc, calls, pts=None, state=None):
    """The state after the calls `calls` = [frame indices of one call], in that order, started from `state` (default zeros)."""
    from dynhor_amd.depth_fuse import integrate
    pts = t["pts"] if pts is None else pts
    num, den, obs = _zeros(pts.shape[0]) if state is None else tuple(s.clone() for s in state)
    for frames in calls:
        idx = torch.tensor(list(frames), device=DEV, dtype=torch.long)
        integrate(pts, t["depth"][idx].contiguous(), t["weight"][idx].contiguous(), t["R"][idx].contiguous(), t["T"][idx].contiguous(),
                  t["K"], trunc, num, den, obs)
    return num, den, obs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, None])
def test_each_frame_alone_against_fp64(n):
    fx, r, t = _case()
    n = fx["pts"].shape[0] if n is None else n
    v64, amb = r["v64"], r["amb"]
    tol = 4 * r["dq"]
    assert 4 <= tol <= 16, tol
    pts = t["pts"][:n].contiguous()
    worst = 0
    for f in range(6):
        num, den, obs = (x.cpu().numpy().astype(np.int64) for x in _run(t, fx["trunc"], [[f]], pts=pts))
        ok, q, wt, a = v64["ok"][f, :n], v64["q"][f, :n], v64["wt"][f, :n], amb[f, :n]
        sure = ~a
        assert np.array_equal(obs[sure], ok[sure].astype(np.int64)) and np.array_equal(den[sure], np.where(ok, wt, 0)[sure])
        err = np.abs(num - np.where(ok, wt * q, 0))
        assert bool((err[sure] <= wt[sure] * tol).all()), (f, int(err[sure].max()))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, int(np.nan_to_num(err[sure & ok] / wt[sure & ok]).max()) if (sure & ok).any() else 0)
        # inside the ambiguous pairs the state is one of the two verdicts: nothing, or one pixel's contribution
        none = (num == 0) & (den == 0) & (obs == 0)
        one = (obs == 1) & (den >= 1) & (den <= 255) & (np.abs(num) <= den * U.Q_ONE)
        assert bool((none | one)[a].all())
        with np.errstate(invalid="ignore"):
            edge = a & (np.abs(v64["d"][f, :n] + float(np.float32(fx["trunc"]))) <= 1e-5) & (wt > 0)      # d = -trunc: skipped, or q about -65536
        slack = int(np.ceil(1e-5 / fx["trunc"] * U.Q_ONE)) + tol
        assert bool((none | ((den == wt) & (np.abs(num + wt * U.Q_ONE) <= wt * slack)))[edge].all())
    print(f"n {n}: tol {tol} (4 x max |q32 - q64| = {r['dq']}) of 65536; the device deviates from fp64 by at most {worst}; "
          f"{100 * amb[:, :n].mean():.3f} % of the pairs ambiguous")


def test_integer_identities():
    fx, r, t = _case()
    tr = fx["trunc"]
    whole = _run(t, tr, [range(6)])
    assert int(whole[2].max()) >= 3 and int((whole[1] > 0).sum()) > 3000
    again = _run(t, tr, [range(6)])
    assert all(torch.equal(x, y) for x, y in zip(whole, again)), "two identical launches differ"
    singles = [_run(t, tr, [[f]]) for f in range(6)]                                  # (a) the sum of the single-frame states
    for k in range(3):
        assert torch.equal(whole[k], sum(s[k] for s in singles)), k
    for calls in ([[5, 4, 3, 2, 1, 0]], [[0], range(1, 6)], [range(3), range(3, 6)], [[f] for f in range(6)], [[4, 5], [0, 1, 2, 3]]):   # (b)
        got = _run(t, tr, calls)
        assert all(torch.equal(x, y) for x, y in zip(whole, got)), calls
    perm = torch.randperm(t["pts"].shape[0], generator=torch.Generator().manual_seed(1)).to(DEV)      # (c) the points in another order
    got = _run(t, tr, [range(6)], pts=t["pts"][perm].contiguous())
    assert all(torch.equal(x[perm], y) for x, y in zip(whole, got))
    for i in (0, 1, 777, 4096):                                                       # ... and one point per call
        got = _run(t, tr, [range(6)], pts=t["pts"][i:i + 1].contiguous())
        assert all(torch.equal(x[i:i + 1], y) for x, y in zip(whole, got)), i
    g = torch.Generator().manual_seed(2)                                              # (d) on top of a state that is not zero
    n = t["pts"].shape[0]
    start = (torch.randint(-2 ** 40, 2 ** 40, (n,), generator=g).to(DEV), torch.randint(0, 2 ** 20, (n,), generator=g).int().to(DEV),
             torch.randint(0, 1000, (n,), generator=g).int().to(DEV))
    got = _run(t, tr, [range(6)], state=start)
    assert all(torch.equal(s + x, y) for s, x, y in zip(start, whole, got))


def _one(pt, depth, weight, trunc=0.5, K=((2.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, 1.0)), state=None):
    """One point against frames of the identity pose: x_cam = p, exact arithmetic for the values below."""
    from dynhor_amd.depth_fuse import integrate
    depth = torch.tensor(depth, dtype=torch.float32, device=DEV)
    F = depth.shape[0]
    weight = torch.tensor(weight, dtype=torch.uint8, device=DEV)
    pts = torch.tensor([pt], dtype=torch.float32, device=DEV)
    num, den, obs = _zeros(1) if state is None else state
    integrate(pts, depth, weight, torch.eye(3, device=DEV).repeat(F, 1, 1), torch.zeros(F, 3, device=DEV),
              torch.tensor(K, dtype=torch.float32, device=DEV), trunc, num, den, obs)
    return int(num), int(den), int(obs)


def test_edges():
    from dynhor_amd.depth_fuse import integrate
    inf, nan = float("inf"), float("nan")
    # a 1 x 1 image: its only pixel covers u, w in [-0.5, 0.5)
    assert _one((0.0, 0.0, 2.0), [[[2.0]]], [[[200]]]) == (0, 200, 1)                 # exactly d = 0: num += 0, den += wt
    assert _one((0.0, 0.0, 2.0), [[[3.0]]], [[[200]]]) == (200 * 65536, 200, 1)       # d = 1 > trunc: exactly wt 65536
    assert _one((0.0, 0.0, 2.0), [[[2.25]]], [[[7]]]) == (7 * 32768, 7, 1)            # d = trunc / 2
    assert _one((0.0, 0.0, 2.0), [[[1.75]]], [[[7]]]) == (-7 * 32768, 7, 1)
    assert _one((0.0, 0.0, 2.0), [[[1.5]]], [[[7]]]) == (-7 * 65536, 7, 1)            # d = -trunc is not < -trunc
    assert _one((0.0, 0.0, 2.0), [[[1.25]]], [[[7]]]) == (0, 0, 0)                    # hidden
    assert _one((0.0, 0.0, 2.0), [[[2.0]]], [[[0]]]) == (0, 0, 0)                     # no weight
    assert _one((0.4, 0.0, 2.0), [[[2.0]]], [[[9]]]) == (0, 9, 1)                     # u = 0.4: this pixel
    assert _one((0.6, 0.0, 2.0), [[[2.0]]], [[[9]]]) == (0, 0, 0)                     # u = 0.6: outside
    assert _one((0.0, -0.6, 2.0), [[[2.0]]], [[[9]]]) == (0, 0, 0)
    assert _one((0.0, 0.0, -2.0), [[[2.0]]], [[[9]]]) == (0, 0, 0)                    # behind the camera
    assert _one((0.0, 0.0, 0.0005), [[[2.0]]], [[[9]]], trunc=4.0) == (0, 0, 0)       # c_2 <= 1e-3
    for p in ((nan, 0.0, 2.0), (0.0, inf, 2.0), (3e38, 3e38, 3e38), (1e30, 0.0, 1.0)):
        assert _one(p, [[[2.0]]], [[[9]]]) == (0, 0, 0), p
    # a 2 x 2 image: each pixel is its own
    d22, w22 = [[[2.0, 3.0], [1.25, inf]]], [[[10, 20], [30, 40]]]
    assert _one((0.0, 0.0, 2.0), d22, w22) == (0, 10, 1)
    assert _one((1.0, 0.0, 2.0), d22, w22) == (20 * 65536, 20, 1)
    assert _one((0.0, 1.0, 2.0), d22, w22) == (0, 0, 0)                               # hidden
    assert _one((1.0, 1.0, 2.0), d22, w22) == (0, 0, 0)                               # no depth
    assert _one((1.49, 1.49, 2.0), d22, w22) == (0, 0, 0) and _one((1.51, 0.0, 2.0), d22, w22) == (0, 0, 0)
    # a depth map with no finite or positive value leaves a state untouched, bit for bit; so do F = 0 and n = 0
    start = (torch.tensor([-(2 ** 45) + 3], device=DEV), torch.tensor([77], dtype=torch.int32, device=DEV),
             torch.tensor([5], dtype=torch.int32, device=DEV))
    for bad in (inf, -inf, nan, 0.0, -2.0, 1e-3):
        assert _one((0.0, 0.0, 2.0), [[[bad]]] * 3, [[[255]]] * 3, trunc=4.0, state=start) == (-(2 ** 45) + 3, 77, 5), bad
    fx, r, t = _case()
    num, den, obs = (s.expand(4).contiguous() for s in start)
    before = [s.clone() for s in (num, den, obs)]
    integrate(t["pts"][:4].contiguous(), t["depth"][:0], t["weight"][:0], t["R"][:0], t["T"][:0], t["K"], 0.05, num, den, obs)     # F = 0
    integrate(t["pts"][:0], t["depth"], t["weight"], t["R"], t["T"], t["K"], 0.05, num[:0], den[:0], obs[:0])                      # n = 0
    assert all(torch.equal(a, b) for a, b in zip(before, (num, den, obs)))
    with pytest.raises(ValueError, match="contiguous"):
        wide = torch.zeros(4, 2, dtype=torch.int64, device=DEV)
        integrate(t["pts"][:4].contiguous(), t["depth"], t["weight"], t["R"], t["T"], t["K"], 0.05, wide[:, 0], den, obs)
    with pytest.raises(ValueError, match="trunc"):
        integrate(t["pts"][:4].contiguous(), t["depth"], t["weight"], t["R"], t["T"], t["K"], 0.0, num, den, obs)
    with pytest.raises(ValueError, match="weight"):
        integrate(t["pts"][:4].contiguous(), t["depth"], t["weight"][:, :-1].contiguous(), t["R"], t["T"], t["K"], 0.05, num, den, obs)


def test_fuse_field_chunks_and_bricks():
    from dynhor_amd.depth_fuse import fuse_field, integrate
    from dynhor_amd.visual_hull import grid_points
    fx, r, t = _case()
    ds = SimpleNamespace(R=t["R"], T=t["T"], K=t["K"], n_images=6, H=fx["H"], W=fx["W"])
    lo, hi, N = [-0.62, -0.6, -0.58], [0.6, 0.62, 0.64], 10                          # N is no multiple of the brick
    base = fuse_field(ds, t["depth"], t["weight"], lo, hi, N, trunc=0.05)
    assert all(x.shape == (N ** 3,) for x in base) and int((base[1] > 0).sum()) > 50
    for kw in ({"frame_chunk": 1}, {"point_chunk": 64}, {"frame_chunk": 4, "point_chunk": 100}):
        got = fuse_field(ds, t["depth"], t["weight"], lo, hi, N, trunc=0.05, **kw)
        assert all(torch.equal(x, y) for x, y in zip(base, got)), kw
    pts, _ = grid_points(lo, hi, N, DEV)
    plain = _zeros(N ** 3)
    integrate(pts, t["depth"], t["weight"], t["R"], t["T"], t["K"], 0.05, *plain)
    assert all(torch.equal(x, y) for x, y in zip(base, plain))
    # step_px 2: the maps of every second pixel under diag(1/2, 1/2, 1) K
    K2 = t["K"].clone()
    K2[:2] *= 0.5
    half = _zeros(N ** 3)
    integrate(pts, t["depth"][:, ::2, ::2].contiguous(), t["weight"][:, ::2, ::2].contiguous(), t["R"], t["T"], K2, 0.05, *half)
    got = fuse_field(ds, t["depth"], t["weight"], lo, hi, N, step_px=2, trunc=0.05)
    assert all(torch.equal(x, y) for x, y in zip(half, got)) and not torch.equal(half[0], plain[0])
    with pytest.raises(ValueError, match="depth and weight"):
        fuse_field(ds, t["depth"][:, :-1], t["weight"][:, :-1], lo, hi, N, trunc=0.05)


# ------------------------------------------------------------------------------------------------------------ the scene, end to end
def _scene_frames(sc):
    F, H, W = sc["depth"].shape
    shade = np.clip(-sc["normal"][..., 2], 0, 1)
    rgb = (np.repeat((40 + 200 * shade)[..., None], 3, axis=-1) * (sc["label"][..., None] != 0)).astype(np.uint8)
    return {"rgb": torch.from_numpy(rgb), "label": torch.from_numpy(sc["label"]), "normal": torch.full((F, H, W, 3), 128, dtype=torch.uint8),
            "R": torch.from_numpy(sc["R"]).float(), "T": torch.from_numpy(sc["T"]).float(), "K": torch.from_numpy(sc["K"]).float()}


@functools.lru_cache(maxsize=None)
def _e2e():
    from dynhor_amd import depth_fuse as df
    from dynhor_amd.dataset import Dataset
    sc = U.scene_inputs()
    ds = Dataset(frames=_scene_frames(sc), device=DEV)
    depth = torch.from_numpy(sc["depth"]).to(DEV)
    normal = torch.from_numpy(sc["normal"]).float().to(DEV)
    weight = df.weights_from_normals(normal, torch.isfinite(depth), ds.Kinv)
    weight = torch.where(torch.isfinite(depth), weight, torch.zeros_like(weight))
    keep = {}
    verts, faces, st = df.fused_mesh(ds, depth, weight, resolution=U.SCENE_N, hull=U.SCENE_HULL, keep=keep)
    return sc, ds, depth, weight, verts, faces, st, keep


def test_fused_mesh_of_the_dented_sphere():
    from dynhor_amd import depth_fuse as df
    from dynhor_amd.mesh import marching_cubes
    from dynhor_amd.visual_hull import grid_points, visual_hull
    sc, ds, depth, weight, verts, faces, st, keep = _e2e()
    N, cell, lo, hi = U.SCENE_N, st["cell"], st["bound_min"], st["bound_max"]
    assert st["resolution"] == N and abs(st["trunc"] - 4 * cell) < 1e-12 and faces.shape[0] == st["faces"] > 1000
    assert abs(st["volume"] - st["inside_cells"] * cell ** 3) < 1e-12 and len(st["pixels"]) == 12 and min(st["pixels"]) > 3000
    assert st["carved_cells"] > 0 and st["observed_cells"] > st["inside_cells"] // 4
    assert U.edges_closed(faces.cpu().numpy())                                       # every edge is shared by two faces
    got = U.dent_stats(verts.cpu().numpy().astype(np.float64))
    # the restatement in fp64 on the same inputs and the same grid, meshed by the same marching cubes
    pts, _ = grid_points(lo, hi, N, DEV)
    p64 = pts.cpu().numpy().astype(np.float64)
    h64 = U.scene_hull_field(sc, p64)
    scw = dict(sc, weight=weight.cpu().numpy())
    v = U.pair_values(p64, scw["depth"], scw["weight"], ds.R.cpu().numpy(), ds.T.cpu().numpy(), ds.K.cpu().numpy(), st["trunc"])
    num, den, obs = U.state(v)
    f64 = U.field(num, den, h64, st["trunc"], 255).reshape(N, N, N)
    rv, rf = marching_cubes(-torch.from_numpy(f64).float().to(DEV), 0.0, lo, hi)
    ref = U.dent_stats(rv.cpu().numpy().astype(np.float64))
    hv, hf, hst = visual_hull(ds, resolution=N, **U.SCENE_HULL)
    assert hst["bound_min"] == lo and hst["bound_max"] == hi                         # the same box: the hull's own coarse pass
    hull = U.dent_stats(hv.cpu().numpy().astype(np.float64))
    dfield = float((keep["field"].cpu().double() - torch.from_numpy(f64)).abs().max())
    print(f"fused mesh at {N}^3, cell {cell:.5f}: dent median {got[0]:.5f}, p95 {got[1]:.5f} over {got[2]} vertices (restatement "
          f"{ref[0]:.5f}, {ref[1]:.5f}; ratios {got[0] / ref[0]:.3f}, {got[1] / ref[1]:.3f}); hull {hull[0]:.5f}, {hull[1]:.5f} "
          f"({hull[0] / got[0]:.1f} x, {hull[1] / got[1]:.1f} x); outside the dent at most {got[3]:.5f} (restatement {ref[3]:.5f}); "
          f"max |field - restatement| {dfield:.3e}; carved {st['carved_cells']}, added {st['added_cells']}, observed {st['observed_cells']}")
    assert got[2] > 100 and ref[2] > 100 and hull[2] > 50
    assert got[0] <= 1.25 * ref[0] and got[1] <= 1.25 * ref[1]
    assert hull[0] >= 5.0 * got[0] and hull[1] >= 5.0 * got[1]
    assert got[3] <= cell                                                            # no vertex further than a cell outside the dent
    # one frame's depth scaled by 1.03: that frame disagrees with the fusion of all
    bad = depth.clone()
    bad[U.BAD_FRAME] *= U.BAD_SCALE
    out = df.fused_field(ds, bad, weight, resolution=N, hull=U.SCENE_HULL)
    names = ["f%02d" % f for f in range(12)]
    rs = df.frame_residuals(out["field"], out["lo"], out["hi"], out["trunc"], bad, weight, ds.R, ds.T, ds.K, names)
    print(f"frame {U.BAD_FRAME} x {U.BAD_SCALE}: residual medians {[round(m, 4) for m in rs['median']]}, worst {rs['worst']}")
    assert rs["worst"][0] == names[U.BAD_FRAME] and len(rs["worst"]) == 5 and min(rs["count"]) > 1000
    assert rs["median"][U.BAD_FRAME] >= 3.0 * sorted(rs["median"])[-2]


def test_fused_mesh_settings():
    from dynhor_amd import depth_fuse as df
    sc, ds, depth, weight, verts, faces, st, keep = _e2e()
    v2, f2, st2 = df.fused_mesh(ds, depth, weight, resolution=U.SCENE_N, hull=U.SCENE_HULL, frame_chunk=5, point_chunk=50000)
    assert torch.equal(verts, v2) and torch.equal(faces, f2) and st2 == st
    with pytest.raises(ValueError, match="unknown"):
        df.fused_mesh(ds, depth, weight, cells=3)
    with pytest.raises(ValueError, match="prior_weight"):
        df.fused_mesh(ds, depth, weight, prior_weight=0)
    # a fixed box, and no depth at all: the prior alone is the hull
    none = torch.full_like(depth, float("inf"))
    v3, f3, st3 = df.fused_mesh(ds, none, torch.zeros_like(weight), resolution=48, hull=dict(U.SCENE_HULL, bound=0.7))
    assert st3["bound_min"] == [-0.7] * 3 and st3["carved_cells"] == st3["added_cells"] == st3["observed_cells"] == 0 and st3["pixels"] == [0] * 12


# ------------------------------------------------------------------------------------------------------------ Runner and CLI
def _tree(d, skip=("fuse", "board")):
    out = {}
    for base, dirs, files in os.walk(d):
        dirs[:] = [x for x in dirs if not (base == d and x in skip)]
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def _conf(root, name):
    return {"seq_name": "fuse", "exp_name": name, "data_info": {"dataroot": root},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100},
            "visual_hull": dict(U.SCENE_HULL), "depth_fuse": {"resolution": 64}}


def _write_maps(d, sc, stems, skip=()):
    """The scene's analytic maps in mvs_depth's layout: depth/<stem>.npy (inf: none), monocular_normal/<stem>.png, mvs.json."""
    from PIL import Image
    from dynhor_amd import mvs
    os.makedirs(os.path.join(d, "depth"))
    os.makedirs(os.path.join(d, "monocular_normal"))
    ok = torch.from_numpy(np.isfinite(sc["depth"]))
    enc = mvs.encode_normals(torch.from_numpy(sc["normal"]).float(), ok).numpy()
    for f, s in enumerate(stems):
        if f in skip:
            continue
        np.save(os.path.join(d, "depth", s + ".npy"), sc["depth"][f])
        Image.fromarray(enc[f]).save(os.path.join(d, "monocular_normal", s + ".png"))
    with open(os.path.join(d, "mvs.json"), "w") as fh:
        json.dump({"settings": {"step_px": 1}}, fh)


def test_runner_fuse_depth_end_to_end_and_cli(tmp_path):
    import yaml
    from dynhor_amd import metrics
    from dynhor_amd.depth_fuse import DEPTH_FUSE_DEFAULTS
    from dynhor_amd.runner import Runner
    from dynhor_amd.scene import write_sequence_to_disk
    from dynhor_amd.tb_events import read_scalars
    sc = U.scene_inputs()
    root = str(tmp_path / "seq")
    write_sequence_to_disk(_scene_frames(sc), root)
    r = Runner(conf=_conf(root, "run"), mode="fuse_depth", device=DEV, exp_root=str(tmp_path))
    stems = r.dataset.stems
    with pytest.raises(ValueError, match="--mode mvs_depth"):                        # no mvs folder yet
        r.fuse_depth()
    with open(os.path.join(r.base_exp_dir, "notes.txt"), "w") as fh:
        fh.write("another mode's output")
    old, new = os.path.join(r.base_exp_dir, "mvs", "00000000"), os.path.join(r.base_exp_dir, "mvs", "00000100")
    _write_maps(old, dict(sc, depth=np.full_like(sc["depth"], np.inf)), stems)       # an older run without a depth: not the one used
    _write_maps(new, sc, stems, skip=(7,))                                           # frame 7 has no file: it contributes nothing
    before = _tree(r.base_exp_dir)
    with pytest.raises(ValueError, match="unknown"):
        r.fuse_depth(nonsense=1)
    assert r.fuse_depth(save=False).get("dir") is None and _tree(r.base_exp_dir, skip=()) == before and r.last_fuse_dir is None
    res = r.fuse_depth()
    d = os.path.join(r.base_exp_dir, "fuse", "00000000")
    assert res["dir"] == d == r.last_fuse_dir and res["mesh"] == os.path.join(d, "fused.ply") and res["mvs_dir"] == new
    assert sorted(os.listdir(d)) == ["fuse.json", "fused.ply"] and _tree(r.base_exp_dir) == before
    js = json.load(open(os.path.join(d, "fuse.json")))
    assert {"settings", "stats", "mvs_dir", "step_px", "silhouette", "residual_median", "residual_worst", "seconds", "iter"} <= set(js)
    assert js["settings"] == dict(DEPTH_FUSE_DEFAULTS, resolution=64) and js["step_px"] == 1 and js["frames_with_depth"] == 11
    assert {"resolution", "bound_min", "bound_max", "cell", "trunc", "verts", "faces", "inside_cells", "volume", "carved_cells", "added_cells",
            "observed_cells", "pixels"} <= set(js["stats"])
    assert js["stats"]["pixels"][7] == 0 and min(p for f, p in enumerate(js["stats"]["pixels"]) if f != 7) > 3000
    assert js["stats"]["carved_cells"] > 0 and js["residual_median"][7] is None and len(js["residual_worst"]) == 5
    assert {"read", "box", "hull", "integrate", "mesh", "residuals", "silhouette"} <= set(js["seconds"])
    assert len(js["silhouette"]["frames"]) == 12 and js["silhouette"]["iou_mean"] > 0.85
    v, f = metrics.load_mesh(res["mesh"])
    assert f.shape[0] == js["stats"]["faces"] and v.shape[0] == js["stats"]["verts"]
    got = U.dent_stats(v.numpy().astype(np.float64))
    print(f"runner: dent median {got[0]:.5f}, outside at most {got[3]:.5f}; IoU mean {js['silhouette']['iou_mean']:.4f}; residual medians "
          f"{[None if m is None else round(m, 4) for m in js['residual_median']]}; seconds {js['seconds']}")
    assert got[0] < 0.02 and got[3] <= js["stats"]["cell"]
    board = os.path.join(r.base_exp_dir, "board")
    tags = {tag for fn in os.listdir(board) for _, tag, _ in read_scalars(os.path.join(board, fn))}
    assert {"fuse/volume", "fuse/carved_cells", "fuse/residual_median"} <= tags, tags
    # a map of another shape than the frames
    np.save(os.path.join(new, "depth", stems[7] + ".npy"), np.zeros((95, 96), dtype=np.float32))
    with pytest.raises(ValueError, match="shape"):
        r.fuse_depth(save=False)
    os.remove(os.path.join(new, "depth", stems[7] + ".npy"))
    # the fused mesh is a mesh for the other modes
    vis = r.visualize_mesh(mesh=res["mesh"], normalize="none", save=False)
    assert vis["iou_mean"] > 0.85
    r.close()
    # the CLI prints one JSON line
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(_conf(root, "cli"), fh)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--exp_root", str(tmp_path), "--mode", "fuse_depth",
                        "--mvs_dir", new, "--fuse_resolution", "48", "--fuse_trunc_cells", "3"],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["settings"]["resolution"] == 48 and out["settings"]["trunc_cells"] == 3.0 and out["mvs_dir"] == new
    assert "frames" not in out["silhouette"] and "residual_median" not in out and len(out["residual_worst"]) == 5
    assert os.path.exists(out["mesh"]) and os.path.exists(os.path.join(out["dir"], "fuse.json"))
