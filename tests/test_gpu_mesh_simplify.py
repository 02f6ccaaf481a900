"""Mesh simplification on the GPU against the fp64 restatement (tests/mesh_simplify_util.py): cell keys bit for bit (beyond 2^31 too),
the per-cell sums within the bound of two summation orders, whole results (faces equal, vertices within one fp32 ulp), edge inputs,
bitwise reproducibility, the provable sqrt(3) h distance bound on the device result, and Runner / CLI wiring."""
import functools
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import mesh_simplify_util as U
from tests.mesh_align_util import three_box_mesh
from tests.pose_sil_util import bent_ellipsoid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "three_box":
        v, f = three_box_mesh(96)
    else:
        v, f = bent_ellipsoid(n_lat=40, n_lon=72)
        assert f.shape[0] == 5616
    return v.float().contiguous(), f.contiguous()


@functools.lru_cache(maxsize=None)
def _ref(name, cells, placement="quadric"):
    return U.simplify_ref(*_mesh(name), cells, placement=placement)


def _gpu(v, f, **kw):
    from dynhor_amd.mesh_simplify import simplify_mesh
    return simplify_mesh(v.to(DEV), f.to(DEV), **kw)


def _ulp(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 2.0 ** -149


COUNT_KEYS = ("cells", "cell_size", "dims", "n_cells_occupied", "n_verts_in", "n_verts_out", "n_faces_in", "n_faces_out", "n_collapsed",
              "n_duplicate", "n_clamped", "n_boundary_edges", "n_nonmanifold_edges", "longest_run")


def _assert_same_result(got, ref, what):
    """faces torch.equal, vertices within one fp32 ulp of the largest |coordinate|, the counts equal.  n_clamped may differ by the
    cells whose unclamped solution lies within 1e-9 h of a face of its box (a flat cell whose plane IS a cell boundary: whether
    rounding puts it outside is not determined; the clamped position is the same either way)."""
    gv, gf, gs = got[:3]
    rv, rf, rs, extra = ref
    assert gv.dtype == torch.float32 and gf.dtype == torch.int64 and gv.is_cuda and gf.is_cuda
    assert torch.equal(gf.cpu(), rf), what
    assert gv.shape == rv.shape, what
    if rv.shape[0]:
        tol = _ulp(float(rv.abs().max()))
        err = (gv.cpu().double() - rv.double()).abs().max(dim=1).values
        worst = int(err.argmax())
        if float(err[worst]) > tol:
            r = int(extra["used"].nonzero().reshape(-1)[worst])
            s = extra["sums"][r]
            A = torch.tensor([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
            M = A + 1e-3 * (A.trace() / 3) * torch.eye(3, dtype=torch.float64)
            print(f"{what}: cell {int(extra['keys'][r])} ({int(extra['counts'][r])} records): error {float(err[worst]):.3e} > {tol:.3e}; "
                  f"sums {s.tolist()}; condition {float(torch.linalg.cond(M)):.3e}; got {gv[worst].tolist()}, "
                  f"restatement {extra['rep64'][r].tolist()}")
        assert float(err[worst]) <= tol, what
    for k in COUNT_KEYS:
        if k == "n_clamped":
            assert abs(gs[k] - rs[k]) <= extra["n_borderline"], (what, k, gs[k], rs[k], extra["n_borderline"])
        else:
            assert gs[k] == rs[k], (what, k, gs[k], rs[k])


# ------------------------------------------------------------------------------------------------ 1. cell keys
def _boundary_cloud(cells, zero_axis=None):
    g = torch.Generator().manual_seed(11)
    lo, ext = torch.tensor([-0.3, 0.1, 0.02]), torch.tensor([1.0, 0.61, 0.27])
    v = [lo[None], (lo + ext)[None], lo + ext * torch.rand(300, 3, generator=g)]
    h = float(ext.max()) / cells
    k = torch.arange(0, min(cells, 64) + 1, dtype=torch.float32)
    for a in range(3):                                     # points on (the fp32 rounding of) cell boundaries, and on hi of every axis
        p = lo + ext * torch.rand(k.shape[0], 3, generator=g)
        p[:, a] = torch.minimum(lo[a] + k * h, lo[a] + ext[a])
        v.append(p)
        q = lo + ext * torch.rand(8, 3, generator=g)
        q[:, a] = lo[a] + ext[a]
        v.append(q)
    v = torch.cat(v).float()
    if zero_axis is not None:
        v[:, zero_axis] = 0.125
    return v.contiguous()


@pytest.mark.parametrize("cells", [1, 2, 7])
def test_cell_keys_match_the_restatement(cells):
    from dynhor_amd.mesh_simplify import cell_keys
    for zero_axis in (None, 1, 0):
        v = _boundary_cloud(cells, zero_axis)
        keys, h, dims = cell_keys(v.to(DEV), cells)
        idx, rkeys, lo, rh, rdims = U.cell_index(v, cells)
        assert h == float(rh) and list(dims) == rdims
        assert keys.dtype == torch.int64 and torch.equal(keys.cpu(), rkeys)
        assert int(idx.max()) == max(rdims) - 1                            # the points on hi sit in the last cell
    one = torch.full((5, 3), 0.75)                                         # extent 0 on every axis: one cell
    keys, h, dims = cell_keys(one.to(DEV), cells)
    assert h == 0.0 and tuple(dims) == (1, 1, 1) and int(keys.abs().max()) == 0


def test_cell_keys_beyond_2_to_31():
    from dynhor_amd.mesh_simplify import cell_keys
    cells = 1 << 20
    v = _boundary_cloud(cells)
    keys, h, dims = cell_keys(v.to(DEV), cells)
    _, rkeys, _, rh, rdims = U.cell_index(v, cells)
    assert len(set(rdims)) == 3 and min(rdims) > 1 << 17
    assert int(rkeys.max()) > 1 << 40
    assert h == float(rh) and list(dims) == rdims and torch.equal(keys.cpu(), rkeys)


# ------------------------------------------------------------------------------------------------ 2. the per-cell sums
def _check_sums(v, f, cells, want_runs=()):
    got = _gpu(v, f, cells=cells, return_sums=True)
    ref = U.simplify_ref(v, f, cells)
    g, e = got[3], ref[3]
    assert torch.equal(g["keys"].cpu(), e["keys"]) and torch.equal(g["counts"].cpu(), e["counts"])
    assert torch.equal(g["used"].cpu(), e["used"])
    n = e["counts"].double()[:, None]
    tol = n * 2.0 ** -53 * e["abs_sums"]                                   # two orderings of an fp64 sum of n terms
    err = (g["sums"].cpu() - e["sums"]).abs()
    worst = float((err / tol.clamp(min=1e-300)).max())
    print(f"cells {cells}: {e['keys'].shape[0]} runs, lengths {sorted(set(e['counts'].tolist()))[-8:]}; "
          f"largest error / tolerance {worst:.3f}")
    assert bool((err <= tol).all())
    for r in want_runs:
        assert r in e["counts"].tolist(), f"no run of {r} records"
    _assert_same_result(got, ref, f"sums fixture at {cells} cells")
    return e["counts"]


def test_sums_of_runs_around_the_wave_size():
    lengths = [1, 63, 64, 65, 129, 1000]
    v, f, cells, centres = U.fans_in_cells(lengths)
    counts = _check_sums(v, f, cells, want_runs=lengths)
    _, keys, _, _, _ = U.cell_index(v, cells)
    ref_keys = U.simplify_ref(v, f, cells)[3]["keys"]
    for n, c in zip(lengths, centres):                                     # the cell of every fan's centre holds exactly its records
        assert int(counts[int((ref_keys == keys[c]).nonzero()[0])]) == n


def test_sums_of_long_runs_on_the_fine_ellipsoid():
    counts = _check_sums(*_mesh("ellipsoid"), 2)
    assert int(counts.max()) > 1000


# ------------------------------------------------------------------------------------------------ 3. whole results
@pytest.mark.parametrize("name,cells", [("three_box", 24), ("ellipsoid", 6), ("ellipsoid", 40)])
def test_whole_result_matches_the_restatement(name, cells):
    v, f = _mesh(name)
    _assert_same_result(_gpu(v, f, cells=cells), _ref(name, cells), f"{name} -> {cells}")


# ------------------------------------------------------------------------------------------------ 4. edge inputs
def test_no_faces_and_one_cell():
    v, f = _mesh("three_box")
    gv, gf, st = _gpu(v, torch.zeros(0, 3, dtype=torch.int64), cells=8)
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and st["n_faces_out"] == 0 and st["n_cells_occupied"] == 0
    gv, gf, st = _gpu(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64), cells=8)
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and st["n_verts_in"] == 0
    gv, gf, st = _gpu(v, f, cells=1)                                       # every vertex in one cell
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and gf.dtype == torch.int64
    assert st["n_collapsed"] == f.shape[0] and st["n_cells_occupied"] == 1 and st["longest_run"] == 3 * f.shape[0]
    _assert_same_result((gv, gf, st), U.simplify_ref(v, f, 1), "one cell")


def test_one_triangle_in_three_cells_is_unchanged_up_to_rotation():
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    f = torch.tensor([[1, 2, 0]])
    got = _gpu(v, f, cells=2)
    assert got[1].tolist() == [[0, 1, 2]]                                  # the smallest cell first, orientation kept
    assert float((got[0].cpu() - v).abs().max()) <= 1e-6                   # one plane per cell: each corner stays where it is
    _assert_same_result(got, U.simplify_ref(v, f, 2), "one triangle")


def _coarse_ellipsoid():
    v, f = bent_ellipsoid(n_lat=12, n_lon=20)
    return v.float().contiguous(), f.contiguous()


def test_zero_area_and_duplicate_faces():
    v, f = _coarse_ellipsoid()
    extra = torch.tensor([[5, 5, 9], [7, 30, 7], [3, 3, 3]])               # zero-area faces: they still count as corners
    mid = 0.5 * (v[10] + v[50])
    v2 = torch.cat([v, mid[None]])
    collinear = torch.tensor([[10, v.shape[0], 50]])                        # zero area (up to rounding) across several cells
    f2 = torch.cat([f[:100], extra, f[40:60], collinear, f[100:], f[:30].roll(1, dims=1)])
    for cells in (3, 9):
        ref = U.simplify_ref(v2, f2, cells)
        assert ref[2]["n_duplicate"] > 0 and ref[2]["n_collapsed"] > 0
        _assert_same_result(_gpu(v2, f2, cells=cells), ref, f"degenerate mesh -> {cells}")


def test_duplicate_triples_keep_the_lower_index_and_opposite_orientations_both_stay():
    # two cells per axis over [0,1]^3; vertices 0..2 and 3..5 lie pairwise in the same three cells, 6 in a fourth
    v = torch.tensor([[0.1, 0.1, 0.0], [0.9, 0.1, 0.0], [0.1, 0.9, 0.0], [0.2, 0.2, 0.0], [0.8, 0.2, 0.0], [0.2, 0.8, 0.0],
                      [0.9, 0.9, 1.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    f = torch.tensor([[0, 1, 2],        # triple X
                      [1, 6, 2],        # triple Y
                      [4, 5, 3],        # X again, rotated, other vertices: dropped for face 0
                      [0, 2, 1],        # X with the opposite orientation: another triple, stays
                      [5, 4, 3]])       # ... and its duplicate: dropped
    got = _gpu(v, f, cells=2)
    ref = U.simplify_ref(v, f, 2)
    _assert_same_result(got, ref, "duplicates")
    gf = got[1].tolist()
    assert len(gf) == 3 and got[2]["n_duplicate"] == 2 and got[2]["n_collapsed"] == 0
    # output order = input order of the survivors: X (face 0) BEFORE Y (face 1); had face 2 survived instead, Y would come first
    assert gf[0] == [0, 1, 2] and gf[2] == [0, 2, 1] and 3 in gf[1]
    assert got[2]["n_boundary_edges"] == 2 and got[2]["n_nonmanifold_edges"] == 1


def test_placement_mean_and_the_errors():
    from dynhor_amd.mesh_simplify import simplify_mesh
    v, f = _mesh("three_box")
    got = _gpu(v, f, cells=24, placement="mean")
    _assert_same_result(got, _ref("three_box", 24, "mean"), "placement mean")
    assert got[2]["n_clamped"] == 0 and torch.equal(got[1].cpu(), _ref("three_box", 24)[1])
    bad = v.clone()
    for val in (float("nan"), float("inf"), -float("inf")):
        bad[17, 1] = val
        with pytest.raises(ValueError, match="finite"):
            _gpu(bad, f, cells=8)
    for idx in (-1, v.shape[0]):
        g = f.clone()
        g[5, 2] = idx
        with pytest.raises(ValueError, match="face indices"):
            _gpu(v, g, cells=8)
    with pytest.raises(ValueError):
        simplify_mesh(v.to(DEV).double(), f.to(DEV), cells=8)
    with pytest.raises(ValueError):
        simplify_mesh(v.to(DEV), f.to(DEV).int(), cells=8)


def test_target_faces_matches_the_restatement_bisection():
    v, f = three_box_mesh(48)
    v = v.float()
    for target, cells_max in ((300, 64), (0, 16)):
        (rv, rf, rs, extra), cells, passes = U.simplify_to_target_ref(v, f, target, cells_max=cells_max)
        got = _gpu(v, f, target_faces=target, cells_max=cells_max)
        st = got[2]
        assert st["cells"] == cells and st["passes"] == passes <= math.ceil(math.log2(cells_max)) + 1
        assert st["n_faces_out"] <= target and st["target_faces"] == target
        _assert_same_result(got, (rv, rf, rs, extra), f"faces:{target}")


# ------------------------------------------------------------------------------------------------ 5. reproducibility
def test_bitwise_reproducible_on_any_stream():
    from dynhor_amd.mesh_simplify import simplify_mesh
    v, f = (t.to(DEV) for t in _mesh("ellipsoid"))
    a = simplify_mesh(v, f, cells=40, return_sums=True)
    b = simplify_mesh(v, f, cells=40, return_sums=True)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = simplify_mesh(v, f, cells=40, return_sums=True)
    side.synchronize()
    for o in (b, c):
        assert torch.equal(a[0].view(torch.int32), o[0].view(torch.int32)) and torch.equal(a[1], o[1]) and a[2] == o[2]
        assert torch.equal(a[3]["sums"].view(torch.int64), o[3]["sums"].view(torch.int64))


# ------------------------------------------------------------------------------------------------ 6. the provable bound
@pytest.mark.parametrize("name,cells", [("three_box", 24), ("ellipsoid", 6), ("ellipsoid", 40)])
def test_output_lies_within_sqrt3_h_of_the_input(name, cells):
    """Every input vertex moves to a point of its own cell, so a point of an output face is within the cell diagonal sqrt(3) h of the
    point of the input face with the same barycentric coordinates.  The distance to the nearest of 200,000 input samples and the input
    vertices bounds the distance to the input surface from above: the check is no weaker than the statement."""
    from dynhor_amd.metrics import nearest_sqdist, sample_surface
    v, f = (t.to(DEV) for t in _mesh(name))
    gv, gf, st = _gpu(v, f, cells=cells)
    assert gf.shape[0] > 0
    pts, _ = sample_surface(gv, gf, 20_000, 1)
    cloud = torch.cat([sample_surface(v, f, 200_000, 2)[0], v]).contiguous()
    d = nearest_sqdist(pts.contiguous(), cloud).double().sqrt()
    h = st["cell_size"]
    print(f"{name} -> {cells}: {f.shape[0]} -> {gf.shape[0]} faces, largest sampled distance {float(d.max()) / h:.3f} h "
          f"(bound {math.sqrt(3.0):.3f} h), {st['n_boundary_edges']} boundary / {st['n_nonmanifold_edges']} non-manifold edges")
    assert float(d.max()) <= math.sqrt(3.0) * h
    if name == "three_box":
        assert st["n_boundary_edges"] == 0 and st["n_nonmanifold_edges"] == 0


# ------------------------------------------------------------------------------------------------ 7. Runner and CLI
def _conf(name):
    return {"seq_name": "msimp", "exp_name": name,
            "data_info": {"synthetic": {"n_frames": 3, "H": 64, "W": 64, "seed": 5}},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100}}


def _ply_counts(path):
    head = open(path, "rb").read(400).split(b"end_header")[0].decode()
    n = {ln.split()[1]: int(ln.split()[2]) for ln in head.splitlines() if ln.startswith("element")}
    return n["vertex"], n["face"]


def test_runner_validate_evaluate_visualize(tmp_path):
    from dynhor_amd.metrics import load_mesh
    from dynhor_amd.runner import Runner
    r = Runner(conf=_conf("runner"), device="cuda:0", exp_root=str(tmp_path))
    d = os.path.join(r.base_exp_dir, "meshes")
    v0, f0 = r.validate_mesh(resolution=64)
    raw = open(os.path.join(d, "00000000.ply"), "rb").read()
    assert not os.path.exists(os.path.join(d, "00000000_simple.ply")) and r.last_simplify_stats is None
    sv, sf = r.validate_mesh(resolution=64, simplify="cells:16")
    assert open(os.path.join(d, "00000000.ply"), "rb").read() == raw
    st = r.last_simplify_stats
    assert st["mode"] == "cells:16" and st["n_faces_in"] == f0.shape[0] and st["n_verts_in"] == v0.shape[0]
    assert 0 < sf.shape[0] == st["n_faces_out"] < f0.shape[0] // 4 and sv.shape[0] == st["n_verts_out"]
    assert _ply_counts(os.path.join(d, "00000000_simple.ply")) == (sv.shape[0], sf.shape[0])
    lv, lf = load_mesh(os.path.join(d, "00000000_simple.ply"))
    assert torch.equal(lv, sv.cpu()) and torch.equal(lf, sf.cpu())
    # the YAML block does what the argument does; the argument "none" switches it off again
    r.conf["mesh_simplify"] = {"mode": "cells:16"}
    bv, bf = r.validate_mesh(resolution=64, save=False)
    assert torch.equal(bv, sv) and torch.equal(bf, sf)
    nv, nf = r.validate_mesh(resolution=64, save=False, simplify="none")
    assert torch.equal(nv, v0) and torch.equal(nf, f0)
    del r.conf["mesh_simplify"]
    res = r.evaluate_mesh(resolution=64, gt_resolution=64, n_samples=20_000, simplify="faces:2000")
    assert 0 < res["n_pred_faces"] <= 2000 and res["n_pred_faces"] == res["simplify"]["n_faces_out"]
    assert res["simplify"]["n_faces_out"] <= 2000 and res["simplify"]["mode"] == "faces:2000" and res["simplify"]["passes"] <= 11
    saved = json.load(open(os.path.join(d, "00000000_eval.json")))
    assert saved["simplify"] == res["simplify"]
    plain = r.evaluate_mesh(resolution=64, gt_resolution=64, n_samples=20_000, save=False)
    assert "simplify" not in plain
    vis = r.visualize_mesh(resolution=64, simplify="cells:16", save=False)
    assert vis["simplify"] == "cells:16" and vis["faces"] == sf.shape[0] and 0.0 <= vis["iou_mean"] <= 1.0
    assert "simplify" not in r.visualize_mesh(resolution=64, save=False)
    r.close()


def test_cli_validate_mesh_simplifies_before_colouring(tmp_path):
    import yaml
    from dynhor_amd.runner import Runner
    conf = _conf("cli")
    r = Runner(conf=conf, device="cuda:0", exp_root=str(tmp_path))
    r.save_checkpoint()
    sv, sf = r.validate_mesh(resolution=64, save=False, simplify="cells:16")
    r.close()
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--mode", "validate_mesh", "--is_continue",
                        "--exp_root", str(tmp_path), "--mesh_simplify", "cells:16", "--mesh_color", "views"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("mesh_simplify cells:16:")]
    assert len(lines) == 1, p.stdout
    d = os.path.join(r.base_exp_dir, "meshes")
    assert _ply_counts(os.path.join(d, "00000000_color.ply")) == (sv.shape[0], sf.shape[0])
    assert _ply_counts(os.path.join(d, "00000000_simple.ply")) == (sv.shape[0], sf.shape[0])
    head = open(os.path.join(d, "00000000_color.ply"), "rb").read(400)
    assert b"property uchar red" in head
