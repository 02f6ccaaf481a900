"""Block-sparse mesh extraction on the GPU (dynhor_amd/mesh_extract.py, csrc/mesh_extract.hip): the same mesh as mesh.marching_cubes bit
for bit on analytic, noise and tabulated network fields, reproducibility, the hole detector, resolutions the dense path cannot reach, the
margin of the default lipschitz on freshly trained networks, and the Runner / CLI surface."""
import itertools
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from dynhor_amd._lib import DynhorHipError
from dynhor_amd.mesh import MAX_DENSE_RESOLUTION, marching_cubes
from dynhor_amd.mesh_extract import DEFAULT_LIPSCHITZ, block_grid, grid_axes, min_safe_lipschitz, sparse_marching_cubes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
INF = float("inf")


# ---- helpers
def _dense_grid(field, N, bmin, bmax, chunk=1 << 22):
    """u [N,N,N] of `field` at the dense path's grid points (renderer.extract_geometry: meshgrid of three linspace axes)."""
    ax = [torch.linspace(float(bmin[i]), float(bmax[i]), N, device=DEV) for i in range(3)]
    u = torch.empty(N * N * N, device=DEV)
    for s in range(0, N * N * N, chunk):
        i = torch.arange(s, min(s + chunk, N * N * N), device=DEV)
        p = torch.stack([ax[0][i // (N * N)], ax[1][(i // N) % N], ax[2][i % N]], dim=-1)
        u[s:s + i.shape[0]] = field(p).reshape(-1)
    return u.view(N, N, N)


def _dense_mesh(field, N, bmin, bmax, threshold=0.0):
    return marching_cubes(_dense_grid(field, N, bmin, bmax), threshold, bmin, bmax)


def _sorted_rows(f):
    """Rows of an int64 [F,3] tensor in lexicographic order (no rotation within a row)."""
    if f.shape[0] == 0:
        return f
    m = int(f.max()) + 1
    return f[torch.argsort((f[:, 0] * m + f[:, 1]) * m + f[:, 2])]


def _assert_same_mesh(sparse, dense, what):
    (sv, sf), (dv, df) = sparse[:2], dense[:2]
    assert sv.dtype == dv.dtype and sf.dtype == df.dtype == torch.int64
    assert sv.shape == dv.shape and sf.shape == df.shape, (what, tuple(sv.shape), tuple(dv.shape), tuple(sf.shape), tuple(df.shape))
    assert torch.equal(sv, dv), (what, "vertices differ", int((sv != dv).any(dim=1).sum()))
    assert torch.equal(_sorted_rows(sf), _sorted_rows(df)), (what, "faces differ")


def _table_field(u, bmin, bmax):
    """A field that looks values up in the grid u [N,N,N]: the stored value at a grid point (exactly), trilinear in between."""
    N = u.shape[0]
    lo = torch.tensor([float(b) for b in bmin], device=DEV, dtype=torch.float64)
    hi = torch.tensor([float(b) for b in bmax], device=DEV, dtype=torch.float64)

    def field(p):
        f = ((p.double() - lo) / (hi - lo) * (N - 1)).clamp(0, N - 1)
        near = f.round()
        f = torch.where((f - near).abs() < 1e-3, near, f)               # a grid point up to the rounding of its fp32 coordinates
        i0 = f.floor().clamp(max=N - 2).long()
        t = (f - i0).float()
        out = torch.zeros(p.shape[0], device=DEV)
        for dx, dy, dz in itertools.product((0, 1), repeat=3):
            w = (t[:, 0] if dx else 1 - t[:, 0]) * (t[:, 1] if dy else 1 - t[:, 1]) * (t[:, 2] if dz else 1 - t[:, 2])
            v = u[i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz]
            out = out + torch.where(w > 0, w * v, torch.zeros_like(v))   # weight 1 x value: the value's own bits
        return out
    return field


def _edges(f, n_verts):
    """(smaller vertex of every undirected edge, the number of faces that hold it); edges as one int64 key each."""
    a = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
    key, cnt = torch.unique(torch.minimum(a, b) * n_verts + torch.maximum(a, b), return_counts=True)
    return key // n_verts, cnt


def _closed_components(v, f):
    """Asserts a closed 2-manifold (every undirected edge in exactly two faces); returns (components, Euler characteristic of each)."""
    from dynhor_amd.mesh_clean import vertex_components
    first, cnt = _edges(f, v.shape[0])
    assert bool((cnt == 2).all()), ("open or non-manifold edges", int((cnt != 2).sum()))
    lab = vertex_components(v.shape[0], f).long()
    roots = torch.unique(lab)
    nv = torch.bincount(lab, minlength=v.shape[0])[roots]
    ne = torch.bincount(lab[first], minlength=v.shape[0])[roots]
    nf = torch.bincount(lab[f[:, 0]], minlength=v.shape[0])[roots]
    return int(roots.shape[0]), (nv - ne + nf).tolist()


def _sphere(p):
    return 0.5 - p.norm(dim=-1)


def _blobs(p):
    a = torch.tensor([0.33, 0.0, 0.0], device=p.device)
    b = torch.tensor([0.33, 0.02, 0.01], device=p.device)
    return torch.maximum(0.36 - (p - a).norm(dim=-1), 0.36 - (p + b).norm(dim=-1))


def _torus(p):
    return 0.07 - ((p[..., :2].norm(dim=-1) - 0.55) ** 2 + p[..., 2] ** 2).sqrt()


def _scene(p):
    from dynhor_amd.scene import scene_sdf
    return -scene_sdf(p)


# ---- 1. the same mesh as dense
ONE, SCENE_BOX = ([-1.0] * 3, [1.0] * 3), ([-0.55] * 3, [0.55] * 3)
ANALYTIC = [  # name, field (1-Lipschitz), N, bounds, threshold, block
    ("sphere", _sphere, 33, ONE, 0.0, 8), ("sphere", _sphere, 97, ONE, 0.0, 4), ("sphere", _sphere, 100, ONE, 0.0, 8),
    ("sphere threshold", _sphere, 100, ONE, 0.13, 8), ("sphere threshold", _sphere, 97, ONE, -0.2, 4),
    ("sphere anisotropic", _sphere, 100, ([-1.0, -0.75, -0.6], [1.0, 1.25, 0.9]), 0.0, 8),
    ("sphere anisotropic", _sphere, 128, ([-0.7, -2.0, -0.9], [0.6, 1.0, 0.8]), 0.05, 4),
    ("scene", _scene, 97, SCENE_BOX, 0.0, 8), ("scene", _scene, 100, SCENE_BOX, 0.0, 4), ("scene", _scene, 128, SCENE_BOX, 0.0, 8),
    ("scene threshold", _scene, 128, SCENE_BOX, -0.03, 4),
    ("touching blobs", _blobs, 33, ONE, 0.0, 8), ("touching blobs", _blobs, 100, ONE, 0.0, 4), ("touching blobs", _blobs, 128, ONE, 0.0, 8),
    ("thin torus", _torus, 33, ONE, 0.0, 4), ("thin torus", _torus, 97, ONE, 0.0, 8), ("thin torus", _torus, 128, ONE, 0.0, 8),
]


@pytest.mark.parametrize("name,field,N,bounds,threshold,block", ANALYTIC, ids=[f"{c[0]}-{c[2]}-B{c[5]}".replace(" ", "_") for c in ANALYTIC])
def test_analytic_fields_give_the_dense_mesh_bit_for_bit(name, field, N, bounds, threshold, block):
    bmin, bmax = bounds
    dense = _dense_mesh(field, N, bmin, bmax, threshold)
    v, f, st = sparse_marching_cubes(field, N, bmin, bmax, threshold=threshold, block=block, lipschitz=1.0)
    assert dense[0].shape[0] > 100
    _assert_same_mesh((v, f), dense, name)
    nbk = math.ceil((N - 1) / block)
    assert st["blocks"] == nbk ** 3 and 0 < st["active_blocks"] < st["blocks"] and st["cut_block_faces"] == 0
    assert st["samples"] == st["blocks"] + st["active_blocks"] * (block + 1) ** 3 and st["dense_samples"] == N ** 3
    assert st["verts"] == v.shape[0] and st["faces"] == f.shape[0]


@pytest.mark.parametrize("N,block", [(33, 8), (33, 4), (97, 8), (100, 4), (100, 8), (128, 8)])
@pytest.mark.parametrize("kind", ["smooth", "white"])
def test_noise_fields_give_the_dense_mesh_with_every_block_kept(kind, N, block):
    """Ambiguous faces and every case of the table; lipschitz = inf keeps every block.  Also through small chunks."""
    g = torch.Generator().manual_seed(N * 10 + block)
    if kind == "smooth":
        u = torch.nn.functional.interpolate(torch.randn(1, 1, 9, 9, 9, generator=g), size=(N, N, N), mode="trilinear",
                                            align_corners=True)[0, 0]
    else:
        u = torch.randn(N, N, N, generator=g)
    u = u.to(DEV).contiguous()
    bmin, bmax = [-1.0, -1.0, -0.5], [1.0, 1.0, 1.5]
    for threshold in (0.0, 0.25):
        dense = marching_cubes(u, threshold, bmin, bmax)
        v, f, st = sparse_marching_cubes(_table_field(u, bmin, bmax), N, bmin, bmax, threshold=threshold, block=block, lipschitz=INF)
        _assert_same_mesh((v, f), dense, (kind, N, block, threshold))
        assert st["active_blocks"] == st["blocks"] and st["cut_block_faces"] == 0
    small = sparse_marching_cubes(_table_field(u, bmin, bmax), N, bmin, bmax, threshold=0.25, block=block, lipschitz=INF,
                                  chunk_points=5 * (block + 1) ** 3 + 7)
    assert torch.equal(small[0], v) and torch.equal(small[1], f)       # chunking changes nothing, the face order included


# ---- 2. reproducible
def test_two_runs_are_identical():
    a = sparse_marching_cubes(_scene, 128, *SCENE_BOX, lipschitz=1.0)
    b = sparse_marching_cubes(_scene, 128, *SCENE_BOX, lipschitz=1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert a[1].shape[0] > 10000


# ---- networks
def _conf(name, family):
    return {"seq_name": "mextract", "exp_name": name,
            "data_info": {"synthetic": {"n_frames": 8, "H": 128, "W": 128, "seed": 5}},
            "train": {"batch_size": 512, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100000},
            "model": {"family": family},
            "eval": {"n_samples": 50_000, "gt_resolution": 128}}


@pytest.fixture(scope="module", params=["neus", "hash"])
def trained(request, tmp_path_factory):
    """A synthetic Runner of each family after 300 iterations."""
    from dynhor_amd.runner import Runner
    r = Runner(conf=_conf("net_" + request.param, request.param), device="cuda:0", exp_root=str(tmp_path_factory.mktemp("mx")))
    r.train(300)
    yield r
    r.close()


def _bbox(r):
    return [float(x) for x in r.dataset.object_bbox_min], [float(x) for x in r.dataset.object_bbox_max]


# ---- 3. a real network field, tabulated
def test_tabulated_network_field_gives_the_dense_mesh_at_the_default_lipschitz(trained):
    """The cull on a learned field, independent of how the SDF kernel batches its points: the field is the dense grid itself."""
    bmin, bmax = _bbox(trained)
    u = _dense_grid(lambda p: -trained.renderer.sdf(p), 128, bmin, bmax)
    dense = marching_cubes(u, 0.0, bmin, bmax)
    assert dense[1].shape[0] > 100
    v, f, st = sparse_marching_cubes(_table_field(u, bmin, bmax), 128, bmin, bmax, lipschitz=DEFAULT_LIPSCHITZ)
    _assert_same_mesh((v, f), dense, "tabulated network")
    assert st["active_blocks"] < st["blocks"]


# ---- 4. end to end through renderer.sdf
def _batch_independent(renderer, n=40000):
    """Do the no-grad SDF values of points keep their bits in other batches (other sizes, neighbours, positions in the launch)?"""
    g = torch.Generator().manual_seed(11)
    a = ((torch.rand(n, 3, generator=g) * 2 - 1) * 0.9).to(DEV)
    far = ((torch.rand(3 * n + 17, 3, generator=g) * 2 - 1) * 1.01).to(DEV)          # batch mates with other magnitudes
    ref = renderer.sdf(a).reshape(-1)
    perm = torch.randperm(n, generator=g).to(DEV)
    same = torch.equal(renderer.sdf(a[perm]).reshape(-1), ref[perm])
    same &= torch.equal(renderer.sdf(torch.cat([far, a]))[far.shape[0]:].reshape(-1), ref)
    same &= torch.equal(renderer.sdf(a[:777]).reshape(-1), ref[:777])
    same &= torch.equal(torch.cat([renderer.sdf(a[i:i + 4999]).reshape(-1) for i in range(0, n, 4999)]), ref)
    return bool(same)


def test_nograd_sdf_of_a_point_does_not_depend_on_its_batch(trained):
    """Sparse and dense evaluate a grid point in different launches (and a shared block face twice): equal bits end to end need an SDF
    kernel whose per-point arithmetic ignores the rest of the launch.  Checked, not assumed, for the default arithmetic."""
    assert _batch_independent(trained.renderer)


def test_extract_geometry_sparse_equals_dense(trained):
    bmin, bmax = _bbox(trained)
    for N, block in ((128, 8), (100, 4)):
        dense = trained.renderer.extract_geometry(bmin, bmax, N)
        sparse = trained.renderer.extract_geometry(bmin, bmax, N, mode="sparse", block=block)
        _assert_same_mesh(sparse, dense, ("extract_geometry", N, block))
        st = trained.renderer.last_extract_stats
        assert st["verts"] == dense[0].shape[0] and 0 < st["active_blocks"] < st["blocks"]
    for bad in (dict(method="tetrahedra", mode="sparse"), dict(mode="octree")):
        with pytest.raises(ValueError):
            trained.renderer.extract_geometry(bmin, bmax, 64, **bad)


# ---- 5. the hole detector
def test_too_small_a_lipschitz_raises_and_names_it():
    steep = lambda p: 3.0 * (0.4 - p.norm(dim=-1))                    # Lipschitz constant 3
    with pytest.raises(DynhorHipError, match="lipschitz"):
        sparse_marching_cubes(steep, 100, *ONE, lipschitz=1.0)
    got = sparse_marching_cubes(steep, 100, *ONE, lipschitz=3.0)
    _assert_same_mesh(got, _dense_mesh(steep, 100, *ONE), "steep sphere")
    assert got[2]["cut_block_faces"] == 0


def test_non_finite_values_raise():

    def nan_at_one_sample(p):
        # grid point (72, 48, 48) of the 97^3 grid over [-1, 1]^3 lies on the sphere and is a block corner, never a block centre
        u = _sphere(p)
        hit = (p - torch.tensor([0.5, 0.0, 0.0], device=p.device)).abs().amax(dim=-1) < 1e-4
        return torch.where(hit, torch.full_like(u, float("nan")), u)

    with pytest.raises(DynhorHipError, match="non-finite field values in the block samples"):
        sparse_marching_cubes(nan_at_one_sample, 97, *ONE, lipschitz=1.0)
    with pytest.raises(DynhorHipError, match="non-finite field values at the block centres"):
        sparse_marching_cubes(lambda p: torch.full((p.shape[0],), float("inf"), device=p.device), 33, *ONE, lipschitz=1.0)


# ---- 6. high resolution
@pytest.fixture(scope="module")
def scene_components_at_256():
    from dynhor_amd.mesh_clean import vertex_components
    v, f = _dense_mesh(_scene, 256, *SCENE_BOX)
    lab = vertex_components(v.shape[0], f)
    return int(torch.unique(lab).shape[0])


@pytest.mark.parametrize("N", [1024, 2048])
def test_analytic_scene_at_high_resolution(scene_components_at_256, N):
    """2048 is beyond the dense weld key's range (MAX_DENSE_RESOLUTION)."""
    from dynhor_amd.scene import scene_sdf
    assert MAX_DENSE_RESOLUTION < 2048
    v, f, st = sparse_marching_cubes(_scene, N, *SCENE_BOX, lipschitz=1.0)
    comps, euler = _closed_components(v, f)
    print(f"scene at {N}: {st}, {comps} components, Euler {euler}")
    assert comps == scene_components_at_256 and all(x == 2 for x in euler)
    d = max(float(scene_sdf(v[i:i + (1 << 22)]).abs().max()) for i in range(0, v.shape[0], 1 << 22))
    assert d < 0.25 * 1.1 / (N - 1), d                                 # a quarter of a cell
    assert st["samples"] < N ** 3 / 30 and st["cut_block_faces"] == 0, st


# ---- 7. the default lipschitz
def test_default_lipschitz_keeps_a_margin_on_a_fresh_training(trained):
    """L_min of a network trained here for 300 iterations, and of the same family at initialisation, stays below the default
    (DESIGN_NEXT_ROWS.md section 11: twice the largest L_min of four recorded checkpoints)."""
    from dynhor_amd.runner import MESH_EXTRACT_DEFAULTS, Runner
    assert MESH_EXTRACT_DEFAULTS["lipschitz"] == DEFAULT_LIPSCHITZ
    family = trained.conf["model"]["family"]
    fresh = Runner(conf=_conf("init_" + family, family), device="cuda:0", exp_root=os.path.dirname(os.path.dirname(trained.base_exp_dir)))
    bmin, bmax = _bbox(trained)
    for what, r in (("trained", trained), ("initialisation", fresh)):
        for N, B in ((256, 8), (128, 4)):
            u = _dense_grid(lambda p: -r.renderer.sdf(p), N, bmin, bmax)
            _, c, rad = block_grid(grid_axes(N, bmin, bmax, DEV), B)
            l_min = min_safe_lipschitz(u, -r.renderer.sdf(c).reshape(-1), rad, 0.0, B)
            print(f"{family} {what} N {N} B {B}: L_min {l_min:.4f} (default {DEFAULT_LIPSCHITZ})")
            assert 0.0 < l_min < DEFAULT_LIPSCHITZ, (family, what, N, B, l_min)
    fresh.close()


# ---- 8. Runner and CLI
def _ply_counts(path):
    head = open(path, "rb").read(400).decode("latin1")
    return int(head.split("element vertex ")[1].split()[0]), int(head.split("element face ")[1].split()[0])


def test_runner_validate_and_evaluate_with_sparse_extraction(trained):
    r = trained
    d = os.path.join(r.base_exp_dir, "meshes")
    dv, df = r.validate_mesh(resolution=128)
    assert r.last_extract_stats is None
    dense_counts = _ply_counts(os.path.join(d, "{:0>8d}.ply".format(r.iter_step)))
    sv, sf = r.validate_mesh(resolution=128, extract="sparse")
    assert _ply_counts(os.path.join(d, "{:0>8d}.ply".format(r.iter_step))) == dense_counts == (dv.shape[0], df.shape[0])
    assert (sv.shape[0], sf.shape[0]) == dense_counts
    xs = r.last_extract_stats
    assert xs["mode"] == "sparse" and xs["verts"] == dv.shape[0] and xs["active_blocks"] < xs["blocks"]

    # The same faces in another order make the area-weighted sampler draw other points: the metrics differ like those of two seeds.
    # Spread = max - min over six dense seeds (~2.5 sigma); sparse at seed 0 must lie within three spreads of dense at seed 0 (the
    # difference of two draws has 1.41 sigma: ~5 of those); the counts must agree exactly.
    dense = [r.evaluate_mesh(resolution=64, seed=s, save=False) for s in range(6)]
    assert not any(k.startswith("extract") for k in dense[0])
    sparse = r.evaluate_mesh(resolution=64, seed=0, save=True, extract="sparse")
    assert sparse["extract"] == "sparse" and sparse["extract_block"] == 8
    assert 0 < sparse["extract_active_blocks"] <= sparse["extract_blocks"]      # (at 64 the default lipschitz culls little)
    assert sparse["extract_samples"] == sparse["extract_blocks"] + sparse["extract_active_blocks"] * 9 ** 3
    assert sparse["extract_dense_samples"] == 64 ** 3 and sparse["extract_lipschitz"] == r._extract_conf()["lipschitz"]
    assert sparse["n_pred_faces"] == dense[0]["n_pred_faces"] and sparse["n_gt_faces"] == dense[0]["n_gt_faces"]
    checked = 0
    for k, v0 in dense[0].items():
        if not isinstance(v0, float) or k.startswith("extract"):
            continue
        vals = [e[k] for e in dense]
        spread = max(vals) - min(vals)
        print(f"{k}: dense {v0:.6g} (spread {spread:.3g} over six seeds), sparse {sparse[k]:.6g}")
        assert abs(sparse[k] - v0) <= 3.0 * spread + 1e-12, (k, sparse[k], vals)
        checked += 1
    assert checked >= 6
    saved = json.load(open(os.path.join(d, "{:0>8d}_eval.json".format(r.iter_step))))
    assert saved["extract_active_blocks"] == sparse["extract_active_blocks"]
    assert set(r._gt_meshes) == {128, (128, "sparse")}                 # the ground truth is cached per mode
    assert torch.equal(r._gt_meshes[128][0], r._gt_meshes[(128, "sparse")][0])


def test_clean_color_and_overlay_work_on_the_sparse_mesh(trained):
    r = trained
    dv, df = r.validate_mesh(resolution=96, save=False, clean="largest", color="views")
    dense_colors = r.last_mesh_colors.clone()
    sv, sf = r.validate_mesh(resolution=96, save=False, clean="largest", color="views", extract="sparse")
    assert torch.equal(sv, dv) and torch.equal(_sorted_rows(sf), _sorted_rows(df))
    assert r.last_mesh_colors.shape == dense_colors.shape and r.last_clean_stats["verts_in"] >= sv.shape[0]
    a = r.visualize_mesh(resolution=96, save=False)
    b = r.visualize_mesh(resolution=96, save=False, extract="sparse")
    assert b["iou_mean"] == a["iou_mean"] and b["iou_min"] == a["iou_min"]          # the same surface covers the same pixels


def test_cli_validate_mesh_sparse(trained, tmp_path):
    import yaml
    r = trained
    r.save_checkpoint()
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(_conf(r.conf["exp_name"], r.conf["model"]["family"]), fh)
    env = dict(os.environ, PYTHONPATH=ROOT)
    exp_root = os.path.dirname(os.path.dirname(r.base_exp_dir))
    outs = {}
    for mode in ("sparse", "dense"):
        p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--mode", "validate_mesh", "--is_continue",
                            "--exp_root", exp_root, "--mesh_extract", mode, "--mesh_resolution", "256"], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        outs[mode] = p.stdout
        outs[mode + "_counts"] = _ply_counts(os.path.join(r.base_exp_dir, "meshes", "{:0>8d}.ply".format(r.iter_step)))
    line = [ln for ln in outs["sparse"].splitlines() if ln.startswith("mesh_extract sparse:")]
    assert len(line) == 1 and "SDF queries" in line[0] and f"{256 ** 3} dense" in line[0], outs["sparse"]
    assert "mesh_extract" not in outs["dense"]
    assert outs["sparse_counts"] == outs["dense_counts"] and outs["dense_counts"][0] > 1000      # --mesh_resolution reaches validate_mesh
