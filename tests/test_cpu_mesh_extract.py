"""CPU: the host side of block-sparse mesh extraction (dynhor_amd/mesh_extract.py) -- block enumeration, the cull rule restated in
torch on the analytic scene, the packed case table, the weld key's order, configuration and CLI, the dh_mc_* entry points' argument
checks (no launches: there is no GPU here) and the dense path's resolution limit."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dh_mc_block_points", "dh_mc_count", "dh_mc_emit")


@pytest.mark.parametrize("N,B,bmin,bmax", [(97, 8, [-1.0] * 3, [1.0] * 3),            # N - 1 a multiple of B
                                           (100, 8, [-0.55] * 3, [0.55] * 3),          # clipped end blocks (3 cells)
                                           (100, 4, [-0.55] * 3, [0.55] * 3),
                                           (33, 8, [-1.0, -0.5, 0.0], [1.0, 0.25, 3.0])])   # anisotropic bounds
def test_block_centres_and_radii_match_closed_forms(N, B, bmin, bmax):
    from dynhor_amd.mesh_extract import block_grid, grid_axes
    axes = grid_axes(N, bmin, bmax)
    for a, lo, hi in zip(axes, bmin, bmax):
        assert torch.equal(a, torch.linspace(lo, hi, N))             # exactly the dense path's coordinates
    nbk, c, r = block_grid(axes, B)
    assert nbk == math.ceil((N - 1) / B) and c.shape == (nbk ** 3, 3) and r.shape == (nbk ** 3,)
    assert c.dtype == torch.float32 and r.dtype == torch.float32
    h = [(hi - lo) / (N - 1) for lo, hi in zip(bmin, bmax)]
    c = c.reshape(nbk, nbk, nbk, 3).double()
    r = r.reshape(nbk, nbk, nbk).double()
    for b in [(0, 0, 0), (1, 0, nbk - 1), (nbk - 1, nbk - 1, nbk - 1), (nbk // 2, nbk - 1, 1)]:
        lo_i = [bb * B for bb in b]
        hi_i = [min(bb * B + B, N - 1) for bb in b]
        centre = [bmin[d] + 0.5 * (lo_i[d] + hi_i[d]) * h[d] for d in range(3)]
        radius = 0.5 * math.sqrt(sum(((hi_i[d] - lo_i[d]) * h[d]) ** 2 for d in range(3))) * (1 + 2.0 ** -10)
        scale = max(abs(v) for v in bmin + bmax)
        assert all(abs(c[b][d].item() - centre[d]) < 4e-7 * scale for d in range(3)), b       # fp32 axis coordinates
        assert abs(r[b].item() - radius) < 1e-6 * radius + 4e-7 * scale, b
    if (N - 1) % B:
        assert r[nbk - 1, 0, 0] < r[0, 0, 0]                          # a clipped block is smaller
    else:
        assert torch.allclose(r, r[0, 0, 0].expand_as(r), rtol=1e-5)


def _cull_on_scene(N, B):
    """(cells with a sign change, of those in a culled block, active blocks, blocks) of scene_sdf over [-0.55, 0.55]^3 at lipschitz 1."""
    from dynhor_amd.mesh_extract import active_blocks, block_grid, grid_axes
    from dynhor_amd.scene import scene_sdf
    axes = grid_axes(N, [-0.55] * 3, [0.55] * 3)
    g = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    u = -scene_sdf(g).reshape(N, N, N)
    nbk, c, r = block_grid(axes, B)
    act = active_blocks(-scene_sdf(c), r, 0.0, 1.0).reshape(nbk, nbk, nbk)
    ins = (u > 0)
    sl = (slice(0, N - 1), slice(1, N))
    n_in = sum(ins[sl[dx], sl[dy], sl[dz]].int() for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    cells = ((n_in > 0) & (n_in < 8)).nonzero()
    blk = cells // B
    kept = act[blk[:, 0], blk[:, 1], blk[:, 2]]
    return cells.shape[0], int((~kept).sum()), int(act.sum()), nbk ** 3


@pytest.mark.parametrize("N,B", [(128, 8), (97, 8), (100, 8), (97, 4)])
def test_cull_rule_keeps_every_crossing_of_the_analytic_scene(N, B):
    cells, missed, active, blocks = _cull_on_scene(N, B)
    print(f"N {N} B {B}: {cells} cells with a sign change, {missed} in culled blocks, {active} of {blocks} blocks active")
    assert cells > 10000 and missed == 0 and active < blocks / 4
    assert (N, B) != (128, 8) or (cells > 20000 and blocks == 4096)


def test_min_safe_lipschitz_of_a_distance_field_is_at_most_one():
    from dynhor_amd.mesh_extract import block_grid, grid_axes, min_safe_lipschitz
    N, B = 65, 8
    axes = grid_axes(N, [-1.0] * 3, [1.0] * 3)
    g = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1)
    nbk, c, r = block_grid(axes, B)
    for k in (1.0, 3.0):
        u = k * (0.4 - g.norm(dim=-1))
        need = min_safe_lipschitz(u, k * (0.4 - c.norm(dim=-1)), r, 0.0, B)
        assert 0.5 * k < need <= k, (k, need)
    assert min_safe_lipschitz(torch.ones(N, N, N), torch.ones(nbk ** 3), r, 0.0, B) == 0.0


def test_packed_table_round_trips():
    from dynhor_amd.mesh import marching_cubes_table
    from dynhor_amd.mesh_extract import packed_table
    p = packed_table()
    assert p.dtype == torch.uint8 and p.shape == (256, 16) and p.is_contiguous()
    tri, n = marching_cubes_table()
    back = p[:, :15].long().reshape(256, 5, 3)
    assert torch.equal(torch.where(back == 255, -1, back), tri) and torch.equal(p[:, 15].long(), n)


@pytest.mark.parametrize("N", [5, 128, 1448])
def test_edge_key_sorts_like_the_dense_key(N):
    """The kernel's key lin(lower corner) * 3 + a (a = 0 / 1 / 2 along z / y / x) against mesh.marching_cubes' min * N^3 + max."""
    gen = torch.Generator().manual_seed(N)
    n = 20000
    axis = torch.randint(0, 3, (n,), generator=gen)
    g = torch.randint(0, N - 1, (n, 3), generator=gen)               # lower corner: the upper one stays inside the grid
    lin = (g[:, 0] * N + g[:, 1]) * N + g[:, 2]
    step = torch.tensor([1, N, N * N])[axis]
    dense, sparse = lin * (N ** 3) + (lin + step), lin * 3 + axis
    assert int(dense.max()) < 2 ** 63 and dense.min() >= 0
    # same order, same ties: the ranks agree
    assert torch.equal(torch.unique(dense, return_inverse=True)[1], torch.unique(sparse, return_inverse=True)[1])
    assert (((1 << 20) ** 3 - 1) * 3 + 2) < 2 ** 63                   # the sparse key fits at any resolution the kernels accept


def test_runner_extract_config_defaults_and_validation():
    from dynhor_amd import mesh_extract
    from dynhor_amd.runner import MESH_EXTRACT_DEFAULTS, Runner
    assert MESH_EXTRACT_DEFAULTS == {"mode": "dense", "block": 8, "lipschitz": mesh_extract.DEFAULT_LIPSCHITZ}
    d = mesh_extract.DEFAULT_LIPSCHITZ
    assert d >= 1.0 and (2 * d) == int(2 * d)                         # a multiple of 0.5, never below a distance field's constant
    r = Runner.__new__(Runner)                                        # _extract_conf reads self.conf only
    r.conf = {}
    assert r._extract_conf() == MESH_EXTRACT_DEFAULTS
    assert r._extract_conf("sparse")["mode"] == "sparse"
    r.conf = {"mesh_extract": {"mode": "sparse", "lipschitz": 4}}
    assert r._extract_conf() == {"mode": "sparse", "block": 8, "lipschitz": 4}
    assert r._extract_conf("dense")["mode"] == "dense"
    for bad in ({"mode": "octree"}, {"block": 0}, {"block": 17}, {"block": 2.5}, {"lipschitz": 0}, {"lipschitz": -1.0},
                {"lipschitz": "big"}):
        r.conf = {"mesh_extract": bad}
        with pytest.raises(ValueError):
            r._extract_conf()
    r.conf = {}
    with pytest.raises(ValueError):
        r._extract_conf("blocks")


def test_cli_lists_mesh_extract():
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "--mesh_extract" in p.stdout and "{dense,sparse}" in p.stdout
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", "x.yaml", "--mesh_extract", "octree"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--mesh_extract" in p.stderr


def test_entry_points_declared_exported_and_bound(hiplib):
    from dynhor_amd import _lib
    header = open(os.path.join(ROOT, "include", "dynhor_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header, name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    blob = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"mc_block_points_kernel", b"mc_count_kernel", b"mc_emit_kernel"):
        assert kernel in blob, kernel


def test_entry_points_reject_bad_arguments_without_launching(hiplib):
    null = ctypes.c_void_p(0)
    # no blocks: a no-op, whatever the pointers
    assert hiplib.dh_mc_block_points(null, null, null, 64, null, 0, 8, null, null) == 0
    assert hiplib.dh_mc_count(null, null, 0, 64, 8, 0.0, null, null, null, null, null, null) == 0
    assert hiplib.dh_mc_emit(null, null, 0, 64, 8, 0.0, null, null, 0, null, null, null) == 0
    # null pointers
    assert hiplib.dh_mc_block_points(null, null, null, 64, null, 5, 8, null, null) == -1
    assert hiplib.dh_mc_count(null, null, 5, 64, 8, 0.0, null, null, null, null, null, null) == -1
    assert hiplib.dh_mc_emit(null, null, 5, 64, 8, 0.0, null, null, 7, null, null, null) == -1
    # negative counts, a one-point grid, an empty block, a NaN threshold
    assert hiplib.dh_mc_block_points(null, null, null, 64, null, -1, 8, null, null) == -1
    assert hiplib.dh_mc_block_points(null, null, null, 1, null, 5, 8, null, null) == -1
    assert hiplib.dh_mc_count(null, null, 5, 64, 0, 0.0, null, null, null, null, null, null) == -1
    assert hiplib.dh_mc_count(null, null, 5, 64, 8, float("nan"), null, null, null, null, null, null) == -1
    assert hiplib.dh_mc_emit(null, null, 5, 64, 8, 0.0, null, null, -1, null, null, null) == -1
    # the LDS tile holds (B + 1)^3 floats for B <= 16; one workgroup per block
    assert hiplib.dh_mc_count(null, null, 5, 64, 17, 0.0, null, null, null, null, null, null) == -2
    assert hiplib.dh_mc_emit(null, null, 1 << 31, 64, 8, 0.0, null, null, 7, null, null, null) == -2


def test_cpu_tensors_raise():
    from dynhor_amd import _lib
    from dynhor_amd.mesh_extract import sparse_marching_cubes
    field = lambda p: 0.4 - p.norm(dim=-1)
    with pytest.raises(_lib.DynhorHipError):
        sparse_marching_cubes(field, 33, [-1.0] * 3, [1.0] * 3, lipschitz=1.0, device="cpu")
    for bad in (dict(resolution=1), dict(block=0), dict(block=17), dict(lipschitz=0.0), dict(chunk_points=0), dict(threshold=float("nan"))):
        kw = dict(resolution=33, block=8, lipschitz=1.0, chunk_points=1 << 20, threshold=0.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            sparse_marching_cubes(field, kw.pop("resolution"), [-1.0] * 3, [1.0] * 3, device="cpu", **kw)


@pytest.mark.parametrize("name", ["marching_cubes", "marching_tetrahedra"])
def test_dense_extraction_refuses_resolutions_whose_keys_overflow(name):
    """1448^6 < 2^63 < 1449^6.  The check reads the shape only: a stride-0 view stands in for the 1449^3 grid."""
    from dynhor_amd import mesh
    assert mesh.MAX_DENSE_RESOLUTION == 1448 and 1448 ** 6 < 2 ** 63 < 1449 ** 6
    u = torch.zeros(1).expand(1449, 1449, 1449)
    with pytest.raises(ValueError, match="1448"):
        getattr(mesh, name)(u, 0.0, [-1.0] * 3, [1.0] * 3)
