"""Mesh distance on the GPU (csrc/mesh_sdf.hip through dynhor_amd/mesh_sdf.py) against the fp64 restatement of tests/mesh_sdf_util.py:
distance, nearest face, winding number and sign on closed, open, degenerate and multi-slab meshes at ragged point counts; bitwise
reproducibility across launches and chunkings; the edge cases of the C ABI."""
import pytest
import torch

from tests import mesh_sdf_util as U
from tests.mesh_eval_util import icosphere

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TILE, SLAB = 256, 512             # csrc/mesh_sdf.hip MS_TILE, MS_SLAB (test_slab_constants checks them through the workspace size)
N_FULL = 4160
SIZES = [1, 63, 64, 65, N_FULL]
NEAR = 1e-4                       # points this close to the surface are left out of the winding / sign assertions (only)

# The tolerances are the fp32 restatement's own error, times 4 for the device's different contraction order: mesh_sdf_util.
# mesh_distance in torch.float32 against itself in float64, on the N_FULL points of every mesh below (measured on a CPU; section 18 of
# DESIGN_NEXT_ROWS.md), largest over the meshes:
F32_DIST_DEV = 8.5e-8             # |dist32 - dist64|, distances up to 1.3
F32_WIND_DEV = 5.2e-6             # |wind32 - wind64| among points farther than NEAR from the surface
TOL_DIST = 4 * F32_DIST_DEV
TOL_WIND = 4 * F32_WIND_DEV


def _triangle():
    return torch.tensor([[0.3, -0.2, 0.1], [-0.25, 0.3, 0.0], [0.05, 0.1, 0.4]]), torch.tensor([[0, 1, 2]])


def _open_ico():
    v, f = icosphere(0.35, 2)
    return v, f[v[f].mean(dim=1)[:, 2] <= 0.2]


def _ico_faces(level, n):
    v, f = icosphere(0.35, level)
    return v, f[:n]


# name -> (verts, faces, closed).  slabs: two slabs, one tile and a ragged rest
MESHES = {
    "triangle": lambda: _triangle() + (False,),
    "cube": lambda: U.cube_mesh() + (True,),
    "ico320": lambda: icosphere(0.35, 2) + (True,),
    "ico320_open": lambda: _open_ico() + (False,),
    "tile-1": lambda: _ico_faces(2, TILE - 1) + (False,),
    "tile": lambda: _ico_faces(2, TILE) + (False,),
    "tile+1": lambda: _ico_faces(2, TILE + 1) + (False,),
    "slabs": lambda: _ico_faces(4, 2 * SLAB + TILE + 37) + (False,),
}

_cache = {}


def reference(name):
    """The mesh on the device, its N_FULL points and the fp64 restatement on them: computed once, shared, never modified."""
    if name not in _cache:
        v, f, closed = MESHES[name]()
        p = U.sample_points(v, f, N_FULL, seed=100 + list(MESHES).index(name))
        v, f, p = v.to(DEV), f.to(DEV), p.to(DEV)
        d, face, wind, _ = U.mesh_distance(p, v, f, chunk=256)
        _cache[name] = dict(v=v, f=f, p=p, d=d, face=face, wind=wind, closed=closed)
    return _cache[name]


def subset(n):
    """Indices of the n-point case: every 64th point of the full set (the first is a vertex of the mesh, the others are ball and
    displaced samples)."""
    return torch.arange(N_FULL, device=DEV) if n == N_FULL else torch.arange(n, device=DEV) * 64


@pytest.mark.parametrize("name", list(MESHES))
def test_point_mix_leaves_out_at_most_two_percent(name):
    r = reference(name)
    left_out = float((r["d"] <= NEAR).double().mean())
    print(f"{name}: {100 * left_out:.2f} % of the points within {NEAR} of the surface")
    assert left_out <= 0.02
    assert int((r["d"] == 0).sum()) >= 3                                  # vertices of the mesh itself are among the points


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(MESHES))
def test_distance_face_winding_and_sign_against_fp64(name, n):
    from dynhor_amd.mesh_sdf import MeshSDF
    r = reference(name)
    idx = subset(n)
    p = r["p"][idx].contiguous()
    d64, w64 = r["d"][idx], r["wind"][idx]
    m = MeshSDF(r["v"], r["f"])
    sdf, face, wind = m.query(p)
    assert sdf.shape == (n,) and face.shape == (n,) and wind.shape == (n,) and face.dtype == torch.int64
    assert bool(torch.isfinite(sdf).all()) and bool(torch.isfinite(wind).all())
    e_d = (sdf.abs().double() - d64).abs().max().item()
    # the reported face need not be fp64's argmin (closest points on shared edges tie): its fp64 distance must be the minimum
    assert int(face.min()) >= 0 and int(face.max()) < r["f"].shape[0]
    e_f = (U.distance_to_faces(p, r["v"], r["f"], face) - d64).abs().max().item()
    keep = d64 > NEAR
    e_w = (wind.double() - w64)[keep].abs().max().item() if bool(keep.any()) else 0.0
    print(f"{name} n={n}: |dist - dist64| {e_d:.3g}, reported face's distance - minimum {e_f:.3g} (tolerance {TOL_DIST:.3g}); "
          f"|wind - wind64| {e_w:.3g} (tolerance {TOL_WIND:.3g}); min |wind64 - 0.5| among kept "
          f"{(w64[keep] - 0.5).abs().min().item() if bool(keep.any()) else float('nan'):.3g}")
    assert e_d <= TOL_DIST
    assert e_f <= TOL_DIST
    assert e_w <= TOL_WIND
    if r["closed"]:
        assert torch.equal((sdf < 0)[keep], (w64 >= 0.5)[keep])
    assert torch.equal((sdf < 0)[sdf != 0], (wind >= 0.5)[sdf != 0])
    if name == "cube":
        v = r["v"].double()
        ref = U.box_sdf(p.double(), (v.max(dim=0).values + v.min(dim=0).values) / 2, (v.max(dim=0).values - v.min(dim=0).values) / 2)
        assert (sdf.abs().double() - ref.abs()).abs().max().item() <= TOL_DIST
        assert torch.equal((sdf < 0)[keep], (ref < 0)[keep])


@pytest.mark.parametrize("name", ["triangle", "cube"])
def test_lowest_face_index_among_exact_ties(name):
    """Ties by construction: a mesh and points on a dyadic grid (edges of length 1/2, coordinates multiples of 1/8), for which every
    fp32 operation of the kernel and of the fp32 restatement is exact (all denominators are powers of two) -- points on the cube's
    edges, diagonals and symmetry planes are equally far from several faces, bit for bit.  The face must be the lowest index that
    attains the minimum, and the squared distance the exact one."""
    from dynhor_amd.mesh_sdf import MeshSDF
    if name == "cube":
        v, f = U.cube_mesh(center=(0.0, 0.0, 0.0), half=0.25)
    else:
        v, f = torch.tensor([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0]]), torch.tensor([[0, 1, 2]])
    ax = torch.arange(-4, 5, dtype=torch.float32) / 8
    p = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
    d32, face32, _, full = U.mesh_distance(p, v, f, dtype=torch.float32)
    d64, _, _, _ = U.mesh_distance(p, v, f)
    if name == "cube":
        assert int(((full == d32[:, None]).sum(dim=1) > 1).sum()) > 300, "the grid must hold many exact ties"
    m = MeshSDF(v.to(DEV), f.to(DEV))
    d2, face, _ = m.query_raw(p.to(DEV))
    assert torch.equal(face.long().cpu(), face32)
    assert torch.equal(d2.cpu().double(), (d64 * d64).float().double())


def _degenerate(v, f):
    """ico320 plus two zero-area faces (an edge and a corner of face 7, as a segment and as a point) and one face with an index
    outside the vertices."""
    a, b, _ = f[7].tolist()
    extra = torch.tensor([[a, b, b], [a, a, a], [3, v.shape[0] + 5, 9]], dtype=f.dtype, device=f.device)
    return torch.cat([f, extra])


@pytest.mark.parametrize("n", SIZES)
def test_degenerate_and_invalid_faces_change_nothing(n):
    from dynhor_amd.mesh_sdf import MeshSDF
    r = reference("ico320")
    p = r["p"][subset(n)].contiguous()
    plain = MeshSDF(r["v"], r["f"]).query_raw(p)
    f2 = _degenerate(r["v"], r["f"])
    with pytest.raises(ValueError, match="outside"):
        MeshSDF(r["v"], f2)                                               # the wrapper validates the index range once per mesh
    got = MeshSDF.unchecked(r["v"], f2).query_raw(p)
    for a, b, what in zip(plain, got, ("sqdist", "face", "wind")):
        assert not bool(torch.isnan(b.float()).any()), what
        assert torch.equal(a, b), what
    # zero-area faces alone, and then they are the nearest faces: a segment and a point for the distance, no winding
    only = MeshSDF.unchecked(r["v"], f2[-3:])
    d2, face, wind = only.query_raw(p)
    assert bool(torch.isfinite(d2).all()) and int(face.max()) <= 1 and int(face.min()) >= 0 and bool((wind == 0).all())
    va, vb = r["v"][f2[-3, 0]].double(), r["v"][f2[-3, 1]].double()
    t = (((p.double() - va) * (vb - va)).sum(-1) / ((vb - va) ** 2).sum()).clamp(0, 1)
    seg = (p.double() - (va + t[:, None] * (vb - va))).norm(dim=1)
    assert (d2.double().sqrt() - seg).abs().max().item() <= TOL_DIST


def test_non_finite_vertex_is_skipped():
    from dynhor_amd.mesh_sdf import MeshSDF
    r = reference("ico320")
    p = r["p"][:650].contiguous()
    f_bad = r["f"][(r["f"] == 5).any(dim=1)]
    keep = r["f"][~(r["f"] == 5).any(dim=1)]
    v2 = r["v"].clone()
    v2[5, 1] = float("nan")
    a = MeshSDF(r["v"], keep).query_raw(p)
    b = MeshSDF(v2, torch.cat([keep, f_bad])).query_raw(p)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_same_call_twice_and_chunked_give_equal_bits():
    from dynhor_amd import _lib
    from dynhor_amd.mesh_sdf import MeshSDF
    r = reference("slabs")
    assert _lib.lib().dh_mesh_sdf_query_workspace(N_FULL, r["f"].shape[0]) == 3 * N_FULL * 16, "this mesh must take three slabs"
    m = MeshSDF(r["v"], r["f"])
    a = m.query_raw(r["p"])
    b = m.query_raw(r["p"])
    c = m.query_raw(r["p"], chunk=1000)
    d = MeshSDF(r["v"], r["f"]).query_raw(r["p"], chunk=37 * 64 + 1)
    for x, y, z, w, what in zip(a, b, c, d, ("sqdist", "face", "wind")):
        assert torch.equal(x, y), what + ": two launches differ"
        assert torch.equal(x, z), what + ": chunks of 1000 differ from one launch"
        assert torch.equal(x, w), what
    # distances and faces alone (NULL outputs) are the same bits
    e = m.query_raw(r["p"], want_face=False, want_wind=False)
    assert torch.equal(e[0], a[0]) and e[1] is None and e[2] is None


def test_slab_constants():
    from dynhor_amd import _lib
    W = _lib.lib().dh_mesh_sdf_query_workspace
    assert W(1, SLAB) == 0 and W(1, SLAB + 1) == 32 and W(1, 2 * SLAB + TILE + 37) == 48


def test_edge_cases():
    from dynhor_amd import _lib
    from dynhor_amd.mesh_sdf import MeshSDF, mesh_signed_distance
    L = _lib.lib()
    r = reference("cube")
    m = MeshSDF(r["v"], r["f"])
    sdf, face, wind = m.query(torch.empty(0, 3, device=DEV))
    assert sdf.shape == face.shape == wind.shape == (0,)
    d2 = torch.full((4,), -7.0, device=DEV)
    p = r["p"][:4].contiguous()
    assert L.dh_mesh_sdf_query(_lib.ptr(m.rec), 12, _lib.ptr(p), 0, _lib.ptr(d2), None, None, None, _lib.stream()) == 0
    assert L.dh_mesh_sdf_query(_lib.ptr(m.rec), 0, _lib.ptr(p), 4, _lib.ptr(d2), None, None, None, _lib.stream()) == -1     # DH_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((d2 == -7.0).all()), "n == 0 and a refused call write nothing"
    q = r["p"][:130].clone()
    q[3, 0], q[64, 2], q[129, 1] = float("nan"), float("inf"), float("-inf")
    sdf, face, wind = m.query(q)
    bad = torch.tensor([3, 64, 129], device=DEV)
    assert bool((sdf[bad] == float("inf")).all()) and bool((face[bad] == -1).all()) and bool((wind[bad] == 0).all())
    ok = torch.ones(130, dtype=torch.bool, device=DEV)
    ok[bad] = False
    ref = m.query(r["p"][:130].contiguous())
    for a, b in zip((sdf, face, wind), ref):
        assert torch.equal(a[ok], b[ok])
    one = mesh_signed_distance(p, r["v"], r["f"])
    assert torch.equal(one[0], ref[0][:4])
    with pytest.raises(ValueError, match="no faces"):
        MeshSDF(r["v"], r["f"][:0])
    with pytest.raises(ValueError, match="float32"):
        m.query(p.double())


def test_query_makes_no_host_synchronisation():
    from dynhor_amd.mesh_sdf import MeshSDF
    r = reference("slabs")
    m = MeshSDF(r["v"], r["f"])
    m.query(r["p"])                                                       # (allocations of the first call)
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.query(r["p"])
        m.query(r["p"], chunk=1000)
    finally:
        torch.cuda.set_sync_debug_mode("default")
