"""CPU: the fp64 restatement of the quadric vertex clustering (tests/mesh_simplify_util.py) has the properties the algorithm claims --
the sqrt(3) h distance bound, a closed manifold result on the three-box fixture, quadric placement far closer to the true surface than
the cell mean, the closed forms of a plane, a corner and a clamped cell -- and the product's host side: mode strings, option checks,
the host-only grid entry point against the restatement, the Runner's config block, and the CLI flag."""
import ctypes
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_simplify_util as U
from tests.mesh_align_util import three_box_mesh, three_box_sdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the three-box fixture
@pytest.fixture(scope="module")
def three_box():
    from dynhor_amd import mesh_simplify  # noqa: F401  (the feature under test: every test of this file needs it)
    v, f = three_box_mesh(96)
    return v, f, U.simplify_ref(v, f, 24, placement="quadric"), U.simplify_ref(v, f, 24, placement="mean")


def test_three_box_distance_bound_manifold_and_quality(three_box):
    from dynhor_amd.metrics import sample_surface
    v, f, (qv, qf, qs, _), (mv, mf, ms, _) = three_box
    h = qs["cell_size"]
    assert qs["n_faces_in"] == f.shape[0] and 0 < qs["n_faces_out"] < f.shape[0] // 3
    assert torch.equal(qf, mf) and ms["n_clamped"] == 0
    # every sampled point of the output within sqrt(3) h of the input: the distance to the nearest input VERTEX bounds the distance
    # to the input surface from above, so the check can only be harder than the statement
    pts, _ = sample_surface(qv, qf, 20_000, 0)
    d = U.point_cloud_distance(pts, v)
    print(f"h {h:.5f}: largest distance of an output sample to the nearest input vertex {float(d.max()) / h:.3f} h")
    assert float(d.max()) <= math.sqrt(3.0) * h
    assert qs["n_boundary_edges"] == 0 and qs["n_nonmanifold_edges"] == 0
    eq, em = three_box_sdf(qv.double()).abs().mean(), three_box_sdf(mv.double()).abs().mean()
    print(f"faces {f.shape[0]} -> {qs['n_faces_out']}; mean |sdf|: quadric {float(eq) / h:.4f} h, cell mean {float(em) / h:.4f} h, "
          f"ratio {float(eq / em):.3f}; clamped cells {qs['n_clamped']}")
    assert float(eq) <= 0.5 * float(em)


# ------------------------------------------------------------------------------------------------ 2. closed forms
def _anchored(verts, faces):
    """The mesh plus two far triangles that pin the bounding box to [0,1]^3 (with 8 cells: h = 1/8)."""
    a = torch.tensor([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0], [0.0, 0.01, 0.0], [1.0, 1.0, 1.0], [0.99, 1.0, 1.0], [1.0, 0.99, 1.0]])
    n = verts.shape[0]
    return torch.cat([verts.float(), a]), torch.cat([faces, torch.tensor([[n, n + 1, n + 2], [n + 3, n + 4, n + 5]])])


def _cell_of(extra, dims, cell):
    key = cell[0] + dims[0] * (cell[1] + dims[1] * cell[2])
    r = int((extra["keys"] == key).nonzero()[0])
    return r


def test_planar_patch_lands_on_its_plane_at_the_centroid():
    """A tilted planar patch inside cell (3,3,3) of 8: the representative is the area-weighted centroid (already on the plane: the
    quadric's pull along the normal is zero there and the Tikhonov term keeps the in-plane position)."""
    c = torch.tensor([3.5, 3.5, 3.5], dtype=torch.float64) / 8
    nrm = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    nrm = nrm / nrm.norm()
    t1 = torch.linalg.cross(nrm, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
    t1 = t1 / t1.norm()
    t2 = torch.linalg.cross(nrm, t1)
    uv = torch.tensor([[-0.03, -0.02], [0.035, -0.025], [0.03, 0.03], [-0.02, 0.035], [0.0, 0.004]], dtype=torch.float64)
    pv = c + 0.01 * nrm + uv[:, :1] * t1 + uv[:, 1:] * t2
    pf = torch.tensor([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]])
    v, f = _anchored(pv, pf)
    _, _, st, ex = U.simplify_ref(v, f, 8)
    assert st["dims"] == [8, 8, 8]
    r = _cell_of(ex, st["dims"], (3, 3, 3))
    assert int(ex["counts"][r]) == 12
    rep = ex["rep64"][r]
    tri = v.double()[pf]
    area = 0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1)
    # the centroid of the 12 corner records, each weighted by its face's area == the area-weighted mean of the face centroids
    centroid = (area[:, None] * tri.mean(dim=1)).sum(0) / area.sum()
    p0 = v.double()[0]
    off_plane = abs(float((rep - p0) @ nrm))
    print(f"off-plane {off_plane:.2e}, distance to the centroid {float((rep - centroid).norm()):.2e}")
    assert off_plane <= 1e-7                                   # the patch's vertices are fp32 roundings of the plane: 0.5 * 2^-24
    assert float((rep - centroid).norm()) <= 1e-7


def _three_plane_patches(corner, centre, size=0.02):
    """Three small square patches on the planes x = corner.x, y = corner.y, z = corner.z, each centred near `centre`."""
    V, Fc = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for i, (s, t) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
            p = [0.0, 0.0, 0.0]
            p[a], p[b], p[c] = corner[a], centre[b] + s * size, centre[c] + t * size
            V.append(p)
        o = 4 * a
        Fc += [[o, o + 1, o + 2], [o, o + 2, o + 3]]
    return torch.tensor(V, dtype=torch.float64), torch.tensor(Fc)


def test_three_orthogonal_planes_give_their_corner():
    lam = 1e-3
    corner = [3.3 / 8, 3.6 / 8, 3.45 / 8]
    centre = [3.5 / 8, 3.5 / 8, 3.5 / 8]
    pv, pf = _three_plane_patches(corner, centre)
    v, f = _anchored(pv, pf)
    _, _, st, ex = U.simplify_ref(v, f, 8, regularization=lam)
    r = _cell_of(ex, st["dims"], (3, 3, 3))
    assert int(ex["counts"][r]) == 18 and st["n_clamped"] == 0
    s = ex["sums"][r].numpy()
    A = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
    w = np.trace(A) / 3
    c = np.array(centre)
    xbar = c + s[10:13] / s[9]
    p = v.double()[[0, 4, 8]].numpy()[[0, 1, 2], [0, 1, 2]]                        # the corner as the fp32 vertices carry it
    bound = lam * w / (np.linalg.eigvalsh(A)[0] + lam * w) * np.linalg.norm(xbar - p)
    err = np.linalg.norm(ex["rep64"][r].numpy() - p)
    print(f"corner error {err:.3e}, Tikhonov bound {bound:.3e}, |xbar - corner| {np.linalg.norm(xbar - p):.3e}")
    assert err <= bound * (1 + 1e-9) + 1e-15
    assert err < 0.01 * np.linalg.norm(xbar - p)


def test_solution_outside_the_cell_is_clamped_and_counted():
    """Planes x = 3.1/8, y = 3.6/8 and the tilted z = 3.5/8 + 4 (x - 3.5/8), all three patches inside cell (3,3,3) = [3/8, 4/8]^3: they
    meet at z = 1.9/8, below the cell, so the representative comes back on the cell's lower z face."""
    centre = [3.5 / 8, 3.5 / 8, 3.5 / 8]
    pv, pf = _three_plane_patches([3.1 / 8, 3.6 / 8, 3.5 / 8], centre)
    pv[8:12, :2] = torch.tensor(centre[:2], dtype=torch.float64) + 0.5 * (pv[8:12, :2] - torch.tensor(centre[:2], dtype=torch.float64))
    pv[8:12, 2] = 3.5 / 8 + 4.0 * (pv[8:12, 0] - 3.5 / 8)
    v, f = _anchored(pv, pf)
    idx = U.cell_index(v, 8)[0]
    assert bool((idx[:12] == 3).all()), "the three patches must lie inside cell (3,3,3)"
    _, _, st, ex = U.simplify_ref(v, f, 8)
    r = _cell_of(ex, st["dims"], (3, 3, 3))
    s = ex["sums"][r].numpy()
    A = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
    xbar = s[10:13] / s[9]
    free = xbar + np.linalg.solve(A + 1e-3 * np.trace(A) / 3 * np.eye(3), -(A @ xbar + s[6:9]))     # relative to the cell's centre
    print(f"unclamped solution (cell units, centre 0, faces at +-0.5): {free * 8}")
    assert free[2] * 8 < -1.0 and abs(free[0] * 8) < 0.5 and abs(free[1] * 8) < 0.5
    rep = ex["rep64"][r].numpy()
    assert st["n_clamped"] == 1
    assert rep[2] == 3.0 / 8                                                        # on the cell's lower z face, exactly
    assert np.allclose(rep[:2], np.array(centre[:2]) + free[:2], rtol=0, atol=1e-12)   # the other axes keep the solution
    assert U.simplify_ref(v, f, 8, placement="mean")[2]["n_clamped"] == 0


# ------------------------------------------------------------------------------------------------ 3. mode strings and ValueErrors
def test_mode_strings():
    from dynhor_amd.mesh_simplify import MAX_CELLS, parse_mode
    assert parse_mode(None) == ("none", None) and parse_mode("none") == ("none", None)
    assert parse_mode("cells:128") == ("cells", 128) and parse_mode("faces:12000") == ("faces", 12000)
    assert parse_mode("cells:1") == ("cells", 1) and parse_mode("faces:0") == ("faces", 0)
    for bad in ("cells", "cells:", "cells:0", "cells:-3", "cells:1.5", "cells:x", f"cells:{MAX_CELLS + 1}", "faces:", "faces:-1",
                "faces:1e3", "quadric", "", "Cells:4", 7, 1.5):
        with pytest.raises(ValueError):
            parse_mode(bad)


def test_option_errors_come_before_the_device_check():
    from dynhor_amd import _lib
    from dynhor_amd.mesh_simplify import MAX_CELLS, simplify_mesh
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for kw in ({}, {"cells": 4, "target_faces": 10}, {"cells": 0}, {"cells": MAX_CELLS + 1}, {"cells": 2.0}, {"cells": True},
               {"target_faces": -1}, {"target_faces": 10, "cells_max": 0}, {"target_faces": 10, "cells_max": MAX_CELLS + 1},
               {"cells": 4, "placement": "median"}, {"cells": 4, "regularization": 0.0}, {"cells": 4, "regularization": -1.0},
               {"cells": 4, "regularization": float("nan")}, {"cells": 4, "regularization": "x"}):
        with pytest.raises(ValueError):
            simplify_mesh(v, f, **kw)
    with pytest.raises(_lib.DynhorHipError, match="no CPU fallback"):               # there is no CPU path
        simplify_mesh(v, f, cells=4)


def test_grid_entry_point_matches_the_restatement(hiplib):
    """dh_simplify_grid is host code: its fp32 cell size and dimensions are the restatement's, bit for bit."""
    g = torch.Generator().manual_seed(3)
    f3, i3 = ctypes.c_float * 3, ctypes.c_int * 3
    for trial in range(40):
        v = (torch.rand(50, 3, generator=g) - 0.5) * torch.tensor([1.0, 0.37, 2.3]) * (10.0 ** (trial % 5 - 2))
        if trial % 7 == 0:
            v[:, 1] = 0.25                                                          # a zero-extent axis
        for cells in (1, 2, 7, 24, 1000, 1 << 20):
            lo, h, dims = U.grid(v, cells)
            hh, dd = ctypes.c_float(), i3()
            assert hiplib.dh_simplify_grid(f3(*lo.tolist()), f3(*v.max(dim=0).values.tolist()), cells, ctypes.byref(hh), dd) == 0
            assert hh.value == float(h) and list(dd) == dims, (trial, cells, hh.value, float(h), list(dd), dims)
    hh, dd = ctypes.c_float(), i3()
    assert hiplib.dh_simplify_grid(f3(1, 1, 1), f3(1, 1, 1), 5, ctypes.byref(hh), dd) == 0 and hh.value == 0.0 and list(dd) == [1, 1, 1]
    assert hiplib.dh_simplify_grid(f3(0, 0, 0), f3(1, 1, 1), 0, ctypes.byref(hh), dd) == -1
    assert hiplib.dh_simplify_grid(f3(0, 0, 0), f3(1, -1, 1), 4, ctypes.byref(hh), dd) == -1
    assert hiplib.dh_simplify_grid(f3(0, 0, 0), f3(1, float("nan"), 1), 4, ctypes.byref(hh), dd) == -1
    assert hiplib.dh_simplify_grid(f3(0, 0, 0), f3(1, 1, 1), (1 << 20) + 1, ctypes.byref(hh), dd) == -2
    null = ctypes.c_void_p(0)
    assert hiplib.dh_simplify_sums() == U.N_SUMS
    assert hiplib.dh_simplify_cells(null, 0, f3(0, 0, 0), 0.1, i3(1, 1, 1), null, null) == 0           # empty input is a no-op
    assert hiplib.dh_simplify_cells(null, 5, f3(0, 0, 0), 0.1, i3(1, 1, 1), null, null) == -1          # null pointers
    assert hiplib.dh_simplify_cells(null, 5, f3(0, 0, 0), -1.0, i3(1, 1, 1), null, null) == -1
    assert hiplib.dh_simplify_quadrics(null, 3, null, 1, null, null, null, 0, f3(0, 0, 0), 0.1, i3(1, 1, 1), 1e-3, 1,
                                       null, null, null, null) == 0
    assert hiplib.dh_simplify_quadrics(null, 3, null, 1, null, null, null, 2, f3(0, 0, 0), 0.1, i3(1, 1, 1), 0.0, 1,
                                       null, null, null, null) == -1
    assert hiplib.dh_simplify_quadrics(null, 3, null, 1, null, null, null, 2, f3(0, 0, 0), 0.1, i3(1, 1, 1), 1e-3, 1,
                                       null, null, null, null) == -1
    assert hiplib.dh_simplify_faces(null, 0, null, 0, 0, null, null, null, null) == 0
    assert hiplib.dh_simplify_faces(null, 2, null, 3, 1, null, null, null, null) == -1


def test_runner_config_block_and_cli_flag():
    from dynhor_amd.runner import MESH_SIMPLIFY_DEFAULTS, Runner
    conf = lambda **kw: SimpleNamespace(conf={"mesh_simplify": kw} if kw else {})
    assert MESH_SIMPLIFY_DEFAULTS == {"mode": "none", "regularization": 1e-3, "cells_max": 1024}
    assert Runner._simplify_conf(conf()) == MESH_SIMPLIFY_DEFAULTS
    assert Runner._simplify_conf(conf(mode="cells:32"))["mode"] == "cells:32"
    assert Runner._simplify_conf(conf(mode="cells:32"), "none")["mode"] == "none"            # the argument overrides the block
    assert Runner._simplify_conf(conf(cells_max=256), "faces:500") == {"mode": "faces:500", "regularization": 1e-3, "cells_max": 256}
    for bad in (dict(mode="cells:0"), dict(mode="fine"), dict(regularization=0), dict(regularization="1e-3"), dict(cells_max=0),
                dict(cells_max=2.5), dict(cells_max=True)):
        with pytest.raises(ValueError):
            Runner._simplify_conf(conf(**bad))
    src = open(os.path.join(ROOT, "dynhor_amd", "run.py")).read()
    assert '"--mesh_simplify"' in src and src.count("simplify=args.mesh_simplify") == 4      # the four modes that take it


# ------------------------------------------------------------------------------------------------ 4. faces:T
def test_target_faces_bisection():
    v, f = three_box_mesh(48)
    for target, cells_max in ((300, 64), (0, 16), (10 ** 6, 32)):
        (qv, qf, st, _), cells, passes = U.simplify_to_target_ref(v, f, target, cells_max=cells_max)
        print(f"target {target}, cells_max {cells_max}: cells {cells}, {st['n_faces_out']} faces, {passes} passes")
        assert st["n_faces_out"] <= target and qf.shape[0] == st["n_faces_out"] and st["cells"] == cells
        assert passes <= math.ceil(math.log2(cells_max)) + 1
    # a generous target takes the finest grid allowed; a target of 0 falls back to one cell
    assert U.simplify_to_target_ref(v, f, 10 ** 6, cells_max=32)[1] == 32
    assert U.simplify_to_target_ref(v, f, 0, cells_max=16)[0][2]["n_faces_out"] == 0
