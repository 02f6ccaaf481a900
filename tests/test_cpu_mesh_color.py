"""CPU: the mesh-colouring entry points' declaration, export and host-side argument checks, the coloured PLY writer (byte-identical
without colours, round trip with them), vertex normals against numpy in fp64, the mesh_color config block and the --mesh_color CLI
option, and the built library's code for the new kernels (no scalar memory writes)."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dh_mesh_raster_depth", "dh_mesh_bake_colors")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def test_entry_points_declared_exported_and_bound(hiplib):
    from dynhor_amd import _lib
    header = open(os.path.join(ROOT, "include", "dynhor_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header, name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name


def test_entry_points_reject_bad_arguments_without_launching(hiplib):
    null = ctypes.c_void_p(0)
    raster, bake = hiplib.dh_mesh_raster_depth, hiplib.dh_mesh_bake_colors
    # empty inputs are no-ops
    assert raster(null, 4, null, 0, null, null, null, 3, 8, 8, null, null) == 0
    assert raster(null, 4, null, 5, null, null, null, 0, 8, 8, null, null) == 0
    assert bake(null, null, 0, null, null, null, null, null, null, 3, 8, 8, 0.01, 0.1, null, null, null) == 0
    assert bake(null, null, 5, null, null, null, null, null, null, 0, 8, 8, 0.01, 0.1, null, null, null) == 0
    # negative sizes, empty images, null pointers, bad thresholds
    assert raster(null, -1, null, 5, null, null, null, 3, 8, 8, null, null) == -1
    assert raster(null, 4, null, -1, null, null, null, 3, 8, 8, null, null) == -1
    assert raster(null, 4, null, 5, null, null, null, -1, 8, 8, null, null) == -1
    assert raster(null, 4, null, 5, null, null, null, 3, 0, 8, null, null) == -1
    assert raster(null, 4, null, 5, null, null, null, 3, 8, 8, null, null) == -1
    assert bake(null, null, -1, null, null, null, null, null, null, 3, 8, 8, 0.01, 0.1, null, null, null) == -1
    assert bake(null, null, 5, null, null, null, null, null, null, 3, 8, 0, 0.01, 0.1, null, null, null) == -1
    assert bake(null, null, 5, null, null, null, null, null, null, 3, 8, 8, 0.01, 0.1, null, null, null) == -1
    assert bake(null, null, 5, null, null, null, null, null, null, 3, 8, 8, -0.01, 0.1, null, null, null) == -1
    assert bake(null, null, 5, null, null, null, null, null, null, 3, 8, 8, float("nan"), 0.1, null, null, null) == -1
    assert bake(null, null, 5, null, null, null, null, null, null, 3, 8, 8, 0.01, float("nan"), null, null, null) == -1
    # face ids are the low 32 bits of a key; n_views is int32; pixel centres must be exact in fp32
    assert raster(null, 4, null, 1 << 32, null, null, null, 3, 8, 8, null, null) == -2
    assert raster(null, 4, null, 5, null, null, null, 3, 8, (1 << 24) + 1, null, null) == -2
    assert bake(null, null, 1 << 31, null, null, null, null, null, null, 3, 8, 8, 0.01, 0.1, null, null, null) == -2


def test_wrappers_reject_cpu_tensors_and_bad_modes():
    from dynhor_amd import _lib
    from dynhor_amd import mesh_color as mc
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int64)
    R, T, K = torch.eye(3).expand(2, 3, 3).contiguous(), torch.zeros(2, 3), torch.eye(3)
    with pytest.raises(_lib.DynhorHipError):
        mc.raster_depth(v, f, R, T, K, 8, 8)
    with pytest.raises(_lib.DynhorHipError):
        mc.network_vertex_colors(None, v)
    with pytest.raises(ValueError):
        mc.color_mesh(v, f, "texture")


# ------------------------------------------------------------------------------------------------ PLY
def _old_write_ply(path, verts, faces):
    """The writer as it was before vertex colours: geometry only."""
    v = verts.detach().cpu().numpy().astype(np.float32)
    f = faces.detach().cpu().numpy().astype(np.int32)
    with open(path, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                  "property float z\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n"
                  % (len(v), len(f))).encode())
        fh.write(v.tobytes())
        rec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        rec["n"] = 3
        rec["i"] = f
        fh.write(rec.tobytes())


def _small_mesh():
    g = torch.Generator().manual_seed(0)
    verts = torch.randn(37, 3, generator=g)
    faces = torch.randint(0, 37, (53, 3), generator=g)
    colors = torch.randint(0, 256, (37, 3), generator=g).to(torch.uint8)
    return verts, faces, colors


def test_write_ply_without_colors_is_byte_identical(tmp_path):
    from dynhor_amd.mesh import write_ply
    verts, faces, _ = _small_mesh()
    _old_write_ply(tmp_path / "old.ply", verts, faces)
    write_ply(str(tmp_path / "new.ply"), verts, faces)
    write_ply(str(tmp_path / "none.ply"), verts, faces, colors=None)
    old = (tmp_path / "old.ply").read_bytes()
    assert (tmp_path / "new.ply").read_bytes() == old
    assert (tmp_path / "none.ply").read_bytes() == old


def test_colored_ply_round_trips(tmp_path):
    from dynhor_amd.mesh import write_ply
    from dynhor_amd.metrics import load_mesh
    verts, faces, colors = _small_mesh()
    p = str(tmp_path / "c.ply")
    write_ply(p, verts, faces, colors=colors)
    lv, lf = load_mesh(p)
    assert torch.equal(lv, verts) and torch.equal(lf, faces)
    data = open(p, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    assert b"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face" in head
    rec = np.frombuffer(body, dtype=[("p", "<f4", (3,)), ("c", "u1", (3,))], count=37)
    np.testing.assert_array_equal(rec["c"], colors.numpy())
    np.testing.assert_array_equal(rec["p"], verts.numpy())
    with pytest.raises(ValueError):
        write_ply(p, verts, faces, colors=colors.int())
    with pytest.raises(ValueError):
        write_ply(p, verts, faces, colors=colors[:5])


# ------------------------------------------------------------------------------------------------ normals
def _normals_fp64(v, f):
    v = v.astype(np.float64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    norm = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(norm > 0, n / np.where(norm > 0, norm, 1.0), 0.0)


def test_vertex_normals_match_fp64_and_are_reproducible():
    from dynhor_amd.mesh_color import vertex_normals
    g = torch.Generator().manual_seed(1)
    verts = torch.randn(500, 3, generator=g)
    faces = torch.randint(0, 480, (2000, 3), generator=g)           # vertices 480..499 are in no face
    n = vertex_normals(verts, faces)
    assert n.dtype == torch.float32 and n.shape == (500, 3)
    ref = _normals_fp64(verts.numpy(), faces.numpy())
    np.testing.assert_allclose(n.numpy(), ref, rtol=0, atol=1e-6)
    assert (n[480:] == 0).all()
    assert torch.equal(n, vertex_normals(verts, faces))
    # a closed, outward-wound shape: the normals point away from the centre
    from dynhor_amd.mesh import marching_cubes
    ax = torch.linspace(-1, 1, 24)
    gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
    sv, sf = marching_cubes(0.6 - torch.sqrt(gx ** 2 + gy ** 2 + gz ** 2), 0.0, [-1.0] * 3, [1.0] * 3)
    sn = vertex_normals(sv, sf)
    cos = (sn * torch.nn.functional.normalize(sv, dim=1)).sum(1)
    assert float(cos.min()) > 0.9, float(cos.min())


# ------------------------------------------------------------------------------------------------ config and CLI
def test_runner_color_config_defaults_and_mode_check():
    from dynhor_amd.runner import MESH_COLOR_DEFAULTS, Runner
    assert MESH_COLOR_DEFAULTS == {"mode": "none", "erode_px": 1, "min_cos": 0.1, "depth_eps": 0.01}
    r = Runner.__new__(Runner)
    r.conf = {"mesh_color": {"mode": "views", "erode_px": 3}}
    assert r._color_conf() == {"mode": "views", "erode_px": 3, "min_cos": 0.1, "depth_eps": 0.01}
    assert r._color_conf("network")["mode"] == "network"
    with pytest.raises(ValueError):
        r._color_conf("texture")
    r.conf = {"mesh_color": {"mode": "vertex"}}
    with pytest.raises(ValueError):
        r._color_conf()
    r.conf = {}
    assert r._color_conf()["mode"] == "none"


def test_cli_lists_mesh_color():
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "{none,views,network,views+network}" in p.stdout.split("--mesh_color", 1)[1]


# ------------------------------------------------------------------------------------------------ code of the new kernels
def _scalar_memory_write(op):
    """A scalar-unit instruction that writes memory: its stores, its atomics and its data-cache write-back."""
    return op.startswith("s_") and any(w in op for w in ("store", "atomic", "dcache_wb"))


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
def test_new_kernels_hold_no_scalar_memory_write(tmp_path):
    """Disassembles the library as built: the raster and bake kernels exist, combine depths with a vector 64-bit atomic minimum, and
    hold no scalar store, scalar atomic or scalar cache write-back."""
    from dynhor_amd import _lib
    lib = tmp_path / "lib.so"
    shutil.copy(_lib.LIB_PATH, lib)
    subprocess.run([OBJDUMP, "--offloading", str(lib)], check=True, cwd=tmp_path, capture_output=True, timeout=300)
    objs = sorted(p for p in os.listdir(tmp_path) if p.endswith("gfx950"))
    found, bad, umin = set(), [], 0
    for o in objs:
        dis = subprocess.run([OBJDUMP, "-d", str(tmp_path / o)], check=True, capture_output=True, text=True, timeout=300).stdout
        kernel = None
        for line in dis.split("\n"):
            t = line.strip()
            if t.endswith(">:"):
                kernel = next((k for k in ("mesh_raster_kernel", "mesh_bake_kernel") if k in t), None)
                if kernel:
                    found.add(kernel)
            elif kernel:
                if t and _scalar_memory_write(t.split()[0]):
                    bad.append((kernel, t[:80]))
                umin += t.startswith("global_atomic_umin_x2")
    assert found == {"mesh_raster_kernel", "mesh_bake_kernel"}, found
    assert not bad, bad
    assert umin >= 1
