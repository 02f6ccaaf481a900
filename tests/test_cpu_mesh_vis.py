"""CPU: the mesh-overlay entry point's declaration, export and host-side argument checks, the turntable cameras against a known circle,
the silhouette summary's arithmetic, the mesh_vis config block and the visualize_mesh CLI options, and the shade kernel's code (no
spills, no register soffset on a wide store, integer atomics only, no scalar memory writes)."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def test_entry_point_declared_exported_and_bound(hiplib):
    from dynhor_amd import _lib
    header = open(os.path.join(ROOT, "include", "dynhor_hip.h")).read()
    assert "int dh_mesh_shade(" in header
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dh_mesh_shade")
    assert "dh_mesh_shade" in _lib.SIGNATURES


def _shade(hiplib, nv=4, nf=5, n_frames=3, H=8, W=8, alpha=0.5, label=False, counts=False, verts=False, zbuf=True):
    """dh_mesh_shade with null pointers everywhere except the flagged ones (dummy non-null addresses: nothing is launched)."""
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    v = some if verts else null
    return hiplib.dh_mesh_shade(v, v, null, nv, v, nf, some if zbuf else null, some, some, some, n_frames, H, W, null,
                                some if label else null, alpha, ctypes.c_void_p(1 << 20), some if counts else null, null)


def test_entry_point_rejects_bad_arguments_without_launching(hiplib):
    assert _shade(hiplib, alpha=1.5) == -1
    assert _shade(hiplib, alpha=-0.1) == -1
    assert _shade(hiplib, alpha=float("nan")) == -1
    assert _shade(hiplib, label=True) == -1                       # label without counts
    assert _shade(hiplib, counts=True) == -1                      # counts without label
    assert _shade(hiplib, verts=False, nf=5) == -1                # null verts / normals / faces with faces to draw
    assert _shade(hiplib, zbuf=False) == -1
    assert _shade(hiplib, nv=-1) == -1 and _shade(hiplib, nf=-1) == -1 and _shade(hiplib, n_frames=-1) == -1
    assert _shade(hiplib, H=0) == -1 and _shade(hiplib, W=0) == -1
    # the z-buffer's limits
    assert _shade(hiplib, nf=1 << 32) == -2
    assert _shade(hiplib, n_frames=1 << 31) == -2
    assert _shade(hiplib, W=(1 << 24) + 1) == -2
    # no frames: a no-op, whatever the pointers (the scalar checks still come first)
    assert _shade(hiplib, n_frames=0) == 0
    assert _shade(hiplib, n_frames=0, zbuf=False) == 0
    assert _shade(hiplib, n_frames=0, alpha=2.0) == -1
    # out overlapping rgb
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    assert hiplib.dh_mesh_shade(null, null, null, 0, null, 0, some, some, some, some, 2, 8, 8, ctypes.c_void_p(8192), null, 0.5,
                                ctypes.c_void_p(8192 + 100), null, null) == -1


def test_wrappers_reject_cpu_tensors():
    from dynhor_amd import _lib
    from dynhor_amd import mesh_vis as mv
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int64)
    R, T, K = torch.eye(3).expand(2, 3, 3).contiguous(), torch.zeros(2, 3), torch.eye(3)
    with pytest.raises(_lib.DynhorHipError):
        mv.shade(v, f, torch.full((2, 8, 8), -1, dtype=torch.int64), R, T, K)
    with pytest.raises(_lib.DynhorHipError):
        mv.turntable(v, f, K, 8, 8, R, T)


# ------------------------------------------------------------------------------------------------ turntable cameras
def _circle_cameras(n=12, radius=2.5, elev_deg=20.0, az0=0.7):
    from dynhor_amd.scene import look_at_pose
    el = math.radians(elev_deg)
    Rs, Ts = [], []
    for k in range(n):
        az = az0 + 2 * math.pi * k / n
        pos = torch.tensor([radius * math.cos(el) * math.cos(az), radius * math.cos(el) * math.sin(az), radius * math.sin(el)],
                           dtype=torch.float64)
        R, T = look_at_pose(pos, up=torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
        Rs.append(R); Ts.append(T)
    return torch.stack(Rs).float(), torch.stack(Ts).float()


def test_orbit_cameras_reproduce_a_known_circle():
    from dynhor_amd.mesh_vis import orbit_cameras
    az0 = 0.7
    R, T = _circle_cameras(az0=az0)
    n = 7
    Ro, To = orbit_cameras(R, T, n)
    assert Ro.shape == (n, 3, 3) and To.shape == (n, 3) and Ro.dtype == torch.float32
    Ro, To = Ro.double(), To.double()
    C = -torch.einsum("fji,fj->fi", Ro, To)
    r = C.norm(dim=1)
    assert float((r - 2.5).abs().max()) < 1e-5
    elev = torch.asin(C[:, 2] / r)
    assert float((elev - math.radians(20.0)).abs().max()) < 1e-5
    # rotations: orthonormal, det +1; every optical axis (row 2 of R, the camera z in object coordinates) passes through the origin
    eye = torch.eye(3, dtype=torch.float64)
    assert float((Ro @ Ro.transpose(1, 2) - eye).abs().max()) < 1e-5
    assert float((torch.linalg.det(Ro) - 1).abs().max()) < 1e-5
    axis = Ro[:, 2, :]
    assert float((torch.linalg.cross(axis, C / r[:, None])).norm(dim=1).max()) < 1e-5
    assert float((axis * C).sum(1).max()) < 0                           # looking towards the origin, not away from it
    # azimuths equally spaced from frame 0's
    az = torch.atan2(C[:, 1], C[:, 0])
    want = torch.tensor([az0 + 2 * math.pi * k / n for k in range(n)], dtype=torch.float64)
    d = torch.remainder(az - want + math.pi, 2 * math.pi) - math.pi
    assert float(d.abs().max()) < 1e-5
    # the cameras keep the training cameras' up direction: image "up" (-y) has a positive z component
    assert float((-Ro[:, 1, 2]).min()) > 0
    with pytest.raises(ValueError):
        orbit_cameras(R, T, 0)


# ------------------------------------------------------------------------------------------------ silhouette summary
def test_silhouette_summary_arithmetic():
    from dynhor_amd.mesh_vis import silhouette_summary
    counts = torch.tensor([[90, 5, 5], [0, 0, 0], [40, 30, 30], [70, 0, 30], [10, 0, 0], [50, 25, 25], [3, 1, 0], [0, 4, 0]])
    stems = ["a", "b", "c", "d", "e", "f", "g", "h"]
    s = silhouette_summary(counts, stems)
    ious = [0.9, None, 0.4, 0.7, 1.0, 0.5, 0.75, 0.0]
    assert [fr["stem"] for fr in s["frames"]] == stems
    for fr, want, c in zip(s["frames"], ious, counts.tolist()):
        assert (fr["tp"], fr["fp"], fr["fn"]) == tuple(c)
        assert (fr["iou"] is None) if want is None else fr["iou"] == pytest.approx(want, abs=1e-12)
    vals = [v for v in ious if v is not None]
    assert s["iou_mean"] == pytest.approx(sum(vals) / len(vals), abs=1e-12)
    assert s["iou_median"] == pytest.approx(0.7, abs=1e-12)               # 7 values: the 4th of 0, .4, .5, .7, .75, .9, 1
    assert s["iou_min"] == 0.0
    assert s["worst"] == ["h", "c", "f", "d", "g"]                       # lowest first; the empty frame "b" is not ranked
    # ties in frame order, an even count's median, a list input, no scored frame at all
    s2 = silhouette_summary([[1, 1, 0], [1, 0, 1], [3, 1, 0], [1, 0, 0]], ["0", "1", "2", "3"])
    assert s2["worst"] == ["0", "1", "2", "3"] and s2["iou_median"] == pytest.approx(0.625, abs=1e-12)
    s3 = silhouette_summary(torch.zeros(2, 3, dtype=torch.int64), ["x", "y"])
    assert s3["iou_mean"] is None and s3["iou_median"] is None and s3["iou_min"] is None and s3["worst"] == []
    with pytest.raises(ValueError):
        silhouette_summary(counts, stems[:3])


# ------------------------------------------------------------------------------------------------ config and CLI
def test_mesh_vis_config_defaults():
    from dynhor_amd.runner import MESH_VIS_DEFAULTS, VIS_WRITERS
    assert MESH_VIS_DEFAULTS == {"mesh": None, "normalize": "none", "resolution": 512, "alpha": 0.6, "turntable": 0}
    assert 1 <= VIS_WRITERS <= 8


def test_cli_lists_visualize_mesh():
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    out = p.stdout
    assert "visualize_mesh" in out.split("--mode", 1)[1].split("--is_continue", 1)[0]
    for flag in ("--vis_mesh", "--vis_normalize", "--turntable"):
        assert flag in out, flag
    assert "{none,reference}" in out.split("--vis_normalize", 1)[1]


# ------------------------------------------------------------------------------------------------ code of the shade kernel
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_shade_kernel_listing_neither_spills_nor_stores_wide_with_a_register_soffset(tmp_path):
    from tests.test_cpu_isa_inflight import LISTING, _no_register_soffset_on_wide_stores
    out = tmp_path / "mesh_vis.s"
    subprocess.run(LISTING + [os.path.join(ROOT, "dynhor_amd", "csrc", "mesh_vis.hip"), "-o", str(out)], check=True, timeout=600,
                   stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels = re.findall(r"^(_ZN2dh\w*mesh_shade_kernel\w*):.*?; ScratchSize: (\d+)", text, flags=re.S | re.M)
    assert len(kernels) == 2, kernels                                    # the dword and the byte instantiation
    assert all(int(scratch) == 0 for _, scratch in kernels), kernels
    assert not [ln for ln in text.split("\n") if ln.strip().startswith("scratch_")]
    _no_register_soffset_on_wide_stores(text)


def _scalar_memory_write(op):
    """A scalar-unit instruction that writes memory: its stores, its atomics and its data-cache write-back."""
    return op.startswith("s_") and any(w in op for w in ("store", "atomic", "dcache_wb"))


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
def test_shade_kernel_in_the_built_library(tmp_path):
    """The library as built: both instantiations exist, add their counts with vector 64-bit integer atomics (no float atomic, no
    compare-and-swap loop), move a full group's pixels as dwords, and hold no scalar memory write."""
    from dynhor_amd import _lib
    lib = tmp_path / "lib.so"
    shutil.copy(_lib.LIB_PATH, lib)
    subprocess.run([OBJDUMP, "--offloading", str(lib)], check=True, cwd=tmp_path, capture_output=True, timeout=300)
    objs = sorted(p for p in os.listdir(tmp_path) if p.endswith("gfx950"))
    ops = {}
    for o in objs:
        dis = subprocess.run([OBJDUMP, "-d", str(tmp_path / o)], check=True, capture_output=True, text=True, timeout=300).stdout
        kernel = None
        for line in dis.split("\n"):
            t = line.strip()
            if t.endswith(">:"):
                kernel = t if "mesh_shade_kernel" in t else None
                if kernel:
                    ops[kernel] = []
            elif kernel and t:
                ops[kernel].append(t.split()[0])
    assert len(ops) == 2, list(ops)
    for name, body in ops.items():
        assert not [o for o in body if _scalar_memory_write(o)], name
        atomics = [o for o in body if "atomic" in o]
        assert atomics and all(o.startswith("global_atomic_add_x2") for o in atomics), (name, sorted(set(atomics)))
    vec = next(b for n, b in ops.items() if "ILb1E" in n)
    assert "global_load_dwordx3" in vec and "global_store_dwordx3" in vec and "global_load_dwordx4" in vec
