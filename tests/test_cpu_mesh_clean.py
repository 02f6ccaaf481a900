"""CPU: the mesh-cleaning entry points' declaration, export and host-side argument checks, the wrappers' tensor checks (no device
calls: there is no GPU here) and the --mesh_clean CLI option."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dh_label_dilate", "dh_mesh_mask_votes", "dh_mesh_components")


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
    # empty inputs are no-ops
    assert hiplib.dh_label_dilate(null, 0, 4, 4, 1, null, null, null) == 0
    assert hiplib.dh_mesh_mask_votes(null, 0, null, null, null, null, 3, 4, 4, null, null, null) == 0
    assert hiplib.dh_mesh_components(null, 0, 0, null, null) == 0
    # negative sizes / radius, empty images, null pointers
    assert hiplib.dh_label_dilate(null, -1, 4, 4, 1, null, null, null) == -1
    assert hiplib.dh_label_dilate(null, 2, 4, 4, -1, null, null, null) == -1
    assert hiplib.dh_label_dilate(null, 2, 0, 4, 1, null, null, null) == -1
    assert hiplib.dh_label_dilate(null, 2, 4, 4, 1, null, null, null) == -1
    assert hiplib.dh_mesh_mask_votes(null, -1, null, null, null, null, 3, 4, 4, null, null, null) == -1
    assert hiplib.dh_mesh_mask_votes(null, 5, null, null, null, null, 3, 4, 4, null, null, null) == -1
    assert hiplib.dh_mesh_mask_votes(null, 5, null, null, null, null, 3, 4, 0, null, null, null) == -1
    assert hiplib.dh_mesh_components(null, -1, 4, null, null) == -1
    assert hiplib.dh_mesh_components(null, 3, 4, null, null) == -1
    # labels are int32
    assert hiplib.dh_mesh_components(null, 0, 1 << 31, null, null) == -2


def test_wrappers_reject_cpu_tensors():
    from dynhor_amd import _lib
    from dynhor_amd import mesh_clean as mc
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int64)
    keep = torch.zeros(2, 8, 8, dtype=torch.uint8)
    R, T, K = torch.eye(3).expand(2, 3, 3).contiguous(), torch.zeros(2, 3), torch.eye(3)
    for call in (lambda: mc.dilate_labels(torch.zeros(2, 8, 8, dtype=torch.int8), 1),
                 lambda: mc.mask_votes(v, keep, R, T, K),
                 lambda: mc.vertex_components(4, f),
                 lambda: mc.cull_by_masks(v, f, keep, R, T, K),
                 lambda: mc.keep_components(v, f)):
        with pytest.raises(_lib.DynhorHipError):
            call()


def test_wrappers_reject_wrong_dtypes_and_shapes(monkeypatch):
    """The checks run before any launch: a tensor that claims to be on the device with a wrong dtype or shape raises ValueError."""
    from dynhor_amd import mesh_clean as mc
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    keep = torch.zeros(2, 8, 8, dtype=torch.uint8)
    R, T, K = torch.eye(3).expand(2, 3, 3).contiguous(), torch.zeros(2, 3), torch.eye(3)
    v = torch.zeros(4, 3)
    bad = [lambda: mc.dilate_labels(torch.zeros(2, 8, 8, dtype=torch.uint8), 1),       # labels must be int8
           lambda: mc.dilate_labels(torch.zeros(8, 8, dtype=torch.int8), 1),           # [F,H,W]
           lambda: mc.dilate_labels(torch.zeros(2, 8, 8, dtype=torch.int8), -1),
           lambda: mc.mask_votes(v.double(), keep, R, T, K),
           lambda: mc.mask_votes(torch.zeros(4, 2), keep, R, T, K),
           lambda: mc.mask_votes(v, keep.bool(), R, T, K),
           lambda: mc.mask_votes(v, keep, R[:1], T, K),                              # one pose per frame
           lambda: mc.mask_votes(v, keep, R, T[:, :2], K),
           lambda: mc.mask_votes(v, keep, R, T, torch.eye(4)),
           lambda: mc.vertex_components(4, torch.zeros(2, 3, dtype=torch.int32)),
           lambda: mc.vertex_components(4, torch.zeros(2, 4, dtype=torch.int64)),
           lambda: mc.vertex_components(-1, torch.zeros(2, 3, dtype=torch.int64)),
           lambda: mc.cull_by_masks(v, torch.zeros(2, 3, dtype=torch.int64), keep, R, T, K, min_bg_votes=0),
           lambda: mc.keep_components(v.half(), torch.zeros(2, 3, dtype=torch.int64)),
           lambda: mc.clean_mesh(v, torch.zeros(2, 3, dtype=torch.int64), None, mode="biggest")]
    for call in bad:
        with pytest.raises(ValueError):
            call()


def test_cli_lists_mesh_clean():
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "--mesh_clean" in p.stdout
    for choice in ("none", "mask", "largest", "mask+largest"):
        assert choice in p.stdout.split("--mesh_clean", 1)[1]
    assert "{none,mask,largest,mask+largest}" in p.stdout


def test_runner_clean_config_defaults():
    from dynhor_amd.runner import MESH_CLEAN_DEFAULTS
    assert MESH_CLEAN_DEFAULTS == {"mode": "none", "dilate_px": 2, "min_bg_votes": 1, "min_area_frac": None}
