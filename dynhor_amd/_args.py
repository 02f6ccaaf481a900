"""What the wrappers of the mesh and frame kernels check alike before a launch, under the caller's name `fn`, and the phase timer of
the pipelines that report seconds.  There is no CPU path: a tensor that is not on the device is a DynhorHipError."""
from __future__ import annotations

import time

import torch

from . import _lib


def device_tensor(fn, name, t, dtype, shape_ok, shape_txt):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.DynhorHipError(f"{fn}: {name} must be a device tensor (the HIP kernel has no CPU fallback)")
    if t.dtype != dtype or not shape_ok(tuple(t.shape)):
        raise ValueError(f"{fn}: {name} must be {dtype} {shape_txt}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def check_verts(fn, verts):
    return device_tensor(fn, "verts", verts, torch.float32, lambda s: len(s) == 2 and s[1] == 3, "[V,3]")


def check_faces(fn, faces):
    return device_tensor(fn, "faces", faces, torch.int64, lambda s: len(s) == 2 and s[1] == 3, "[M,3]")


def same_device(fn, device, *tensors):
    if any(t is not None and t.device != device for t in tensors):
        raise ValueError(f"{fn}: every tensor must be on {device}")


def _rtk(fn, F, R, T, K):
    R = device_tensor(fn, "R", R, torch.float32, lambda s: s in ((F, 3, 3), (F, 9)), f"[{F},3,3]")
    T = device_tensor(fn, "T", T, torch.float32, lambda s: s in ((F, 3), (F, 1, 3)), f"[{F},3]")
    K = device_tensor(fn, "K", K, torch.float32, lambda s: s == (3, 3), "[3,3]")
    return R, T, K


def check_cams(fn, F, R, T, K, device):
    R, T, K = _rtk(fn, F, R, T, K)
    same_device(fn, device, R, T, K)
    return R, T, K


def check_poses(fn, keep, R, T, K):
    """check_cams for the F frames of a keep map u8 [F,H,W], which is checked with them."""
    keep = device_tensor(fn, "keep", keep, torch.uint8, lambda s: len(s) == 3, "[F,H,W]")
    R, T, K = _rtk(fn, keep.shape[0], R, T, K)
    if len({t.device for t in (keep, R, T, K)}) != 1:
        raise ValueError(f"{fn}: keep, R, T and K must be on one device")
    return keep, R, T, K


def lap(timer, key, t0, device):
    """The clock now, after timer[key] has gained the seconds since t0 behind a device synchronise (key None: the synchronise
    alone).  timer None: nothing is timed and nothing waits."""
    if timer is not None:
        torch.cuda.synchronize(device)
        if key is not None:
            timer[key] = timer.get(key, 0.0) + time.perf_counter() - t0
    return time.perf_counter()
