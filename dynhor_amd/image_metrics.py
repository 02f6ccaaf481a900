"""Image metrics: renderings scored against the frames (csrc/image_metrics.hip, include/dynhor_hip.h).

PSNR alone says little about structure, and a hand-held capture needs its metrics masked: the rendering has a flat background and no
hand, so a plain window that straddles the silhouette compares the object with things the model never draws.

  * ``gaussian_taps_q16``: the window as integers that sum to exactly 2^16, formed in fp64 on the host.
  * ``ssim_frames`` (dh_ssim): per frame the mean and deviation of a masked SSIM over the counted pixels, PSNR and L1 over the usable
    ones.  Every window sum runs over the usable pixels under the window alone and is an exact integer; the formula is a dozen fp64
    operations, each rounded once, so tests/image_metrics_util.py restates the kernel bit for bit in numpy.  A pixel is counted
    when it is usable and at least ``min_weight`` of its window's weight lies on usable pixels: a sliver of three pixels has no
    local structure to compare.

The kernel runs on the current stream; there is no CPU path.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib

SUMS = 6
MAX_RADIUS = 16
MAX_FRAMES_PER_CALL = 65535


def gaussian_taps_q16(sigma: float, radius: int):
    """2 radius + 1 non-negative Python ints that sum to exactly 65536: round(65536 g / sum g) with g = exp(-k^2 / 2 sigma^2) in fp64,
    the remainder on the centre tap.  radius 0: [65536]."""
    sigma, radius = float(sigma), int(radius)
    if not 0.0 < sigma < float("inf"):
        raise ValueError(f"gaussian_taps_q16: sigma must be a number > 0, got {sigma}")
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"gaussian_taps_q16: radius must lie in 0..{MAX_RADIUS}, got {radius}")
    g = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(-radius, radius + 1)]
    s = math.fsum(g)
    taps = [int(math.floor(65536.0 * x / s + 0.5)) for x in g]
    taps[radius] += 65536 - sum(taps)
    if min(taps) < 0:
        raise ValueError(f"gaussian_taps_q16: sigma {sigma} with radius {radius} leaves a negative centre tap")
    return taps


def weight_threshold(min_weight: float) -> int:
    """w_min of dh_ssim = ceil(min_weight 2^32) in 1..2^32 for min_weight in (0, 1]."""
    min_weight = float(min_weight)
    if not 0.0 < min_weight <= 1.0:
        raise ValueError(f"ssim_frames: min_weight must lie in (0, 1], got {min_weight}")
    return max(1, int(math.ceil(min_weight * 4294967296.0)))


def _image(fn, name, t, shape, shape_txt):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.DynhorHipError(f"{fn}: {name} must be a device tensor (the HIP kernel has no CPU fallback)")
    if t.dtype != torch.uint8:
        raise TypeError(f"{fn}: {name} must be torch.uint8, got {t.dtype}")
    if not shape(tuple(t.shape)):
        raise ValueError(f"{fn}: {name} must be {shape_txt}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{fn}: {name} must be contiguous (strides {tuple(t.stride())})")
    return t


def psnr_from_sums(se: float, n_usable: float):
    """10 log10(255^2 3 n / se) over n usable pixels of three channels; inf at se == 0, None at n == 0."""
    if n_usable <= 0:
        return None
    if se <= 0:
        return float("inf")
    return 10.0 * math.log10(65025.0 * 3.0 * n_usable / se)


def ssim_frames(a, b, usable=None, sigma: float = 1.5, radius: int = 5, min_weight: float = 0.5, want_map: bool = False,
                chunk: int = 16):
    """Per-frame scores of the renderings a u8 [F,H,W,3] against the frames b u8 [F,H,W,3] over the pixels with usable u8 [F,H,W] set
    (None: all).  Returns a dict of lists of F entries: ``ssim`` (mean over the counted pixels, None without one), ``ssim_std``,
    ``psnr`` (psnr_from_sums), ``l1`` (mean |a - b| / 255 over usable pixels and channels, None without one), ``counted``, ``usable``
    (ints); with want_map also ``map``, float32 [F,H,W] on the device: the score of a counted pixel, 0 elsewhere.  ``sums`` is the
    kernel's float64 [F,6] on the host.  Frames go to the kernel `chunk` at a time; the result does not depend on the chunk, and nothing
    is read back before the last chunk is enqueued."""
    fn = "ssim_frames"
    a = _image(fn, "a", a, lambda s: len(s) == 4 and s[3] == 3, "[F,H,W,3]")
    F, H, W = a.shape[:3]
    b = _image(fn, "b", b, lambda s: s == (F, H, W, 3), f"[{F},{H},{W},3]")
    if b.device != a.device:
        raise ValueError(f"{fn}: a on {a.device}, b on {b.device}")
    if usable is not None:
        usable = _image(fn, "usable", usable, lambda s: s == (F, H, W), f"[{F},{H},{W}]")
        if usable.device != a.device:
            raise ValueError(f"{fn}: a on {a.device}, usable on {usable.device}")
    if H == 0 or W == 0:
        raise ValueError(f"{fn}: empty images {H}x{W}")
    chunk = int(chunk)
    if not 1 <= chunk <= MAX_FRAMES_PER_CALL:
        raise ValueError(f"{fn}: chunk must lie in 1..{MAX_FRAMES_PER_CALL}, got {chunk}")
    taps = gaussian_taps_q16(sigma, radius)
    radius = int(radius)
    w_min = weight_threshold(min_weight)
    taps_c = (ctypes.c_int32 * len(taps))(*taps)
    L = _lib.lib()
    out = torch.zeros(F, SUMS, dtype=torch.float64, device=a.device)
    smap = torch.empty(F, H, W, dtype=torch.float32, device=a.device) if want_map else None
    with torch.cuda.device(a.device):
        if F > 0:
            n = min(chunk, F)
            ws = torch.empty(max(16, int(L.dh_ssim_workspace(n, H, W))), dtype=torch.uint8, device=a.device)
        for f0 in range(0, F, chunk):
            f1 = min(F, f0 + chunk)
            _lib.check(L.dh_ssim(_lib.ptr(a[f0:f1]), _lib.ptr(b[f0:f1]), _lib.ptr(usable[f0:f1]) if usable is not None else None,
                                 f1 - f0, H, W, taps_c, radius, w_min, _lib.ptr(smap[f0:f1]) if want_map else None,
                                 _lib.ptr(out[f0:f1]), _lib.ptr(ws), _lib.stream()))
    sums = out.cpu()
    res = {"ssim": [], "ssim_std": [], "psnr": [], "l1": [], "counted": [], "usable": [], "sums": sums}
    for s, nc, se, ae, nu, s2 in sums.tolist():
        mean = s / nc if nc > 0 else None
        res["ssim"].append(mean)
        res["ssim_std"].append(math.sqrt(max(0.0, s2 / nc - mean * mean)) if nc > 0 else None)
        res["psnr"].append(psnr_from_sums(se, nu))
        res["l1"].append(ae / (255.0 * 3.0 * nu) if nu > 0 else None)
        res["counted"].append(int(nc))
        res["usable"].append(int(nu))
    if want_map:
        res["map"] = smap
    return res
