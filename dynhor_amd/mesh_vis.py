"""The reconstructed (or any) mesh drawn over every frame at the dataset's current poses, and its silhouette scored against the
object masks the frames carry.

  * ``shade``: the mesh shaded from a ``mesh_color.raster_depth`` z-buffer and composited over the frames (csrc/mesh_vis.hip,
    dh_mesh_shade): perspective-correct normals (and vertex colours, if given) at every covered pixel centre, a double-sided
    headlight along the optical axis, c = min(1, base (0.3 + 0.7 |n_cam.z| / |n|)), out = alpha c + (1 - alpha) frame.  Uncovered
    pixels keep the frame.  With labels it also counts per frame, over the pixels with label >= 0 (hand pixels excluded, the keep
    convention of the losses), tp = covered object pixels, fp = covered background pixels, fn = uncovered object pixels.
  * ``overlay_frames``: raster + shade over the dataset in frame chunks; ``silhouette_summary``: per-frame IoU = tp / (tp + fp + fn)
    and its mean / median / minimum, with the worst frames named.
  * ``orbit_cameras`` / ``turntable``: a ring of cameras around the object origin derived from the training cameras (their mean up
    axis, distance and elevation), and the mesh rendered from it on white.

The image functions run on the current stream; there is no CPU path.  orbit_cameras and silhouette_summary are plain torch / Python
and take CPU tensors too.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._args import check_cams, check_faces, check_verts, device_tensor, same_device
from .mesh_color import _draw_args, frame_chunks, vertex_normals

BASE_COLOR = (0.8, 0.46, 0.51)      # the constant base colour of a mesh without vertex colours
N_WORST = 5


def shade(verts, faces, zbuf, R, T, K, normals=None, colors=None, rgb=None, label=None, alpha: float = 1.0):
    """(out u8 [F,H,W,3], counts int64 [F,3] or None).  zbuf: raster_depth(verts, faces, R, T, K, H, W) (int64 [F,H,W]); normals:
    unit vertex normals (default vertex_normals(verts, faces)); colors: u8 [V,3] or None for BASE_COLOR; rgb: u8 [F,H,W,3] frames or
    None for white; label: i8 [F,H,W] (1 object, 0 background, -1 hand) or None for no counts; alpha in [0, 1]."""
    fn = "shade"
    verts, faces, zbuf, R, T, K, alpha, normals, rgb = _draw_args(fn, verts, faces, zbuf, R, T, K, alpha, normals, rgb)
    F, H, W = zbuf.shape
    if colors is not None:
        colors = device_tensor(fn, "colors", colors, torch.uint8, lambda s: s == tuple(verts.shape), "[V,3]")
    if label is not None:
        label = device_tensor(fn, "label", label, torch.int8, lambda s: s == (F, H, W), f"[{F},{H},{W}]")
    same_device(fn, zbuf.device, colors, label)
    out = torch.empty(F, H, W, 3, dtype=torch.uint8, device=zbuf.device)
    counts = torch.zeros(F, 3, dtype=torch.int64, device=zbuf.device) if label is not None else None
    opt = lambda t: _lib.ptr(t) if t is not None else ctypes.c_void_p(0)
    with torch.cuda.device(zbuf.device):
        _lib.check(_lib.lib().dh_mesh_shade(_lib.ptr(verts), _lib.ptr(normals), opt(colors), verts.shape[0], _lib.ptr(faces),
                                            faces.shape[0], _lib.ptr(zbuf), _lib.ptr(R), _lib.ptr(T), _lib.ptr(K), F, H, W, opt(rgb),
                                            opt(label), alpha, _lib.ptr(out), opt(counts), _lib.stream()))
    return out, counts


def _draw(verts, faces, zbuf, Rc, Tc, K, normals, colors, texture, rgb=None, label=None, alpha: float = 1.0):
    """(out, counts) of one chunk: shade, or with texture = (uv, tex) the counts of shade and the image of render_textured, lit."""
    out, counts = None, None
    if texture is None or label is not None:
        out, counts = shade(verts, faces, zbuf, Rc, Tc, K, normals=normals, colors=colors, rgb=rgb, label=label, alpha=alpha)
    if texture is not None:
        from .mesh_texture import render_textured
        out = render_textured(verts, faces, zbuf, Rc, Tc, K, texture[0], texture[1], normals=normals, rgb=rgb, alpha=alpha, lit=True)[0]
    return out, counts


def overlay_frames(verts, faces, dataset, colors=None, alpha: float = 0.6, frame_chunk: int = 16, sink=None, texture=None):
    """counts int64 [F,3] (tp, fp, fn per frame) of the mesh drawn over the dataset's frames with its current poses (Dataset.R / T /
    K, refined in place by pose refinement), its rgb and its labels.  Frames go in chunks of `frame_chunk` (frame_chunks: raster, then
    shade); sink(f0, out_chunk u8 [n,H,W,3]) is called for every chunk when given.  texture = (uv, tex) of a mesh that has one: the
    same counts (shade's, from the same z-buffer), the images drawn lit through mesh_texture.render_textured.  Images and counts are
    bitwise the same for every chunk size."""
    fn = "overlay_frames"
    verts = check_verts(fn, verts)
    faces = check_faces(fn, faces)
    ds = dataset
    F, H, W = ds.n_images, ds.H, ds.W
    R, T, K = check_cams(fn, F, ds.R, ds.T, ds.K, verts.device)
    normals = vertex_normals(verts, faces)
    counts = torch.zeros(F, 3, dtype=torch.int64, device=verts.device)
    for f0, f1, Rc, Tc, zbuf in frame_chunks(fn, verts, faces, R, T, K, H, W, frame_chunk):
        out, counts[f0:f1] = _draw(verts, faces, zbuf, Rc, Tc, K, normals, colors, texture, rgb=ds.rgb[f0:f1], label=ds.label[f0:f1],
                                   alpha=alpha)
        if sink is not None:
            sink(f0, out)
        del out
    return counts


def silhouette_summary(counts, stems) -> dict:
    """Per-frame silhouette IoU from counts [F,3] (tp, fp, fn; tensor or nested list) and the frames' names: frames = [{stem, iou,
    tp, fp, fn}] with iou = tp / (tp + fp + fn), None when that is 0; iou_mean, iou_median and iou_min over the frames that have an
    IoU (None when none has); worst = the stems of the N_WORST lowest IoUs, lowest first (ties in frame order)."""
    rows = counts.tolist() if torch.is_tensor(counts) else [list(r) for r in counts]
    stems = list(stems)
    if len(stems) != len(rows) or any(len(r) != 3 for r in rows):
        raise ValueError(f"silhouette_summary: counts [F,3] and F stems, got {len(rows)} rows and {len(stems)} stems")
    frames = []
    for s, (tp, fp, fn) in zip(stems, rows):
        tp, fp, fn = int(tp), int(fp), int(fn)
        d = tp + fp + fn
        frames.append({"stem": s, "iou": tp / d if d else None, "tp": tp, "fp": fp, "fn": fn})
    scored = [(fr["iou"], k) for k, fr in enumerate(frames) if fr["iou"] is not None]
    vals = sorted(v for v, _ in scored)
    n = len(vals)
    median = None if not n else (vals[n // 2] if n % 2 else 0.5 * (vals[n // 2 - 1] + vals[n // 2]))
    return {"frames": frames, "iou_mean": sum(vals) / n if n else None, "iou_median": median, "iou_min": vals[0] if n else None,
            "worst": [frames[k]["stem"] for _, k in sorted(scored)[:N_WORST]]}


def orbit_cameras(R, T, n: int):
    """(R [n,3,3], T [n,3]) of a turntable around the object origin, from the training cameras R [F,3,3], T [F,3] (x_cam = R x + T):
    up axis u = the normalised mean of R_f^T (0, -1, 0); radius = the mean camera distance |C_f|, C_f = -R_f^T T_f; elevation = the
    mean of asin(<C_f / |C_f|, u>); n azimuths equally spaced about u, starting at frame 0's; each camera is scene.look_at_pose(pos,
    up=u).  Computed in fp64; returned in R's dtype on R's device."""
    from .scene import look_at_pose
    n = int(n)
    if n < 1:
        raise ValueError(f"orbit_cameras: n must be >= 1, got {n}")
    R64 = R.detach().reshape(-1, 3, 3).to("cpu", torch.float64)
    T64 = T.detach().reshape(-1, 3).to("cpu", torch.float64)
    if R64.shape[0] == 0 or R64.shape[0] != T64.shape[0]:
        raise ValueError(f"orbit_cameras: R [F,3,3] and T [F,3] with F >= 1, got {tuple(R.shape)} and {tuple(T.shape)}")
    u = torch.nn.functional.normalize(-R64[:, 1, :].mean(dim=0), dim=0)
    C = -torch.einsum("fji,fj->fi", R64, T64)
    dist = C.norm(dim=1)
    Chat = C / dist[:, None]
    radius = float(dist.mean())
    elev = float(torch.asin((Chat @ u).clamp(-1.0, 1.0)).mean())
    e1 = Chat[0] - (Chat[0] @ u) * u                        # frame 0's direction in the plane about u
    if float(e1.norm()) < 1e-9:                             # frame 0 looks along u: any direction in the plane
        e1 = torch.linalg.cross(u, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64))
        if float(e1.norm()) < 1e-9:
            e1 = torch.linalg.cross(u, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64))
    e1 = e1 / e1.norm()
    e2 = torch.linalg.cross(u, e1)
    Rs, Ts = [], []
    for k in range(n):
        az = 2.0 * math.pi * k / n
        pos = radius * (math.cos(elev) * (math.cos(az) * e1 + math.sin(az) * e2) + math.sin(elev) * u)
        Rk, Tk = look_at_pose(pos, up=u)
        Rs.append(Rk); Ts.append(Tk)
    return torch.stack(Rs).to(R.device, R.dtype), torch.stack(Ts).to(R.device, R.dtype)


def turntable(verts, faces, K, H: int, W: int, R, T, colors=None, frame_chunk: int = 16, texture=None):
    """u8 [n,H,W,3]: the mesh from the cameras R [n,3,3], T [n,3] (e.g. orbit_cameras) with intrinsics K, on white, alpha 1; with
    texture = (uv, tex) drawn with its texture, lit."""
    verts = check_verts("turntable", verts)
    faces = check_faces("turntable", faces)
    n = R.shape[0]
    R, T, K = check_cams("turntable", n, R, T, K, verts.device)
    normals = vertex_normals(verts, faces)
    out = torch.empty(n, int(H), int(W), 3, dtype=torch.uint8, device=verts.device)
    for f0, f1, Rc, Tc, zbuf in frame_chunks("turntable", verts, faces, R, T, K, H, W, frame_chunk):
        out[f0:f1] = _draw(verts, faces, zbuf, Rc, Tc, K, normals, colors, texture)[0]
    return out
