"""Vertex colours for an extracted mesh, from the observed pixels of the training frames or from the colour network.

  * ``raster_depth``: z-buffer of the mesh in every frame (csrc/mesh_color.hip, dh_mesh_raster_depth): the key
    (float_bits(depth) << 32) | face of the nearest face at every pixel centre, by a 64-bit atomic minimum (bitwise reproducible).
  * ``bake_vertex_colors``: per vertex, the cosine-weighted mean of the pixels that see it (dh_mesh_bake_colors): a frame counts when
    the vertex is in front of the camera and inside the image, its nearest pixel is usable (object label, eroded by ``erode_px`` so
    that silhouette edges bleed neither background nor hand colour), the vertex is not hidden (camera depth <= z-buffer depth +
    ``depth_eps``), and it faces the camera (cos >= ``min_cos``).  Hand (-1) and background (0) pixels never colour the object.
  * ``network_vertex_colors``: the colour MLP at each vertex, seen along -n (n the normalised SDF gradient; instant-nsr-pl's export
    rule), through the renderer's family hooks, so the neus and hash families both work.
  * ``color_mesh``: "none" | "views" | "network" | "views+network" (unseen vertices take the network colour; in "views" 0.5 grey).

The kernels run on the current stream; there is no CPU path.
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import check_cams, check_faces, check_verts, device_tensor, same_device
from .mesh_clean import dilate_labels

MODES = ("none", "views", "network", "views+network")


def _normals(fn, verts, faces, normals):
    if normals is None:
        normals = vertex_normals(verts, faces)
    return device_tensor(fn, "normals", normals, torch.float32, lambda s: s == tuple(verts.shape), "[V,3]")


def _draw_args(fn, verts, faces, zbuf, R, T, K, alpha, normals, rgb):
    """What mesh_vis.shade and mesh_texture.render_textured check alike, under the caller's name `fn`: (verts, faces, zbuf int64
    [F,H,W] with H, W > 0, R, T, K for its F frames, alpha as a float in [0, 1], normals (default vertex_normals), rgb u8 [F,H,W,3] or
    None), all on zbuf's device."""
    verts = check_verts(fn, verts)
    faces = check_faces(fn, faces)
    zbuf = device_tensor(fn, "zbuf", zbuf, torch.int64, lambda s: len(s) == 3, "[F,H,W]")
    F, H, W = zbuf.shape
    if H == 0 or W == 0:
        raise ValueError(f"{fn}: empty images {H}x{W}")
    R, T, K = check_cams(fn, F, R, T, K, zbuf.device)
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"{fn}: alpha must lie in [0, 1], got {alpha}")
    normals = _normals(fn, verts, faces, normals)
    if rgb is not None:
        rgb = device_tensor(fn, "rgb", rgb, torch.uint8, lambda s: s == (F, H, W, 3), f"[{F},{H},{W},3]")
    same_device(fn, zbuf.device, verts, faces, normals, rgb)
    return verts, faces, zbuf, R, T, K, alpha, normals, rgb


def _check_bake_args(fn, erode_px, min_cos, depth_eps, frame_chunk, sharpen=None):
    want, got = "erode_px >= 0, frame_chunk >= 1, depth_eps >= 0, min_cos a number", f"{erode_px}, {frame_chunk}, {depth_eps}, {min_cos}"
    bad = int(erode_px) < 0 or int(frame_chunk) < 1 or not float(depth_eps) >= 0 or float(min_cos) != float(min_cos)
    if sharpen is not None:
        want, got, bad = want + ", sharpen in 0..4", got + f", {sharpen}", bad or not 0 <= int(sharpen) <= 4
    if bad:
        raise ValueError(f"{fn}: {want}; got {got}")


def raster_depth(verts, faces, R, T, K, H: int, W: int) -> torch.Tensor:
    """zbuf int64 [F,H,W]: the uint64 keys (float_bits(camera depth) << 32) | face of the nearest face whose screen triangle covers
    each pixel centre (integer coordinates; both windings), -1 where none does.  R [F,3,3], T [F,3], K [3,3] (Dataset.R / T / K).
    zbuf >> 32 (as int32 bits) is the depth as float32; zbuf & 0xffffffff the face."""
    verts = check_verts("raster_depth", verts)
    faces = check_faces("raster_depth", faces)
    if verts.device != faces.device:
        raise ValueError(f"raster_depth: verts on {verts.device}, faces on {faces.device}")
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError(f"raster_depth: empty images {H}x{W}")
    F = R.shape[0] if torch.is_tensor(R) and R.dim() >= 1 else -1
    R, T, K = check_cams("raster_depth", F, R, T, K, verts.device)
    zbuf = torch.full((F, H, W), -1, dtype=torch.int64, device=verts.device)
    with torch.cuda.device(verts.device):
        _lib.check(_lib.lib().dh_mesh_raster_depth(_lib.ptr(verts), verts.shape[0], _lib.ptr(faces), faces.shape[0], _lib.ptr(R),
                                                   _lib.ptr(T), _lib.ptr(K), F, H, W, _lib.ptr(zbuf), _lib.stream()))
    return zbuf


def frame_chunks(fn, verts, faces, R, T, K, H: int, W: int, frame_chunk: int):
    """The frames of the cameras R [F,3,3], T [F,3] in chunks of `frame_chunk`: yields (f0, f1, Rc, Tc, zbuf) with Rc, Tc the chunk's
    contiguous cameras and zbuf = raster_depth(verts, faces, Rc, Tc, K, H, W), which holds frame_chunk * H * W * 8 bytes and is freed
    when the chunk is done.  Every kernel that consumes a chunk works per frame or adds the frames in order, so results are bitwise
    the same for every chunk size."""
    if int(frame_chunk) < 1:
        raise ValueError(f"{fn}: frame_chunk must be >= 1, got {frame_chunk}")
    F = R.shape[0]
    for f0 in range(0, F, int(frame_chunk)):
        f1 = min(F, f0 + int(frame_chunk))
        Rc, Tc = R[f0:f1].contiguous(), T[f0:f1].contiguous()
        zbuf = raster_depth(verts, faces, Rc, Tc, K, H, W)
        yield f0, f1, Rc, Tc, zbuf
        zbuf.untyped_storage().resize_(0)            # the consumer's loop variable still names it: give the memory back now
        del zbuf


def zbuf_depth(zbuf: torch.Tensor) -> torch.Tensor:
    """float32 depth of a raster_depth buffer (inf where empty)."""
    d = (zbuf >> 32).to(torch.int32).view(torch.float32)
    return torch.where(zbuf == -1, torch.full_like(d, float("inf")), d)


def vertex_normals(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """Unit vertex normals float32 [V,3]: the sum of the cross products (b - a) x (c - a) (area-weighted face normals) of the faces
    around each vertex, in fp64, as segment sums over the face corners sorted by vertex (stable sort: a fixed order, no float atomics,
    bitwise reproducible), then normalised; 0 for a vertex in no face.  CPU or device tensors."""
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int64:
        raise ValueError(f"vertex_normals: verts [V,3] and faces int64 [M,3], got {tuple(verts.shape)} and {faces.dtype} "
                         f"{tuple(faces.shape)}")
    v = verts.double()
    nv = v.shape[0]
    fn = torch.linalg.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    corner = faces.reshape(-1)
    order = torch.sort(corner, stable=True).indices
    counts = torch.bincount(corner, minlength=nv)
    per = fn.repeat_interleave(3, dim=0)[order]
    n = torch.segment_reduce(per, "sum", lengths=counts, axis=0, unsafe=True) if nv else per.new_zeros(0, 3)
    norm = n.norm(dim=1, keepdim=True)
    return torch.where(norm > 0, n / norm.clamp(min=1e-300), torch.zeros_like(n)).float()


def usable_map(label: torch.Tensor, erode_px: int) -> torch.Tensor:
    """u8 [F,H,W]: 1 on object pixels (label 1) whose (2 erode_px + 1)^2 window, clipped to the image, holds only object pixels."""
    not_obj = (label != 1).to(torch.int8)
    return 1 - dilate_labels(not_obj, int(erode_px))


def bake_vertex_colors(verts, faces, dataset, erode_px: int = 1, min_cos: float = 0.1, depth_eps: float = 0.01, frame_chunk: int = 16,
                       normals=None):
    """(colors f32 [V,3], weight [V], n_views int32 [V]) from the dataset's frames with its current poses (Dataset.R / T, refined in
    place by pose refinement): colors = sum(c rgb/255) / sum(c) over the contributing frames (module docstring), weight = sum(c); NaN
    colour where no frame contributes.  Frames go in chunks of `frame_chunk` (frame_chunks); the per-vertex sums run over the frames
    in order whatever the chunking, so the result is bitwise the same for every chunk size.
    normals: unit vertex normals (default: vertex_normals(verts, faces))."""
    fn = "bake_vertex_colors"
    verts = check_verts(fn, verts)
    faces = check_faces(fn, faces)
    _check_bake_args(fn, erode_px, min_cos, depth_eps, frame_chunk)
    normals = _normals(fn, verts, faces, normals)
    ds = dataset
    F, H, W = ds.n_images, ds.H, ds.W
    R, T, K = check_cams(fn, F, ds.R, ds.T, ds.K, verts.device)
    rgb = device_tensor(fn, "dataset.rgb", ds.rgb, torch.uint8, lambda s: s == (F, H, W, 3), f"[{F},{H},{W},3]")
    nv = verts.shape[0]
    acc = torch.zeros(nv, 4, dtype=torch.float32, device=verts.device)
    n_views = torch.zeros(nv, dtype=torch.int32, device=verts.device)
    L = _lib.lib()
    with torch.cuda.device(verts.device):
        for f0, f1, Rc, Tc, zbuf in frame_chunks(fn, verts, faces, R, T, K, H, W, frame_chunk):
            usable = usable_map(ds.label[f0:f1].contiguous(), erode_px)
            _lib.check(L.dh_mesh_bake_colors(_lib.ptr(verts), _lib.ptr(normals), nv, _lib.ptr(rgb[f0:f1]), _lib.ptr(usable),
                                             _lib.ptr(zbuf), _lib.ptr(Rc), _lib.ptr(Tc), _lib.ptr(K), f1 - f0, H, W,
                                             float(depth_eps), float(min_cos), _lib.ptr(acc), _lib.ptr(n_views), _lib.stream()))
    w = acc[:, 3]
    colors = torch.where((n_views > 0)[:, None], acc[:, :3] / w[:, None], torch.full_like(acc[:, :3], float("nan")))
    return colors, w, n_views


@torch.no_grad()
def network_vertex_colors(renderer, verts, normals=None):
    """Colour network at every vertex f32 [V,3], viewed along -n: n = normals (unit) if given, else the normalised SDF gradient at the
    vertex: renderer.eval_points, a first pass for the gradient (direction 0), a second for the colour with the direction.  Non-finite
    output (split_f16 range exceeded, or a diverged network) raises DynhorHipError."""
    verts = check_verts("network_vertex_colors", verts)
    if normals is None:
        normals = torch.nn.functional.normalize(renderer.eval_points(verts, torch.zeros_like(verts), "network_vertex_colors")[0], dim=1)
    else:
        normals = device_tensor("network_vertex_colors", "normals", normals, torch.float32, lambda s: s == tuple(verts.shape), "[V,3]")
    return renderer.eval_points(verts, -normals, "network_vertex_colors")[1]


def color_mesh(verts, faces, mode: str, dataset=None, renderer=None, erode_px: int = 1, min_cos: float = 0.1, depth_eps: float = 0.01,
               frame_chunk: int = 16):
    """(colors u8 [V,3] or None for mode "none", stats).  "views": bake_vertex_colors, unseen vertices 0.5 grey; "network":
    network_vertex_colors; "views+network": the views, unseen vertices the network colour.  stats: mode, verts_in, unseen_verts (no
    contributing view), mean_views (mean n_views over the seen vertices; 0.0 when none is seen)."""
    if mode not in MODES:
        raise ValueError(f"color_mesh: mode must be one of {MODES}, got {mode!r}")
    verts = check_verts("color_mesh", verts)
    faces = check_faces("color_mesh", faces)
    stats = {"mode": mode, "verts_in": int(verts.shape[0])}
    if mode == "none":
        return None, stats
    if "views" in mode and dataset is None:
        raise ValueError(f"color_mesh: mode {mode!r} needs the dataset")
    if "network" in mode and renderer is None:
        raise ValueError(f"color_mesh: mode {mode!r} needs the renderer")
    if "views" in mode:
        col, _, n_views = bake_vertex_colors(verts, faces, dataset, erode_px=erode_px, min_cos=min_cos, depth_eps=depth_eps,
                                             frame_chunk=frame_chunk)
        seen = n_views > 0
        n_seen = int(seen.sum())
        stats.update(unseen_verts=int(verts.shape[0] - n_seen),
                     mean_views=float(n_views[seen].double().sum()) / n_seen if n_seen else 0.0)
        if mode == "views+network":
            if n_seen < verts.shape[0]:
                col[~seen] = network_vertex_colors(renderer, verts[~seen].contiguous())
        else:
            col[~seen] = 0.5
    else:
        col = network_vertex_colors(renderer, verts)
        stats.update(unseen_verts=int(verts.shape[0]), mean_views=0.0)
    colors = (col.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8)
    return colors, stats
