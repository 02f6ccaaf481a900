"""A texture atlas for an extracted (and simplified) mesh, baked from the training frames, and the textured Wavefront OBJ the
reference's stage 1 consumes (``obj_path``: X.obj + X.obj.mtl + X_texture_kd.<ext>).

  * ``face_atlas``: one right-angled UV triangle per face, two faces per square cell of an S x S image (layout below).  Plain torch,
    CPU or device.  Every face gets the same number of texels whatever its area, so a mesh with very uneven faces wastes texels on
    the small ones; chart-based or area-proportional packing is out of scope.
  * ``bake_texture``: per texel, the weighted mean of the frames that see its surface point (csrc/mesh_texture.hip,
    dh_texture_bake): the visibility rule of ``mesh_color.bake_vertex_colors`` (usable label eroded by ``erode_px``, z-buffer depth
    test with ``depth_eps``, cos >= ``min_cos``) at the point and normal interpolated to the texel centre, the colour fetched
    bilinearly, the weight cos^(2^sharpen) (sharpen 2 = cos^4: grazing views do not blur the texture).  Modes "views" (unseen owned
    texels 0.5 grey) and "views+network" (unseen owned texels take ``mesh_color.network_vertex_colors`` at the texel's point and
    normal).  Texels no face owns stay black.
  * ``render_textured``: the mesh drawn with its texture from a ``mesh_color.raster_depth`` z-buffer (dh_mesh_shade_tex), optionally
    lit by dh_mesh_shade's headlight and composited over the frames, with the squared error against the frames summed per frame.
  * ``texture_psnr``: re-render PSNR of the textured mesh against the dataset's frames, per frame and pooled.
  * ``write_textured_obj`` / ``load_textured_obj``: the reference asset's layout, and Meshlab's dialect on the way in.

Atlas layout.  g = ceil(sqrt(ceil(nf / 2))) cells per side, c = size // g texels per cell (c >= MIN_CELL = 8); face k lies in cell
k // 2 (row-major: column (k // 2) % g, row (k // 2) // g) and is its half k & 1.  With (i, j) the texel's column and row inside the
cell, half 0 owns the texels with i + j <= c - 1 (the anti-diagonal included), half 1 those with i + j >= c.  Texel (i, j) has its
centre at (i + 0.5, j + 0.5); the UV corners, in the face's vertex order, relative to the cell's corner:
    half 0:  (1, 1)          (c - 3, 1)      (1, c - 3)
    half 1:  (c - 1, c - 1)  (4, c - 1)      (c - 1, 4)
A bilinear fetch at (s, t) taps the columns i0 = floor(s - 0.5) and i0 + 1 and the rows j0 = floor(t - 0.5) and j0 + 1, and
floor(s + t - 1) - 1 <= i0 + j0 <= floor(s + t - 1).  In half 0, s, t >= 1 keeps the taps at >= 0 and s + t <= c - 2 keeps the far tap
at (i0 + 1) + (j0 + 1) <= c - 1; in half 1, s, t <= c - 1 keeps the taps at <= c - 1 and s + t >= c + 3 keeps the near tap at
i0 + j0 >= c + 1.  Every tap of
every point of a UV triangle -- and of every point within half a texel of it, which absorbs the fp32 rounding of an interpolated
(s, t) -- is therefore a texel of the same face: faces never bleed into each other and no dilation pass is needed.  Both triangles have
positive signed area (c - 4)^2 / 2 and (c - 5)^2 / 2.  MIN_CELL = 8 leaves legs of 4 and 3 texels.

The kernels run on the current stream; baking and rendering have no CPU path.
"""
from __future__ import annotations

import ctypes
import math
import os

import torch

from . import _lib
from ._args import check_cams, check_faces, check_verts, device_tensor, same_device
from .mesh_color import _check_bake_args, _draw_args, _normals, frame_chunks, network_vertex_colors, usable_map, vertex_normals

MODES = ("none", "views", "views+network")
MIN_CELL = 8
IMAGES = ("png", "jpg")


def atlas_capacity(size: int) -> int:
    """The largest face count face_atlas lays out on a size x size image."""
    g = int(size) // MIN_CELL
    return 2 * g * g


def atlas_min_size(n_faces: int) -> int:
    """The smallest size face_atlas accepts for n_faces faces."""
    return MIN_CELL * math.isqrt(max((int(n_faces) + 1) // 2, 1) - 1) + MIN_CELL if n_faces > 0 else MIN_CELL


def face_atlas(n_faces: int, size: int, device=None):
    """(uv f32 [nf,3,2] in continuous texel units, owner int32 [size,size]: the face of every texel or -1, info) for the layout of
    the module docstring; a function of (n_faces, size) alone.  info: size, cells_per_side g, cell c, faces, owned_texels,
    owned_frac.  ValueError when the cells would be smaller than MIN_CELL texels."""
    nf, size = int(n_faces), int(size)
    if nf < 1 or size < 1:
        raise ValueError(f"face_atlas: n_faces and size must be >= 1, got {n_faces} and {size}")
    g = math.isqrt((nf + 1) // 2 - 1) + 1                            # ceil(sqrt(ceil(nf / 2)))
    c = size // g
    if c < MIN_CELL:
        raise ValueError(f"face_atlas: a {size} x {size} texture holds at most {atlas_capacity(size)} faces ({MIN_CELL} texels per "
                         f"cell edge), the mesh has {nf}: simplify it further (--mesh_simplify faces:T) or raise --texture_size "
                         f"(at least {atlas_min_size(nf)})")
    k = torch.arange(nf, device=device, dtype=torch.int64)
    cell, half = k // 2, k & 1
    ox, oy = ((cell % g) * c).double(), ((cell // g) * c).double()
    lo = torch.tensor([[1.0, 1.0], [c - 3.0, 1.0], [1.0, c - 3.0]], dtype=torch.float64, device=device)
    hi = torch.tensor([[c - 1.0, c - 1.0], [4.0, c - 1.0], [c - 1.0, 4.0]], dtype=torch.float64, device=device)
    uv = torch.where((half == 0)[:, None, None], lo[None], hi[None]) + torch.stack([ox, oy], -1)[:, None, :]
    ax = torch.arange(size, device=device, dtype=torch.int64)
    cx, i = ax // c, ax % c
    in_cell = (cx < g)
    cellmap = cx[:, None] * g + cx[None, :]                          # [row, column]: (row // c) * g + column // c
    face = 2 * cellmap + ((i[:, None] + i[None, :]) >= c).long()
    ok = in_cell[:, None] & in_cell[None, :] & (face < nf)
    owner = torch.where(ok, face, torch.full_like(face, -1)).to(torch.int32)
    owned = int(ok.sum())
    info = {"size": size, "cells_per_side": g, "cell": c, "faces": nf, "owned_texels": owned, "owned_frac": owned / float(size * size)}
    return uv.float().contiguous(), owner.contiguous(), info


def _uv(fn, uv, nf, device):
    uv = device_tensor(fn, "uv", uv, torch.float32, lambda s: s == (nf, 3, 2), f"[{nf},3,2]")
    same_device(fn, device, uv)
    return uv


def bake_texture_sums(verts, faces, dataset, uv, owner, erode_px: int = 1, min_cos: float = 0.1, depth_eps: float = 0.01,
                      sharpen: int = 2, frame_chunk: int = 16, normals=None):
    """(acc f32 [S,S,4], n_views int32 [S,S]) of dh_texture_bake over the dataset's frames with its current poses: acc = (sum of weight
    colour, sum of weight) over the contributing frames, in frame order whatever the chunking (bitwise the same for every
    frame_chunk).  Texels no face owns keep 0."""
    fn = "bake_texture_sums"
    verts = check_verts(fn, verts)
    faces = check_faces(fn, faces)
    _check_bake_args(fn, erode_px, min_cos, depth_eps, frame_chunk, sharpen)
    nf, nv, dev = faces.shape[0], verts.shape[0], verts.device
    uv = _uv(fn, uv, nf, dev)
    owner = device_tensor(fn, "owner", owner, torch.int32, lambda s: len(s) == 2 and s[0] == s[1], "[S,S]")
    normals = _normals(fn, verts, faces, normals)
    ds = dataset
    F, H, W = ds.n_images, ds.H, ds.W
    R, T, K = check_cams(fn, F, ds.R, ds.T, ds.K, dev)
    rgb = device_tensor(fn, "dataset.rgb", ds.rgb, torch.uint8, lambda s: s == (F, H, W, 3), f"[{F},{H},{W},3]")
    same_device(fn, dev, faces, owner, normals, rgb)
    S = owner.shape[0]
    acc = torch.zeros(S, S, 4, dtype=torch.float32, device=dev)
    n_views = torch.zeros(S, S, dtype=torch.int32, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        for f0, f1, Rc, Tc, zbuf in frame_chunks(fn, verts, faces, R, T, K, H, W, frame_chunk):
            usable = usable_map(ds.label[f0:f1].contiguous(), erode_px)
            _lib.check(L.dh_texture_bake(_lib.ptr(verts), _lib.ptr(normals), nv, _lib.ptr(faces), nf, _lib.ptr(uv), _lib.ptr(owner), S,
                                         _lib.ptr(rgb[f0:f1]), _lib.ptr(usable), _lib.ptr(zbuf), _lib.ptr(Rc), _lib.ptr(Tc), _lib.ptr(K),
                                         f1 - f0, H, W, float(depth_eps), float(min_cos), int(sharpen), _lib.ptr(acc),
                                         _lib.ptr(n_views), _lib.stream()))
    return acc, n_views


def texel_points(verts, normals, faces, uv, owner, index):
    """(points f32 [n,3], unit normals f32 [n,3]) of the texels `index` (flat indices into owner, all owned): the surface point and
    normal dh_texture_bake gives the texel centre (barycentrics in the UV triangle, negatives clamped to 0, renormalised)."""
    S = owner.shape[1]
    face = owner.reshape(-1)[index].long()
    q = torch.stack([(index % S).float() + 0.5, (index // S).float() + 0.5], -1)
    t = uv[face]

    def edge(a, b, p):
        return (b[:, 0] - a[:, 0]) * (p[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (p[:, 0] - a[:, 0])

    area = edge(t[:, 0], t[:, 1], t[:, 2])
    b = torch.stack([edge(t[:, 1], t[:, 2], q), edge(t[:, 2], t[:, 0], q), edge(t[:, 0], t[:, 1], q)], -1) / area[:, None]
    b = b.clamp(min=0.0)
    b = b / b.sum(-1, keepdim=True)
    tri = faces[face]
    p = (b[:, :, None] * verts[tri]).sum(1)
    n = torch.nn.functional.normalize((b[:, :, None] * normals[tri]).sum(1), dim=1)
    return p.contiguous(), n.contiguous()


def bake_texture(verts, faces, dataset, size: int = 1024, mode: str = "views", renderer=None, erode_px: int = 1, min_cos: float = 0.1,
                 depth_eps: float = 0.01, sharpen: int = 2, frame_chunk: int = 16):
    """(tex u8 [S,S,3], uv f32 [nf,3,2], owner int32 [S,S], stats) for mode "views" | "views+network"; mode "none" gives (None, None,
    None, stats).  tex = round(255 clamp(acc.rgb / acc.w)) where a view contributes; an owned texel no view sees is 0.5 grey
    ("views") or the colour network at its point, seen along its normal ("views+network"); a texel no face owns is 0.  stats: mode,
    size, faces, cell, owned_texels, owned_frac, unseen_texels (owned, no contributing view), mean_views (over the seen texels)."""
    if mode not in MODES:
        raise ValueError(f"bake_texture: mode must be one of {MODES}, got {mode!r}")
    stats = {"mode": mode}
    if mode == "none":
        return None, None, None, stats
    verts = check_verts("bake_texture", verts)
    faces = check_faces("bake_texture", faces)
    if dataset is None:
        raise ValueError(f"bake_texture: mode {mode!r} needs the dataset")
    if "network" in mode and renderer is None:
        raise ValueError(f"bake_texture: mode {mode!r} needs the renderer")
    if faces.shape[0] == 0:
        raise ValueError("bake_texture: the mesh has no faces")
    uv, owner, info = face_atlas(faces.shape[0], size, device=verts.device)
    normals = vertex_normals(verts, faces)
    acc, n_views = bake_texture_sums(verts, faces, dataset, uv, owner, erode_px=erode_px, min_cos=min_cos, depth_eps=depth_eps,
                                     sharpen=sharpen, frame_chunk=frame_chunk, normals=normals)
    owned, seen = owner >= 0, n_views > 0
    col = torch.where(seen[..., None], acc[..., :3] / acc[..., 3:], torch.zeros_like(acc[..., :3]))
    unseen = owned & ~seen
    n_unseen, n_seen = int(unseen.sum()), int(seen.sum())
    if n_unseen:
        if mode == "views+network":
            index = unseen.reshape(-1).nonzero().squeeze(1)
            pts, nrm = texel_points(verts, normals, faces, uv, owner, index)
            col.view(-1, 3)[index] = network_vertex_colors(renderer, pts, normals=nrm)
        else:
            col[unseen] = 0.5
    tex = (col.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8)
    stats.update(size=info["size"], faces=info["faces"], cell=info["cell"], owned_texels=info["owned_texels"],
                 owned_frac=info["owned_frac"], unseen_texels=n_unseen,
                 mean_views=float(n_views[seen].double().sum()) / n_seen if n_seen else 0.0)
    return tex.contiguous(), uv, owner, stats


def render_textured(verts, faces, zbuf, R, T, K, uv, tex, normals=None, rgb=None, usable=None, alpha: float = 1.0, lit: bool = False):
    """(out u8 [F,H,W,3], sums int64 [F,2] or None): the z-buffer's faces (raster_depth of the same mesh and cameras) drawn with the
    texture tex u8 [Sh,Sw,3] at the coordinates uv f32 [nf,3,2] (texel units), unlit (the texel colour alone) or with mesh_vis.shade's
    headlight, composited over rgb u8 [F,H,W,3] (white without) with alpha.  usable u8 [F,H,W] (needs rgb): sums[f] = (sum over the
    covered usable pixels and the three channels of (out - rgb)^2, their number)."""
    fn = "render_textured"
    verts, faces, zbuf, R, T, K, alpha, normals, rgb = _draw_args(fn, verts, faces, zbuf, R, T, K, alpha, normals, rgb)
    F, H, W = zbuf.shape
    dev = zbuf.device
    uv = _uv(fn, uv, faces.shape[0], dev)
    tex = device_tensor(fn, "tex", tex, torch.uint8, lambda s: len(s) == 3 and s[2] == 3 and s[0] > 0 and s[1] > 0, "[Sh,Sw,3]")
    if usable is not None:
        if rgb is None:
            raise ValueError(f"{fn}: usable needs rgb (the error sums are taken against it)")
        usable = device_tensor(fn, "usable", usable, torch.uint8, lambda s: s == (F, H, W), f"[{F},{H},{W}]")
    same_device(fn, dev, tex, usable)
    out = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    sums = torch.zeros(F, 2, dtype=torch.int64, device=dev) if usable is not None else None
    opt = lambda t: _lib.ptr(t) if t is not None else ctypes.c_void_p(0)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dh_mesh_shade_tex(_lib.ptr(verts), _lib.ptr(normals), verts.shape[0], _lib.ptr(faces), faces.shape[0],
                                                _lib.ptr(uv), _lib.ptr(tex), tex.shape[0], tex.shape[1], _lib.ptr(zbuf), _lib.ptr(R),
                                                _lib.ptr(T), _lib.ptr(K), F, H, W, opt(rgb), opt(usable), alpha, int(bool(lit)),
                                                _lib.ptr(out), opt(sums), _lib.stream()))
    return out, sums


def psnr_from_sums(sse, count):
    """10 log10(255^2 * 3 count / sse): None without pixels, inf for an exact match."""
    sse, count = int(sse), int(count)
    if count == 0:
        return None
    return float("inf") if sse == 0 else 10.0 * math.log10(255.0 ** 2 * 3.0 * count / sse)


def texture_psnr(verts, faces, dataset, uv, tex, erode_px: int = 1, frame_chunk: int = 16) -> dict:
    """Re-render PSNR of the textured mesh, unlit, against the dataset's frames at its current poses, over the pixels the mesh covers
    whose label is usable (object, eroded by erode_px): {"frames": [psnr or None per frame], "pooled", "sse", "count"}."""
    fn = "texture_psnr"
    verts = check_verts(fn, verts)
    faces = check_faces(fn, faces)
    if int(erode_px) < 0:
        raise ValueError(f"{fn}: erode_px must be >= 0, got {erode_px}")
    ds = dataset
    F, H, W = ds.n_images, ds.H, ds.W
    R, T, K = check_cams(fn, F, ds.R, ds.T, ds.K, verts.device)
    normals = vertex_normals(verts, faces)
    sums = torch.zeros(F, 2, dtype=torch.int64, device=verts.device)
    for f0, f1, Rc, Tc, zbuf in frame_chunks(fn, verts, faces, R, T, K, H, W, frame_chunk):
        usable = usable_map(ds.label[f0:f1].contiguous(), erode_px)
        sums[f0:f1] = render_textured(verts, faces, zbuf, Rc, Tc, K, uv, tex, normals=normals, rgb=ds.rgb[f0:f1].contiguous(),
                                      usable=usable)[1]
    rows = sums.tolist()
    sse, count = sum(r[0] for r in rows), sum(r[1] for r in rows)
    return {"frames": [psnr_from_sums(*r) for r in rows], "pooled": psnr_from_sums(sse, count), "sse": sse, "count": count}


# ------------------------------------------------------------------------------------------------ files
def textured_obj_paths(path: str):
    """(X.obj, X.obj.mtl, X_texture_kd) for `path` = X.obj: the three files of the asset, the image without its extension."""
    if not str(path).lower().endswith(".obj"):
        raise ValueError(f"textured OBJ: the path must end in .obj, got {path!r}")
    stem = str(path)[:-4]
    return str(path), str(path) + ".mtl", stem + "_texture_kd"


def write_textured_obj(path, verts, faces, uv, tex, image: str = "png"):
    """X.obj (`path`), X.obj.mtl and X_texture_kd.<image> in the layout of the reference's asset: `mtllib ./X.obj.mtl`, the `v` lines,
    `usemtl material_0`, then per face its three `vt` lines and `f a/ta b/tb c/tc`.  vt = (s / Sw, 1 - t / Sh) for uv = (s, t) in
    texel units: image row 0 is the top of the texture, v = 1.  image "png" (lossless) or "jpg" (quality 95).  Returns the three paths."""
    from PIL import Image
    if image not in IMAGES:
        raise ValueError(f"write_textured_obj: image must be one of {IMAGES}, got {image!r}")
    obj, mtl, img = textured_obj_paths(path)
    img = img + "." + image
    v = verts.detach().cpu().double()
    f = faces.detach().cpu().long()
    t = uv.detach().cpu().double()
    px = tex.detach().cpu()
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or tuple(t.shape) != (f.shape[0], 3, 2) or \
            px.dtype != torch.uint8 or px.dim() != 3 or px.shape[2] != 3:
        raise ValueError(f"write_textured_obj: verts [V,3], faces [M,3], uv [M,3,2], tex u8 [Sh,Sw,3]; got {tuple(verts.shape)}, "
                         f"{tuple(faces.shape)}, {tuple(uv.shape)}, {tex.dtype} {tuple(tex.shape)}")
    Sh, Sw = px.shape[0], px.shape[1]
    name = os.path.basename(obj)
    lines = ["####", "#", f"# Object {name}", "#", f"# Vertices: {v.shape[0]}", f"# Faces: {f.shape[0]}", "#", "####",
             f"mtllib ./{os.path.basename(mtl)}"]
    lines += ["v %.9g %.9g %.9g" % tuple(r) for r in v.tolist()]
    lines += [f"# {v.shape[0]} vertices, 0 vertices normals", "", "usemtl material_0"]
    vt = torch.stack([t[..., 0] / Sw, 1.0 - t[..., 1] / Sh], -1).tolist()
    for k, (tri, corners) in enumerate(zip(f.tolist(), vt)):
        lines += ["vt %.10f %.10f" % tuple(cr) for cr in corners]
        lines.append("f %d/%d %d/%d %d/%d" % (tri[0] + 1, 3 * k + 1, tri[1] + 1, 3 * k + 2, tri[2] + 1, 3 * k + 3))
    lines += [f"# {f.shape[0]} faces, {3 * f.shape[0]} coords texture", "", "# End of File", ""]
    with open(obj, "w") as fh:
        fh.write("\n".join(lines))
    with open(mtl, "w") as fh:
        fh.write("#\n# Wavefront material file\n#\n\nnewmtl material_0\nKa 0.200000 0.200000 0.200000\nKd 1.000000 1.000000 1.000000\n"
                 "Ks 1.000000 1.000000 1.000000\nTr 0.000000\nillum 2\nNs 0.000000\nmap_Kd %s\n\n" % os.path.basename(img))
    Image.fromarray(px.numpy()).save(img, **({"quality": 95} if image == "jpg" else {}))
    return obj, mtl, img


def load_textured_obj(path):
    """(verts f32 [V,3], faces int64 [M,3], uv f32 [M,3,2] in texel units or None, tex u8 [Sh,Sw,3] or None), CPU tensors, from a
    Wavefront OBJ: `v`, `vt`, `vn` in any order and interleaved with the faces; corners `a`, `a/t`, `a//n`, `a/t/n`, negative =
    relative to the elements read so far; polygons fan-triangulated together with their `vt`.  The texture is the first `map_Kd` of
    the `mtllib` file, both resolved relative to the file that names them; uv = (u Sw, (1 - v) Sh).  Without `vt` on any corner, or
    without a texture image, uv and tex are None; `vt` on some corners only is a ValueError."""
    from .metrics import _check_indices
    verts, vts, tris, tts, mtllib = [], [], [], [], None
    with open(path, "r") as fh:
        for line in fh:
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(x) for x in tok[1:4]])
            elif tok[0] == "vt":
                vts.append([float(tok[1]), float(tok[2]) if len(tok) > 2 else 0.0])
            elif tok[0] == "mtllib" and mtllib is None:
                mtllib = line.split("#", 1)[0].split(None, 1)[1].strip()
            elif tok[0] == "f":
                pv, pt = [], []
                for c in tok[1:]:
                    part = c.split("/")
                    i = int(part[0])
                    pv.append(i - 1 if i > 0 else len(verts) + i)
                    if len(part) > 1 and part[1]:
                        j = int(part[1])
                        pt.append(j - 1 if j > 0 else len(vts) + j)
                    else:
                        pt.append(None)
                for k in range(1, len(pv) - 1):
                    tris.append((pv[0], pv[k], pv[k + 1]))
                    tts.append((pt[0], pt[k], pt[k + 1]))
    v = torch.tensor(verts, dtype=torch.float32).reshape(-1, 3)
    f = torch.tensor(tris, dtype=torch.int64).reshape(-1, 3)
    _check_indices(f, v.shape[0], path)
    flat = [j for tri in tts for j in tri]
    if not flat or all(j is None for j in flat):
        return v, f, None, None
    if any(j is None for j in flat):
        raise ValueError(f"load_textured_obj: {path}: some face corners have a vt index and others have none")
    ti = torch.tensor(tts, dtype=torch.int64).reshape(-1, 3)
    if int(ti.min()) < 0 or int(ti.max()) >= len(vts):
        raise ValueError(f"load_textured_obj: {path}: a vt index lies outside the {len(vts)} vt lines")
    image = None
    if mtllib is not None:
        mtl = os.path.join(os.path.dirname(os.path.abspath(path)), mtllib)
        if os.path.exists(mtl):
            with open(mtl, "r") as fh:
                for line in fh:
                    tok = line.split("#", 1)[0].split(None, 1)
                    if len(tok) == 2 and tok[0] == "map_Kd":
                        image = os.path.join(os.path.dirname(mtl), tok[1].strip().split()[-1])
                        break
    if image is None or not os.path.exists(image):
        return v, f, None, None
    import numpy as np
    from PIL import Image
    tex = torch.from_numpy(np.array(Image.open(image).convert("RGB"), dtype=np.uint8))
    Sh, Sw = tex.shape[0], tex.shape[1]
    t = torch.tensor(vts, dtype=torch.float64)[ti]
    uv = torch.stack([t[..., 0] * Sw, (1.0 - t[..., 1]) * Sh], -1).float().contiguous()
    return v, f, uv, tex
