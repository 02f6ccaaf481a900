"""A photometric term for the mesh pose refinement (dynhor_amd/pose_sil.py): classical direct alignment of coloured surface points.

A silhouette sees depth only through scale and says nothing about a rotation the outline does not show (a symmetric template, a
sphere).  This term samples coloured points on the mesh once per run and asks that each point, projected into every frame that sees
it, lands on a pixel of its colour (csrc/pose_photo.hip, include/dynhor_hip.h):
  * ``blur_frames`` (dh_image_blur): the frames as float32 [F,H,W,4] = (colour, a), a masked, normalised separable Gaussian over the
    usable pixels (``mesh_color.usable_map``: object pixels, eroded; hand and background never count), a = the usable share under the
    kernel.  A fine texture needs the frames blurred coarse to fine (DESIGN_NEXT_ROWS.md section 19), so the levels are part of the term.
  * ``photo_sums`` (dh_photo_loss_grad): per frame sum om rho, sum om, d/dR (9), d/dT (3), the contributing pairs and the pairs inside
    the Huber band.  A (point, frame) pair contributes when the point passes the bake's view test on the mesh's z-buffer (in front of the
    camera, nearest pixel in the image, not hidden, cos >= min_cos), its four bilinear taps lie in the image and each has a >= a_min;
    rho = sum over the channels of huber(I - c, delta), om = cos (constant in the gradient).  There is no gradient at an occlusion
    boundary: the decisions are fp32 and discrete, the values fp64.
  * ``surface_points``: area-weighted samples (``metrics.sample_surface``) with interpolated unit normals and colours from vertex
    colours or a texture.
  * ``PhotometricTerm``: the points, the blurred active frames of the current level and the settings.  Bound to a
    ``SilhouettePoseOptimizer`` (``photo=``) it evaluates the active frames in the optimiser's chunks and adds lw_photo / n_active *
    rows[2:14] / max(sum om, TINY) to the pose gradient; L_photo = the mean over the active frames of sum om rho / max(sum om, TINY).

Limits: lighting that moves with the hand is absorbed only by the Huber term (no per-frame gain and bias); colours baked from the views
at wrong poses are a blurred but consistent target; the point colours are not blurred at the coarse levels.  ``pose_init`` does not use
the term: its template is category-level and its texture is not the object's.

The kernels run on the current stream; there is no CPU path.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._args import check_cams, check_faces, check_verts, device_tensor
from .mesh_color import _check_bake_args, raster_depth, usable_map, vertex_normals

# defaults of the YAML's pose_photo: block; DESIGN_NEXT_ROWS.md section 19 says where each comes from
DEFAULTS = {"mode": "none", "points": 20000, "levels": (2.0, 1.0, 0.0), "lw_photo": 0.25, "delta": 0.1, "a_min": 0.5, "min_cos": 0.2,
            "depth_eps": 0.01, "erode_px": 1, "seed": 0}
MODES = ("none", "views", "mesh")
MAX_BYTES = 8 << 30
TINY = 1e-12


def gaussian_taps(sigma: float):
    """(taps as a list of 2 r + 1 Python floats that sum to 1 in fp64, r = ceil(3 sigma)); sigma 0: ([1.0], 0)."""
    sigma = float(sigma)
    if not 0.0 <= sigma < float("inf"):
        raise ValueError(f"gaussian_taps: sigma must be a number >= 0, got {sigma}")
    r = int(math.ceil(3.0 * sigma))
    if r == 0:
        return [1.0], 0
    g = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(-r, r + 1)]
    s = math.fsum(g)
    return [x / s for x in g], r


def blur_frames(rgb, usable, sigma: float) -> torch.Tensor:
    """float32 [F,H,W,4]: (colour in 0..1, a) of the frames rgb u8 [F,H,W,3] blurred by a Gaussian of `sigma` pixels (radius
    ceil(3 sigma)) over the pixels with usable u8 [F,H,W] set, normalised by a = the kernel's usable share; all 0 where a == 0.
    sigma 0: (usable ? rgb / 255 : 0, usable)."""
    fn = "blur_frames"
    rgb = device_tensor(fn, "rgb", rgb, torch.uint8, lambda s: len(s) == 4 and s[3] == 3, "[F,H,W,3]")
    F, H, W = rgb.shape[:3]
    usable = device_tensor(fn, "usable", usable, torch.uint8, lambda s: s == (F, H, W), f"[{F},{H},{W}]")
    if usable.device != rgb.device:
        raise ValueError(f"{fn}: rgb on {rgb.device}, usable on {usable.device}")
    if H == 0 or W == 0:
        raise ValueError(f"{fn}: empty images {H}x{W}")
    taps, r = gaussian_taps(sigma)
    out = torch.empty(F, H, W, 4, dtype=torch.float32, device=rgb.device)
    if F == 0:
        return out
    with torch.cuda.device(rgb.device):
        t = torch.tensor(taps, dtype=torch.float64).to(torch.float32).to(rgb.device)
        tmp = torch.empty_like(out)
        _lib.check(_lib.lib().dh_image_blur(_lib.ptr(rgb), _lib.ptr(usable), F, H, W, _lib.ptr(t), r, _lib.ptr(tmp), _lib.ptr(out),
                                            _lib.stream()))
    return out


def photo_sums(pts, normals, colors, img, zbuf, R, T, K, depth_eps: float = DEFAULTS["depth_eps"], min_cos: float = DEFAULTS["min_cos"],
               a_min: float = DEFAULTS["a_min"], delta: float = DEFAULTS["delta"]) -> torch.Tensor:
    """float64 [F,16] on the device, the layout of dh_photo_loss_grad: [0] sum om rho, [1] sum om, [2..10] d[0] / dR row-major,
    [11..13] d[0] / dT, [14] contributing pairs, [15] pairs with every channel inside delta.  img: blur_frames of the F frames; zbuf:
    mesh_color.raster_depth of the mesh the points lie on, at R, T, K.  Nothing is read back."""
    fn = "photo_sums"
    pts = device_tensor(fn, "pts", pts, torch.float32, lambda s: len(s) == 2 and s[1] == 3, "[N,3]")
    n = pts.shape[0]
    normals = device_tensor(fn, "normals", normals, torch.float32, lambda s: s == (n, 3), f"[{n},3]")
    colors = device_tensor(fn, "colors", colors, torch.float32, lambda s: s == (n, 3), f"[{n},3]")
    zbuf = device_tensor(fn, "zbuf", zbuf, torch.int64, lambda s: len(s) == 3, "[F,H,W]")
    F, H, W = zbuf.shape
    if H == 0 or W == 0:
        raise ValueError(f"{fn}: empty images {H}x{W}")
    img = device_tensor(fn, "img", img, torch.float32, lambda s: s == (F, H, W, 4), f"[{F},{H},{W},4]")
    R, T, K = check_cams(fn, F, R, T, K, zbuf.device)
    if any(t.device != zbuf.device for t in (pts, normals, colors, img)):
        raise ValueError(f"{fn}: every tensor must be on {zbuf.device}")
    depth_eps, min_cos, a_min, delta = float(depth_eps), float(min_cos), float(a_min), float(delta)
    if not depth_eps >= 0 or min_cos != min_cos or not a_min >= 0 or not delta > 0:
        raise ValueError(f"{fn}: depth_eps >= 0, min_cos a number, a_min >= 0 and delta > 0; got {depth_eps}, {min_cos}, {a_min}, {delta}")
    L = _lib.lib()
    out = torch.empty(F, int(L.dh_photo_loss_sums()), dtype=torch.float64, device=zbuf.device)
    if F == 0:
        return out
    with torch.cuda.device(zbuf.device):
        ws = torch.empty(max(16, int(L.dh_photo_loss_grad_workspace(F, n))), dtype=torch.uint8, device=zbuf.device)
        _lib.check(L.dh_photo_loss_grad(_lib.ptr(pts), _lib.ptr(normals), _lib.ptr(colors), n, _lib.ptr(img), _lib.ptr(zbuf), _lib.ptr(R),
                                        _lib.ptr(T), _lib.ptr(K), F, H, W, depth_eps, min_cos, a_min, delta, _lib.ptr(out), _lib.ptr(ws),
                                        _lib.stream()))
    return out


def surface_points(verts, faces, n: int, seed: int, vertex_colors=None, uv=None, texture=None):
    """(points f32 [n,3], unit normals f32 [n,3], colours f32 [n,3] in 0..1): area-weighted samples of the mesh
    (metrics.sample_surface, the same seed gives the same samples), the vertex normals (mesh_color.vertex_normals) interpolated and
    normalised, and the colour either interpolated from vertex_colors ([V,3], u8 or float in 0..1) or fetched bilinearly from texture
    (u8 [S,S,3]) at the interpolated uv ([nf,3,2] in texel units, texel centres at + 0.5: mesh_texture's layout).  Plain torch, once per
    run; CPU or device tensors."""
    from .metrics import sample_surface
    if (vertex_colors is None) == (uv is None or texture is None):
        raise ValueError("surface_points: give either vertex_colors or both uv and texture")
    n = int(n)
    if n < 1:
        raise ValueError(f"surface_points: n must be >= 1, got {n}")
    dev = verts.device
    faces = faces.to(dev).long()
    pts, _, fi = sample_surface(verts, faces, n, int(seed), return_faces=True)
    tri = verts.double()[faces[fi]]
    # barycentric weights of the samples in their faces, recovered from the points (sample_surface does not return them)
    e0, e1, d = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], pts.double() - tri[:, 0]
    a00, a01, a11 = (e0 * e0).sum(1), (e0 * e1).sum(1), (e1 * e1).sum(1)
    b0, b1 = (d * e0).sum(1), (d * e1).sum(1)
    det = (a00 * a11 - a01 * a01).clamp(min=1e-300)
    w1, w2 = (a11 * b0 - a01 * b1) / det, (a00 * b1 - a01 * b0) / det
    w = torch.stack([1.0 - w1 - w2, w1, w2], 1).clamp(0.0, 1.0)
    w = w / w.sum(1, keepdim=True)
    vn = vertex_normals(verts, faces).double()
    nrm = torch.nn.functional.normalize((w[:, :, None] * vn[faces[fi]]).sum(1), dim=1)
    if vertex_colors is not None:
        vc = vertex_colors.to(dev)
        vc = vc.double() / 255.0 if vc.dtype == torch.uint8 else vc.double()
        if tuple(vc.shape) != (verts.shape[0], 3):
            raise ValueError(f"surface_points: vertex_colors must be [{verts.shape[0]},3], got {tuple(vc.shape)}")
        col = (w[:, :, None] * vc[faces[fi]]).sum(1)
    else:
        tex = texture.to(dev).double() / 255.0
        Sh, Sw = tex.shape[0], tex.shape[1]
        st = (w[:, :, None] * uv.to(dev).double()[fi]).sum(1) - 0.5
        i0, j0 = torch.floor(st[:, 0]), torch.floor(st[:, 1])
        fx, fy = (st[:, 0] - i0)[:, None], (st[:, 1] - j0)[:, None]
        ia, ib = i0.clamp(0, Sw - 1).long(), (i0 + 1).clamp(0, Sw - 1).long()
        ja, jb = j0.clamp(0, Sh - 1).long(), (j0 + 1).clamp(0, Sh - 1).long()
        col = (tex[ja, ia] * (1 - fx) + tex[ja, ib] * fx) * (1 - fy) + (tex[jb, ia] * (1 - fx) + tex[jb, ib] * fx) * fy
    return pts, nrm.float().contiguous(), col.clamp(0.0, 1.0).float().contiguous()


def level_at(k: int, iters: int, levels) -> float:
    """The blur sigma of iteration k of `iters`: levels[floor(k len(levels) / iters)]."""
    return float(levels[min(len(levels) - 1, (int(k) * len(levels)) // max(1, int(iters)))])


class PhotometricTerm:
    """The coloured points (pts, normals, colors f32 [N,3] on the device), the frames (rgb u8 [F,H,W,3], usable u8 [F,H,W]) and the
    settings.  set_frames(active_idx) picks the frames the optimiser moves; set_level(sigma) blurs them (16 bytes per pixel and
    frame: an error that names --pose_frames when that exceeds max_bytes).  bind(opt, weight) attaches the term to a
    SilhouettePoseOptimizer, which then calls sums / add_grads / stats; settings() is the term's share of refine_poses' result."""

    def __init__(self, pts, normals, colors, rgb, usable, levels=DEFAULTS["levels"], delta=DEFAULTS["delta"], a_min=DEFAULTS["a_min"],
                 min_cos=DEFAULTS["min_cos"], depth_eps=DEFAULTS["depth_eps"], max_bytes=MAX_BYTES):
        fn = "PhotometricTerm"
        self.pts = device_tensor(fn, "pts", pts, torch.float32, lambda s: len(s) == 2 and s[1] == 3 and s[0] > 0, "[N,3], N > 0")
        n = self.pts.shape[0]
        self.normals = device_tensor(fn, "normals", normals, torch.float32, lambda s: s == (n, 3), f"[{n},3]")
        self.colors = device_tensor(fn, "colors", colors, torch.float32, lambda s: s == (n, 3), f"[{n},3]")
        self.rgb = device_tensor(fn, "rgb", rgb, torch.uint8, lambda s: len(s) == 4 and s[3] == 3, "[F,H,W,3]")
        F, H, W = self.rgb.shape[:3]
        self.usable = device_tensor(fn, "usable", usable, torch.uint8, lambda s: s == (F, H, W), f"[{F},{H},{W}]")
        self.levels = tuple(float(s) for s in levels)
        if not self.levels or any(not 0.0 <= s <= 21.0 for s in self.levels):
            raise ValueError(f"{fn}: levels must be a non-empty list of blur sigmas in [0, 21] pixels, got {levels}")
        _check_bake_args(fn, 0, min_cos, depth_eps, 1)
        if not float(delta) > 0 or not float(a_min) >= 0:
            raise ValueError(f"{fn}: delta > 0 and a_min >= 0, got {delta}, {a_min}")
        self.delta, self.a_min, self.min_cos, self.depth_eps = float(delta), float(a_min), float(min_cos), float(depth_eps)
        self.max_bytes = int(max_bytes)
        self.set_frames(None)

    def set_frames(self, active_idx):
        """The frames (int64 indices on the device, None = all) that sums() addresses as 0..n_active-1."""
        if active_idx is None:
            self._rgb, self._usable = self.rgb, self.usable
        else:
            self._rgb, self._usable = self.rgb[active_idx].contiguous(), self.usable[active_idx].contiguous()
        n, H, W = self._usable.shape
        need = n * H * W * 16
        if need > self.max_bytes:
            raise ValueError(f"PhotometricTerm: the blurred frames of {n} frames of {H}x{W} take {need} bytes, more than max_bytes = "
                             f"{self.max_bytes}; refine fewer frames at a time (--pose_frames) or raise max_bytes")
        self.sigma, self.img = None, None

    def set_level(self, sigma: float):
        sigma = float(sigma)
        if self.img is None or sigma != self.sigma:
            self.img = None
            self.img = blur_frames(self._rgb, self._usable, sigma)
            self.sigma = sigma

    def bind(self, opt, weight: float):
        """Attach the term at weight `weight` to the optimiser `opt`: its active frames and its frame_chunk."""
        if tuple(self.rgb.shape[:3]) != (opt.F, opt.H, opt.W) or self.rgb.device != opt.device:
            raise ValueError(f"SilhouettePoseOptimizer: photo holds frames {tuple(self.rgb.shape[:3])} on {self.rgb.device}, the labels "
                             f"are {(opt.F, opt.H, opt.W)} on {opt.device}")
        self.weight = float(weight)
        self.frame_chunk, self.active_idx = opt.frame_chunk, opt.active_idx
        self.set_frames(opt.active_idx if len(opt.active_list) != opt.F else None)

    def sums(self, verts, faces, R, T, K) -> torch.Tensor:
        """photo_sums of the active frames, float64 [n_active,16], at the poses R f32 [F,3,3], T f32 [F,3] of all frames: each chunk of
        frame_chunk frames on the z-buffer of the mesh (verts, faces) at its poses."""
        if self.img is None:
            self.set_level(self.levels[0])
        R, T = R[self.active_idx], T[self.active_idx]
        n, H, W = self._usable.shape
        out = []
        for f0 in range(0, n, self.frame_chunk):
            f1 = min(n, f0 + self.frame_chunk)
            Rc, Tc = R[f0:f1].contiguous(), T[f0:f1].contiguous()
            zbuf = raster_depth(verts, faces, Rc, Tc, K, H, W)
            out.append(photo_sums(self.pts, self.normals, self.colors, self.img[f0:f1], zbuf, Rc, Tc, K, self.depth_eps, self.min_cos,
                                  self.a_min, self.delta))
        return torch.cat(out)

    def add_grads(self, rows, gR, gT):
        """gR [F,3,3], gT [F,3] (float64) += weight / n_active * rows[2:14] / max(sum om, TINY) at the active frames.  No host read."""
        n = rows.shape[0]
        scale = (self.weight / n) / rows[:, 1].clamp(min=TINY)
        gR[self.active_idx] += rows[:, 2:11].reshape(n, 3, 3) * scale[:, None, None]
        gT[self.active_idx] += rows[:, 11:14] * scale[:, None]

    def stats(self, rows):
        """(L_photo, the stats' extra keys) of the rows of sums() on the CPU."""
        loss = float((rows[:, 0] / rows[:, 1].clamp(min=TINY)).mean())
        return loss, {"loss_photo": loss, "photo_pairs": [int(x) for x in rows[:, 14].round().tolist()],
                      "photo_inliers": float(rows[:, 15].sum() / rows[:, 14].sum().clamp(min=1.0))}

    def settings(self) -> dict:
        return {"points": int(self.pts.shape[0]), "levels": list(self.levels), "lw_photo": self.weight, "delta": self.delta,
                "a_min": self.a_min, "min_cos": self.min_cos, "depth_eps": self.depth_eps}


def make_term(verts, faces, dataset, n_points=DEFAULTS["points"], seed=DEFAULTS["seed"], vertex_colors=None, uv=None, texture=None,
              erode_px=DEFAULTS["erode_px"], **settings) -> PhotometricTerm:
    """A PhotometricTerm of `n_points` samples of the mesh, coloured from vertex_colors or (uv, texture), over the dataset's frames
    with their usable maps (object pixels eroded by erode_px)."""
    verts = check_verts("make_term", verts)
    faces = check_faces("make_term", faces)
    pts, nrm, col = surface_points(verts, faces, n_points, seed, vertex_colors=vertex_colors, uv=uv, texture=texture)
    usable = usable_map(dataset.label, int(erode_px))
    return PhotometricTerm(pts, nrm, col, dataset.rgb, usable, **settings)
