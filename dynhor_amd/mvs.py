"""Multi-view stereo: per-frame depth maps, normal maps in the ``monocular_normal/`` encoding and a fused oriented point cloud from the
frames' texture, by a mesh-guided plane sweep (csrc/mvs.hip, include/dynhor_hip.h).  The classical stand-in for the reference's learned
normal model (StableNormal), as silhouette retrieval stands in for DINOv2 in ``pose_init`` and block matching for DKM in ``match``.

  * ``sweep`` (dh_mvs_sweep): per pixel (fi, px, py) with a guide (z0, n): D depth hypotheses z_k = z0 + (k - (D-1)/2) step along the
    pixel's ray; for each, the plane through z_k e with the guide's normal induces a homography into every neighbour frame, through which
    the (2P+1)^2 patch is fetched bilinearly from ``match.gray_frames``' grey bytes and scored by ZNCC in fp32; c_k = the mean over the
    valid neighbours; the best k, the second peak beyond |k - k*| > 1, a parabola step, flags (1 source patch unusable, 2 no valid
    hypothesis, 4 best on the sweep's border, 8 guide unusable).
  * ``check`` (dh_mvs_check): per pixel with a depth, the number of neighbour frames whose own depth map agrees at the pixel's projection.
  * ``guide_from_mesh``: z0 and the camera-frame face normal per pixel from ``mesh_color.raster_depth`` of any guide mesh.
  * ``depth_maps``: grey frames, guide, a wide pass (``range`` over D = 33), a fine pass about its result (a quarter of the step,
    D = 9, the same normal), the gates (flags, ``score_min``, ``peak_margin`` on the wide pass; flags on the fine pass), then ``check``
    with ``min_consistent``.
  * ``normals_from_depth`` (torch): central differences of the back-projected kept neighbours; ``fuse``: the kept pixels as an oriented
    coloured point cloud in the object frame, optionally one point per voxel.

Every default is a first setting, not tuned.  Limits: one plane per pixel, with the guide's normal (a facet on a coarse mesh); a surface
further than ``range`` from the guide is lost (flag 4 counts it); textureless areas score nothing and a highlight that moves with the hand
matches itself; the normals are finite differences of a noisy depth map.  DESIGN_NEXT_ROWS.md section 25 has the rule and the numbers.

The kernels run on the current stream; there is no CPU path.
"""
from __future__ import annotations

import time

import torch

from . import _lib
from .match import default_min_va, gray_frames, usable_sources
from ._args import check_cams, check_faces, check_verts, device_tensor, lap
from .mesh_color import raster_depth, usable_map
from .settings import merge

# defaults of the YAML's mvs: block -- first settings, none of them tuned.  min_va None: match's 4 N^2; min_vb None: float(min_va)
DEFAULTS = {"offsets": (1, 2), "sigma": 1.0, "a_min": 0.5, "erode_px": 1, "patch": 4, "range": 0.04, "depths": 33, "fine_depths": 9,
            "step_px": 1, "min_va": None, "min_vb": None, "min_views": 2, "min_cos": 0.2, "score_min": 0.6, "peak_margin": 0.02,
            "depth_rel": 0.01, "min_consistent": 2, "frame_chunk": 8}
PIXEL_CHUNK = 1 << 20
MAX_PATCH, MAX_DEPTHS, MAX_NEIGHBOURS = 7, 63, 8
NONE = -2.0
LOST = ("flags", "score", "margin", "refine", "consistency")


def _kinv(K):
    """Kinv f32 [9] on K's device: the fp64 inverse formed on the host, as Dataset.Kinv is."""
    return torch.inverse(K.detach().cpu().double().reshape(3, 3)).float().reshape(9).to(K.device).contiguous()


def _nbr(fn, nbr, F, device):
    nbr = device_tensor(fn, "nbr", nbr, torch.int32, lambda s: len(s) == 2 and s[0] == F and 1 <= s[1] <= MAX_NEIGHBOURS,
                        f"[{F},1..{MAX_NEIGHBOURS}]")
    if nbr.device != device:
        raise ValueError(f"{fn}: every tensor must be on {device}")
    return nbr


def sweep(gray, valid, R, T, K, pix, guide, nbr, depths: int, step: float, patch: int = DEFAULTS["patch"], min_va=None, min_vb=None,
          min_views: int = DEFAULTS["min_views"], min_cos: float = DEFAULTS["min_cos"]):
    """(out_f f32 [n,4] = (z, c_best, c_second, sub), out_i int32 [n,4] = (k_best, views at k_best, flags, valid hypotheses)) of the
    pixels pix int32 [n,3] = (fi, px, py) with guide f32 [n,4] = (z0, nx, ny, nz) on gray, valid u8 [F,H,W]; R [F,3,3], T [F,3], K [3,3]
    float32; nbr int32 [F,Nn] (dh_mvs_sweep, in calls of at most PIXEL_CHUNK pixels)."""
    fn = "sweep"
    gray = device_tensor(fn, "gray", gray, torch.uint8, lambda s: len(s) == 3 and s[1] > 0 and s[2] > 0, "[F,H,W]")
    F, H, W = gray.shape
    dev = gray.device
    valid = device_tensor(fn, "valid", valid, torch.uint8, lambda s: s == (F, H, W), f"[{F},{H},{W}]")
    R, T, K = check_cams(fn, F, R, T, K, dev)
    pix = device_tensor(fn, "pix", pix, torch.int32, lambda s: len(s) == 2 and s[1] == 3, "[n,3]")
    n = pix.shape[0]
    guide = device_tensor(fn, "guide", guide, torch.float32, lambda s: s == (n, 4), f"[{n},4]")
    nbr = _nbr(fn, nbr, F, dev)
    if valid.device != dev or pix.device != dev or guide.device != dev:
        raise ValueError(f"{fn}: every tensor must be on {dev}")
    depths, patch = int(depths), int(patch)
    if not (3 <= depths <= MAX_DEPTHS and depths % 2 == 1 and 1 <= patch <= MAX_PATCH and float(step) > 0 and int(min_views) >= 1):
        raise ValueError(f"{fn}: depths odd in 3..{MAX_DEPTHS}, patch in 1..{MAX_PATCH}, step > 0, min_views >= 1; got {depths}, {patch}, "
                         f"{step}, {min_views}")
    min_va = default_min_va(patch) if min_va is None else int(min_va)
    min_vb = float(min_va) if min_vb is None else float(min_vb)
    Kinv = _kinv(K)
    out_f = torch.empty(n, 4, dtype=torch.float32, device=dev)
    out_i = torch.empty(n, 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for q0 in range(0, n, PIXEL_CHUNK):
            q1 = min(n, q0 + PIXEL_CHUNK)
            _lib.check(_lib.lib().dh_mvs_sweep(_lib.ptr(gray), _lib.ptr(valid), F, H, W, _lib.ptr(R), _lib.ptr(T), _lib.ptr(K), _lib.ptr(Kinv),
                                               _lib.ptr(pix[q0:q1]), _lib.ptr(guide[q0:q1]), q1 - q0, _lib.ptr(nbr), nbr.shape[1], depths,
                                               float(step), patch, min_va, min_vb, int(min_views), float(min_cos), _lib.ptr(out_f[q0:q1]),
                                               _lib.ptr(out_i[q0:q1]), _lib.stream()))
    return out_f, out_i


def check(depth, R, T, K, nbr, depth_rel: float = DEFAULTS["depth_rel"]):
    """count u8 [F,H,W]: per pixel of depth f32 [F,H,W] (NaN or inf: none), the neighbour frames of nbr int32 [F,Nn] whose depth z_j at
    the nearest pixel to the point's projection has |z_pred - z_j| <= depth_rel z_j (dh_mvs_check)."""
    fn = "check"
    depth = device_tensor(fn, "depth", depth, torch.float32, lambda s: len(s) == 3 and s[1] > 0 and s[2] > 0, "[F,H,W]")
    F, H, W = depth.shape
    dev = depth.device
    R, T, K = check_cams(fn, F, R, T, K, dev)
    nbr = _nbr(fn, nbr, F, dev)
    if not float(depth_rel) >= 0:
        raise ValueError(f"{fn}: depth_rel >= 0, got {depth_rel}")
    Kinv = _kinv(K)
    count = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
    if F:
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().dh_mvs_check(_lib.ptr(depth), F, H, W, _lib.ptr(R), _lib.ptr(T), _lib.ptr(K), _lib.ptr(Kinv), _lib.ptr(nbr),
                                               nbr.shape[1], float(depth_rel), _lib.ptr(count), _lib.stream()))
    return count


def neighbours(n_frames: int, offsets=DEFAULTS["offsets"]):
    """int32 [n_frames, 2 len(offsets)] on the CPU: for frame i the frames i - o, i + o for every offset o in ascending order (default
    1, 2: i - 1, i + 1, i - 2, i + 2); -1 past either end of the sequence."""
    offs = sorted({int(o) for o in offsets})
    if not offs or offs[0] < 1 or 2 * len(offs) > MAX_NEIGHBOURS:
        raise ValueError(f"neighbours: 1..{MAX_NEIGHBOURS // 2} positive offsets, got {offsets}")
    n = int(n_frames)
    out = torch.full((n, 2 * len(offs)), -1, dtype=torch.int32)
    for i in range(n):
        for k, o in enumerate(offs):
            if i - o >= 0:
                out[i, 2 * k] = i - o
            if i + o < n:
                out[i, 2 * k + 1] = i + o
    return out


def guide_from_mesh(verts, faces, R, T, K, H: int, W: int, pix=None):
    """f32 [F,H,W,4] = (z0, nx, ny, nz): the camera z of the mesh's nearest face at every pixel (mesh_color.raster_depth) and that face's
    unit normal in the frame's camera frame, turned to face the camera (n . x_cam <= 0); NaN where no face covers the pixel.  The normal
    is formed in fp64 and rounded once.  pix (int64 [n,3] = (frame, x, y), frame an index into R): f32 [n,4], the same values at those
    pixels only -- the fp64 work is done for n pixels, not for F H W."""
    verts, faces = check_verts("guide_from_mesh", verts), check_faces("guide_from_mesh", faces)
    F, H, W = R.shape[0], int(H), int(W)
    R, T, K = check_cams("guide_from_mesh", F, R, T, K, verts.device)
    zbuf = raster_depth(verts, faces, R, T, K, H, W)
    if pix is None:
        fyx = torch.ones(F, H, W, dtype=torch.bool, device=zbuf.device).nonzero()
        f, y, x = fyx[:, 0], fyx[:, 1], fyx[:, 2]
    else:
        f, x, y = pix[:, 0].long(), pix[:, 1].long(), pix[:, 2].long()
    key = zbuf[f, y, x]
    has = key != -1
    z = (key >> 32).to(torch.int32).view(torch.float32)                           # zbuf_depth's bits
    del zbuf
    face = (key & 0xFFFFFFFF).clamp(0, max(faces.shape[0] - 1, 0))
    tri = verts.double()[faces[face]]                                             # [n,3,3]
    fn = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    fn = fn / fn.norm(dim=1, keepdim=True).clamp(min=1e-300)
    n_cam = torch.einsum("nij,nj->ni", R.double().reshape(F, 3, 3)[f], fn)
    Kinv = torch.inverse(K.cpu().double()).to(K.device)
    e = torch.stack([x.double(), y.double(), torch.ones_like(x, dtype=torch.float64)], 1) @ Kinv.T
    n_cam = torch.where(((n_cam * e).sum(1) > 0)[:, None], -n_cam, n_cam)
    out = torch.cat([z[:, None].double(), n_cam], 1).float()
    out = torch.where(has[:, None], out, torch.full_like(out, float("nan"))).contiguous()
    return out if pix is not None else out.reshape(F, H, W, 4)


def normals_from_depth(depth, kept, Kinv, depth_rel: float = DEFAULTS["depth_rel"], step: int = 1):
    """(normal f32 [...,H,W,3], ok bool [...,H,W]) of depth [...,H,W] (camera z) where kept (bool): with X(x, y) = z Kinv (x, y, 1) the
    normal is cross(X(x + s, y) - X(x - s, y), X(x, y + s) - X(x, y - s)), unit length, turned to face the camera (n . X <= 0), in fp64
    and rounded once.  ok: the pixel and its four neighbours at distance s = `step` are kept and neither pair differs in depth by more
    than depth_rel z (a depth edge); elsewhere the normal is 0.  Plain torch, CPU or device."""
    s = int(step)
    if s < 1:
        raise ValueError(f"normals_from_depth: step >= 1, got {step}")
    H, W = depth.shape[-2:]
    dev = depth.device
    z = depth.double()
    k = kept.bool() & torch.isfinite(z)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    e = torch.stack([xs, ys, torch.ones_like(xs)], -1) @ Kinv.double().reshape(3, 3).to(dev).T
    X = torch.where(k[..., None], z[..., None] * e, torch.zeros_like(e))
    zz = torch.where(k, z, torch.zeros_like(z))
    ok = torch.zeros_like(k)
    n = torch.zeros_like(X)
    if H > 2 * s and W > 2 * s:
        c = (slice(s, H - s), slice(s, W - s))
        l, r = (slice(s, H - s), slice(0, W - 2 * s)), (slice(s, H - s), slice(2 * s, W))
        u, d = (slice(0, H - 2 * s), slice(s, W - s)), (slice(2 * s, H), slice(s, W - s))
        at = lambda t, w: t[(Ellipsis,) + w]
        lim = float(depth_rel) * at(zz, c)
        good = at(k, c) & at(k, l) & at(k, r) & at(k, u) & at(k, d) & ((at(zz, r) - at(zz, l)).abs() <= lim) & ((at(zz, d) - at(zz, u)).abs() <= lim)
        dx = X[(Ellipsis,) + r + (slice(None),)] - X[(Ellipsis,) + l + (slice(None),)]
        dy = X[(Ellipsis,) + d + (slice(None),)] - X[(Ellipsis,) + u + (slice(None),)]
        m = torch.linalg.cross(dx, dy)
        ln = m.norm(dim=-1, keepdim=True)
        good = good & (ln[..., 0] > 0)
        m = m / ln.clamp(min=1e-300)
        m = torch.where(((m * X[(Ellipsis,) + c + (slice(None),)]).sum(-1) > 0)[..., None], -m, m)
        ok[(Ellipsis,) + c] = good
        n[(Ellipsis,) + c + (slice(None),)] = torch.where(good[..., None], m, torch.zeros_like(m))
    return n.float(), ok


def encode_normals(normal, ok):
    """u8 [...,3]: round((n 0.5 + 0.5) 255) of camera-frame unit normals where ok, 128 elsewhere -- what Dataset reads from
    monocular_normal/ and decodes as u8 / 255 * 2 - 1."""
    enc = torch.floor((normal.double() * 0.5 + 0.5) * 255.0 + 0.5).clamp(0, 255).to(torch.uint8)
    return torch.where(ok[..., None], enc, torch.full_like(enc, 128))


def fuse(depth, kept, normal, ok, rgb, R, T, K, voxel=None):
    """(points f32 [n,3], normals f32 [n,3], colors u8 [n,3], index int64 [n,3] = (frame, y, x)): the pixels with kept and ok set as
    object-frame points X = R_f^T (z Kinv (x, y, 1) - T_f), their normals R_f^T n and the frames' colours, in (frame, y, x) order.
    voxel (a cell size in object units, or None): one point per cell floor(X / voxel), the one of the lowest frame and then the lowest
    pixel index y W + x, so the result does not depend on scheduling."""
    F, H, W = depth.shape
    dev = depth.device
    idx = (kept.bool() & ok.bool()).nonzero()                                      # sorted by (frame, y, x)
    f, y, x = idx[:, 0], idx[:, 1], idx[:, 2]
    Rd, Td = R.double().reshape(F, 3, 3), T.double().reshape(F, 3)
    Kinv = torch.inverse(K.cpu().double()).to(dev)
    e = torch.stack([x.double(), y.double(), torch.ones_like(x, dtype=torch.float64)], 1) @ Kinv.T
    cam = depth[f, y, x].double()[:, None] * e
    X = torch.einsum("nji,nj->ni", Rd[f], cam - Td[f])
    nrm = torch.einsum("nji,nj->ni", Rd[f], normal[f, y, x].double())
    if voxel is not None and idx.shape[0]:
        if not float(voxel) > 0:
            raise ValueError(f"fuse: voxel > 0, got {voxel}")
        cell = torch.floor(X / float(voxel)).long()
        cell = cell - cell.min(0).values
        span = cell.max(0).values + 1
        key = (cell[:, 0] * span[1] + cell[:, 1]) * span[2] + cell[:, 2]
        order = torch.sort(key, stable=True).indices                              # within a cell: (frame, y, x) order survives
        ks = key[order]
        firsts = torch.ones_like(ks, dtype=torch.bool)
        firsts[1:] = ks[1:] != ks[:-1]
        pick = torch.sort(order[firsts]).values
        idx, X, nrm = idx[pick], X[pick], nrm[pick]
    col = rgb[idx[:, 0], idx[:, 1], idx[:, 2]]
    return X.float(), nrm.float(), col, idx


def write_cloud_ply(path: str, points, normals, colors):
    """Binary little-endian PLY of a point cloud: float x y z nx ny nz and uchar red green blue per vertex, no faces."""
    import numpy as np
    p = points.detach().cpu().numpy().astype(np.float32)
    rec = np.empty(len(p), dtype=[("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
    rec["p"] = p
    rec["n"] = normals.detach().cpu().numpy().astype(np.float32)
    rec["c"] = colors.detach().cpu().numpy().astype(np.uint8)
    with open(path, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                  "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
                  "property uchar blue\nend_header\n" % len(p)).encode())
        fh.write(rec.tobytes())


def check_settings(settings: dict) -> dict:
    """DEFAULTS overlaid with `settings`; an unknown key or a value out of range raises ValueError.  min_va and min_vb are resolved."""
    s = merge("mvs", DEFAULTS, None, settings, check_overrides=True)
    if isinstance(s["offsets"], str):
        s["offsets"] = tuple(int(o) for o in s["offsets"].split(",") if o.strip())
    s["offsets"] = tuple(int(o) for o in s["offsets"])
    for k in ("patch", "depths", "fine_depths", "step_px", "min_views", "min_consistent", "erode_px", "frame_chunk"):
        s[k] = int(s[k])
    for k in ("range", "min_cos", "score_min", "peak_margin", "depth_rel", "sigma", "a_min"):
        s[k] = float(s[k])
    s["min_va"] = default_min_va(s["patch"]) if s["min_va"] is None else int(s["min_va"])
    s["min_vb"] = float(s["min_va"]) if s["min_vb"] is None else float(s["min_vb"])
    nn = 2 * len(set(s["offsets"]))
    ok = (1 <= s["patch"] <= MAX_PATCH and all(3 <= d <= MAX_DEPTHS and d % 2 == 1 for d in (s["depths"], s["fine_depths"]))
          and s["offsets"] and min(s["offsets"]) >= 1 and nn <= MAX_NEIGHBOURS and s["range"] > 0 and s["step_px"] >= 1
          and 1 <= s["min_views"] <= nn and 0 <= s["min_consistent"] <= nn and s["min_va"] >= 1 and s["min_vb"] > 0
          and -1 <= s["min_cos"] <= 1 and s["depth_rel"] >= 0 and s["sigma"] >= 0 and s["erode_px"] >= 0 and s["frame_chunk"] >= 1)
    if not ok:
        raise ValueError(f"mvs: patch in 1..{MAX_PATCH}, depths and fine_depths odd in 3..{MAX_DEPTHS}, 1..{MAX_NEIGHBOURS // 2} positive "
                         f"offsets, range > 0, step_px >= 1, min_views in 1..{nn}, min_consistent in 0..{nn}, min_va >= 1, min_vb > 0, "
                         f"min_cos in [-1, 1], depth_rel >= 0, sigma >= 0, erode_px >= 0, frame_chunk >= 1; got {s}")
    return s


def depth_maps(dataset, verts, faces, frames=None, **settings):
    """The pipeline for the frames of `dataset` (rgb, label, R, T, K at their current values) about the guide mesh verts f32 [V,3],
    faces int64 [M,3] in the object frame.  frames: the frames to work on (default all; neighbours are any frame).  Returns a dict of
    device tensors: depth f32 [F,H,W] (camera z, NaN where not kept), kept bool [F,H,W], normal f32 [F,H,W,3] and normal_ok bool [F,H,W]
    (normals_from_depth at the grid's step), score f32 [F,H,W] (c_best of the fine pass, NaN where not swept), guide_z f32 [F,H,W]; and
    "stats": the resolved settings, per frame the pixels swept, the count lost to each gate of LOST (flags: either pass 1's flags or an
    unusable guide; score / margin: pass 1; refine: pass 2's flags; consistency: check), the kept share, the mean c_best of the kept
    and the median and 95th percentile of |z - z_guide| over the kept; totals; seconds per phase."""
    s = check_settings(settings)
    F, H, W = dataset.label.shape
    dev = dataset.label.device
    verts, faces = check_verts("depth_maps", verts), check_faces("depth_maps", faces)
    R, T, K = check_cams("depth_maps", F, dataset.R, dataset.T, dataset.K, dev)
    todo = list(range(F)) if frames is None else sorted({int(f) for f in frames})
    if any(f < 0 or f >= F for f in todo):
        raise ValueError(f"depth_maps: frames must lie in [0, {F}), got {frames}")
    sec = {}

    t0 = time.perf_counter()
    usable = usable_map(dataset.label, s["erode_px"])
    gray, valid = gray_frames(dataset.rgb, usable, s["sigma"], s["a_min"], s["frame_chunk"])
    src_ok = usable_sources(gray, valid, s["patch"], s["min_va"], s["frame_chunk"])
    nbr = neighbours(F, s["offsets"]).to(dev)
    lap(sec, "gray", t0, dev)
    D1, D2 = s["depths"], s["fine_depths"]
    step1 = 2.0 * s["range"] / (D1 - 1)
    step2 = 0.25 * step1
    nan = float("nan")
    depth = torch.full((F, H, W), nan, dtype=torch.float32, device=dev)
    score = torch.full((F, H, W), nan, dtype=torch.float32, device=dev)
    guide_z = torch.full((F, H, W), nan, dtype=torch.float32, device=dev)
    lost = torch.zeros(F, H, W, dtype=torch.uint8, device=dev)                  # 0: not swept or kept so far; 1 + index into LOST
    swept = torch.zeros(F, H, W, dtype=torch.bool, device=dev)
    grid = torch.zeros(H, W, dtype=torch.bool, device=dev)
    grid[::s["step_px"], ::s["step_px"]] = True
    for c0 in range(0, len(todo), s["frame_chunk"]):
        fr = torch.tensor(todo[c0:c0 + s["frame_chunk"]], dtype=torch.int64, device=dev)
        t0 = time.perf_counter()
        fyx = (src_ok[fr] & grid[None]).nonzero()
        pix = torch.stack([fr[fyx[:, 0]], fyx[:, 2], fyx[:, 1]], 1).to(torch.int32).contiguous()
        gd = guide_from_mesh(verts, faces, R[fr].contiguous(), T[fr].contiguous(), K, H, W, pix=fyx[:, [0, 2, 1]])
        t0 = lap(sec, "guide", t0, dev)
        f1, i1 = sweep(gray, valid, R, T, K, pix, gd, nbr, D1, step1, s["patch"], s["min_va"], s["min_vb"], s["min_views"], s["min_cos"])
        t0 = lap(sec, "sweep", t0, dev)
        why = torch.zeros(pix.shape[0], dtype=torch.uint8, device=dev)
        why[i1[:, 2] != 0] = 1
        why[(why == 0) & ~(f1[:, 1] >= s["score_min"])] = 2
        why[(why == 0) & ~(f1[:, 1] - f1[:, 2] >= s["peak_margin"])] = 3
        sel = (why == 0).nonzero().reshape(-1)
        gd2 = gd[sel].clone()
        gd2[:, 0] = f1[sel, 0]
        t0 = lap(sec, "gates", t0, dev)
        f2, i2 = sweep(gray, valid, R, T, K, pix[sel].contiguous(), gd2, nbr, D2, step2, s["patch"], s["min_va"], s["min_vb"],
                       s["min_views"], s["min_cos"])
        t0 = lap(sec, "sweep", t0, dev)
        bad2 = i2[:, 2] != 0
        why[sel[bad2]] = 4
        pf, py, px = pix[:, 0].long(), pix[:, 2].long(), pix[:, 1].long()
        swept[pf, py, px] = True
        lost[pf, py, px] = why
        guide_z[pf, py, px] = gd[:, 0]
        good = sel[~bad2]
        depth[pf[good], py[good], px[good]] = f2[~bad2, 0]
        score[pf[good], py[good], px[good]] = f2[~bad2, 1]
        lap(sec, "gates", t0, dev)
    t0 = time.perf_counter()
    if s["min_consistent"] > 0:
        # on the grid's own image: pixel (x, y) of the grid is pixel (x / step_px, y / step_px) of the camera diag(1/s, 1/s, 1) K, so the
        # nearest pixel in a neighbour is the nearest grid pixel there
        sp = s["step_px"]
        Ks = (torch.diag(torch.tensor([1.0 / sp, 1.0 / sp, 1.0], dtype=torch.float64)) @ K.cpu().double()).float().to(dev)
        count = torch.zeros(F, H, W, dtype=torch.uint8, device=dev)
        count[:, ::sp, ::sp] = check(depth[:, ::sp, ::sp].contiguous(), R, T, Ks, nbr, s["depth_rel"])
        drop = torch.isfinite(depth) & (count < s["min_consistent"])
        lost[drop] = 5
        depth[drop] = nan
    kept = torch.isfinite(depth)
    t0 = lap(sec, "check", t0, dev)
    normal, normal_ok = normals_from_depth(depth, kept, _kinv(K).reshape(3, 3), s["depth_rel"], s["step_px"])
    lap(sec, "normals", t0, dev)
    per, tot = [], {"swept": 0, "kept": 0, "lost": {name: 0 for name in LOST}}
    dev_all = []
    for f in todo:
        n_sw, k = int(swept[f].sum()), kept[f]
        nk = int(k.sum())
        dz = (depth[f][k] - guide_z[f][k]).abs().double()
        row = {"frame": f, "swept": n_sw, "kept": nk, "kept_share": nk / max(1, n_sw),
               "lost": {name: int((lost[f] == m + 1).sum()) for m, name in enumerate(LOST)},
               "mean_c_best": float(score[f][k].double().mean()) if nk else None,
               "guide_dev_median": float(dz.median()) if nk else None,
               "guide_dev_p95": float(torch.quantile(dz, 0.95)) if nk else None}
        per.append(row)
        dev_all.append(dz)
        tot["swept"] += n_sw
        tot["kept"] += nk
        for name in LOST:
            tot["lost"][name] += row["lost"][name]
    tot["kept_share"] = tot["kept"] / max(1, tot["swept"])
    dz = torch.cat(dev_all) if dev_all else torch.zeros(0, dtype=torch.float64, device=dev)
    tot["guide_dev_median"] = float(dz.median()) if dz.numel() else None
    tot["normals"] = int(normal_ok.sum())
    stats = {"settings": {k: (list(v) if isinstance(v, tuple) else v) for k, v in s.items()}, "frames": len(todo), "H": H, "W": W,
             "step": step1, "fine_step": step2, "per_frame": per, "totals": tot,
             "lowest_kept_share": [r["frame"] for r in sorted(per, key=lambda r: (r["kept_share"], r["frame"]))[:5]], "seconds": sec}
    return {"depth": depth, "kept": kept, "normal": normal, "normal_ok": normal_ok, "score": score, "guide_z": guide_z, "lost": lost,
            "stats": stats}
