"""Dense frame matching: ``correspondence_infos`` from the frames themselves, by guided block matching (csrc/match.hip,
include/dynhor_hip.h).  The classical stand-in for the reference's learned dense matcher (DKM), as silhouette retrieval stands in for
DINOv2 in ``pose_init`` and direct alignment for a learned photometric prior in ``pose_photo``.

  * ``gray_frames`` (dh_image_blur, dh_match_gray): the frames as 8-bit grey, blurred by a masked Gaussian over the usable pixels
    (``mesh_color.usable_map``: object pixels, eroded; hand and background never enter a patch), and the validity map a >= a_min.
  * ``search`` (dh_match_search): per query (fi, fj, p, g) the (2P+1)^2 patch about p in frame fi against every displacement within R
    of the guess g in frame fj, scored by zero-mean normalised cross-correlation (ZNCC) on exact integer sums: the best candidate, the
    second peak outside ``excl``, a sub-pixel step per axis, flags (1 source patch unusable, 2 no valid candidate, 4 best on the
    window's border).
  * ``select_queries``: the pixels of a grid whose source patch is usable; the grid's step is raised per frame until at most
    ``max_per_pair`` remain.
  * the guess: ``guide="none"`` moves p by the rounded displacement of the object's box centre (``pose_init.label_boxes``) -- for
    neighbouring frames of a video; ``guide="mesh"`` back-projects p with the z-buffer of a mesh at the dataset's current poses
    (``mesh_color.raster_depth``), projects the point into frame j and drops the query when the point is hidden there, faces away
    from camera j or has no depth.
  * ``match_pairs``: forward search, backward search from the found pixel with the guess p, and the gates: both flags 0,
    s1 >= zncc_min, s1 - s2 >= peak_margin, the way back within fb_px of p.  kpts0 = p, kpts1 = q + sub, conf = s1 min(1, (s1 - s2) /
    peak_full).
  * ``match_frames``: all of it for a Dataset; returns the list ``Dataset.set_correspondences`` takes, and the counts.
  * ``warp="affine"`` (with ``guide="mesh"``; ``mesh_affines``, ``search_warp`` = dh_match_search_warp): the plane of the face seen
    at p induces a 2 x 2 affine map J between the two images; the forward search samples its source patch through J^-1 and the
    backward search through J (Q16 entries, 8-bit bilinear weights, integers throughout), so the integer ZNCC search compares patches
    of the same shape again across wide baselines and in-plane rotation.  A query whose J mirrors or scales beyond ``warp_max`` is
    dropped.

Limits: without the warp a patch knows neither scale nor rotation (beyond roughly 20 degrees of viewpoint change or 10 degrees in the
image plane the score fades); with it the patch follows one plane per query: the faceted normal of a coarse mesh, a depth edge inside
the patch and a scale beyond ``warp_max`` (no anti-aliasing beyond the blur) are not followed; there is no pyramid, a displacement
beyond R from the guess is lost; the result is semi-dense, on a grid; a highlight that moves with the hand matches itself.
DESIGN_NEXT_ROWS.md sections 20 and 23 have the numbers.

The kernels run on the current stream; there is no CPU path.
"""
from __future__ import annotations

import time

import torch

from . import _lib
from ._args import check_cams, check_faces, check_verts, device_tensor
from .mesh_color import raster_depth, usable_map
from .settings import merge
from .pose_photo import blur_frames

GUIDES = ("none", "mesh")
# defaults of the YAML's match: block; DESIGN_NEXT_ROWS.md section 20 says where each comes from.  range None: 16 (guide none), 12
# (guide mesh); min_va None: 4 N^2, N = (2 patch + 1)^2 (a patch variance of 4 grey levels^2)
DEFAULTS = {"guide": "none", "offsets": (1, 2, 5), "sigma": 1.0, "a_min": 0.5, "erode_px": 1, "patch": 4, "range": None, "excl": 2,
            "min_va": None, "zncc_min": 0.8, "peak_margin": 0.05, "peak_full": 0.2, "fb_px": 1, "step": 1, "max_per_pair": 4096,
            "depth_eps": 0.01, "min_cos": 0.2, "frame_chunk": 16, "warp": "none", "warp_max": 3.0}
WARPS = ("none", "affine")
WARP_MAX_LIMIT = 8.0                                         # dh_match_search_warp takes no entry beyond 2^19 in Q16
RANGE_DEFAULT = {"none": 16, "mesh": 12}
QUERY_CHUNK = 1 << 20
MAX_STEP = 1 << 12
LOST = ("flags", "zncc", "margin", "backward")


def default_min_va(patch: int) -> int:
    n = (2 * int(patch) + 1) ** 2
    return 4 * n * n


def match_gray(img, a_min: float):
    """(gray, valid) u8 [F,H,W] of img f32 [F,H,W,4] = blur_frames' output (dh_match_gray)."""
    img = device_tensor("match_gray", "img", img, torch.float32, lambda s: len(s) == 4 and s[3] == 4 and s[1] > 0 and s[2] > 0,
                        "[F,H,W,4]")
    F, H, W = img.shape[:3]
    gray = torch.empty(F, H, W, dtype=torch.uint8, device=img.device)
    valid = torch.empty_like(gray)
    if F:
        with torch.cuda.device(img.device):
            _lib.check(_lib.lib().dh_match_gray(_lib.ptr(img), F, H, W, float(a_min), _lib.ptr(gray), _lib.ptr(valid), _lib.stream()))
    return gray, valid


def gray_frames(rgb, usable, sigma: float = DEFAULTS["sigma"], a_min: float = DEFAULTS["a_min"], frame_chunk: int = DEFAULTS["frame_chunk"]):
    """(gray, valid) u8 [F,H,W]: pose_photo.blur_frames(rgb, usable, sigma) turned into grey bytes, `frame_chunk` frames at a time (the
    blurred frames take 32 bytes per pixel while a chunk is worked on).  Every frame is worked on alone."""
    if int(frame_chunk) < 1:
        raise ValueError(f"gray_frames: frame_chunk must be >= 1, got {frame_chunk}")
    F = rgb.shape[0]
    parts = [match_gray(blur_frames(rgb[f0:f0 + int(frame_chunk)], usable[f0:f0 + int(frame_chunk)], sigma), a_min)
             for f0 in range(0, F, int(frame_chunk))]
    if not parts:
        return match_gray(blur_frames(rgb, usable, sigma), a_min)
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def search(gray, valid, queries, patch: int = DEFAULTS["patch"], rng: int = 16, excl: int = DEFAULTS["excl"], min_va=None):
    """(out_i int32 [n,4] = (qx, qy, flags, valid candidates), out_f f64 [n,4] = (s1, s2, sub_x, sub_y)) of the queries int32 [n,6] =
    (fi, fj, px, py, gx, gy) on gray, valid u8 [F,H,W] (dh_match_search, in calls of at most QUERY_CHUNK queries)."""
    return _search("search", 6, gray, valid, queries, patch, rng, excl, min_va)


def _search(fn, words, gray, valid, queries, patch, rng, excl, min_va):
    """search (words 6, dh_match_search) and search_warp (words 10, dh_match_search_warp)."""
    gray = device_tensor(fn, "gray", gray, torch.uint8, lambda s: len(s) == 3 and s[1] > 0 and s[2] > 0, "[F,H,W]")
    F, H, W = gray.shape
    valid = device_tensor(fn, "valid", valid, torch.uint8, lambda s: s == (F, H, W), f"[{F},{H},{W}]")
    queries = device_tensor(fn, "queries", queries, torch.int32, lambda s: len(s) == 2 and s[1] == words, f"[n,{words}]")
    if valid.device != gray.device or queries.device != gray.device:
        raise ValueError(f"{fn}: every tensor must be on {gray.device}")
    min_va = default_min_va(patch) if min_va is None else int(min_va)
    n = queries.shape[0]
    out_i = torch.empty(n, 4, dtype=torch.int32, device=gray.device)
    out_f = torch.empty(n, 4, dtype=torch.float64, device=gray.device)
    entry = _lib.lib().dh_match_search_warp if words == 10 else _lib.lib().dh_match_search
    with torch.cuda.device(gray.device):
        for q0 in range(0, n, QUERY_CHUNK):
            q1 = min(n, q0 + QUERY_CHUNK)
            _lib.check(entry(_lib.ptr(gray), _lib.ptr(valid), F, H, W, _lib.ptr(queries[q0:q1]), q1 - q0, int(patch), int(rng), int(excl),
                             min_va, _lib.ptr(out_i[q0:q1]), _lib.ptr(out_f[q0:q1]), _lib.stream()))
    return out_i, out_f


def _box_sums(x, P: int):
    """Sums of x int64 [F,H,W] over the (2P+1)^2 window about every pixel, windows that leave the image counted as they lie inside it."""
    F, H, W = x.shape
    c = torch.zeros(F, H + 1, W + 1, dtype=torch.int64, device=x.device)
    c[:, 1:, 1:] = x.cumsum(1).cumsum(2)
    y0 = (torch.arange(H, device=x.device) - P).clamp(min=0)
    y1 = (torch.arange(H, device=x.device) + P + 1).clamp(max=H)
    x0 = (torch.arange(W, device=x.device) - P).clamp(min=0)
    x1 = (torch.arange(W, device=x.device) + P + 1).clamp(max=W)
    return c[:, y1][:, :, x1] - c[:, y0][:, :, x1] - c[:, y1][:, :, x0] + c[:, y0][:, :, x0]


def usable_sources(gray, valid, patch: int = DEFAULTS["patch"], min_va=None, frame_chunk: int = DEFAULTS["frame_chunk"]):
    """bool [F,H,W]: the pixels whose (2P+1)^2 patch dh_match_search accepts as a source: all N pixels valid (and inside the image) and
    N sum a^2 - (sum a)^2 >= min_va, by integer box sums.  Plain torch."""
    P = int(patch)
    N = (2 * P + 1) ** 2
    min_va = default_min_va(P) if min_va is None else int(min_va)
    out = []
    for f0 in range(0, gray.shape[0], int(frame_chunk)):
        g = gray[f0:f0 + int(frame_chunk)].long()
        v = valid[f0:f0 + int(frame_chunk)].ne(0).long()
        g = g * v
        out.append((_box_sums(v, P) == N) & (N * _box_sums(g * g, P) - _box_sums(g, P) ** 2 >= min_va))
    return torch.cat(out) if out else torch.zeros(gray.shape, dtype=torch.bool, device=gray.device)


def select_queries(src_ok, step: int = DEFAULTS["step"], max_per_pair: int = DEFAULTS["max_per_pair"]):
    """(pix int32 [n,3] = (frame, x, y) in (frame, y, x) order, steps: the grid step of every frame): the pixels with x and y multiples
    of the frame's step and src_ok (bool [F,H,W], usable_sources) set; the step of a frame is the smallest >= `step` that leaves at
    most `max_per_pair` of them.  Two host reads per run."""
    step, max_per_pair = int(step), int(max_per_pair)
    if step < 1 or max_per_pair < 1:
        raise ValueError(f"select_queries: step >= 1 and max_per_pair >= 1, got {step}, {max_per_pair}")
    F, H, W = src_ok.shape
    dev = src_ok.device
    steps = torch.full((F,), step, dtype=torch.int64)
    todo = list(range(F))
    s = step
    while todo and s <= MAX_STEP:
        cand = list(range(s, s + 16))
        counts = torch.stack([src_ok[todo][:, ::c, ::c].sum((1, 2)) for c in cand], 1).cpu()          # [len(todo), 16]
        fits = counts <= max_per_pair
        nxt = []
        for k, f in enumerate(todo):
            hit = fits[k].nonzero()
            if hit.numel():
                steps[f] = cand[int(hit[0])]
            else:
                nxt.append(f)
        todo, s = nxt, s + 16
    for f in todo:
        steps[f] = MAX_STEP
    sd = steps.to(dev)[:, None, None]
    ys = torch.arange(H, device=dev)[None, :, None]
    xs = torch.arange(W, device=dev)[None, None, :]
    fyx = (src_ok & (ys % sd == 0) & (xs % sd == 0)).nonzero()
    pix = torch.stack([fyx[:, 0], fyx[:, 2], fyx[:, 1]], 1).to(torch.int32).contiguous()
    return pix, steps.tolist()


def frame_pairs(n_frames: int, offsets):
    """[(i, i + off)] for every offset in order of i, then the offset; no wrap-around."""
    offs = sorted({int(o) for o in offsets})
    if not offs or offs[0] < 1:
        raise ValueError(f"frame_pairs: offsets must be positive integers, got {offsets}")
    return [(i, i + o) for i in range(int(n_frames)) for o in offs if i + o < int(n_frames)]


def box_shifts(label):
    """int64 [F,2] on the device: (xmin + xmax, ymin + ymax) of the object's box per frame: twice its centre, kept as integers."""
    from .pose_init import label_boxes
    b = label_boxes(label).long()
    return torch.stack([b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1)


def pair_queries(pix, pairs, n_frames: int):
    """(rows int64 [n]: indices into pix, pair int64 [n]: indices into pairs) of the queries of all pairs, pair-major, a pair's queries
    in pix's order."""
    dev = pix.device
    f = pix[:, 0].long()
    start = torch.searchsorted(f, torch.arange(n_frames + 1, device=dev)).tolist()
    rows, pid = [], []
    for k, (i, _) in enumerate(pairs):
        a, b = start[i], start[i + 1]
        rows.append(torch.arange(a, b, device=dev))
        pid.append(torch.full((b - a,), k, dtype=torch.int64, device=dev))
    if not rows:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return z, z
    return torch.cat(rows), torch.cat(pid)


def guide_none(pix, rows, pid, pairs, label):
    """queries int32 [n,6] with g = p + floor((centre_j - centre_i) + 0.5) per axis, the centres those of the object boxes."""
    c2 = box_shifts(label)
    pr = torch.tensor(pairs, dtype=torch.int64, device=pix.device).reshape(-1, 2)
    fi, fj = pr[pid, 0], pr[pid, 1]
    p = pix[rows, 1:3].long()
    d = torch.div(c2[fj] - c2[fi] + 1, 2, rounding_mode="floor")
    return torch.cat([fi[:, None], fj[:, None], p, p + d], 1).to(torch.int32).contiguous()


def _mesh_points(fi, fj, p, zbuf, verts, faces, R, T, K):
    """What mesh_guesses and mesh_affines share, fp64 on the device: has bool [n] (p has a depth), ci f64 [n,3] = z K^-1 (x, y, 1) the
    point in camera i (z = 1 where there is no depth), X = R_i^T (ci - T_i), cam = R_j X + T_j, zs = cam's z kept away from 0,
    guide f64 [n,2] = the projection of cam, nrm the normal of the face seen at p turned towards camera i (not normalised), Ci, Cj
    the camera centres, Rd, Td, Kd."""
    from .mesh_color import zbuf_depth
    F, H, W = zbuf.shape
    Rd, Td, Kd = R.double().reshape(F, 3, 3), T.double().reshape(F, 3), K.double()
    Kinv = torch.inverse(Kd.cpu()).to(Kd.device)
    key = zbuf[fi, p[:, 1], p[:, 0]]
    has = key != -1
    z = zbuf_depth(zbuf)[fi, p[:, 1], p[:, 0]].double()
    z = torch.where(has, z, torch.ones_like(z))
    ray = torch.cat([p.double(), torch.ones(p.shape[0], 1, dtype=torch.float64, device=p.device)], 1) @ Kinv.T
    ci = ray * z[:, None]
    X = torch.einsum("nji,nj->ni", Rd[fi], ci - Td[fi])
    cam = torch.einsum("nij,nj->ni", Rd[fj], X) + Td[fj]
    zj = cam[:, 2]
    zs = torch.where(zj.abs() > 1e-12, zj, torch.full_like(zj, 1e-12))
    guide = torch.stack([(cam @ Kd[0]) / zs, (cam @ Kd[1]) / zs], 1)
    face = (key & 0xFFFFFFFF).clamp(0, max(faces.shape[0] - 1, 0))
    tri = verts.double()[faces[face]]
    nrm = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    Ci = -torch.einsum("nji,nj->ni", Rd[fi], Td[fi])
    Cj = -torch.einsum("nji,nj->ni", Rd[fj], Td[fj])
    nrm = torch.where(((nrm * (Ci - X)).sum(1) < 0)[:, None], -nrm, nrm)
    return {"has": has, "ci": ci, "X": X, "cam": cam, "zs": zs, "guide": guide, "nrm": nrm, "Ci": Ci, "Cj": Cj, "Rd": Rd, "Td": Td, "Kd": Kd}


def mesh_guesses(fi, fj, p, zbuf, verts, faces, R, T, K, depth_eps: float = DEFAULTS["depth_eps"], min_cos: float = DEFAULTS["min_cos"]):
    """(g int64 [n,2], keep bool [n], guide f64 [n,2]) for the pixels p int64 [n,2] = (x, y) of the frames fi seen in the frames fj
    (int64 [n]) through the mesh: with z the z-buffer depth at p (zbuf int64 [F,H,W], mesh_color.raster_depth at R, T, K) the point
    X = R_i^T (z K^-1 (x, y, 1) - T_i) is projected into frame j, (u, w) = guide, g = floor(guide + 0.5).  keep: p has a depth; X lies
    in front of camera j (z_j > 1e-3) and g in the image; j's z-buffer is not empty at g and z_j <= its depth + depth_eps; and the
    face seen at p, its normal turned towards camera i, has cos = <n, normalize(C_j - X)> >= min_cos.  fp64 torch on the device."""
    from .mesh_color import zbuf_depth
    F, H, W = zbuf.shape
    m = _mesh_points(fi, fj, p, zbuf, verts, faces, R, T, K)
    has, X, zj, guide, nrm, Cj = m["has"], m["X"], m["cam"][:, 2], m["guide"], m["nrm"], m["Cj"]
    g = torch.floor(guide + 0.5)
    ins = (zj > 1e-3) & (g[:, 0] >= 0) & (g[:, 0] < W) & (g[:, 1] >= 0) & (g[:, 1] < H)
    g = torch.where(ins[:, None], g, torch.zeros_like(g)).long()
    dj = zbuf_depth(zbuf)[fj, g[:, 1], g[:, 0]].double()
    seen = ins & torch.isfinite(dj) & (zj <= dj + float(depth_eps))
    dj3 = Cj - X
    cos = (nrm * dj3).sum(1) / (nrm.norm(dim=1) * dj3.norm(dim=1)).clamp(min=1e-300)
    return g, has & seen & (cos >= float(min_cos)), guide


def _projection_jacobian(c, uw, Kd, Rf):
    """D f64 [n,2,3] = (1 / c_z) [K0 - u e3^T; K1 - w e3^T] R_f: the derivative of frame f's projection (u, w) = uw by the object point,
    c f64 [n,3] the point in the camera (K's last row is e3)."""
    e3 = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=c.device)
    M = torch.stack([Kd[0][None, :] - uw[:, 0:1] * e3, Kd[1][None, :] - uw[:, 1:2] * e3], 1) / c[:, 2, None, None]
    return M @ Rf


def quantise_affine(A):
    """int64 [n,4] = floor(A 65536 + 0.5) of A f64 [n,2,2], row-major (a00, a01, a10, a11): dh_match_search_warp's Q16."""
    return torch.floor(A.reshape(-1, 4) * 65536.0 + 0.5).long()


def mesh_affines(fi, fj, p, zbuf, verts, faces, R, T, K, warp_max: float = DEFAULTS["warp_max"]):
    """(J f64 [n,2,2], fwd int64 [n,4], bwd int64 [n,4], keep bool [n]) for mesh_guesses' queries: the plane through the surface point X
    of p with the normal n of the face seen there induces an affine map between the two images.  With D_f the 2 x 3 derivative of frame
    f's projection at X and B_i = [D_i; n^T], an offset dp in frame i moves X by B_i^-1 (dp, 0) within the plane, so
    J = D_j B_i^-1[:, :2] maps frame-i pixel offsets to frame-j pixel offsets.  fwd = floor(J^-1 65536 + 0.5): the forward search
    samples frame i at target (frame j) offsets; bwd = floor(J 65536 + 0.5): the backward search (fj, fi, q, p) samples frame j at
    frame-i offsets.  keep: det J > 0 and both singular values of J within [1 / warp_max, warp_max] (a NaN fails); where keep is
    False, fwd and bwd are the identity.  A pixel without depth gives numbers of no meaning: mesh_guesses drops it.  fp64 torch on the
    device."""
    m = _mesh_points(fi, fj, p, zbuf, verts, faces, R, T, K)
    ci = torch.einsum("nij,nj->ni", m["Rd"][fi], m["X"]) + m["Td"][fi]            # not m["ci"]: a float32 R is orthogonal to 1e-7 only
    Di = _projection_jacobian(ci, torch.stack([(ci @ m["Kd"][0]) / ci[:, 2], (ci @ m["Kd"][1]) / ci[:, 2]], 1), m["Kd"], m["Rd"][fi])
    cam = torch.cat([m["cam"][:, :2], m["zs"][:, None]], 1)
    Dj = _projection_jacobian(cam, m["guide"], m["Kd"], m["Rd"][fj])
    r0, r1, n = Di[:, 0], Di[:, 1], m["nrm"]
    c0, c1 = torch.linalg.cross(r1, n), torch.linalg.cross(n, r0)                 # det B_i times the first two columns of B_i^-1
    det_b = (r0 * c0).sum(1)
    J = (Dj @ torch.stack([c0, c1], 2)) / det_b[:, None, None]
    a, b, c, d = J[:, 0, 0], J[:, 0, 1], J[:, 1, 0], J[:, 1, 1]
    det = a * d - b * c
    s1 = a * a + b * b + c * c + d * d
    s2 = torch.sqrt((a * a + b * b - c * c - d * d) ** 2 + 4.0 * (a * c + b * d) ** 2)
    smax = torch.sqrt(0.5 * (s1 + s2))
    smin = det.abs() / smax
    keep = (det > 0) & (smax <= float(warp_max)) & (smin >= 1.0 / float(warp_max))
    Jinv = torch.stack([d, -b, -c, a], 1).reshape(-1, 2, 2) / det[:, None, None]
    eye = torch.tensor([65536, 0, 0, 65536], dtype=torch.int64, device=J.device)
    k4 = keep[:, None]
    fwd = torch.where(k4, quantise_affine(torch.where(k4[:, :, None], Jinv, torch.zeros_like(Jinv))), eye)
    bwd = torch.where(k4, quantise_affine(torch.where(k4[:, :, None], J, torch.zeros_like(J))), eye)
    return J, fwd, bwd, keep


def search_warp(gray, valid, queries, patch: int = DEFAULTS["patch"], rng: int = 16, excl: int = DEFAULTS["excl"], min_va=None):
    """search with the source patch sampled through a 2 x 2 map per query: queries int32 [n,10] = (fi, fj, px, py, gx, gy, a00, a01,
    a10, a11), A = a / 65536 maps an offset in the target patch to an offset in the source image (dh_match_search_warp, in calls of
    at most QUERY_CHUNK queries).  The identity (65536, 0, 0, 65536) gives search's outputs bit for bit."""
    return _search("search_warp", 10, gray, valid, queries, patch, rng, excl, min_va)


def match_pairs(gray, valid, queries, patch: int = DEFAULTS["patch"], rng: int = 16, excl: int = DEFAULTS["excl"], min_va=None,
                zncc_min: float = DEFAULTS["zncc_min"], peak_margin: float = DEFAULTS["peak_margin"],
                peak_full: float = DEFAULTS["peak_full"], fb_px=DEFAULTS["fb_px"], affine_fwd=None, affine_bwd=None):
    """The forward search of the queries int32 [n,6], the backward search (fj, fi, q, p) of those that pass the forward gates, and the
    verdict per query.  Returns a dict of device tensors over the n queries: keep bool, lost int64 (0 kept, else 1 + the index into
    LOST of the first gate that rejected it), kpts1 f32 [n,2] = q + sub, conf f32 = s1 min(1, (s1 - s2) / peak_full), s1 f64, and
    out_i / out_f of the forward search.  affine_fwd, affine_bwd (both or neither; [n,4] integers in Q16, mesh_affines): both
    searches go through search_warp, the forward one with affine_fwd, the backward one with the same query's affine_bwd."""
    if (affine_fwd is None) != (affine_bwd is None):
        raise ValueError("match_pairs: affine_fwd and affine_bwd come together")
    if affine_fwd is not None:
        if tuple(affine_fwd.shape) != (queries.shape[0], 4) or tuple(affine_bwd.shape) != (queries.shape[0], 4):
            raise ValueError(f"match_pairs: affine_fwd and affine_bwd must be [{queries.shape[0]},4]")
        with_affine = lambda q, a: torch.cat([q, a.to(torch.int32)], 1).contiguous()
        return _match_pairs(lambda q: search_warp(gray, valid, with_affine(q, affine_fwd), patch, rng, excl, min_va),
                            lambda q, idx: search_warp(gray, valid, with_affine(q, affine_bwd[idx]), patch, rng, excl, min_va),
                            queries, zncc_min, peak_margin, peak_full, fb_px)
    return _match_pairs(lambda q: search(gray, valid, q, patch, rng, excl, min_va),
                        lambda q, idx: search(gray, valid, q, patch, rng, excl, min_va), queries, zncc_min, peak_margin, peak_full, fb_px)


def _match_pairs(forward, backward, queries, zncc_min, peak_margin, peak_full, fb_px):
    """match_pairs' gates about the two searches: forward(queries), backward(back queries, their indices into queries)."""
    oi, of = forward(queries)
    s1, s2 = of[:, 0], of[:, 1]
    lost = torch.zeros(queries.shape[0], dtype=torch.int64, device=queries.device)
    lost[oi[:, 2] != 0] = 1
    lost[(lost == 0) & ~(s1 >= float(zncc_min))] = 2
    lost[(lost == 0) & ~(s1 - s2 >= float(peak_margin))] = 3
    idx = (lost == 0).nonzero().reshape(-1)
    qf = queries[idx]
    back = torch.stack([qf[:, 1], qf[:, 0], oi[idx, 0], oi[idx, 1], qf[:, 2], qf[:, 3]], 1).contiguous()
    bi, _ = backward(back, idx)
    ok = (bi[:, 2] == 0) & ((bi[:, 0] - qf[:, 2]).abs() <= fb_px) & ((bi[:, 1] - qf[:, 3]).abs() <= fb_px)
    lost[idx[~ok]] = 4
    kpts1 = (oi[:, :2].double() + of[:, 2:4]).float()
    conf = (s1 * ((s1 - s2) / float(peak_full)).clamp(max=1.0)).float()
    return {"keep": lost == 0, "lost": lost, "kpts1": kpts1, "conf": conf, "s1": s1, "out_i": oi, "out_f": of}


def check_settings(settings: dict) -> dict:
    """DEFAULTS overlaid with `settings`; an unknown key or a value out of range raises ValueError.  range and min_va are resolved."""
    s = merge("match", DEFAULTS, None, settings, check_overrides=True)
    if s["guide"] not in GUIDES:
        raise ValueError(f"match: guide must be one of {GUIDES}, got {s['guide']!r}")
    if isinstance(s["offsets"], str):
        s["offsets"] = tuple(int(o) for o in s["offsets"].split(",") if o.strip())
    s["offsets"] = tuple(int(o) for o in s["offsets"])
    s["range"] = RANGE_DEFAULT[s["guide"]] if s["range"] is None else int(s["range"])
    s["patch"] = int(s["patch"])
    s["min_va"] = default_min_va(s["patch"]) if s["min_va"] is None else int(s["min_va"])
    if not (1 <= s["patch"] <= 7 and 0 <= s["range"] <= 32 and int(s["excl"]) >= 0 and s["min_va"] >= 1 and float(s["peak_full"]) > 0
            and float(s["fb_px"]) >= 0 and float(s["sigma"]) >= 0 and int(s["erode_px"]) >= 0 and s["offsets"] and min(s["offsets"]) >= 1):
        raise ValueError(f"match: patch in 1..7, range in 0..32, excl >= 0, min_va >= 1, peak_full > 0, fb_px >= 0, sigma >= 0, erode_px "
                         f">= 0 and positive offsets; got {s}")
    s["warp_max"] = float(s["warp_max"])
    if s["warp"] not in WARPS:
        raise ValueError(f"match: warp must be one of {WARPS}, got {s['warp']!r}")
    if s["warp"] == "affine" and s["guide"] != "mesh":
        raise ValueError("match: warp 'affine' takes its planes from a mesh: it needs guide 'mesh'")
    if not 1.0 <= s["warp_max"] <= WARP_MAX_LIMIT:
        raise ValueError(f"match: warp_max in [1, {WARP_MAX_LIMIT:g}], got {s['warp_max']}")
    return s


def match_frames(dataset, verts=None, faces=None, **settings):
    """(matches, stats) for the frames of `dataset` (rgb, label, and with guide "mesh" R, T, K and the mesh verts f32 [V,3], faces int64
    [M,3] in the object frame).  matches: per pair (i, j = i + offset) with at least one kept match {i, j, kpts0 f32 [M,2], kpts1 f32
    [M,2], conf f32 [M]} on the CPU -- what Dataset.set_correspondences and scene.write_correspondences_to_disk take.  stats: the
    resolved settings, per pair the queries (grid pixels with a usable source patch), searched (those the guide kept), kept, the count
    lost to each gate of LOST, the mean s1 of the kept, warp_dropped (with warp "affine": the queries the guide kept and mesh_affines
    did not, which are not searched) and, with a mesh, the median distance of the kept kpts1 from the guide; totals; seconds.
    warp "affine" (guide "mesh" only): both searches sample their source patch through the affine map the mesh's face plane induces
    between the two frames (mesh_affines, dh_match_search_warp)."""
    t0 = time.time()
    s = check_settings(settings)
    F, H, W = dataset.label.shape
    dev = dataset.label.device
    usable = usable_map(dataset.label, int(s["erode_px"]))
    gray, valid = gray_frames(dataset.rgb, usable, s["sigma"], s["a_min"], s["frame_chunk"])
    src_ok = usable_sources(gray, valid, s["patch"], s["min_va"], s["frame_chunk"])
    pix, steps = select_queries(src_ok, s["step"], s["max_per_pair"])
    del src_ok
    pairs = frame_pairs(F, s["offsets"])
    rows, pid = pair_queries(pix, pairs, F)
    n_queries = torch.bincount(pid, minlength=len(pairs))
    guide = affine_fwd = affine_bwd = None
    warp_dropped = torch.zeros(len(pairs), dtype=torch.int64, device=dev)
    if s["guide"] == "none":
        queries = guide_none(pix, rows, pid, pairs, dataset.label)
    else:
        if verts is None or faces is None:
            raise ValueError("match_frames: guide 'mesh' needs a mesh (verts, faces)")
        verts, faces = check_verts("match_frames", verts), check_faces("match_frames", faces)
        R, T, K = check_cams("match_frames", F, dataset.R, dataset.T, dataset.K, dev)
        zbuf = raster_depth(verts, faces, R, T, K, H, W)
        pr = torch.tensor(pairs, dtype=torch.int64, device=dev).reshape(-1, 2)
        fi, fj, p = pr[pid, 0], pr[pid, 1], pix[rows, 1:3].long()
        g, keep, guide = mesh_guesses(fi, fj, p, zbuf, verts, faces, R, T, K, s["depth_eps"], s["min_cos"])
        if s["warp"] == "affine":
            _, affine_fwd, affine_bwd, ok = mesh_affines(fi, fj, p, zbuf, verts, faces, R, T, K, s["warp_max"])
            warp_dropped = torch.bincount(pid[keep & ~ok], minlength=len(pairs))
            keep = keep & ok
        del zbuf
        sel = keep.nonzero().reshape(-1)
        if affine_fwd is not None:
            affine_fwd, affine_bwd = affine_fwd[sel], affine_bwd[sel]
        queries = torch.cat([fi[:, None], fj[:, None], p, g], 1)[sel].to(torch.int32).contiguous()
        pid, guide = pid[sel], guide[sel]
    res = match_pairs(gray, valid, queries, s["patch"], s["range"], s["excl"], s["min_va"], s["zncc_min"], s["peak_margin"],
                      s["peak_full"], s["fb_px"], affine_fwd, affine_bwd)
    npair = len(pairs)
    keep = res["keep"]
    searched = torch.bincount(pid, minlength=npair)
    kept = torch.bincount(pid[keep], minlength=npair)
    lost = torch.stack([torch.bincount(pid[res["lost"] == k + 1], minlength=npair) for k in range(len(LOST))], 1)
    s1_sum = torch.zeros(npair, dtype=torch.float64, device=dev).index_add_(0, pid[keep], res["s1"][keep])
    counts = torch.cat([n_queries[:, None], searched[:, None], kept[:, None], lost, warp_dropped[:, None]], 1).cpu()
    s1_sum = s1_sum.cpu()
    kq = queries[keep].cpu()
    k1, cf, kp = res["kpts1"][keep].cpu(), res["conf"][keep].cpu(), pid[keep].cpu()
    dist = (res["kpts1"][keep].double() - guide[keep]).norm(dim=1).cpu() if guide is not None else None
    matches, per_pair = [], []
    bounds = torch.searchsorted(kp, torch.arange(npair + 1)).tolist()                                  # pid is sorted: pair-major queries
    for k, (i, j) in enumerate(pairs):
        a, b = bounds[k], bounds[k + 1]
        row = {"i": i, "j": j, "queries": int(counts[k, 0]), "searched": int(counts[k, 1]), "kept": int(counts[k, 2]),
               "lost": {name: int(counts[k, 3 + m]) for m, name in enumerate(LOST)},
               "mean_s1": float(s1_sum[k]) / (b - a) if b > a else None, "warp_dropped": int(counts[k, 3 + len(LOST)])}
        if dist is not None:
            row["median_guide_px"] = float(dist[a:b].median()) if b > a else None
        per_pair.append(row)
        if b > a:
            matches.append({"i": i, "j": j, "kpts0": kq[a:b, 2:4].float(), "kpts1": k1[a:b].clone(), "conf": cf[a:b].clone()})
    tot = counts.sum(0)
    stats = {"settings": {k: (list(v) if isinstance(v, tuple) else v) for k, v in s.items()}, "frames": F, "H": H, "W": W, "steps": steps,
             "pairs": per_pair,
             "totals": {"pairs": npair, "queries": int(tot[0]), "searched": int(tot[1]), "kept": int(tot[2]),
                        "kept_share": float(tot[2]) / max(1, int(tot[1])),
                        "lost": {name: int(tot[3 + m]) for m, name in enumerate(LOST)}, "warp_dropped": int(tot[3 + len(LOST)])},
             "seconds": time.time() - t0}
    return matches, stats
