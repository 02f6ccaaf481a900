"""Plain-torch / numpy restatement of the pose initialisation's retrieval (dynhor_amd/pose_init.py, csrc/pose_init.hip): the yardstick
of the pose_init tests.  Everything runs on the CPU; tests/test_cpu_pose_init.py licenses it before anything is compared with it.

  boxes      (xmin, ymin, xmax, ymax) over label == 1, (W, H, -1, -1) for an image without one
  squares    centre of the tight box, b = 1.3 max(width, height) in pixels (xmax - xmin + 1), x0 = cx - b / 2, y0 = cy - b / 2,
             step = b / S in fp64, rounded once to fp32; (0, 0, 0) for an empty box
  crop       sample (r, c) reads the pixel px = floor(fma(c + 0.5, step, x0) + 0.5), py likewise, in fp32; obj = label == 1 and
             keep = label >= 0 inside the image, both 0 outside; all 0 when step is not > 0
  pack       sample s = r S + c is bit (s & 63) of word (s >> 6)
  score      inter = |fo & bo & fk|, union = |(fo | bo) & fk|;  IoU = inter / union in fp64, 0 where the union is 0
  top-K      stable descending sort: a tie goes to the lower view index
  depth      the box-driven fixed point of the reference (utils/camera.py:132-176), one hypothesis at a time
  Viterbi    brute force over all paths
"""
import functools
import itertools
import math

import numpy as np
import torch

from tests import pose_sil_util as U

F64 = torch.float64
EXPANSION = 1.3


def arvo(n, seed):
    """float64 [n,3,3]: Arvo's rotations from torch.rand(3, n, float64) of a CPU generator, one matrix at a time."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(3, n, dtype=F64, generator=g).numpy()
    out = np.empty((n, 3, 3))
    for i in range(n):
        a, b, c = 2 * math.pi * x[0, i], 2 * math.pi * x[1, i], x[2, i]
        Rz = np.array([[math.cos(a), math.sin(a), 0.0], [-math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        v = np.array([math.cos(b) * math.sqrt(c), math.sin(b) * math.sqrt(c), math.sqrt(1.0 - c)])
        out[i] = (2.0 * np.outer(v, v) - np.eye(3)) @ Rz
    return torch.from_numpy(out)


def angle_deg(Ra, Rb):
    tr = (Ra * Rb).sum(dim=(-2, -1))
    return torch.rad2deg(torch.acos(((tr - 1.0) / 2.0).clamp(-1.0, 1.0)))


def boxes(label):
    n, H, W = label.shape
    out = torch.empty(n, 4, dtype=torch.int32)
    for i in range(n):
        ys, xs = (label[i] == 1).nonzero(as_tuple=True)
        out[i] = torch.tensor([int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] if xs.numel() else [W, H, -1, -1])
    return out


def squares(bx, S):
    out = np.zeros((bx.shape[0], 3), dtype=np.float64)
    for i, (x0, y0, x1, y1) in enumerate(bx.tolist()):
        if x1 < x0:
            continue
        b = EXPANSION * max(x1 - x0 + 1, y1 - y0 + 1)
        out[i] = ((x0 + x1) / 2.0 - b / 2.0, (y0 + y1) / 2.0 - b / 2.0, b / S)
    return torch.from_numpy(out.astype(np.float32))


def sample_pixels(sq, S):
    """(px, py) int64 [n,S] each: the pixel column of every sample column and the pixel row of every sample row, in the kernel's fp32
    arithmetic (the product of two fp32 numbers is exact in fp64, so fp64 multiply-add rounded to fp32 is the fused operation up to a
    double rounding that needs a 29-bit tie); plus the fp64 coordinates (before the + 0.5 and the floor) for boundary tests."""
    q = sq.numpy().astype(np.float32)
    t = (np.arange(S, dtype=np.float32) + np.float32(0.5)).astype(np.float64)
    exact_x = t[None, :] * q[:, 2:3].astype(np.float64) + q[:, 0:1].astype(np.float64)
    exact_y = t[None, :] * q[:, 2:3].astype(np.float64) + q[:, 1:2].astype(np.float64)
    px = np.floor(exact_x.astype(np.float32) + np.float32(0.5)).astype(np.int64)
    py = np.floor(exact_y.astype(np.float32) + np.float32(0.5)).astype(np.int64)
    return torch.from_numpy(px), torch.from_numpy(py), torch.from_numpy(exact_x), torch.from_numpy(exact_y)


def crop(label, sq, S):
    """(obj, keep) bool [n,S,S]."""
    n, H, W = label.shape
    px, py, _, _ = sample_pixels(sq, S)
    obj = torch.zeros(n, S, S, dtype=torch.bool)
    keep = torch.zeros(n, S, S, dtype=torch.bool)
    for i in range(n):
        if not float(sq[i, 2]) > 0.0:
            continue
        okx, oky = (px[i] >= 0) & (px[i] < W), (py[i] >= 0) & (py[i] < H)
        v = label[i][py[i].clamp(0, H - 1)][:, px[i].clamp(0, W - 1)]
        inside = oky[:, None] & okx[None, :]
        obj[i] = inside & (v == 1)
        keep[i] = inside & (v >= 0)
    return obj, keep


def pack(bits):
    """int64 [n, S^2 / 64] from bool [n,S,S] (or [n,S^2])."""
    n = bits.shape[0]
    b = bits.reshape(n, -1, 64).numpy().astype(np.uint64)
    words = (b << np.arange(64, dtype=np.uint64)[None, None, :]).sum(axis=2, dtype=np.uint64)
    return torch.from_numpy(words.view(np.int64).copy())


def unpack(words):
    """bool [n, 64 Wd] from int64 [n,Wd]."""
    w = words.numpy().view(np.uint64)
    return torch.from_numpy(((w[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool).reshape(w.shape[0], -1))


def score(fo, fk, bo):
    """int32 [F,V,2] from bool [F,N], [F,N], [V,N]: (|fo & bo & fk|, |(fo | bo) & fk|); counts < 2^53 are exact in fp64 products."""
    a = (fo & fk).to(F64)
    rest = (fk & ~fo).to(F64)
    b = bo.to(F64)
    inter = a @ b.T
    union = a.sum(dim=1, keepdim=True) + rest @ b.T
    return torch.stack([inter, union], -1).round().to(torch.int32)


def iou(counts):
    c = counts.to(F64)
    return torch.where(c[..., 1] > 0, c[..., 0] / c[..., 1].clamp(min=1.0), torch.zeros_like(c[..., 0]))


def topk(iou_all, k):
    val, idx = torch.sort(iou_all, dim=1, descending=True, stable=True)
    return idx[:, :k], val[:, :k]


def depth(verts, R, box, K, iters=10):
    """T float64 [3] of ONE hypothesis: verts [V,3], R [3,3], box (x0, y0, x1, y1) continuous, K [3,3]."""
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    p = (verts.to(F64) @ R.to(F64).T).numpy()
    x0, y0, x1, y1 = [float(v) for v in box]
    diag = math.hypot(x1 - x0, y1 - y0)
    bx, by = (x0 + x1) / 2.0, (y0 + y1) / 2.0
    z = 1.0
    tx, ty = (bx - cx) * z / fx, (by - cy) * z / fy
    for _ in range(iters):
        u = (p[:, 0] + tx) / (p[:, 2] + z) * fx + cx
        w = (p[:, 1] + ty) / (p[:, 2] + z) * fy + cy
        z = z * math.hypot(u.max() - u.min(), w.max() - w.min()) / diag
        tx += (bx - (u.max() + u.min()) / 2.0) * z / fx
        ty += (by - (w.max() + w.min()) / 2.0) * z / fy
    return torch.tensor([tx, ty, z], dtype=F64)


def viterbi_brute(node, edges):
    """(path, cost) minimising sum node[f, k_f] + sum edges[f][k_f, k_{f+1}] over ALL K^n paths; the lexicographically first minimum."""
    n, Kc = node.shape
    best, arg = None, None
    for path in itertools.product(range(Kc), repeat=n):
        c = sum(float(node[f, k]) for f, k in enumerate(path)) + sum(float(edges[f][path[f], path[f + 1]]) for f in range(n - 1))
        if best is None or c < best:
            best, arg = c, list(path)
    return arg, best


def coverage(verts, faces, R, T, K, H, W):
    """bool [n,H,W] in fp64: a pixel centre is covered when some face (no vertex at z <= 1e-3, non-zero screen area) has its three edge
    functions all >= 0 or all <= 0 with a non-zero sum: pose_sil_util.nearest's d2 == 0.  One view at a time, over the pixels of the
    projected vertices' box only (no face reaches beyond it)."""
    v, K = verts.to(F64), K.to(F64)
    out = torch.zeros(R.shape[0], H, W, dtype=torch.bool)
    for n in range(R.shape[0]):
        uv, z = U.project(v, R[n].to(F64), T[n].to(F64), K)
        tri, zt = uv[faces], z[faces]
        ok = (zt > 1e-3).all(-1) & (U._edge(tri[:, 0], tri[:, 1], tri[:, 2]) != 0)
        if not bool(ok.any()):
            continue
        used = tri[ok].reshape(-1, 2)
        x0, y0 = max(0, math.floor(float(used[:, 0].min()))), max(0, math.floor(float(used[:, 1].min())))
        x1, y1 = min(W - 1, math.ceil(float(used[:, 0].max()))), min(H - 1, math.ceil(float(used[:, 1].max())))
        if x1 < x0 or y1 < y0:
            continue
        yy, xx = torch.meshgrid(torch.arange(y0, y1 + 1, dtype=F64), torch.arange(x0, x1 + 1, dtype=F64), indexing="ij")
        q = torch.stack([xx.reshape(-1), yy.reshape(-1)], -1)[:, None, :]
        a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
        e0, e1, e2 = U._edge(b, c, q), U._edge(c, a, q), U._edge(a, b, q)
        cov = (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & ((e0 + e1 + e2) != 0) & ok[None, :]
        out[n, y0:y1 + 1, x0:x1 + 1] = cov.any(dim=-1).view(y1 - y0 + 1, x1 - x0 + 1)
    return out


def bank_camera(verts, render_size, distance_scale):
    """(K, T) float64 of the bank's views: focal 1.2 render_size, centre (render_size - 1) / 2, the template at distance_scale x its
    largest vertex norm on the optical axis."""
    c = (render_size - 1) / 2.0
    K = torch.tensor([[1.2 * render_size, 0.0, c], [0.0, 1.2 * render_size, c], [0.0, 0.0, 1.0]], dtype=F64)
    return K, torch.tensor([0.0, 0.0, distance_scale * float(verts.to(F64).norm(dim=1).max())], dtype=F64)


def pack_label(label, S):
    """(obj words, keep words, boxes, squares) of label i8 [n,H,W]: the restatement's whole frame / view path."""
    bx = boxes(label)
    sq = squares(bx, S)
    o, k = crop(label, sq, S)
    return pack(o), pack(k), bx, sq


# ---------------------------------------------------------------------------------------------------- the recall fixture of the issue
RECALL = dict(n_frames=8, H=96, W=96, seed=3, n_views=1500, bank_seed=11, render_size=64, crop_size=48, distance_scale=3.5,
              candidates=32)


@functools.lru_cache(maxsize=1)
def recall_scene():
    """The scene of the recall claim, its frames packed at S = 48, the bank's rotations and camera (computed once per process)."""
    c = RECALL
    sc = U.small_scene(n_frames=c["n_frames"], H=c["H"], W=c["W"], seed=c["seed"], hand=True)
    R = arvo(c["n_views"], c["bank_seed"])
    K, T = bank_camera(sc["verts"], c["render_size"], c["distance_scale"])
    fo, fk, bx, sq = pack_label(sc["label"], c["crop_size"])
    return {"scene": sc, "R": R, "K": K, "T": T, "frame_obj": fo, "frame_keep": fk, "frame_boxes": bx, "frame_sq": sq}


def retrieval(bank_cov, fx=None):
    """The restatement's retrieval against the bank coverage bool [V,rs,rs]: {"index", "iou" [F,K], "iou_all" [F,V], "near_deg" [F] the
    angle of the bank view nearest to the truth, "best_deg" [F] the smallest angle among the top K, "argmax_deg" [F] the top view's,
    "angles" [F,V]}."""
    fx = recall_scene() if fx is None else fx
    c = RECALL
    bo = pack_label(bank_cov.to(torch.int8), c["crop_size"])[0]
    counts = score(unpack(fx["frame_obj"]), unpack(fx["frame_keep"]), unpack(bo))
    iou_all = iou(counts)
    idx, val = topk(iou_all, c["candidates"])
    ang = angle_deg(fx["scene"]["R_true"][:, None], fx["R"][None, :])
    top = torch.gather(ang, 1, idx)
    return {"index": idx, "iou": val, "iou_all": iou_all, "counts": counts, "bank_obj": bo, "angles": ang,
            "near_deg": ang.min(dim=1).values, "best_deg": top.min(dim=1).values, "argmax_deg": top[:, 0]}
