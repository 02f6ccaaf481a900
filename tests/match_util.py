"""numpy restatement of the dense frame matcher (dynhor_amd/match.py, csrc/match.hip): the yardstick of the match tests.
tests/test_cpu_match.py licenses it before anything is compared with it.

Grey: valid = a >= a_min; gray = valid ? clamp(floor(fma(255, fma(0.114, b, fma(0.587, g, 0.299 r)), 0.5)), 0, 255) : 0 in float32, the
fused multiply-adds formed exactly (fma32: a float64 product of two float32 is exact, the sum is rounded to odd, then to float32).

Search, per query (fi, fj, px, py, gx, gy): int64 sums over the (2P+1)^2 patches, a pixel outside the image invalid;
score = num / sqrt(va * vb) in float64, one rounding per operation; best score, smallest candidate index on a tie; second peak outside
excl; sub-pixel parabola per axis; flags 1 (source unusable), 2 (no valid candidate), 4 (best on the border).

Pipeline (match_pairs): forward, backward from the found pixel with the guess p, the gates, kpts1 = q + sub, conf.
"""
import numpy as np
import torch

from . import mesh_texture_util as TU
from . import pose_photo_util as PU
from . import pose_sil_util as SU

NONE = -2.0
LOST = ("flags", "zncc", "margin", "backward")


# ------------------------------------------------------------------------------------------------ grey
def fma32(a, b, c):
    """fma(a, b, c) of float32 arrays, correctly rounded to float32."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b                                                    # exact: 24 + 24 bits
    s = p + c
    bb = s - p                                                   # TwoSum: s + e == p + c exactly
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    toward = np.where(e > 0, np.inf, -np.inf)
    odd = np.where((e != 0) & ((bits & 1) == 0), np.nextafter(s, toward), s)     # round to odd: the sticky bit of the discarded part
    return odd.astype(np.float32)


def gray_ref(img, a_min):
    """(gray, valid) u8 arrays of img float32 [...,4] = (r, g, b, a)."""
    img = np.asarray(img, np.float32)
    r, g, b, a = img[..., 0], img[..., 1], img[..., 2], img[..., 3]
    valid = a >= np.float32(a_min)
    y = fma32(np.float32(0.587), g, np.float32(0.299) * r)
    y = fma32(np.float32(0.114), b, y)
    y = np.floor(fma32(np.float32(255.0), y, np.float32(0.5)))
    y = np.clip(y, 0, 255)
    return np.where(valid, y, 0).astype(np.uint8), valid.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ search
def _patch(gray, valid, f, cx, cy, half):
    """(values int64, valid bool) of the (2 half + 1)^2 window about (cx, cy) of frame f; outside the image: 0, invalid."""
    H, W = gray.shape[1:]
    ys = cy + np.arange(-half, half + 1, dtype=np.int64)
    xs = cx + np.arange(-half, half + 1, dtype=np.int64)
    iy, ix = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    yy, xx = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
    ok = (iy[:, None] & ix[None, :]) & (valid[f][yy[:, None], xx[None, :]] != 0)
    return np.where(ok, gray[f][yy[:, None], xx[None, :]].astype(np.int64), 0), ok


def _box(x, S):
    """Sums of x over every S x S window (valid positions only)."""
    c = np.zeros((x.shape[0] + 1, x.shape[1] + 1), np.int64)
    c[1:, 1:] = x.cumsum(0).cumsum(1)
    return c[S:, S:] - c[:-S, S:] - c[S:, :-S] + c[:-S, :-S]


def search_one(gray, valid, q, P, R, excl, min_va):
    """((qx, qy, flags, count), (s1, s2, sub_x, sub_y), scores [C,C] or None) of one query."""
    fi, fj, px, py, gx, gy = (int(v) for v in q)
    S, C = 2 * P + 1, 2 * R + 1
    N = S * S
    a, aok = _patch(gray, valid, fi, px, py, P)
    sa, sa2 = int(a.sum()), int((a * a).sum())
    va = N * sa2 - sa * sa
    if not aok.all() or va < min_va:
        return (gx, gy, 1, 0), (NONE, NONE, 0.0, 0.0), None
    b, bok = _patch(gray, valid, fj, gx, gy, R + P)
    sb, sb2, cnt = _box(b, S), _box(b * b, S), _box(bok.astype(np.int64), S)
    vb = N * sb2 - sb * sb
    ok = (cnt == N) & (vb >= min_va)
    win = np.lib.stride_tricks.sliding_window_view(b, (S, S))                    # [C,C,S,S]
    sab = np.einsum("ijkl,kl->ij", win, a)
    num = N * sab - sa * sb
    with np.errstate(divide="ignore", invalid="ignore"):
        score = num.astype(np.float64) / np.sqrt(np.float64(va) * vb.astype(np.float64))
    score = np.where(ok, score, NONE)
    count = int(ok.sum())
    if count == 0:
        return (gx, gy, 2, 0), (NONE, NONE, 0.0, 0.0), score
    c = int(np.argmax(score))                                                    # the first maximum in row-major order: the smallest c
    by, bx = divmod(c, C)
    s1 = float(score[by, bx])
    yy, xx = np.mgrid[0:C, 0:C]
    far = ok & (np.maximum(np.abs(xx - bx), np.abs(yy - by)) > excl)
    s2 = float(score[far].max()) if far.any() else NONE
    sub = [0.0, 0.0]
    for k, (pos, m_at, p_at) in enumerate(((bx, (by, bx - 1), (by, bx + 1)), (by, (by - 1, bx), (by + 1, bx)))):
        if 0 < pos < C - 1 and ok[m_at] and ok[p_at]:
            m, p = np.float64(score[m_at]), np.float64(score[p_at])
            den = m - np.float64(2.0) * np.float64(s1) + p
            if den < 0:
                sub[k] = float(min(max(np.float64(0.5) * (m - p) / den, -0.5), 0.5))
    flags = 4 if bx in (0, C - 1) or by in (0, C - 1) else 0
    return (gx + bx - R, gy + by - R, flags, count), (s1, s2, sub[0], sub[1]), score


def search_ref(gray, valid, queries, P, R, excl, min_va):
    """(out_i int32 [n,4], out_f float64 [n,4]) of the queries int [n,6]."""
    n = len(queries)
    oi, of = np.zeros((n, 4), np.int32), np.zeros((n, 4), np.float64)
    for k in range(n):
        oi[k], of[k], _ = search_one(gray, valid, queries[k], P, R, excl, min_va)
    return oi, of


# ------------------------------------------------------------------------------------------------ queries, gates
def default_min_va(P):
    return 4 * ((2 * P + 1) ** 2) ** 2


def usable_sources_ref(gray, valid, P, min_va):
    """bool [F,H,W]: the pixels whose patch is a usable source (all inside and valid, va >= min_va)."""
    S = 2 * P + 1
    N = S * S
    F, H, W = gray.shape
    out = np.zeros((F, H, W), bool)
    for f in range(F):
        v = valid[f] != 0
        g = np.where(v, gray[f].astype(np.int64), 0)
        if H >= S and W >= S:
            ok = (_box(v.astype(np.int64), S) == N) & (N * _box(g * g, S) - _box(g, S) ** 2 >= min_va)
            out[f, P:H - P, P:W - P] = ok
    return out


def select_queries_ref(src_ok, step, max_per_pair):
    """(pix int64 [n,3] = (f, x, y) in (f, y, x) order, steps) as match.select_queries."""
    rows, steps = [], []
    for f in range(src_ok.shape[0]):
        s = step
        while src_ok[f, ::s, ::s].sum() > max_per_pair:
            s += 1
        steps.append(s)
        m = np.zeros_like(src_ok[f])
        m[::s, ::s] = src_ok[f, ::s, ::s]
        y, x = np.nonzero(m)
        rows.append(np.stack([np.full_like(x, f), x, y], 1))
    return np.concatenate(rows).astype(np.int64), steps


def box_guess_ref(label, i, j):
    """floor((centre_j - centre_i) + 0.5) per axis of the object boxes (label == 1) of frames i and j."""
    c2 = []
    for f in (i, j):
        y, x = np.nonzero(label[f] == 1)
        c2.append((int(x.min() + x.max()), int(y.min() + y.max())))
    return ((c2[1][0] - c2[0][0] + 1) // 2, (c2[1][1] - c2[0][1] + 1) // 2)


def match_pairs_ref(gray, valid, queries, P, R, excl=2, min_va=None, zncc_min=0.8, peak_margin=0.05, peak_full=0.2, fb_px=1, gates=True):
    """dict(keep bool [n], lost int [n], kpts1 float32 [n,2], conf float32 [n], out_i, out_f) as match.match_pairs.  gates False: only
    the flags reject (what the matcher gives without its checks)."""
    min_va = default_min_va(P) if min_va is None else min_va
    queries = np.asarray(queries, np.int64)
    oi, of = search_ref(gray, valid, queries, P, R, excl, min_va)
    s1, s2 = of[:, 0], of[:, 1]
    lost = np.zeros(len(queries), np.int64)
    lost[oi[:, 2] != 0] = 1
    if gates:
        lost[(lost == 0) & ~(s1 >= zncc_min)] = 2
        lost[(lost == 0) & ~(s1 - s2 >= peak_margin)] = 3
        idx = np.nonzero(lost == 0)[0]
        back = np.stack([queries[idx, 1], queries[idx, 0], oi[idx, 0], oi[idx, 1], queries[idx, 2], queries[idx, 3]], 1)
        bi, _ = search_ref(gray, valid, back, P, R, excl, min_va)
        ok = (bi[:, 2] == 0) & (np.abs(bi[:, 0] - queries[idx, 2]) <= fb_px) & (np.abs(bi[:, 1] - queries[idx, 3]) <= fb_px)
        lost[idx[~ok]] = 4
    kpts1 = (oi[:, :2].astype(np.float64) + of[:, 2:4]).astype(np.float32)
    conf = (s1 * np.minimum((s1 - s2) / peak_full, 1.0)).astype(np.float32)
    return {"keep": lost == 0, "lost": lost, "kpts1": kpts1, "conf": conf, "out_i": oi, "out_f": of}


# ------------------------------------------------------------------------------------------------ mesh guide
def mesh_guesses_ref(fi, fj, p, zbuf, verts, faces, R, T, K, depth_eps=0.01, min_cos=0.2):
    """(g int64 [n,2], keep bool [n], ambiguous bool [n]) of match.mesh_guesses in fp64 on the CPU from the given z-buffer; ambiguous:
    the projection within PU.TOL_PX of a rounding boundary, or the depth / cosine / front test within pose_photo_util's tolerances."""
    F, H, W = zbuf.shape
    Rd, Td, Kd = R.double().reshape(F, 3, 3), T.double().reshape(F, 3), K.double()
    depth = TU.zbuf_depth64(zbuf)
    key = zbuf[fi, p[:, 1], p[:, 0]]
    has = key != -1
    z = torch.where(has, depth[fi, p[:, 1], p[:, 0]], torch.ones(len(fi), dtype=torch.float64))
    ray = torch.cat([p.double(), torch.ones(len(fi), 1, dtype=torch.float64)], 1) @ torch.inverse(Kd).T
    X = ((ray * z[:, None] - Td[fi])[:, None, :] @ Rd[fi])[:, 0]                # R^T v as a row vector times R
    cam = (Rd[fj] @ X[:, :, None])[:, :, 0] + Td[fj]
    zj = cam[:, 2]
    u, w = (cam @ Kd[0]) / zj, (cam @ Kd[1]) / zj
    gx, gy = torch.floor(u + 0.5), torch.floor(w + 0.5)
    ins = (zj > 1e-3) & (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H)
    gxi, gyi = torch.where(ins, gx, torch.zeros_like(gx)).long(), torch.where(ins, gy, torch.zeros_like(gy)).long()
    dj = depth[fj, gyi, gxi]
    seen = ins & torch.isfinite(dj) & (zj <= dj + depth_eps)
    tri = verts.double()[faces[(key & 0xFFFFFFFF).clamp(0, faces.shape[0] - 1)]]
    n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    Ci = -(Td[fi][:, None, :] @ Rd[fi])[:, 0]
    Cj = -(Td[fj][:, None, :] @ Rd[fj])[:, 0]
    n = torch.where(((n * (Ci - X)).sum(1) < 0)[:, None], -n, n)
    d = Cj - X
    cos = (n * d).sum(1) / (n.norm(dim=1) * d.norm(dim=1))
    keep = has & seen & (cos >= min_cos)
    near = lambda t: (t - t.round()).abs() < PU.TOL_PX
    amb = has & (((zj - 1e-3).abs() < PU.TOL_Z) | near(u + 0.5) | near(w + 0.5)
                 | (ins & torch.isfinite(dj) & ((zj - dj - depth_eps).abs() < PU.TOL_DEPTH)) | ((cos - min_cos).abs() < PU.TOL_COS))
    return torch.stack([gxi, gyi], 1), keep, amb


# ------------------------------------------------------------------------------------------------ the sphere scenes
H_SCENE, W_SCENE = 192, 256
AXIS = (0.3, 1.0, 0.2)
HAND_RGB = (217, 158, 128)


def turned_sphere(degs, hands=None, k=12, H=H_SCENE, W=W_SCENE):
    """The textured sphere of pose_photo_util (pattern(k)) seen by one camera of mesh_texture_util.cameras(1, H, W, radius=2.2, seed=3),
    the object turned by `degs` degrees about AXIS.  hands: per frame None or (cx, cy, a, b) of an ellipse labelled -1 and painted
    skin.  Returns dict(rgb u8 [F,H,W,3], label i8 [F,H,W], R f64 [F,3,3], T f64 [F,3], K, pts f64 [F,H,W,3] the object point seen at
    every pixel, hit bool [F,H,W])."""
    R0, T0, K = TU.cameras(1, H, W, radius=2.2, seed=3)
    R = torch.stack([R0[0].double() @ SU.axis_angle(AXIS, float(d)) for d in degs])
    T = T0.double().expand(len(degs), 3).contiguous()
    rgb, label = PU.sphere_frames(R, T, K, H, W, PU.pattern(k))
    hit, pts, _ = PU.sphere_hits(R, T, K, H, W)
    if hands is not None:
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        for f, e in enumerate(hands):
            if e is None:
                continue
            cx, cy, a, b = e
            m = ((xs - cx) / a) ** 2 + ((ys - cy) / b) ** 2 < 1.0
            label[f][m] = -1
            rgb[f][m] = torch.tensor(HAND_RGB, dtype=torch.uint8)
    return {"rgb": rgb, "label": label, "R": R, "T": T, "K": K, "pts": pts, "hit": hit, "H": H, "W": W}


def project(X, R, T, K):
    """(u, w) fp64 of the object points X [n,3] in the camera R, T."""
    cam = X.double() @ R.double().T + T.double()
    return (cam @ K[0].double()) / cam[:, 2], (cam @ K[1].double()) / cam[:, 2]


def gray_of_scene(sc, sigma=1.0, a_min=0.5, erode_px=1):
    """(gray, valid) u8 numpy arrays of a scene by the restatements: erode_object, the float32 blur, gray_ref."""
    usable = TU.erode_object(sc["label"], erode_px)
    img = PU.blur(sc["rgb"], usable, PU.taps(sigma)[0], torch.float32)
    return gray_ref(img.numpy(), a_min)


def error_stats(kpts1, u, w):
    """(median, p95, share beyond 1.5 px) of |kpts1 - (u, w)|."""
    e = np.hypot(kpts1[:, 0].astype(np.float64) - u, kpts1[:, 1].astype(np.float64) - w)
    return float(np.median(e)), float(np.percentile(e, 95)), float((e > 1.5).mean())
