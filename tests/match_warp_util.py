"""numpy restatement of the affine-warped frame matcher (dynhor_amd/match.py warp="affine", csrc/match.hip
match_search_kernel<P, true>): the yardstick of tests/test_cpu_match_warp.py and tests/test_gpu_match_warp.py.  It stands on
tests/match_util.py, which tests/test_cpu_match.py licenses.

Warped patch (warp_patch): cell (c, r), c, r in [-P, P], samples frame fi at (X, Y) / 65536 with X = px 65536 + a00 c + a01 r,
Y = py 65536 + a10 c + a11 r in int64; (x0, y0) = (X >> 16, Y >> 16), fx = (X & 0xFFFF) >> 8, fy likewise; the four taps weigh
(256 - fx, fx) x (256 - fy, fy); a tap of weight 0 is not needed; the cell is valid iff every needed tap is inside and valid;
value = (sum w gray + 32768) >> 16.

Search (search_warp_ref): the warped patch, with its validity, is pasted into an extra frame and match_util.search_one searches
from that frame at (P, P): everything after the source patch is match_util's, unchanged.

Affine map (affines_fd): the plane through the surface point X with the normal n of the face seen at p; the projections of both
frames differentiated by central differences along two tangents of that plane; J = M_j M_i^-1 maps frame-i pixel offsets to frame-j
pixel offsets.  The forward search uses J^-1, the backward search J, both as floor(A 65536 + 0.5).
"""
import numpy as np
import torch

from . import match_util as M
from . import mesh_texture_util as TU
from . import pose_photo_util as PU
from . import pose_sil_util as SU

IDENTITY = (65536, 0, 0, 65536)
MAX_AFFINE = 1 << 19
WARP_MAX = 3.0
FD_STEP = 5e-5             # object units: the smallest of 1e-4, 5e-5, 2e-5, 1e-5 at which the restatement's distance from its half step
                           # still falls by 4 when the step is halved (truncation, not rounding noise; test_cpu_match_warp.py checks it)


# ------------------------------------------------------------------------------------------------ the warped patch, the search
def warp_patch(gray, valid, f, px, py, a, P):
    """(values int64 [S,S], valid bool [S,S]) of the source patch about (px, py) of frame f through a = (a00, a01, a10, a11) in Q16;
    row index = r + P, column index = c + P."""
    H, W = gray.shape[1:]
    k = np.arange(-P, P + 1, dtype=np.int64)
    cc, rr = np.meshgrid(k, k)                                # cc varies along a row
    a00, a01, a10, a11 = (int(v) for v in a)
    X = int(px) * 65536 + a00 * cc + a01 * rr
    Y = int(py) * 65536 + a10 * cc + a11 * rr
    x0, y0 = X >> 16, Y >> 16                                 # numpy's >> on int64 is arithmetic: a floor
    fx, fy = (X & 0xFFFF) >> 8, (Y & 0xFFFF) >> 8
    total = np.zeros_like(X)
    ok = np.ones(X.shape, bool)
    for j, wy in enumerate((256 - fy, fy)):
        for i, wx in enumerate((256 - fx, fx)):
            w = wx * wy
            x, y = x0 + i, y0 + j
            inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            xc, yc = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
            good = inside & (valid[f][yc, xc] != 0)
            need = w != 0
            ok &= ~need | good
            total += np.where(need & good, w * gray[f][yc, xc].astype(np.int64), 0)
    return np.where(ok, (total + 32768) >> 16, 0), ok


def search_warp_ref(gray, valid, queries, P, R, excl, min_va):
    """(out_i int32 [n,4], out_f float64 [n,4]) of the queries int [n,10] = (fi, fj, px, py, gx, gy, a00, a01, a10, a11)."""
    F, H, W = gray.shape
    S = 2 * P + 1
    assert H >= S and W >= S
    ge = np.concatenate([gray, np.zeros((1, H, W), gray.dtype)])
    ve = np.concatenate([valid, np.zeros((1, H, W), valid.dtype)])
    n = len(queries)
    oi, of = np.zeros((n, 4), np.int32), np.zeros((n, 4), np.float64)
    for k in range(n):
        fi, fj, px, py, gx, gy = (int(v) for v in queries[k][:6])
        vals, ok = warp_patch(gray, valid, fi, px, py, queries[k][6:10], P)
        ge[F, :S, :S] = vals
        ve[F, :S, :S] = ok
        oi[k], of[k], _ = M.search_one(ge, ve, (F, fj, P, P, gx, gy), P, R, excl, min_va)
    return oi, of


def match_pairs_warp_ref(gray, valid, queries, fwd, bwd, P, R, excl=2, min_va=None, zncc_min=0.8, peak_margin=0.05, peak_full=0.2, fb_px=1):
    """match_util.match_pairs_ref with both searches warped: the forward one by fwd int [n,4], the backward one (fj, fi, q, p) by the
    same query's bwd."""
    min_va = M.default_min_va(P) if min_va is None else min_va
    queries = np.asarray(queries, np.int64)
    oi, of = search_warp_ref(gray, valid, np.concatenate([queries, fwd], 1), P, R, excl, min_va)
    s1, s2 = of[:, 0], of[:, 1]
    lost = np.zeros(len(queries), np.int64)
    lost[oi[:, 2] != 0] = 1
    lost[(lost == 0) & ~(s1 >= zncc_min)] = 2
    lost[(lost == 0) & ~(s1 - s2 >= peak_margin)] = 3
    idx = np.nonzero(lost == 0)[0]
    back = np.concatenate([np.stack([queries[idx, 1], queries[idx, 0], oi[idx, 0], oi[idx, 1], queries[idx, 2], queries[idx, 3]], 1),
                           bwd[idx]], 1)
    bi, _ = search_warp_ref(gray, valid, back, P, R, excl, min_va)
    ok = (bi[:, 2] == 0) & (np.abs(bi[:, 0] - queries[idx, 2]) <= fb_px) & (np.abs(bi[:, 1] - queries[idx, 3]) <= fb_px)
    lost[idx[~ok]] = 4
    kpts1 = (oi[:, :2].astype(np.float64) + of[:, 2:4]).astype(np.float32)
    conf = (s1 * np.minimum((s1 - s2) / peak_full, 1.0)).astype(np.float32)
    return {"keep": lost == 0, "lost": lost, "kpts1": kpts1, "conf": conf, "out_i": oi, "out_f": of}


# ------------------------------------------------------------------------------------------------ affines for the search tests
def random_affines(g, n):
    """int64 [n,4]: rotation over the full circle, scale 0.35 .. 2.8 per axis, shear, fractional Q16 parts."""
    th = g.uniform(0, 2 * np.pi, n)
    sx, sy = g.uniform(0.35, 2.8, n), g.uniform(0.35, 2.8, n)
    sh = g.uniform(-0.5, 0.5, n)
    c, s = np.cos(th), np.sin(th)
    A = np.stack([c * sx, (c * sh - s) * sy, s * sx, (s * sh + c) * sy], 1)
    return np.floor(A * 65536 + 0.5).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the affine map of a face plane
def _np(t):
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def project_np(X, R, T, K):
    """(u, w) float64 [...,2] of the object points X in the cameras R [...,3,3], T [...,3]."""
    c = np.einsum("...ij,...j->...i", R, X) + T
    return np.stack([c @ K[0] / c[..., 2], c @ K[1] / c[..., 2]], -1)


def surface_points(fi, p, zbuf, verts, faces, R, T, K):
    """(has bool [n], X float64 [n,3], n float64 [n,3]) from a z-buffer in dh_mesh_raster_depth's format: the point seen at the pixel
    p of frame fi, X = R_i^T (z K^-1 (x, y, 1) - T_i), and the normal of the face seen there turned towards camera i (z = 1, face 0
    where the pixel is empty)."""
    fi, p = np.asarray(fi), np.asarray(p)
    zb = zbuf.cpu().numpy() if isinstance(zbuf, torch.Tensor) else zbuf
    R, T, K, v = _np(R).reshape(-1, 3, 3), _np(T).reshape(-1, 3), _np(K), _np(verts)
    fc = faces.cpu().numpy() if isinstance(faces, torch.Tensor) else faces
    key = zb[fi, p[:, 1], p[:, 0]]
    has = key != -1
    z = np.where(has, (key >> 32).astype(np.int32).view(np.float32).astype(np.float64), 1.0)
    ray = np.concatenate([p.astype(np.float64), np.ones((len(p), 1))], 1) @ np.linalg.inv(K).T
    X = np.einsum("nji,nj->ni", R[fi], ray * z[:, None] - T[fi])
    tri = v[fc[np.clip(key & 0xFFFFFFFF, 0, len(fc) - 1)]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    Ci = -np.einsum("nji,nj->ni", R[fi], T[fi])
    n = np.where(((n * (Ci - X)).sum(1) < 0)[:, None], -n, n)
    return has, X, n


def affines_fd(fi, fj, X, n, R, T, K, h=FD_STEP):
    """J float64 [n,2,2] by central differences with the step h along two tangents of the plane (X, n): with M_f the 2 x 2 derivative of
    frame f's projection by the two tangent coordinates, J = M_j M_i^-1."""
    R, T, K = _np(R).reshape(-1, 3, 3), _np(T).reshape(-1, 3), _np(K)
    nn = n / np.linalg.norm(n, axis=1, keepdims=True)
    e = np.eye(3)[np.argmin(np.abs(nn), axis=1)]                                 # the axis the normal leans on least
    t1 = np.cross(nn, e)
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nn, t1)
    Ms = []
    for f in (fi, fj):
        cols = [(project_np(X + h * t, R[f], T[f], K) - project_np(X - h * t, R[f], T[f], K)) / (2 * h) for t in (t1, t2)]
        Ms.append(np.stack(cols, 2))
    return Ms[1] @ np.linalg.inv(Ms[0])


def affine_verdict(J, warp_max=WARP_MAX):
    """(keep bool [n], singular values [n,2], det [n]): det J > 0 and both singular values within [1 / warp_max, warp_max]."""
    sv = np.linalg.svd(J, compute_uv=False)
    det = np.linalg.det(J)
    return (det > 0) & (sv[:, 0] <= warp_max) & (sv[:, 1] >= 1.0 / warp_max), sv, det


def quantise(A):
    return np.floor(A.reshape(-1, 4) * 65536.0 + 0.5).astype(np.int64)


def fd_bound(fi, fj, X, n, R, T, K, h=FD_STEP):
    """(J at the step h, bound_J [n], bound_Jinv [n]): per query 4 times the largest entry by which J (J^-1) at the step h differs from
    the one at h / 2.  The truncation error of a central difference is c h^2: the two differ by 0.75 c h^2, so the error at h is 4/3 of
    the difference; the factor 4 leaves a margin of 3.  The truncation term changes from query to query with the viewing angles (a
    grazing view has a large one), the rounding noise of the differences (about 1e-16 x 200 px / h) does not and can cancel in one
    query's difference by chance: a query's bound is not taken below the median over the queries."""
    Jh, Jq = affines_fd(fi, fj, X, n, R, T, K, h), affines_fd(fi, fj, X, n, R, T, K, h / 2)
    dj = np.abs(Jh - Jq).reshape(-1, 4).max(1)
    di = np.abs(np.linalg.inv(Jh) - np.linalg.inv(Jq)).reshape(-1, 4).max(1)
    return Jh, 4.0 * np.maximum(dj, np.median(dj)), 4.0 * np.maximum(di, np.median(di))


def near_rounding(A, bound):
    """bool [n]: an entry of A 65536 within `bound` [n] 65536 of a rounding boundary (k + 0.5)."""
    t = A.reshape(-1, 4) * 65536.0 + 0.5
    return (np.abs(t - np.round(t)) <= np.asarray(bound).reshape(-1, 1) * 65536.0).any(1)


# ------------------------------------------------------------------------------------------------ the wide-baseline scenes
def three_cameras(H, W):
    """The cameras of tests/test_gpu_match.py's mesh-guide test: one camera of mesh_texture_util.cameras and the object turned by 15
    and 40 degrees about match_util.AXIS before it, the third view off-centre."""
    R0, T0, K = TU.cameras(1, H, W, radius=2.2, seed=3)
    R = torch.stack([(R0[0].double() @ SU.axis_angle(M.AXIS, d)).float() for d in (0.0, 15.0, 40.0)])
    T = T0.expand(3, 3).clone()
    T[2, 0] += 0.35
    return R.contiguous(), T.contiguous(), K


def three_camera_queries(H, W):
    """(fi, fj, p): every second pixel of every frame as a query into both other frames, in the order (0,1) (0,2) (1,0) (1,2) (2,0) (2,1)."""
    ys, xs = torch.meshgrid(torch.arange(0, H, 2), torch.arange(0, W, 2), indexing="ij")
    p1 = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    fi = torch.cat([torch.full((len(p1),), i) for i in range(3) for _ in range(2)])
    fj = torch.cat([torch.full((len(p1),), j) for i in range(3) for j in range(3) if j != i])
    return fi, fj, p1.repeat(6, 1)


def rolled_sphere(deg, roll, k=12, H=M.H_SCENE, W=M.W_SCENE):
    """match_util.turned_sphere([0, deg]) with the second camera rolled by `roll` degrees about its optical axis: its pose is
    (Rz R, Rz T) and its image is rendered from that pose, so image and pose roll together."""
    sc = M.turned_sphere([0.0, float(deg)], None, k, H, W)
    Rz = SU.axis_angle((0.0, 0.0, 1.0), float(roll)).double()
    R = torch.stack([sc["R"][0], Rz @ sc["R"][1]])
    T = torch.stack([sc["T"][0], Rz @ sc["T"][1]])
    rgb, label = PU.sphere_frames(R, T, sc["K"], H, W, PU.pattern(k))
    hit, pts, _ = PU.sphere_hits(R, T, sc["K"], H, W)
    return {"rgb": rgb, "label": label, "R": R, "T": T, "K": sc["K"], "pts": pts, "hit": hit, "H": H, "W": W}


SCENE_P, SCENE_R, SCENE_STEP = 4, 12, 3                       # guide "mesh": the default range


def scene_pair_ref(sc, warp, verts, faces, zbuf=None):
    """The restatement's pipeline on the pair (0, 1) of a sphere scene with guide "mesh" at the true poses: grey, queries on a 3 px
    grid, mesh_guesses_ref on the brute-force fp64 z-buffer (or `zbuf`), with warp the affines of affines_fd, forward, backward, the
    gates.  Returns dict(searched, kept, warp_dropped, median, p95, far): the errors against the analytic projection of the sphere
    point seen at kpts0."""
    P, R = SCENE_P, SCENE_R
    gray, valid = M.gray_of_scene(sc)
    src = M.usable_sources_ref(gray, valid, P, M.default_min_va(P))
    pix, _ = M.select_queries_ref(src[:1], SCENE_STEP, 4096)
    Rf, Tf = sc["R"].float(), sc["T"].float()
    if zbuf is None:
        zbuf = TU.raster_fp64(verts, faces, Rf, Tf, sc["K"], sc["H"], sc["W"])
    p = torch.from_numpy(pix[:, 1:3])
    fi, fj = torch.zeros(len(p), dtype=torch.int64), torch.ones(len(p), dtype=torch.int64)
    g, keep, _ = M.mesh_guesses_ref(fi, fj, p, zbuf, verts, faces, Rf, Tf, sc["K"])
    keep = keep.numpy()
    dropped = 0
    fwd = bwd = None
    if warp:
        _, X, n = surface_points(fi.numpy(), p.numpy(), zbuf, verts, faces, Rf, Tf, sc["K"])
        with np.errstate(all="ignore"):
            J = affines_fd(fi.numpy(), fj.numpy(), X, n, Rf, Tf, sc["K"])
            J = np.where(np.isfinite(J).all((1, 2))[:, None, None], J, 0.0)
            ok = affine_verdict(J)[0]
        dropped = int((keep & ~ok).sum())
        keep = keep & ok
        fwd, bwd = quantise(np.linalg.inv(J[keep])), quantise(J[keep])
    q = np.concatenate([np.zeros((len(p), 1), np.int64), np.ones((len(p), 1), np.int64), pix[:, 1:3], g.numpy()], 1)[keep]
    res = match_pairs_warp_ref(gray, valid, q, fwd, bwd, P, R) if warp else M.match_pairs_ref(gray, valid, q, P, R)
    k = res["keep"]
    out = {"searched": len(q), "kept": int(k.sum()), "warp_dropped": dropped, "median": None, "p95": None, "far": None}
    if k.any():
        X = sc["pts"][0][q[k, 3], q[k, 2]]
        u, w = (t.numpy() for t in M.project(X, sc["R"][1], sc["T"][1], sc["K"]))
        out["median"], out["p95"], out["far"] = M.error_stats(res["kpts1"][k], u, w)
    return out


def scene_errors(match, sc):
    """(median, p95, share beyond 1.5 px) of one match_frames entry of the pair (0, 1) against the analytic projection."""
    k0 = match["kpts0"].long()
    X = sc["pts"][0][k0[:, 1], k0[:, 0]]
    u, w = (t.numpy() for t in M.project(X, sc["R"][1], sc["T"][1], sc["K"]))
    return M.error_stats(match["kpts1"].numpy(), u, w)
