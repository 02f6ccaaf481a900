"""numpy restatement of the multi-view stereo pass (dynhor_amd/mvs.py, csrc/mvs.hip): the yardstick of the mvs tests.
tests/test_cpu_mvs.py licenses it before anything is compared with it.

sweep_ref / check_ref take the kernels' own inputs and a dtype.  float64 is the yardstick; float32 repeats the kernel's operations in the
kernel's order (every product and sum rounded once, the tap sums sequential in row-major order: numpy's cumsum adds in order), so its
deviation from float64 is the deviation the arithmetic itself causes: the margin of the GPU tests is four times it.

Ambiguity (sweep_ref's `amb`): a pixel one of whose validity decisions could flip under that deviation -- a tap whose four pixels change
validity when it moves by TOL_TAP px, vb within TOL_VB (relative) of min_vb, h_2 or z_k within TOL_Z of 1e-3, the guide's cosine within
TOL_COS of min_cos, z0 within TOL_Z of 1e-3.  argmax_ambiguous adds the pixels whose best score leads the next by less than a given gap.
"""
import numpy as np
import torch

from . import match_util as MU
from . import mesh_texture_util as TU
from . import pose_photo_util as PU

NONE = -2.0
Z_MIN = 1e-3
TOL_TAP = 2e-4          # px: a tap against a pixel boundary (fp32 pixel coordinates of a few tens carry ~1e-5)
TOL_VB = 1e-3           # relative: vb against min_vb (N sb2 - sb^2 cancels about four digits in fp32)
TOL_Z = 1e-6
TOL_COS = 1e-5
TOL_CHECK_PX = 1e-3     # dh_mvs_check: the projection against a rounding boundary
TOL_CHECK_REL = 1e-6    # dh_mvs_check: the depth ratio against depth_rel
AMBIGUOUS_CAP = 0.02
CHECK_AMBIGUOUS_CAP = 0.01
LOST = ("flags", "score", "margin", "refine", "consistency")


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _tap_valid(vj, tx, ty, H, W):
    """bool: the four pixels of the bilinear tap at (tx, ty) of the validity maps vj [n,H,W] (broadcast over [n,D,N]) are inside and valid."""
    with np.errstate(invalid="ignore"):
        inb = (tx >= 0) & (tx < W - 1) & (ty >= 0) & (ty < H - 1)
    x0 = np.floor(np.where(inb, tx, 0)).astype(np.int64)
    y0 = np.floor(np.where(inb, ty, 0)).astype(np.int64)
    ii = np.arange(vj.shape[0])[:, None, None]
    v = (vj[ii, y0, x0] != 0) & (vj[ii, y0, x0 + 1] != 0) & (vj[ii, y0 + 1, x0] != 0) & (vj[ii, y0 + 1, x0 + 1] != 0)
    return inb & v, inb, x0, y0


def sweep_ref(gray, valid, R, T, K, Kinv, pix, guide, nbr, D, step, P, min_va, min_vb, min_views, min_cos, dtype=np.float64, chunk=48, ambiguity=True):
    """dict(out_f dtype [n,4], out_i int32 [n,4], c dtype [n,D] (NONE where invalid), views int [n,D], amb bool [n]) of dh_mvs_sweep's
    rule on numpy inputs (gray, valid u8 [F,H,W]; R [F,9] or [F,3,3], T [F,3], K, Kinv [9] or [3,3]; pix int [n,3]; guide [n,4]; nbr int
    [F,Nn])."""
    dt = np.dtype(dtype).type
    F, H, W = gray.shape
    pix = np.asarray(pix, np.int64).reshape(-1, 3)
    guide = np.asarray(guide).reshape(-1, 4)
    n = len(pix)
    out = {"out_f": np.zeros((n, 4), dt), "out_i": np.zeros((n, 4), np.int32), "c": np.full((n, D), NONE, dt),
           "views": np.zeros((n, D), np.int64), "amb": np.zeros(n, bool)}
    for a0 in range(0, n, chunk):
        sl = slice(a0, min(n, a0 + chunk))
        part = _sweep_chunk(gray, valid, np.asarray(R).reshape(F, 3, 3).astype(dt), np.asarray(T).reshape(F, 3).astype(dt),
                            np.asarray(K).reshape(3, 3).astype(dt), np.asarray(Kinv).reshape(3, 3).astype(dt), pix[sl],
                            guide[sl].astype(dt), np.asarray(nbr, np.int64), int(D), dt(step), int(P), int(min_va), dt(min_vb),
                            int(min_views), dt(min_cos), dt, ambiguity)
        for k in out:
            out[k][sl] = part[k]
    return out


def _sweep_chunk(gray, valid, Rm, Tm, Km, Ki, pix, guide, nbr, D, step, P, min_va, min_vb, min_views, min_cos, dt, ambiguity=True):
    F, H, W = gray.shape
    S = 2 * P + 1
    N = S * S
    n = len(pix)
    fi, px, py = pix[:, 0], pix[:, 1], pix[:, 2]
    f_in = (fi >= 0) & (fi < F)
    fic = np.clip(fi, 0, F - 1)
    offs = np.arange(-P, P + 1, dtype=np.int64)
    ys, xs = py[:, None, None] + offs[None, :, None], px[:, None, None] + offs[None, None, :]
    inside = f_in[:, None, None] & (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    yc, xc = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
    aok = inside & (valid[fic[:, None, None], yc, xc] != 0)
    a = np.where(aok, gray[fic[:, None, None], yc, xc].astype(np.int64), 0).reshape(n, N)           # row-major taps
    sa, sa2 = a.sum(1), (a * a).sum(1)
    va = N * sa2 - sa * sa
    flags = np.where(~aok.reshape(n, N).all(1) | (va < min_va), 1, 0)
    zmin = dt(Z_MIN)
    fx, fy = px.astype(dt), py.astype(dt)
    e = [(Ki[r, 0] * fx + Ki[r, 1] * fy) + Ki[r, 2] for r in range(3)]
    z0, n0, n1, n2 = (guide[:, k] for k in range(4))
    with np.errstate(all="ignore"):
        cosv = -_dot3(n0, n1, n2, *e) / np.sqrt(_dot3(*e, *e))
        gbad = ~np.isfinite(z0) | ~(z0 > zmin) | ~(cosv >= min_cos)
        amb = np.isfinite(z0) & ((np.abs(z0 - Z_MIN) < TOL_Z) | (np.abs(cosv - min_cos) < TOL_COS)) & (flags == 0)
    flags = flags | np.where(gbad, 8, 0)
    live = flags == 0
    half = (D - 1) // 2
    kk = (np.arange(D) - half).astype(dt)
    with np.errstate(all="ignore"):
        zk = z0[:, None] + kk[None, :] * step                                                        # [n,D]
        X = [zk * e[r][:, None] for r in range(3)]
        d = _dot3(n0[:, None], n1[:, None], n2[:, None], *X)
        s = [n0[:, None] / d, n1[:, None] / d, n2[:, None] / d]
        hyp_ok = live[:, None] & (zk > zmin)
        amb |= live & (np.abs(zk - Z_MIN) < TOL_Z).any(1)
    csum = np.zeros((n, D), dt)
    views = np.zeros((n, D), np.int64)
    cc = np.tile(offs, S).astype(dt)                                                                 # the column offset of tap t = r S + c
    rr = np.repeat(offs, S).astype(dt)
    fN, fsa, fva = dt(N), sa.astype(dt), va.astype(dt)
    af = a.astype(dt)[:, None, :]
    Ri, Ti = Rm[fic], Tm[fic]
    for jn in range(nbr.shape[1]):
        j = nbr[fic, jn]
        jok = (j >= 0) & (j < F)
        jc = np.clip(j, 0, F - 1)
        Rj, Tj = Rm[jc], Tm[jc]
        with np.errstate(all="ignore"):
            Rij = [[_dot3(Rj[:, r, 0], Rj[:, r, 1], Rj[:, r, 2], Ri[:, c, 0], Ri[:, c, 1], Ri[:, c, 2]) for c in range(3)] for r in range(3)]
            t = [Tj[:, r] - _dot3(Rij[r][0], Rij[r][1], Rij[r][2], Ti[:, 0], Ti[:, 1], Ti[:, 2]) for r in range(3)]
            M = [[Rij[r][c][:, None] + t[r][:, None] * s[c] for c in range(3)] for r in range(3)]
            G = [[_dot3(Km[r, 0], Km[r, 1], Km[r, 2], M[0][c], M[1][c], M[2][c]) for c in range(3)] for r in range(3)]
            Hm = [[_dot3(G[r][0], G[r][1], G[r][2], Ki[0, c], Ki[1, c], Ki[2, c]) for c in range(3)] for r in range(3)]
            h = [(Hm[r][0] * fx[:, None] + Hm[r][1] * fy[:, None]) + Hm[r][2] for r in range(3)]
            ok = hyp_ok & jok[:, None] & (h[2] > zmin)
            amb |= (hyp_ok & jok[:, None] & (np.abs(h[2] - Z_MIN) < TOL_Z)).any(1)
            qx, qy = h[0] / h[2], h[1] / h[2]
            A00, A01 = (Hm[0][0] - qx * Hm[2][0]) / h[2], (Hm[0][1] - qx * Hm[2][1]) / h[2]
            A10, A11 = (Hm[1][0] - qy * Hm[2][0]) / h[2], (Hm[1][1] - qy * Hm[2][1]) / h[2]
            tx = qx[:, :, None] + (A00[:, :, None] * cc + A01[:, :, None] * rr)                      # [n,D,N]
            ty = qy[:, :, None] + (A10[:, :, None] * cc + A11[:, :, None] * rr)
        vj, gj = valid[jc], gray[jc]
        tv, inb, x0, y0 = _tap_valid(vj, tx, ty, H, W)
        strict, loose = tv.copy(), tv.copy()
        for ddx, ddy in ((-TOL_TAP, 0.0), (TOL_TAP, 0.0), (0.0, -TOL_TAP), (0.0, TOL_TAP)) if ambiguity else ():
            pv = _tap_valid(vj, tx.astype(np.float64) + ddx, ty.astype(np.float64) + ddy, H, W)[0]
            strict &= pv
            loose |= pv
        amb |= (ok & (strict.all(2) != loose.all(2))).any(1)
        nb_ok = ok & tv.all(2)
        ii = np.arange(n)[:, None, None]
        g00, g01 = gj[ii, y0, x0].astype(dt), gj[ii, y0, x0 + 1].astype(dt)
        g10, g11 = gj[ii, y0 + 1, x0].astype(dt), gj[ii, y0 + 1, x0 + 1].astype(dt)
        with np.errstate(all="ignore"):
            txs, tys = np.where(inb, tx, 0), np.where(inb, ty, 0)
            wx, wy = txs - np.floor(txs), tys - np.floor(tys)
            top, bot = g00 + wx * (g01 - g00), g10 + wx * (g11 - g10)
            b = top + wy * (bot - top)
            b = np.where(nb_ok[:, :, None], b, 0).astype(dt)
            sb = np.cumsum(b, axis=2, dtype=dt)[:, :, -1]
            sb2 = np.cumsum(b * b, axis=2, dtype=dt)[:, :, -1]
            sab = np.cumsum(af * b, axis=2, dtype=dt)[:, :, -1]
            vb = fN * sb2 - sb * sb
            amb |= (nb_ok & (np.abs(vb.astype(np.float64) - float(min_vb)) < TOL_VB * np.maximum(vb.astype(np.float64), float(min_vb)))).any(1)
            nb_ok = nb_ok & (vb >= min_vb)
            score = (fN * sab - fsa[:, None] * sb) / np.sqrt(fva[:, None] * vb)
            csum = np.where(nb_ok, csum + score, csum)
        views += nb_ok
    with np.errstate(all="ignore"):
        has = (views >= min_views) & (views > 0)
        c = np.where(has, csum / np.maximum(views, 1).astype(dt), dt(NONE))
    count = (c > -1.5).sum(1)
    kb = np.argmax(c, 1)                                                                             # the first maximum: the lowest k
    rows = np.arange(n)
    best = c[rows, kb]
    far = np.abs(np.arange(D)[None, :] - kb[:, None]) > 1
    sec = np.where(far, c, dt(NONE)).max(1)
    border = (kb == 0) | (kb == D - 1)
    cm, cp = c[rows, np.maximum(kb - 1, 0)], c[rows, np.minimum(kb + 1, D - 1)]
    with np.errstate(all="ignore"):
        den = (cm - dt(2) * best) + cp
        tt = np.clip((dt(0.5) * (cm - cp)) / den, dt(-0.5), dt(0.5))
    sub = np.where(~border & (cm > -1.5) & (cp > -1.5) & (den < 0), tt, dt(0)).astype(dt)
    z = z0 + ((kb - half).astype(dt) + sub) * step
    none = (flags != 0) | (count == 0)
    flags = np.where((flags == 0) & (count == 0), 2, flags)
    out_f = np.stack([z, best, sec, sub], 1).astype(dt)
    out_f[none] = (0, NONE, NONE, 0)
    out_i = np.stack([kb, views[rows, kb], np.where(none, flags, np.where(border, 4, 0)), count], 1).astype(np.int32)
    out_i[none, 0] = 0
    out_i[none, 1] = 0
    out_i[none, 3] = 0
    return {"out_f": out_f, "out_i": out_i, "c": c, "views": views, "amb": amb & live}


def argmax_ambiguous(c, gap):
    """bool [n]: the best c_k leads the best of the other hypotheses by less than `gap` (rows without two valid hypotheses: False)."""
    c = np.asarray(c, np.float64)
    srt = np.sort(c, 1)
    return (srt[:, -2] > -1.5) & (srt[:, -1] - srt[:, -2] < gap)


def check_ref(depth, R, T, K, Kinv, nbr, depth_rel, dtype=np.float64):
    """(count u8 [F,H,W], amb bool [F,H,W]) of dh_mvs_check's rule."""
    dt = np.dtype(dtype).type
    F, H, W = depth.shape
    Rm, Tm = np.asarray(R).reshape(F, 3, 3).astype(dt), np.asarray(T).reshape(F, 3).astype(dt)
    Km, Ki = np.asarray(K).reshape(3, 3).astype(dt), np.asarray(Kinv).reshape(3, 3).astype(dt)
    dz = np.asarray(depth).astype(dt)
    nbr = np.asarray(nbr, np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    fx, fy = xs.astype(dt), ys.astype(dt)
    count = np.zeros((F, H, W), np.uint8)
    amb = np.zeros((F, H, W), bool)
    rel = dt(depth_rel)
    for f in range(F):
        has = np.isfinite(dz[f])
        z = np.where(has, dz[f], dt(1))
        c = [z * ((Ki[r, 0] * fx + Ki[r, 1] * fy) + Ki[r, 2]) - Tm[f, r] for r in range(3)]
        X = [_dot3(Rm[f, 0, r], Rm[f, 1, r], Rm[f, 2, r], *c) for r in range(3)]
        for jn in range(nbr.shape[1]):
            j = int(nbr[f, jn])
            if j < 0 or j >= F:
                continue
            y = [_dot3(Rm[j, r, 0], Rm[j, r, 1], Rm[j, r, 2], *X) + Tm[j, r] for r in range(3)]
            with np.errstate(all="ignore"):
                front = has & (y[2] > dt(Z_MIN))
                uu = _dot3(Km[0, 0], Km[0, 1], Km[0, 2], *y) / y[2] + dt(0.5)
                ww = _dot3(Km[1, 0], Km[1, 1], Km[1, 2], *y) / y[2] + dt(0.5)
                u, w = np.floor(uu), np.floor(ww)
                ins = front & (u >= 0) & (u < W) & (w >= 0) & (w < H)
                ui, wi = np.where(ins, u, 0).astype(np.int64), np.where(ins, w, 0).astype(np.int64)
                zj = dz[j][wi, ui]
                ok = ins & np.isfinite(zj)
                agree = ok & (np.abs(y[2] - zj) <= rel * zj)
                near = (np.abs(uu - np.round(uu)) < TOL_CHECK_PX) | (np.abs(ww - np.round(ww)) < TOL_CHECK_PX)
                ratio = np.abs(np.abs(y[2] - zj) / zj - rel) < TOL_CHECK_REL
                amb[f] |= front & (near | (ok & ratio))
            count[f] += agree.astype(np.uint8)
    return count, amb


# ------------------------------------------------------------------------------------------------ the pieces in torch / numpy
def neighbours_ref(n, offsets=(1, 2)):
    offs = sorted(set(int(o) for o in offsets))
    out = -np.ones((n, 2 * len(offs)), np.int32)
    for i in range(n):
        for k, o in enumerate(offs):
            out[i, 2 * k] = i - o if i - o >= 0 else -1
            out[i, 2 * k + 1] = i + o if i + o < n else -1
    return out


def normals_ref(depth, kept, Kinv, depth_rel=0.01, step=1):
    """(normal f64 [H,W,3], ok bool [H,W]) of one depth map by a plain loop over the pixels."""
    H, W = depth.shape
    Ki = np.asarray(Kinv, np.float64).reshape(3, 3)
    n = np.zeros((H, W, 3))
    ok = np.zeros((H, W), bool)
    P = lambda x, y: depth[y, x] * (Ki @ np.array([x, y, 1.0]))
    s = step
    for y, x in zip(*np.nonzero(kept)):
        if y < s or y >= H - s or x < s or x >= W - s:
            continue
        for _ in (0,):
            if not (kept[y, x] and kept[y, x - s] and kept[y, x + s] and kept[y - s, x] and kept[y + s, x]):
                continue
            z = depth[y, x]
            if abs(depth[y, x + s] - depth[y, x - s]) > depth_rel * z or abs(depth[y + s, x] - depth[y - s, x]) > depth_rel * z:
                continue
            m = np.cross(P(x + s, y) - P(x - s, y), P(x, y + s) - P(x, y - s))
            if np.linalg.norm(m) == 0:
                continue
            m = m / np.linalg.norm(m)
            n[y, x] = -m if m @ P(x, y) > 0 else m
            ok[y, x] = True
    return n, ok


def icosphere(r, level=3):
    """(verts f32 [V,3], faces int64 [M,3]) of an icosahedron subdivided `level` times, on the sphere of radius r."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return torch.tensor(np.stack(v) * r, dtype=torch.float32), torch.tensor(f, dtype=torch.int64)


def sphere_guide(R, T, K, H, W, r):
    """f64 [F,H,W,4] = (z0, n) of the analytic sphere |p| = r in every camera: what guide_from_mesh gives for a mesh without facets;
    NaN where a pixel misses it."""
    hit, pts, depth = PU.sphere_hits(R, T, K, H, W, r)
    n_cam = torch.einsum("fij,fhwj->fhwi", R.double(), pts / r)
    g = torch.cat([depth[..., None], n_cam], -1)
    return torch.where(hit[..., None], g, torch.full_like(g, float("nan")))


# ------------------------------------------------------------------------------------------------ the pipeline
def depth_maps_ref(gray, valid, src_ok, guide, R, T, K, Kinv, nbr, frames, dtype=np.float64, patch=4, rng=0.04, depths=33, fine_depths=9,
                   step_px=1, min_va=None, min_vb=None, min_views=2, min_cos=0.2, score_min=0.6, peak_margin=0.02, depth_rel=0.01,
                   min_consistent=2):
    """dict(depth f64 [F,H,W] NaN where not kept, kept, lost u8 [F,H,W] (1 + index into LOST), swept bool, score) of mvs.depth_maps'
    passes and gates for the frames `frames`, from numpy inputs: gray, valid, src_ok [F,H,W], guide [F,H,W,4] (NaN where none)."""
    F, H, W = gray.shape
    min_va = MU.default_min_va(patch) if min_va is None else min_va
    min_vb = float(min_va) if min_vb is None else min_vb
    step1 = 2.0 * rng / (depths - 1)
    depth = np.full((F, H, W), np.nan)
    score = np.full((F, H, W), np.nan)
    lost = np.zeros((F, H, W), np.uint8)
    swept = np.zeros((F, H, W), bool)
    for f in frames:
        m = np.zeros((H, W), bool)
        m[::step_px, ::step_px] = True
        y, x = np.nonzero(src_ok[f] & m)
        pix = np.stack([np.full_like(x, f), x, y], 1)
        gd = np.asarray(guide[f][y, x], np.float32)
        a = sweep_ref(gray, valid, R, T, K, Kinv, pix, gd, nbr, depths, np.float32(step1), patch, min_va, np.float32(min_vb), min_views,
                      np.float32(min_cos), dtype)
        f1, i1 = a["out_f"].astype(np.float64), a["out_i"]
        why = np.zeros(len(pix), np.uint8)
        why[i1[:, 2] != 0] = 1
        why[(why == 0) & ~(f1[:, 1] >= np.float32(score_min))] = 2
        why[(why == 0) & ~(f1[:, 1] - f1[:, 2] >= np.float32(peak_margin))] = 3
        sel = np.nonzero(why == 0)[0]
        gd2 = gd[sel].copy()
        gd2[:, 0] = a["out_f"][sel, 0].astype(np.float32)
        b = sweep_ref(gray, valid, R, T, K, Kinv, pix[sel], gd2, nbr, fine_depths, np.float32(0.25 * step1), patch, min_va,
                      np.float32(min_vb), min_views, np.float32(min_cos), dtype)
        bad2 = b["out_i"][:, 2] != 0
        why[sel[bad2]] = 4
        swept[f, y, x] = True
        lost[f, y, x] = why
        good = sel[~bad2]
        depth[f, y[good], x[good]] = b["out_f"][~bad2, 0]
        score[f, y[good], x[good]] = b["out_f"][~bad2, 1]
    if min_consistent > 0:
        sp = step_px
        Ks = (np.diag([1.0 / sp, 1.0 / sp, 1.0]) @ np.asarray(K, np.float64).reshape(3, 3)).astype(np.float32)
        Ksi = np.linalg.inv(Ks.astype(np.float64)).astype(np.float32)
        count = np.zeros((F, H, W), np.uint8)
        count[:, ::sp, ::sp] = check_ref(depth[:, ::sp, ::sp].astype(np.float32), R, T, Ks, Ksi, nbr, np.float32(depth_rel), dtype)[0]
        drop = np.isfinite(depth) & (count < min_consistent)
        lost[drop] = 5
        depth[drop] = np.nan
    return {"depth": depth, "kept": np.isfinite(depth), "lost": lost, "swept": swept, "score": score}


def f32_inputs(sc):
    """(R f32 [F,9], T f32 [F,3], K f32 [9], Kinv f32 [9]) numpy arrays of a match_util scene, rounded as Dataset rounds them."""
    R = sc["R"].float().reshape(-1, 9).numpy()
    T = sc["T"].float().reshape(-1, 3).numpy()
    K = sc["K"].float()
    Kinv = torch.inverse(K.double()).float()
    return R, T, K.reshape(9).numpy(), Kinv.reshape(9).numpy()


# ------------------------------------------------------------------------------------------------ the scenes of the GPU tests
CASES = ((1, 3, 1), (4, 9, 2), (4, 33, 4), (7, 63, 8))           # (P, D, Nn)
KH, KW, KF = 40, 48, 5
K_STEPS = {3: 0.2, 9: 0.08, 33: 0.03, 63: 0.02}      # per D: the sweep spans about +-0.5 of the unit distance to the plane
E2E_DEGS = (-12.0, -6.0, 0.0, 6.0, 12.0)
E2E_STEP_PX = 4
E2E_FRAMES = (1, 2, 3)
E2E_MARGIN = 0.002                                             # a peak_margin inside the sphere scene's spread of c_best - c_second
SPHERE_E2E_R = TU.SPHERE_R


def plane_scene(seed=0, H=KH, W=KW, F=KF):
    """A textured plane z = 0 of the object frame seen by F cameras about one unit away, 0.15 apart along x and slightly turned: gray,
    valid u8 [F,H,W] (a hole and a ragged strip invalid, a flat block in frame 2), R, T fp64, K, and per frame the true camera depth and
    the plane's camera-frame normal."""
    from . import pose_sil_util as SU
    g = np.random.default_rng(seed)
    ph = g.random(6) * 6.0
    tex = lambda X, Y: (128 + 45 * np.sin(40.0 * X + ph[0]) * np.cos(33.0 * Y + ph[1]) + 35 * np.sin(19.0 * X + 27.0 * Y + ph[2])
                        + 25 * np.cos(61.0 * X - 13.0 * Y + ph[3]))
    f = 1.2 * min(H, W)
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float64)
    Ki = np.linalg.inv(K)
    ys, xs = np.mgrid[0:H, 0:W]
    e = np.stack([xs, ys, np.ones_like(xs)], -1) @ Ki.T
    Rs, Ts, grays, zs, ns = [], [], [], [], []
    for i in range(F):
        R = SU.axis_angle((0.2, 1.0, 0.1), 3.0 * (i - F // 2)).numpy() @ SU.axis_angle((1.0, 0.0, 0.0), 180.0).numpy()
        C = np.array([0.15 * (i - F // 2), 0.02 * i, 1.0 + 0.03 * i])          # the camera centre, in front of the plane (looking down -z)
        T = -R @ C
        d = e @ R                                                               # R^T e per pixel
        s = -C[2] / d[..., 2]                                                   # C + s R^T e on z = 0
        X = C + s[..., None] * d
        grays.append(np.clip(np.floor(tex(X[..., 0], X[..., 1]) + 0.5), 0, 255).astype(np.uint8))
        zs.append(s)
        n = R @ np.array([0.0, 0.0, 1.0])
        ns.append(n if n[2] < 0 else -n)
        Rs.append(R)
        Ts.append(T)
    gray = np.stack(grays)
    valid = np.ones_like(gray)
    valid[1, 14:19, 20:27] = 0
    valid[3, :, 40:] = (g.random((H, W - 40)) < 0.5).astype(np.uint8)
    valid[2, 30, 12] = 0
    gray[2, 4:22, 30:46] = 140
    gray = np.where(valid != 0, gray, 0).astype(np.uint8)
    return {"gray": gray, "valid": valid, "R": np.stack(Rs), "T": np.stack(Ts), "K": K, "z": np.stack(zs), "n": np.stack(ns), "H": H, "W": W}


def kernel_nbr(F, Nn):
    """int32 [F,Nn]: i + 1 (Nn 1), i -+ 1 (2), i -+ 1, 2 (4), i -+ 1 .. 4 (8); the last frame's row is all -1."""
    nbr = -np.ones((F, Nn), np.int32)
    offs = [1] if Nn == 1 else [o for k in range(1, Nn // 2 + 1) for o in (-k, k)]
    for i in range(F - 1):
        for c, o in enumerate(offs):
            if 0 <= i + o < F:
                nbr[i, c] = i + o
    return nbr


def kernel_case(case, seed=0):
    """The inputs of one (P, D, Nn) comparison on plane_scene: dict(args = sweep_ref's positional arguments, all as the kernel takes them
    (float32 poses), n).  Pixels: a grid of step 4 and every third border pixel of frame 2, a coarser grid of the other frames (frame 4
    has no neighbours; frame 0 lacks the earlier ones), and nine special guides: NaN z0, inf z0, z0 below 1e-3, a sweep that crosses
    1e-3, a grazing normal, a normal facing away, a zero normal, a far guide, a NaN normal."""
    P, D, Nn = case
    K_STEP = K_STEPS[D]
    sc = plane_scene(seed)
    H, W, F = sc["H"], sc["W"], len(sc["R"])
    g = np.random.default_rng(100 + seed)
    rows = [(2, x, y) for y in range(0, H, 4) for x in range(0, W, 4)]
    ring = [(x, 0) for x in range(W)] + [(W - 1, y) for y in range(H)] + [(x, H - 1) for x in range(W)] + [(0, y) for y in range(H)]
    rows += [(2, x, y) for x, y in ring[::3]]
    for f in (0, 1, 3, 4):
        rows += [(f, x, y) for y in range(8, H - 8, 8) for x in range(8, W - 8, 8)]
    pix = np.array(rows[::2] if D * Nn > 200 else rows, np.int64)       # the largest case on every other pixel: the restatement's time
    n = len(pix)
    z_true = sc["z"][pix[:, 0], pix[:, 2], pix[:, 1]]
    z0 = z_true + K_STEP * g.uniform(-0.3 * D, 0.3 * D, n)
    nrm = sc["n"][pix[:, 0]] + g.normal(0, 0.08, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    guide = np.concatenate([z0[:, None], nrm], 1)
    mid = np.array([2, 22, 26])
    special = [(np.nan, sc["n"][2]), (np.inf, sc["n"][2]), (0.0005, sc["n"][2]), (0.0012 + K_STEP * ((D - 1) // 2 - 1), sc["n"][2]),
               (1.0, (0.995, 0.0, -0.0998)), (1.0, -sc["n"][2]), (1.0, (0.0, 0.0, 0.0)), (40.0, sc["n"][2]), (1.0, (np.nan, 0.0, -1.0))]
    pix = np.concatenate([pix, np.tile(mid, (len(special), 1))])
    guide = np.concatenate([guide, np.array([[z, *v] for z, v in special])])
    R32, T32 = sc["R"].astype(np.float32).reshape(F, 9), sc["T"].astype(np.float32)
    K32 = sc["K"].astype(np.float32).reshape(9)
    Ki32 = np.linalg.inv(sc["K"].astype(np.float32).astype(np.float64)).astype(np.float32).reshape(9)
    S = 2 * P + 1
    min_va = 4 * S ** 4
    args = (sc["gray"], sc["valid"], R32, T32, K32, Ki32, pix, guide.astype(np.float32), kernel_nbr(F, Nn), D, np.float32(K_STEP), P, min_va,
            np.float32(min_va), min(2, Nn), np.float32(0.2))
    return {"args": args, "n": len(pix), "scene": sc}


CHECK_OFFSETS = ((1,), (2,), (1, 2))
CHECK_NO_DEPTH = {(1,): 0.1, (2,): 0.1, (1, 2): 0.45}           # the share of pixels without a depth


def check_case(offsets, seed=3):
    """(depth f32 [F,H,W], R, T, K, Kinv float32, nbr) for dh_mvs_check on plane_scene: the true depth, a tenth of the pixels moved by up
    to 3 %, CHECK_NO_DEPTH[offsets] of them without depth, one inf; the neighbours i -+ o for the given offsets.  Every projection of a
    pixel with a depth has two chances of lying within TOL_CHECK_PX of a rounding boundary: with four neighbours and a tenth without
    depth 1.1 % of the pixels are ambiguous, so the four-neighbour case (the pipeline's default) has sparser maps, as kept depths are."""
    sc = plane_scene()
    g = np.random.default_rng(seed)
    depth = sc["z"].astype(np.float32)
    moved = g.random(depth.shape) < 0.1
    depth = np.where(moved, depth * (1 + g.uniform(-0.03, 0.03, depth.shape)), depth).astype(np.float32)
    depth[g.random(depth.shape) < CHECK_NO_DEPTH[tuple(offsets)]] = np.nan
    depth[1, 5, 5] = np.inf
    K32 = sc["K"].astype(np.float32)
    return (depth, sc["R"].astype(np.float32), sc["T"].astype(np.float32), K32, np.linalg.inv(K32.astype(np.float64)).astype(np.float32),
            neighbours_ref(len(depth), offsets))


def e2e_scene():
    """match_util.turned_sphere at five poses 6 degrees apart, textured by pattern(36): a period near the 9 px patch."""
    return MU.turned_sphere(E2E_DEGS, k=36)
