"""The rule of dh_ray_depth / dh_warp_loss / dh_ray_depth_bwd (include/dynhor_hip.h) restated in torch on the CPU, dtype as a parameter.

  * float32: the tap coordinates follow the kernel's operation order, one IEEE operation per torch operation, so floor tx, floor ty -- the
    cells -- equal the kernel's bit for bit.  Its deviation from the fp64 form is the error the kernel is allowed four times of
    (tests/ray_kernels_util.py: ErrorLedger).
  * float64: takes the cells from the float32 form and makes no floor of its own (a tap 1e-6 px from a pixel boundary would otherwise
    flip its one-sided derivative); z and n may require grad, and autograd of sum_r l_r gives g_z, g_n per ray, the rays being
    independent.  It also reports the rays whose discrete outcome lies within rounding (`amb`).
tests/test_cpu_warp_loss.py licenses it: its autograd gradient equals central differences of itself.
"""
from types import SimpleNamespace

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
NONE = -2.0
Z_MIN = 1e-3
TOL_PX = 1e-4          # a tap this close to 0, W - 1 or H - 1 may be inside in one arithmetic and outside in the other
TOL_TOPK = 1e-5        # two l_j this close at the top-k boundary may swap
TOL_COS = 1e-5
TOL_H2 = 1e-6
TOL_VB_REL = 1e-5      # of N sum b^2: the fp32 form's N sb2 - sb sb carries a few 1e-7 of either term


def settings(patch=5, topk=4, min_views=2, min_cos=0.1, min_wsum=0.5, min_va=None, min_vb=None):
    N = (2 * patch + 1) ** 2
    min_va = 4 * N * N if min_va is None else int(min_va)
    return SimpleNamespace(patch=int(patch), topk=int(topk), min_views=int(min_views), min_cos=float(min_cos), min_wsum=float(min_wsum),
                           min_va=min_va, min_vb=float(min_va if min_vb is None else min_vb))


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def warp_rule(gray, valid, R, T, K, Kinv, nbr, frame, pix, z, wsum, n, st, dtype=F64, cells=None):
    """gray, valid u8 [F,H,W]; R [F,3,3] or [F,9], T [F,3], K, Kinv [9] float32 tensors; nbr int [F,Nn]; pix int [B,2]; z [B], wsum [B],
    n [B,3] (float32 values; as float64 leaves they may require grad).  cells: the float32 form's result["cells"] (None: this form's own
    floors).  Returns a dict: l, score, best [B] dtype (0, NONE, NONE on rays that do not count), valid_n, chosen_n, flags, mask int64 [B],
    lj [B,Nn] (inf: invalid), cells, amb bool [B], margin f64 [B] (the least distance of a tap from a cell boundary), stats (L, count, mean score, rays with flag 1, 2, 8, 16) as python floats."""
    D = dtype
    Fn, H, W = gray.shape
    B = pix.shape[0]
    P = st.patch
    S = 2 * P + 1
    N = S * S
    Rm = R.reshape(Fn, 9).to(D)
    Tm = T.reshape(Fn, 3).to(D)
    Km, Ki = K.reshape(9).to(D), Kinv.reshape(9).to(D)
    nbr = torch.as_tensor(nbr).long()
    Nn = nbr.shape[1]
    px, py = pix[:, 0].long(), pix[:, 1].long()
    ti = torch.arange(N)
    cx, ry = ti % S - P, ti // S - P
    g64, v64 = gray.long(), valid.long()

    # ---- source
    xs, ys = px[:, None] + cx[None], py[:, None] + ry[None]
    inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    xc, yc = xs.clamp(0, W - 1), ys.clamp(0, H - 1)
    ok = inside & (v64[frame][yc, xc] != 0)
    a_i = torch.where(ok, g64[frame][yc, xc], torch.zeros_like(xc))
    sa, sa2 = a_i.sum(1), (a_i * a_i).sum(1)
    va = N * sa2 - sa * sa
    flags = torch.zeros(B, dtype=torch.long)
    flags |= ((~ok.all(1)) | (va < st.min_va)).long()
    flags |= (~(wsum.float() >= torch.tensor(st.min_wsum, dtype=F32))).long() * 16

    # ---- plane
    zz, nn_ = z.to(D), n.to(D)
    fx, fy = px.to(D), py.to(D)
    e = [(Ki[3 * r] * fx + Ki[3 * r + 1] * fy) + Ki[3 * r + 2] for r in range(3)]
    Ri = Rm[frame]
    nc = [_dot3(Ri[3 * r], Ri[3 * r + 1], Ri[3 * r + 2], nn_[:, 0], nn_[:, 1], nn_[:, 2]) for r in range(3)]
    ne = _dot3(*nc, *e)
    nlen, elen = torch.sqrt(_dot3(*nc, *nc)), torch.sqrt(_dot3(*e, *e))
    cosv = -ne / (nlen * elen)
    with torch.no_grad():
        plane_ok = torch.isfinite(zz) & (zz > Z_MIN) & (nlen > 1e-6) & (cosv >= st.min_cos)
        flags |= (~plane_ok).long() * 8
        amb = plane_ok & ((cosv - st.min_cos).abs() < TOL_COS)
        live = flags == 0
    # rays with a flag run through the arithmetic on harmless stand-ins, and are masked out of every result
    zs = torch.where(live, zz, torch.ones_like(zz))
    g = zs * torch.where(live, ne, -torch.ones_like(ne))

    # ---- taps
    x = (px[:, None] + cx[None]).to(D)
    y = (py[:, None] + ry[None]).to(D)
    u = [(Ki[3 * r] * x + Ki[3 * r + 1] * y) + Ki[3 * r + 2] for r in range(3)]
    sg = _dot3(nc[0][:, None], nc[1][:, None], nc[2][:, None], *u) / g[:, None]
    sg = torch.where(live[:, None], sg, torch.ones_like(sg))
    a = a_i.to(D)
    fsa, fva, fN = sa.to(D), va.to(D), float(N)

    lj = torch.full((B, Nn), float("inf"), dtype=D)
    scj = torch.full((B, Nn), NONE, dtype=D)
    out_cells = []
    margin = torch.full((B,), 0.5, dtype=F64)          # the least distance of a tap of a valid neighbour from a cell boundary, in px
    Ti = Tm[frame]
    for jn in range(Nn):
        j = int(nbr[frame, jn])
        if j < 0 or j >= Fn:
            out_cells.append(None)
            continue
        Rj, Tj = Rm[j], Tm[j]
        Rij = [[_dot3(Rj[3 * r], Rj[3 * r + 1], Rj[3 * r + 2], Ri[3 * c], Ri[3 * c + 1], Ri[3 * c + 2]) for c in range(3)] for r in range(3)]
        t = [Tj[r] - _dot3(Rij[r][0], Rij[r][1], Rij[r][2], Ti[0], Ti[1], Ti[2]) for r in range(3)]
        G = [[_dot3(Km[3 * r], Km[3 * r + 1], Km[3 * r + 2], Rij[0][c], Rij[1][c], Rij[2][c]) for c in range(3)] for r in range(3)]
        A = [[_dot3(G[r][0], G[r][1], G[r][2], Ki[c], Ki[3 + c], Ki[6 + c]) for c in range(3)] for r in range(3)]
        bv = [_dot3(Km[3 * r], Km[3 * r + 1], Km[3 * r + 2], t[0], t[1], t[2]) for r in range(3)]
        h = [((A[r][0] * x + A[r][1] * y) + A[r][2]) + bv[r] * sg for r in range(3)]
        with torch.no_grad():
            h_ok = h[2] > Z_MIN
        h2 = torch.where(h_ok, h[2], torch.ones_like(h[2]))
        tx, ty = h[0] / h2, h[1] / h2
        with torch.no_grad():
            inb = h_ok & (tx >= 0) & (tx < W - 1) & (ty >= 0) & (ty < H - 1)
            if cells is None:
                cxj = torch.floor(torch.where(inb, tx, torch.zeros_like(tx))).long()
                cyj = torch.floor(torch.where(inb, ty, torch.zeros_like(ty))).long()
            else:
                cxj, cyj = cells[jn]
            cxj, cyj = cxj.clamp(0, W - 2), cyj.clamp(0, H - 2)
            vj, gj = v64[j], g64[j]
            tap_ok = inb & (vj[cyj, cxj] != 0) & (vj[cyj, cxj + 1] != 0) & (vj[cyj + 1, cxj] != 0) & (vj[cyj + 1, cxj + 1] != 0)
            g00, g01, g10, g11 = (gj[cyj, cxj].to(D), gj[cyj, cxj + 1].to(D), gj[cyj + 1, cxj].to(D), gj[cyj + 1, cxj + 1].to(D))
            near_edge = (h[2] - Z_MIN).abs() < TOL_H2
            near_edge |= h_ok & ((tx.abs() < TOL_PX) | ((tx - (W - 1)).abs() < TOL_PX) | (ty.abs() < TOL_PX) | ((ty - (H - 1)).abs() < TOL_PX))
            amb |= live & near_edge.any(1)
        out_cells.append((cxj, cyj))
        wx, wy = tx - cxj.to(D), ty - cyj.to(D)
        top, bot = g00 + wx * (g01 - g00), g10 + wx * (g11 - g10)
        b = top + wy * (bot - top)
        b = torch.where(tap_ok, b, torch.zeros_like(b))
        sb, sb2, sab = b.sum(1), (b * b).sum(1), (a * b).sum(1)
        vb = fN * sb2 - sb * sb
        with torch.no_grad():
            all_ok = live & tap_ok.all(1)
            j_ok = all_ok & (vb >= st.min_vb)
            amb |= all_ok & ((vb - st.min_vb).abs() < TOL_VB_REL * fN * sb2)
            fr = torch.minimum(torch.minimum(wx, 1 - wx), torch.minimum(wy, 1 - wy)).min(1).values.double()
            margin = torch.where(j_ok, torch.minimum(margin, fr), margin)
        vbs = torch.where(j_ok, vb, torch.ones_like(vb))
        fvas = torch.where(j_ok, fva, torch.ones_like(fva))
        score = (fN * sab - fsa * sb) / torch.sqrt(fvas * vbs)
        col = torch.zeros(B, Nn, dtype=torch.bool)
        col[:, jn] = j_ok
        lj = torch.where(col, (1.0 - score)[:, None], lj)
        scj = torch.where(col, score[:, None], scj)

    # ---- the ray
    with torch.no_grad():
        nvalid = torch.isfinite(lj).sum(1)
        counts = live & (nvalid >= st.min_views) & (nvalid > 0)
        kk = torch.clamp(nvalid, max=st.topk)
        srt, order = torch.sort(lj.detach(), dim=1, stable=True)                  # ties: the earlier entry of nbr first
        rank = torch.empty_like(order)
        rank.scatter_(1, order, torch.arange(Nn)[None].expand(B, Nn).contiguous())
        chosen = counts[:, None] & torch.isfinite(lj) & (rank < kk[:, None])
        if Nn > 1:
            lo = srt.gather(1, (kk - 1).clamp(min=0)[:, None])[:, 0]
            hi = srt.gather(1, kk.clamp(max=Nn - 1)[:, None])[:, 0]
            amb |= counts & (nvalid > kk) & ((hi - lo) < TOL_TOPK)
        flags = torch.where(live & ~counts, torch.full_like(flags, 2), flags)
        mask = (chosen.long() << torch.arange(Nn)[None]).sum(1)
        kks = torch.where(counts, kk, torch.ones_like(kk)).to(D)
    zero = torch.zeros((), dtype=D)
    l = torch.where(chosen, lj, zero).sum(1) / kks
    sc = torch.where(chosen, scj, zero).sum(1) / kks
    l = torch.where(counts, l, zero)
    sc = torch.where(counts, sc, torch.full_like(sc, NONE))
    best = torch.where(counts, scj.max(1).values, torch.full_like(sc, NONE))
    cnt = int(counts.sum())
    stats = (float(l.detach().sum()) / max(cnt, 1), float(cnt), float(torch.where(counts, sc.detach(), zero).sum()) / max(cnt, 1),
             float((flags & 1).ne(0).sum()), float((flags & 2).ne(0).sum()), float((flags & 8).ne(0).sum()), float((flags & 16).ne(0).sum()))
    return {"l": l, "score": sc, "best": best, "valid_n": nvalid, "chosen_n": torch.where(counts, kk, torch.zeros_like(kk)), "flags": flags,
            "mask": mask, "lj": lj, "cells": out_cells, "amb": amb, "counts": counts, "stats": stats, "margin": margin}


def warp_eval(gray, valid, R, T, K, Kinv, nbr, frame, pix, z, wsum, n, st, dtype=F64, cells=None, grad=True):
    """warp_rule plus g_z [B], g_n [B,3] by autograd of sum_r l_r (the float32 form differentiates itself: the error yardstick)."""
    zz = z.detach().to(dtype).clone().requires_grad_(grad)
    nn_ = n.detach().to(dtype).clone().requires_grad_(grad)
    r = warp_rule(gray, valid, R, T, K, Kinv, nbr, frame, pix, zz, wsum, nn_, st, dtype, cells)
    if grad:
        tot = r["l"].sum()
        if tot.requires_grad:
            gz, gn = torch.autograd.grad(tot, (zz, nn_), allow_unused=True)
        else:
            gz = gn = None
        r["g_z"] = torch.zeros_like(zz) if gz is None else torch.nan_to_num(gz, nan=0.0, posinf=0.0, neginf=0.0)
        r["g_n"] = torch.zeros_like(nn_) if gn is None else torch.nan_to_num(gn, nan=0.0, posinf=0.0, neginf=0.0)
        keep = r["counts"]
        r["g_z"] = torch.where(keep, r["g_z"], torch.zeros_like(r["g_z"]))
        r["g_n"] = torch.where(keep[:, None], r["g_n"], torch.zeros_like(r["g_n"]))
    r["l"], r["score"], r["best"] = r["l"].detach(), r["score"].detach(), r["best"].detach()
    return r


def both_forms(*args, **kw):
    """(r64, r32): the float32 form, then the float64 form on its cells."""
    r32 = warp_eval(*args, dtype=F32, **kw)
    r64 = warp_eval(*args, dtype=F64, cells=r32["cells"], **kw)
    return r64, r32


def discrete_equal(a, b):
    """bool [B]: two results agree in flags, valid neighbours, chosen count and the chosen bitmask."""
    return (a["flags"] == b["flags"]) & (a["valid_n"] == b["valid_n"]) & (a["chosen_n"] == b["chosen_n"]) & (a["mask"] == b["mask"])


# ------------------------------------------------------------------------------------------------ ray depth
def mids(z, sample_dist):
    """m_k of a dense row [B,n] (dh_prior_loss's): z_k + 0.5 (z_{k+1} - z_k), sample_dist for the last interval; in z's dtype."""
    dz = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], sample_dist)], 1)
    return z + 0.5 * dz


def ray_depth_dense(rays, R, z, weights, sample_dist, dtype=F64):
    """(t, W, zc) [B] of dh_ray_depth in `dtype`; weights may require grad.  m_k is formed in float32 as the kernel does."""
    m = mids(z.float(), float(torch.tensor(sample_dist, dtype=F32))).to(dtype)
    w = weights.to(dtype)
    W = w.sum(1)
    t = (w * m).sum(1) / W
    Rm = R.reshape(9).to(dtype)
    d = rays[:, 3:6].to(dtype)
    cz = Rm[6] * d[:, 0] + Rm[7] * d[:, 1] + Rm[8] * d[:, 2]
    return t, W, t * cz


def ray_depth_packed(rays, R, t_start, weights, off, cnt, max_samples, step, dtype=F64):
    """The packed form: ray r owns [off[r], off[r] + min(cnt[r], max_samples)); m_k = t_start_k + 0.5 step in float32; a ray without a
    sample gives (0, 0, 0)."""
    B = rays.shape[0]
    step32 = torch.tensor(step, dtype=F32)
    m_all = (t_start.float() + 0.5 * step32).to(dtype)
    w_all = weights.to(dtype)
    Rm = R.reshape(9).to(dtype)
    ts, Ws, zs = [], [], []
    for r in range(B):
        c = min(max(int(cnt[r]), 0), max_samples)
        o = int(off[r])
        d = rays[r, 3:6].to(dtype)
        cz = Rm[6] * d[0] + Rm[7] * d[1] + Rm[8] * d[2]
        if c == 0:
            zero = (w_all[:0]).sum()
            ts.append(zero); Ws.append(zero); zs.append(zero)
            continue
        w, m = w_all[o:o + c], m_all[o:o + c]
        W = w.sum()
        t = (w * m).sum() / W
        ts.append(t); Ws.append(W); zs.append(t * cz)
    return torch.stack(ts), torch.stack(Ws), torch.stack(zs)


# ------------------------------------------------------------------------------------------------ scenes of the kernel tests
def plane_case(H, W, F, seed=0, hand=True):
    """mvs_util.plane_scene at H x W with F frames and a hand: a disc of invalid pixels that moves from frame to frame.  Returns float32
    torch tensors as the kernel takes them, plus the true camera depth z [F,H,W] and the plane's object-frame normal per frame."""
    from . import mvs_util as VU
    sc = VU.plane_scene(seed=seed, H=H, W=W, F=F)
    gray, valid = sc["gray"].copy(), sc["valid"].copy()
    if hand:
        ys, xs = np.mgrid[0:H, 0:W]
        for i in range(F):
            cx, cy = 0.2 * W + 0.05 * W * i, 0.75 * H - 0.03 * H * i
            disc = (xs - cx) ** 2 + (ys - cy) ** 2 <= (0.09 * min(H, W)) ** 2
            valid[i][disc] = 0
        gray = np.where(valid != 0, gray, 0).astype(np.uint8)
    R = torch.from_numpy(sc["R"]).float().reshape(F, 9)
    T = torch.from_numpy(sc["T"]).float()
    K = torch.from_numpy(sc["K"]).float().reshape(9)
    Kinv = torch.inverse(torch.from_numpy(sc["K"]).double()).float().reshape(9)
    n_obj = torch.stack([torch.from_numpy(sc["R"][i].T @ sc["n"][i]).float() for i in range(F)])
    return {"gray": torch.from_numpy(gray), "valid": torch.from_numpy(valid), "R": R, "T": T, "K": K, "Kinv": Kinv,
            "z": torch.from_numpy(sc["z"]).float(), "n_obj": n_obj, "H": H, "W": W, "F": F}


def random_rays(case, frame, B, seed, margin, dz=0.01, dn=0.05):
    """B rays of `frame`: pixels at least `margin` from the border, the true depth moved by up to +-dz, the true normal tilted by noise
    of size dn and scaled to a length in [0.5, 1.5], wsum in [0.6, 1]."""
    g = torch.Generator().manual_seed(seed)
    H, W = case["H"], case["W"]
    px = torch.randint(margin, W - margin, (B,), generator=g)
    py = torch.randint(margin, H - margin, (B,), generator=g)
    z = case["z"][frame][py, px] + dz * (2 * torch.rand(B, generator=g) - 1)
    n = case["n_obj"][frame][None] + dn * torch.randn(B, 3, generator=g)
    n = n / n.norm(dim=1, keepdim=True) * (0.5 + torch.rand(B, 1, generator=g))
    wsum = 0.6 + 0.4 * torch.rand(B, generator=g)
    return torch.stack([px, py], 1).int(), z.float().contiguous(), wsum.float(), n.float().contiguous()
