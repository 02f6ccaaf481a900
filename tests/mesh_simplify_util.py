"""Plain-torch restatement of the quadric vertex clustering of dynhor_amd/mesh_simplify.py, written from its specification: fp32 for
the grid as stated, fp64 for everything else, every sum sequential in ascending record order.  Runs on the CPU and shares no code with
the product.  Also the small meshes the simplification tests are built from."""
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
N_SUMS = 17


def grid(verts: torch.Tensor, cells: int):
    """(lo fp32 [3], h fp32 scalar tensor, dims list of 3 ints): every operation a single fp32 IEEE operation."""
    v = verts.detach().cpu().to(F32)
    lo, hi = v.min(dim=0).values, v.max(dim=0).values
    ext = hi - lo
    h = ext.max() / torch.tensor(float(cells), dtype=F32)
    if float(h) > 0.0:
        dims = [max(1, int(torch.ceil(ext[a] / h))) for a in range(3)]
    else:
        dims = [1, 1, 1]
    return lo, h, dims


def cell_index(verts: torch.Tensor, cells: int):
    """(idx int64 [V,3], keys int64 [V], lo, h, dims)."""
    v = verts.detach().cpu().to(F32)
    lo, h, dims = grid(v, cells)
    if not bool(torch.isfinite(v).all()):
        raise ValueError("non-finite vertex")
    if float(h) > 0.0:
        q = torch.floor((v - lo) / h)                                          # fp32 subtraction, division, floor
        idx = torch.minimum(q.to(torch.int64), torch.tensor(dims, dtype=torch.int64) - 1)
    else:
        idx = torch.zeros(v.shape, dtype=torch.int64)
    keys = idx[:, 0] + dims[0] * (idx[:, 1] + dims[1] * idx[:, 2])
    return idx, keys, lo, h, dims


def record_terms(verts, faces, idx, lo, h):
    """terms fp64 [3 F,17] of the records 3 f + k, each product and sum a single fp64 operation in the order the kernel's header gives."""
    P = verts.detach().cpu().to(F32).to(F64)[faces]                            # [F,3,3]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    cr = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                      e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], dim=1)
    ln = torch.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
    a = 0.5 * ln
    n = torch.where(ln[:, None] > 0, cr / torch.where(ln > 0, ln, torch.ones_like(ln))[:, None], torch.zeros_like(cr))
    terms = torch.zeros(faces.shape[0], 3, N_SUMS, dtype=F64)
    lo64, h64 = lo.to(F64), h.to(F64)
    for k in range(3):
        c = lo64 + (idx[faces[:, k]].to(F64) + 0.5) * h64                      # the centre of corner k's cell
        d = (n[:, 0] * (c[:, 0] - P[:, 0, 0]) + n[:, 1] * (c[:, 1] - P[:, 0, 1])) + n[:, 2] * (c[:, 2] - P[:, 0, 2])
        g = a[:, None] * n
        q = P[:, k] - c
        t = terms[:, k]
        t[:, 0], t[:, 1], t[:, 2] = g[:, 0] * n[:, 0], g[:, 0] * n[:, 1], g[:, 0] * n[:, 2]
        t[:, 3], t[:, 4], t[:, 5] = g[:, 1] * n[:, 1], g[:, 1] * n[:, 2], g[:, 2] * n[:, 2]
        t[:, 6:9] = g * d[:, None]
        t[:, 9] = a
        t[:, 10:13] = a[:, None] * q
        t[:, 13:16] = q
        t[:, 16] = 1.0
    return terms.reshape(-1, N_SUMS)


def solve_cell(s, h, lam, placement):
    """(x relative to the cell centre fp64 [3], clamped bool, borderline bool: the unclamped solution lies within 1e-9 h of a face of
    the box, so rounding decides on which side) from the 17 sums of a cell (numpy fp64)."""
    if s[9] > 0.0:
        x = s[10:13] / s[9]
    else:
        x = s[13:16] / s[16]
    A = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
    w = (s[0] + s[3] + s[5]) / 3.0
    if placement != "quadric" or not s[9] > 0.0 or not w > 0.0:
        return x, False, False
    M = A + lam * w * np.eye(3)
    Lc = np.linalg.cholesky(M)
    rhs = -(A @ x + s[6:9])
    y = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))
    z = x + y
    half = 0.5 * h
    zc = np.clip(z, -half, half)
    return zc, bool((zc != z).any()), bool((np.abs(np.abs(z) - half) <= 1e-9 * h).any())


def edge_counts(faces):
    if faces.shape[0] == 0:
        return 0, 0
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = torch.sort(e, dim=1).values
    n = torch.unique(e, dim=0, return_counts=True)[1]
    return int((n == 1).sum()), int((n > 2).sum())


def simplify_ref(verts, faces, cells, regularization=1e-3, placement="quadric"):
    """(verts fp32 [V',3], faces int64 [F',3], stats, extra): extra holds keys / counts / sums / abs_sums (sum of |terms|) of every
    occupied cell in ascending key order, rep64 (the representatives before the rounding to fp32), used and n_borderline."""
    verts, faces = verts.detach().cpu().to(F32), faces.detach().cpu().to(torch.int64)
    nf = faces.shape[0]
    idx, keys, lo, h, dims = cell_index(verts, cells)
    if nf and (int(faces.min()) < 0 or int(faces.max()) >= verts.shape[0]):
        raise ValueError("face index out of range")
    rkey = keys[faces.reshape(-1)]
    terms = record_terms(verts, faces, idx, lo, h).numpy()
    order = np.argsort(rkey.numpy(), kind="stable")
    run_key, run_len = np.unique(rkey.numpy(), return_counts=True)
    R = len(run_key)
    sums, abs_sums = np.zeros((R, N_SUMS)), np.zeros((R, N_SUMS))
    pos = 0
    for r in range(R):
        acc, aacc = np.zeros(N_SUMS), np.zeros(N_SUMS)
        for rec in order[pos:pos + run_len[r]]:                                 # sequential, ascending record index
            acc = acc + terms[rec]
            aacc = aacc + np.abs(terms[rec])
        sums[r], abs_sums[r] = acc, aacc
        pos += run_len[r]
    h64, lo64 = float(h), lo.to(F64).numpy()
    rep64, n_clamped, n_borderline = np.zeros((R, 3)), 0, 0
    for r in range(R):
        k = int(run_key[r])
        cell = np.array([k % dims[0], (k // dims[0]) % dims[1], k // (dims[0] * dims[1])], dtype=np.float64)
        c = lo64 + (cell + 0.5) * h64
        x, cl, bl = solve_cell(sums[r], h64, regularization, placement)
        n_clamped += cl
        n_borderline += bl
        rep64[r] = c + x
    rank = {int(k): r for r, k in enumerate(run_key)}
    seen, out_tri, n_collapsed, n_dup = set(), [], 0, 0
    for f in range(nf):
        t = [rank[int(keys[int(i)])] for i in faces[f]]
        if len(set(t)) < 3:
            n_collapsed += 1
            continue
        m = t.index(min(t))
        t = tuple(t[m:] + t[:m])
        if t in seen:
            n_dup += 1
            continue
        seen.add(t)
        out_tri.append(t)
    tri = torch.tensor(out_tri, dtype=torch.int64).reshape(-1, 3)
    used = np.zeros(R, dtype=bool)
    used[tri.reshape(-1).numpy()] = True
    new_index = torch.from_numpy(np.cumsum(used) - 1)
    out_f = new_index[tri].reshape(-1, 3)
    out_v = torch.from_numpy(rep64[used]).to(F32).reshape(-1, 3)
    b, nm = edge_counts(out_f)
    stats = {"cells": int(cells), "cell_size": float(h), "dims": list(dims), "n_cells_occupied": R, "n_verts_in": int(verts.shape[0]),
             "n_faces_in": nf, "n_verts_out": int(out_v.shape[0]), "n_faces_out": int(out_f.shape[0]), "n_collapsed": n_collapsed,
             "n_duplicate": n_dup, "n_clamped": int(n_clamped), "n_boundary_edges": b, "n_nonmanifold_edges": nm,
             "longest_run": int(run_len.max()) if R else 0}
    extra = {"keys": torch.from_numpy(run_key.astype(np.int64)), "counts": torch.from_numpy(run_len.astype(np.int64)),
             "sums": torch.from_numpy(sums), "abs_sums": torch.from_numpy(abs_sums), "rep64": torch.from_numpy(rep64),
             "used": torch.from_numpy(used), "n_borderline": int(n_borderline)}
    return out_v, out_f, stats, extra


def simplify_to_target_ref(verts, faces, target_faces, cells_max=1024, **kw):
    """The faces:T bisection: (result of simplify_ref, cells chosen, passes)."""
    lo, hi, best, passes = 1, cells_max + 1, None, 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        res = simplify_ref(verts, faces, mid, **kw)
        passes += 1
        if res[2]["n_faces_out"] <= target_faces:
            lo, best = mid, res
        else:
            hi = mid
    if best is None:
        best = simplify_ref(verts, faces, 1, **kw)
        passes += 1
    return best, lo, passes


# ------------------------------------------------------------------------------------------------ fixtures
def fan(center, n_tri, radius=0.01, tilt=0.3):
    """n_tri triangles around `center` (3 n_tri corner records, n_tri of them at the centre vertex): (verts fp32 [n_tri + 2, 3],
    faces).  The rim is not closed, and it wobbles out of the plane so that the normals differ."""
    cx, cy, cz = center
    vs = [(cx, cy, cz)]
    for j in range(n_tri + 1):
        a = 2.0 * math.pi * j / (n_tri + 1)
        vs.append((cx + radius * math.cos(a), cy + radius * math.sin(a), cz + tilt * radius * math.sin(3.0 * a)))
    fs = [(0, 1 + j, 2 + j) for j in range(n_tri)]
    return torch.tensor(vs, dtype=F32), torch.tensor(fs, dtype=torch.int64)


def fans_in_cells(run_lengths, cells=8):
    """One fan per requested run length, each around a vertex in a cell of its own on a grid of `cells` cells over [0,1]^3 (two far
    anchor triangles pin the bounding box); the rim vertices lie in neighbouring cells.  Returns (verts, faces, cells, centre vertex
    index of every fan): the cell of fan i's centre holds exactly run_lengths[i] records."""
    h = 1.0 / cells
    V = [torch.tensor([[0.0, 0.0, 0.0], [h / 4, 0.0, 0.0], [0.0, h / 4, 0.0],
                       [1.0, 1.0, 1.0], [1.0 - h / 4, 1.0, 1.0], [1.0, 1.0 - h / 4, 1.0]], dtype=F32)]
    Fc = [torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int64)]
    centres, off = [], 6
    for i, n in enumerate(run_lengths):
        c = ((1 + 2 * (i % 3) + 0.5) * h, (1 + 2 * ((i // 3) % 3) + 0.5) * h, (3 + 0.5) * h)
        v, f = fan(c, n, radius=0.75 * h)                   # rim at 0.75 h from the cell's centre: outside the cell (half edge 0.5 h)
        V.append(v)
        Fc.append(f + off)
        centres.append(off)
        off += v.shape[0]
    return torch.cat(V), torch.cat(Fc), cells, centres


def point_cloud_distance(p, q, chunk=2048):
    """Distance from every point of p [N,3] to its nearest point of q [M,3], fp64 on the CPU."""
    p, q = p.double(), q.double()
    return torch.cat([torch.cdist(p[s:s + chunk], q).min(dim=1).values for s in range(0, p.shape[0], chunk)])
