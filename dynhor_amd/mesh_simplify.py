"""Mesh simplification by vertex clustering with per-cell quadrics (Rossignac-Borrel cells, Lindstrom's quadric placement): a mesh of
millions of faces reduced to a few thousand in one gather and one segmented reduction, bitwise reproducible.

The bounding box of the vertices is cut into `cells` cubes of edge h along its longest axis (fp32 arithmetic, csrc/mesh_simplify.hip's
header gives every operation).  All vertices of a cell become ONE vertex, the cell's representative:

  * every (face, corner) is a record of the cell of that corner's vertex -- faces that will collapse included: their planes still
    shape the cell -- and carries the face's unit normal n, its area a, the plane offset d relative to the cell's centre c and the
    corner's position relative to c, all in fp64;
  * per cell, in a fixed order (no float atomics): A = sum a n n^T, b = sum a d n, sum a, sum a (corner - c), sum (corner - c), count;
  * xbar = the area-weighted mean of the corners (the plain mean in a cell without area).  placement "quadric" solves
    (A + regularization w I) y = -(A xbar + b), w = trace(A) / 3, by a 3 x 3 Cholesky factorisation and takes xbar + y clamped to the
    cell's box: the point closest to the cell's planes, pulled towards xbar by a Tikhonov term that keeps the system positive
    definite (condition <= (3 + regularization) / regularization), keeps a flat cell's in-plane position at the centroid and has no
    singular-value threshold.  placement "mean" takes xbar;
  * a face survives when its three cells differ.  It is rotated so that the smallest cell comes first (orientation kept); of several
    faces with the same rotated triple the one with the smallest input index survives; a pair with opposite orientations is two
    triples and both stay.  Output faces are in the order of their input faces, output vertices are the cells a surviving face
    references, in ascending cell-key order.

Property: every input vertex moves to a point of its own cell, so every point of an output face lies within sqrt(3) h of the input
surface.  The other direction holds for everything except components that vanish inside a cell.  Limits: the result need not be
manifold (two sheets that pass through one cell are welded); a closed component smaller than one cell disappears; the order of the
faces changes the rounding of the sums, so the result depends on the face order -- but not on the launch or on any chunking.

dh_simplify_cells, dh_simplify_quadrics and dh_simplify_faces are HIP; the sorts, unique and compaction between them are torch on the
device.  There is no CPU path: CPU tensors raise DynhorHipError.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._args import check_faces, check_verts

PLACEMENTS = ("mean", "quadric")
MAX_CELLS = 1 << 20
SUMS = 17
DEFAULTS = {"mode": "none", "regularization": 1e-3, "cells_max": 1024}


def parse_mode(mode):
    """("none", None) | ("cells", N) | ("faces", T) of a mode string none | cells:N | faces:T (None is "none")."""
    if mode is None or mode == "none":
        return "none", None
    if isinstance(mode, str):
        for kind, least in (("cells", 1), ("faces", 0)):
            if mode.startswith(kind + ":"):
                try:
                    n = int(mode[len(kind) + 1:])
                except ValueError:
                    n = -1
                if n < least:
                    raise ValueError(f"mesh_simplify: mode '{kind}:N' needs an integer N >= {least}, got {mode!r}")
                if kind == "cells" and n > MAX_CELLS:
                    raise ValueError(f"mesh_simplify: at most {MAX_CELLS} cells, got {mode!r}")
                return kind, n
    raise ValueError(f"mesh_simplify: mode must be none, cells:N or faces:T, got {mode!r}")


def _check_options(fn, cells, target_faces, regularization, placement, cells_max):
    if (cells is None) == (target_faces is None):
        raise ValueError(f"{fn}: give exactly one of cells and target_faces")
    for name, v, least, most in (("cells", cells, 1, MAX_CELLS), ("target_faces", target_faces, 0, None),
                                 ("cells_max", cells_max, 1, MAX_CELLS)):
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, int) or v < least or (most is not None and v > most):
            raise ValueError(f"{fn}: {name} must be an integer in [{least}, {most if most is not None else 'inf'}], got {v!r}")
    if placement not in PLACEMENTS:
        raise ValueError(f"{fn}: placement must be one of {PLACEMENTS}, got {placement!r}")
    if isinstance(regularization, bool) or not isinstance(regularization, (int, float)) or not 0.0 < regularization <= 1e6:
        raise ValueError(f"{fn}: regularization must be a number in (0, 1e6], got {regularization!r}")


class _Grid:
    """lo, h, dims of dh_simplify_grid as the ctypes values the device entry points take."""

    def __init__(self, lo, hi, cells):
        f3, i3 = _lib._f32 * 3, _lib._i32 * 3
        self.lo, self.dims, h = f3(*lo), i3(), _lib._f32()
        _lib.check(_lib.lib().dh_simplify_grid(self.lo, f3(*hi), int(cells), ctypes.byref(h), self.dims))
        self.h = h.value


def cell_keys(verts: torch.Tensor, cells: int):
    """(keys int64 [V], cell_size float, dims (dx, dy, dz)): the cell key i_x + dx (i_y + dy i_z) of every vertex on the grid that cuts
    the bounding box's longest axis into `cells` cells (dh_simplify_grid, dh_simplify_cells).  ValueError: a non-finite vertex."""
    keys, g = _cell_keys("cell_keys", check_verts("cell_keys", verts), int(cells))
    return keys, g.h, tuple(g.dims)


def _cell_keys(fn, verts, cells):
    nv = verts.shape[0]
    if nv == 0:
        return torch.empty(0, dtype=torch.int64, device=verts.device), _Grid((0.0,) * 3, (0.0,) * 3, cells)
    box = torch.stack([verts.amin(dim=0), verts.amax(dim=0)]).cpu()
    if not bool(torch.isfinite(box).all()) or not bool(torch.isfinite(box[1] - box[0]).all()):
        raise ValueError(f"{fn}: verts must be finite (and their extent must not overflow float32)")
    g = _Grid(box[0].tolist(), box[1].tolist(), cells)
    keys = torch.empty(nv, dtype=torch.int64, device=verts.device)
    with torch.cuda.device(verts.device):
        _lib.check(_lib.lib().dh_simplify_cells(_lib.ptr(verts), nv, g.lo, g.h, g.dims, _lib.ptr(keys), _lib.stream()))
    return keys, g


def edge_counts(faces: torch.Tensor):
    """(boundary, non-manifold): the undirected edges of faces int64 [F,3] used by exactly one face, and by more than two."""
    if faces.shape[0] == 0:
        return 0, 0
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    lo, hi = e.min(dim=1).values, e.max(dim=1).values
    n = torch.unique(lo * (int(faces.max()) + 1) + hi, return_counts=True)[1]
    return int((n == 1).sum()), int((n > 2).sum())


def _simplify_cells(fn, verts, faces, cells, regularization, placement, return_sums):
    dev, nv, nf = verts.device, verts.shape[0], faces.shape[0]
    L = _lib.lib()
    keys, g = _cell_keys(fn, verts, cells)
    stats = {"cells": int(cells), "cell_size": g.h, "dims": [int(d) for d in g.dims], "n_verts_in": nv, "n_faces_in": nf}
    with torch.cuda.device(dev):
        # records: corner k of face f is record 3 f + k, in the cell of its vertex; a stable sort lists every cell's records in order
        rkey = keys[faces.reshape(-1)] if nf else keys.new_empty(0)
        rkey, order = torch.sort(rkey, stable=True)
        run_key, run_len = torch.unique_consecutive(rkey, return_counts=True)
        n_runs = int(run_key.shape[0])
        run_start = torch.zeros(n_runs + 1, dtype=torch.int64, device=dev)
        torch.cumsum(run_len, 0, out=run_start[1:])
        rep = torch.empty(n_runs, 3, dtype=torch.float32, device=dev)
        clamped = torch.empty(n_runs, dtype=torch.int32, device=dev)
        sums = torch.empty(n_runs, SUMS, dtype=torch.float64, device=dev) if return_sums else None
        _lib.check(L.dh_simplify_quadrics(_lib.ptr(verts), nv, _lib.ptr(faces), nf, _lib.ptr(order), _lib.ptr(run_start),
                                          _lib.ptr(run_key), n_runs, g.lo, g.h, g.dims, float(regularization),
                                          PLACEMENTS.index(placement), _lib.ptr(rep), _lib.ptr(clamped),
                                          _lib.ptr(sums) if return_sums else None, _lib.stream()))
        # faces on cell ranks, rotated; the duplicates of a rotated triple fall to the one with the smallest input index
        vrank = torch.searchsorted(run_key, keys).to(torch.int32) if n_runs else torch.zeros(nv, dtype=torch.int32, device=dev)
        tri = torch.empty(nf, 3, dtype=torch.int64, device=dev)
        keep = torch.empty(nf, dtype=torch.uint8, device=dev)
        key = torch.empty(nf, dtype=torch.int64, device=dev)
        _lib.check(L.dh_simplify_faces(_lib.ptr(faces), nf, _lib.ptr(vrank), nv, n_runs, _lib.ptr(tri), _lib.ptr(keep), _lib.ptr(key),
                                       _lib.stream()))
        idx = torch.nonzero(keep).reshape(-1)                                  # ascending input index
        n_distinct = int(idx.shape[0])
        t, k = tri[idx], key[idx]
        if n_runs < (1 << 21):                                                 # the whole triple fits one int64
            k, perm = torch.sort(k * n_runs + t[:, 2], stable=True)
            first = torch.ones_like(k, dtype=torch.bool)
            first[1:] = k[1:] != k[:-1]
        else:
            perm = torch.sort(t[:, 2], stable=True)[1]
            k, p2 = torch.sort(k[perm], stable=True)
            perm = perm[p2]
            c = t[perm, 2]
            first = torch.ones_like(k, dtype=torch.bool)
            first[1:] = (k[1:] != k[:-1]) | (c[1:] != c[:-1])
        survivors = torch.sort(idx[perm[first]])[0]
        tri = tri[survivors]
        used = torch.zeros(n_runs, dtype=torch.bool, device=dev)
        used[tri.reshape(-1)] = True
        new_index = torch.cumsum(used, 0) - 1
        out_v, out_f = rep[used].contiguous(), new_index[tri].contiguous()
        boundary, nonmanifold = edge_counts(out_f)
        stats.update(n_cells_occupied=n_runs, n_verts_out=int(out_v.shape[0]), n_faces_out=int(out_f.shape[0]),
                     n_collapsed=nf - n_distinct, n_duplicate=n_distinct - int(out_f.shape[0]), n_clamped=int(clamped.sum()),
                     n_boundary_edges=boundary, n_nonmanifold_edges=nonmanifold,
                     longest_run=int(run_len.max()) if n_runs else 0, placement=placement, regularization=float(regularization))
    if return_sums:
        return out_v, out_f, stats, {"sums": sums, "keys": run_key, "counts": run_len, "used": used}
    return out_v, out_f, stats


def simplify_mesh(verts, faces, cells=None, target_faces=None, regularization=1e-3, placement="quadric", cells_max=1024,
                  return_sums=False):
    """The mesh (verts float32 [V,3], faces int64 [F,3], on the device) clustered on a grid of `cells` cells along the bounding box's
    longest axis (module docstring).  Returns (verts float32 [V',3], faces int64 [F',3], stats).

    Exactly one of `cells` (1 .. 2^20) and `target_faces` is given.  target_faces T chooses `cells` by bisection over [1, cells_max]
    in at most ceil(log2 cells_max) + 1 simplifications and returns the result of the largest tested value with at most T faces
    (cells = 1 gives no face, so there always is one); stats then also holds target_faces and passes.

    stats: cells, cell_size (h), dims, n_cells_occupied (cells with a record), n_verts_in / out, n_faces_in / out, n_collapsed (faces
    whose cells were not distinct), n_duplicate (faces dropped for an earlier face with the same rotated triple), n_clamped (cells whose
    solution left the cell), n_boundary_edges and n_nonmanifold_edges of the output, longest_run (the most records in one cell),
    placement, regularization.

    return_sums: a fourth value, a dict of sums float64 [n_cells_occupied,17] (the layout of dh_simplify_quadrics), keys and counts
    (the key and record count of those cells, ascending) and used (bool: which of them became output vertices).

    Every point of an output face lies within sqrt(3) cell_size of the input surface.  The result need not be manifold, a closed
    component smaller than a cell disappears, and the result depends on the order of the faces (through the rounding of the sums) but
    not on the launch.  ValueError: non-finite vertices, face indices outside [0, V), bad options.  CPU tensors: DynhorHipError."""
    fn = "simplify_mesh"
    _check_options(fn, cells, target_faces, regularization, placement, cells_max)
    verts, faces = check_verts(fn, verts), check_faces(fn, faces)
    if verts.device != faces.device:
        raise ValueError(f"{fn}: verts on {verts.device}, faces on {faces.device}")
    if faces.shape[0] and (int(faces.min()) < 0 or int(faces.max()) >= verts.shape[0]):
        raise ValueError(f"{fn}: face indices must lie in [0, {verts.shape[0]}), got [{int(faces.min())}, {int(faces.max())}]")
    if verts.shape[0] >= 1 << 31 or faces.shape[0] >= (1 << 31) // 3:
        raise ValueError(f"{fn}: at most 2^31 vertices and records")
    if cells is not None:
        return _simplify_cells(fn, verts, faces, cells, regularization, placement, return_sums)
    lo, hi, best, passes = 1, int(cells_max) + 1, None, 0       # lo always meets the target (cells = 1 has no face), hi never does
    while hi - lo > 1:
        mid = (lo + hi) // 2
        res = _simplify_cells(fn, verts, faces, mid, regularization, placement, return_sums)
        passes += 1
        if res[2]["n_faces_out"] <= target_faces:
            lo, best = mid, res
        else:
            hi = mid
    if best is None:
        best = _simplify_cells(fn, verts, faces, 1, regularization, placement, return_sums)
        passes += 1
    assert passes <= math.ceil(math.log2(cells_max)) + 1
    best[2].update(target_faces=int(target_faces), passes=passes, cells_max=int(cells_max))
    return best


def simplify_by_mode(verts, faces, mode, regularization=1e-3, cells_max=1024):
    """simplify_mesh for a mode string cells:N | faces:T (parse_mode)."""
    kind, n = parse_mode(mode)
    if kind == "none":
        raise ValueError("simplify_by_mode: mode 'none' simplifies nothing")
    return simplify_mesh(verts, faces, cells=n if kind == "cells" else None, target_faces=n if kind == "faces" else None,
                         regularization=regularization, cells_max=cells_max)
