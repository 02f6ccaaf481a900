"""Block-sparse mesh extraction: the mesh of ``mesh.marching_cubes`` on the full grid, from field samples near the surface only.

The grid of N points per axis is cut into blocks of B cells per axis; block b covers the grid indices [b B, min(b B + B, N - 1)] (the
far blocks are clipped).  One batched field call evaluates u at every block's centre c; the block is ACTIVE iff |u(c) - threshold| <=
lipschitz * r, r = half its diagonal times (1 + 2^-10).  Under a field whose Lipschitz constant is at most ``lipschitz`` an inactive
block has no sign change anywhere in its closed extent, so no crossing, on a shared face or elsewhere, is lost.  The rule looks at the
field's local value only: a floater is kept like any other surface.  lipschitz = inf keeps every block.

The active blocks are sampled at their (B + 1)^3 grid points (coordinates read from the dense path's linspace axes: the dense grid's
bits; shared faces are sampled by both blocks) in chunks, and triangulated by csrc/mesh_extract.hip with the case table of
``mesh.marching_cubes_table``: one (edge key, position) pair per triangle corner, in the dense code's arithmetic.  All pairs are welded
once by ``torch.unique``.  The key lin(lower corner) * 3 + axis sorts like the dense key and fits int64 at any resolution
(``mesh.marching_cubes``: N <= 1448).  Memory grows with (N / B)^3 (the centre pass, the int32 block map), the chunk and the mesh.
No CPU path; only sizes and two flags are read back from the device.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .mesh import marching_cubes_table

# Default cull constant.  An SDF network is not 1-Lipschitz: L_min, the smallest constant that keeps every block holding a crossing
# (min_safe_lipschitz), of configs/synthetic.yaml at resolution 512 is 1.018 (neus) / 1.130 (hash) at initialisation and 2.326 / 2.584
# after 2,000 iterations (scripts/bench_mesh_extract.py --lipschitz_record; DESIGN_NEXT_ROWS.md section 11).  The default is twice the
# largest, rounded up to a multiple of 0.5: single checkpoints of that training differ chaotically
DEFAULT_LIPSCHITZ = 5.5
MODES = ("dense", "sparse")
MAX_BLOCK = 16                   # dh_mc_*: (B + 1)^3 floats of LDS per workgroup
_TABLE = None


def packed_table() -> torch.Tensor:
    """marching_cubes_table() as the kernels read it: u8 [256,16], bytes 0..14 the edge ids of the case's triangles in table order
    (unused: 255), byte 15 the triangle count."""
    global _TABLE
    if _TABLE is None:
        tri, n_tri = marching_cubes_table()
        t = torch.full((256, 16), 255, dtype=torch.uint8)
        flat = tri.reshape(256, 15)
        t[:, :15] = torch.where(flat >= 0, flat, torch.full_like(flat, 255)).to(torch.uint8)
        t[:, 15] = n_tri.to(torch.uint8)
        _TABLE = t
    return _TABLE


def _check_grid(fn, resolution, block):
    N, B = int(resolution), int(block)
    if N < 2:
        raise ValueError(f"{fn}: resolution must be >= 2, got {resolution}")
    if not 1 <= B <= MAX_BLOCK:
        raise ValueError(f"{fn}: block must be in [1, {MAX_BLOCK}], got {block}")
    return N, B


def grid_axes(resolution, bound_min, bound_max, device=None):
    """The three axis coordinate arrays exactly as the dense path makes them (renderer.extract_geometry)."""
    N = int(resolution)
    return [torch.linspace(float(bound_min[i]), float(bound_max[i]), N, device=device) for i in range(3)]


def block_grid(axes, block):
    """(nbk, centres f32 [nbk^3,3], radii f32 [nbk^3]) of the blocks of `block` cells over the grid whose axis arrays are `axes`
    (three f32 [N] tensors, any device), in (bx, by, bz) lexicographic order; nbk = ceil((N - 1) / block) blocks per axis.  A block's
    centre is the midpoint of its two end coordinates per axis, its radius half the length of its diagonal times (1 + 2^-10) -- the
    margin covers the rounding of the centre to fp32 many times over.  Both are computed in float64 and cast to fp32."""
    N, B = _check_grid("block_grid", axes[0].shape[0], block)
    nbk = (N - 2) // B + 1
    dev = axes[0].device
    lo = torch.arange(nbk, device=dev) * B
    hi = torch.clamp(lo + B, max=N - 1)
    mid = [0.5 * (a.double()[lo] + a.double()[hi]) for a in axes]
    ext = [a.double()[hi] - a.double()[lo] for a in axes]
    cx, cy, cz = torch.meshgrid(*mid, indexing="ij")
    ex, ey, ez = torch.meshgrid(*ext, indexing="ij")
    centres = torch.stack([cx, cy, cz], dim=-1).reshape(-1, 3).float().contiguous()
    radii = (0.5 * torch.sqrt(ex * ex + ey * ey + ez * ez) * (1.0 + 2.0 ** -10)).reshape(-1).float()
    return nbk, centres, radii


def active_blocks(u_centre, radii, threshold, lipschitz):
    """bool [nbk^3]: |u(c) - threshold| <= lipschitz * r (lipschitz = inf: every block)."""
    return (u_centre.reshape(-1).float() - float(threshold)).abs() <= float(lipschitz) * radii


def min_safe_lipschitz(u, u_centre, radii, threshold, block):
    """L_min of a dense grid u [N,N,N]: the largest |u(c) - threshold| / r over the blocks that hold a cell with a sign change -- the
    smallest `lipschitz` that keeps them all (0.0 when no cell has one).  u_centre, radii: the field at block_grid's centres and its
    radii.  Torch ops on u's device; for measuring, not on any extraction path."""
    import torch.nn.functional as F
    N, B = _check_grid("min_safe_lipschitz", u.shape[0], block)
    nbk = (N - 2) // B + 1
    inside = ((u - float(threshold)) > 0).float()[None, None]
    some = F.max_pool3d(inside, 2, 1)
    every = -F.max_pool3d(-inside, 2, 1)
    mixed = (some - every)                                          # [1,1,N-1,N-1,N-1]: 1 where the cell's corners disagree
    per_block = F.max_pool3d(mixed, B, B, ceil_mode=True).reshape(-1) > 0
    assert per_block.shape[0] == nbk ** 3
    need = (u_centre.reshape(-1).float() - float(threshold)).abs() / radii
    if not bool(per_block.any()):
        return 0.0
    return float(need[per_block].max())


def _field_values(field, pts, what):
    u = field(pts)
    if not torch.is_tensor(u) or u.numel() != pts.shape[0]:
        raise ValueError(f"sparse_marching_cubes: field must map [M,3] points to [M] or [M,1] values ({what})")
    return u.reshape(-1).float().contiguous()


def _nonfinite(what):
    return _lib.DynhorHipError(f"sparse_marching_cubes: non-finite field values {what} (split_f16 range exceeded, or the network has "
                               "diverged); use arithmetic 'split_bf16' for queries this far out")


@torch.no_grad()
def sparse_marching_cubes(field, resolution, bound_min, bound_max, threshold=0.0, block=8, lipschitz=DEFAULT_LIPSCHITZ,
                          chunk_points=1 << 24, device=None):
    """The marching-cubes mesh of `field` on the grid of `resolution` points per axis over [bound_min, bound_max], from the blocks near
    the surface only (module docstring).  field: device points f32 [M,3] -> u [M] or [M,1] (u = -sdf, inside > threshold), called
    once for the block centres and once per chunk of at most `chunk_points` samples.  Returns (verts f32 [V,3] in world units, faces
    int64 [F,3], stats): for the same field values the vertices are torch.equal to mesh.marching_cubes' in order and the faces equal
    up to their order; two calls return identical bits.  stats: blocks, active_blocks, samples (centres + (B + 1)^3 per active
    block), dense_samples (N^3), cut_block_faces, verts, faces.

    A non-finite centre value or sample raises DynhorHipError, as the dense path does.  cut_block_faces counts cell faces between an
    active and a culled block whose corners disagree: the mesh would have a hole there, so a count above 0 raises DynhorHipError
    naming `lipschitz`.  What this CANNOT see: a closed component wholly inside culled blocks, which is silently absent; only a
    `lipschitz` that bounds the field's true constant rules that out.  device: default the current CUDA device; CPU raises."""
    N, B = _check_grid("sparse_marching_cubes", resolution, block)
    lipschitz = float(lipschitz)
    if not lipschitz > 0:
        raise ValueError(f"sparse_marching_cubes: lipschitz must be > 0, got {lipschitz}")
    if int(chunk_points) < 1:
        raise ValueError(f"sparse_marching_cubes: chunk_points must be >= 1, got {chunk_points}")
    if not math.isfinite(float(threshold)):
        raise ValueError(f"sparse_marching_cubes: threshold must be finite, got {threshold}")
    dev = torch.device(device) if device is not None else (torch.device("cuda", torch.cuda.current_device())
                                                            if torch.cuda.is_available() else torch.device("cpu"))
    if dev.type != "cuda":
        raise _lib.DynhorHipError("sparse_marching_cubes: needs a device (the HIP kernels have no CPU fallback)")
    L = _lib.lib()
    P3 = (B + 1) ** 3
    with torch.cuda.device(dev):
        axes = grid_axes(N, bound_min, bound_max, dev)
        bmin = torch.as_tensor(bound_min, dtype=torch.float32, device=dev)
        bmax = torch.as_tensor(bound_max, dtype=torch.float32, device=dev)
        nbk, centres, radii = block_grid(axes, B)
        u_c = _field_values(field, centres, "block centres")
        if not bool(torch.isfinite(u_c).all()):
            raise _nonfinite("at the block centres")
        active = active_blocks(u_c, radii, threshold, lipschitz)
        del centres, u_c, radii
        block_map = (torch.cumsum(active, 0, dtype=torch.int32) - 1).masked_fill_(~active, -1).contiguous()
        blocks = active.reshape(nbk, nbk, nbk).nonzero().to(torch.int32).contiguous()       # [nb,3], lexicographic
        del active
        nb = int(blocks.shape[0])
        table = packed_table().to(dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)                                # cut faces, non-finite
        per_chunk = max(1, int(chunk_points) // P3)
        keys, poss = [], []
        for b0 in range(0, nb, per_chunk):
            blk = blocks[b0:b0 + per_chunk]
            n = int(blk.shape[0])
            pts = torch.empty(n * P3, 3, device=dev)
            _lib.check(L.dh_mc_block_points(_lib.ptr(axes[0]), _lib.ptr(axes[1]), _lib.ptr(axes[2]), N, _lib.ptr(blk), n, B,
                                            _lib.ptr(pts), _lib.stream()))
            vals = _field_values(field, pts, "block samples")
            del pts
            counts = torch.empty(n, dtype=torch.int32, device=dev)
            _lib.check(L.dh_mc_count(_lib.ptr(vals), _lib.ptr(blk), n, N, B, float(threshold), _lib.ptr(table), _lib.ptr(block_map),
                                     _lib.ptr(counts), _lib.ptr(flags[0:1]), _lib.ptr(flags[1:2]), _lib.stream()))
            incl = torch.cumsum(counts, 0, dtype=torch.int64)
            offsets = (incl - counts).contiguous()
            n_tri = int(incl[-1])
            if n_tri == 0:
                continue
            key = torch.empty(n_tri * 3, dtype=torch.int64, device=dev)
            pos = torch.empty(n_tri * 3, 3, device=dev)
            _lib.check(L.dh_mc_emit(_lib.ptr(vals), _lib.ptr(blk), n, N, B, float(threshold), _lib.ptr(table), _lib.ptr(offsets), n_tri,
                                    _lib.ptr(key), _lib.ptr(pos), _lib.stream()))
            keys.append(key); poss.append(pos)
        cut, bad = (int(v) for v in flags.tolist())
        if bad:
            raise _nonfinite("in the block samples")
        if cut:
            raise _lib.DynhorHipError(
                f"sparse_marching_cubes: the surface crosses {cut} cell faces into culled blocks (the mesh would have holes): lipschitz = "
                f"{lipschitz:g} is below the field's Lipschitz constant here; raise lipschitz (inf keeps every block)")
        stats = {"blocks": nbk ** 3, "active_blocks": nb, "samples": nbk ** 3 + nb * P3, "dense_samples": N ** 3, "cut_block_faces": cut}
        if not keys:
            stats.update(verts=0, faces=0)
            return torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev), stats
        key = torch.cat(keys) if len(keys) > 1 else keys[0]
        flat = torch.cat(poss) if len(poss) > 1 else poss[0]
        del keys, poss
        # the weld and the clean-up of mesh.marching_cubes, expression for expression
        uniq, inv = torch.unique(key, return_inverse=True)
        verts = torch.zeros(uniq.shape[0], 3, device=dev).index_copy_(0, inv, flat)
        faces = inv.reshape(-1, 3)
        ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
        faces = faces[ok]
        verts = verts / (N - 1) * (bmax - bmin) + bmin
        stats.update(verts=int(verts.shape[0]), faces=int(faces.shape[0]))
        return verts, faces, stats
