"""Iso-surface extraction for ``validate_mesh`` (upstream NeuSRenderer.extract_geometry uses
mcubes.marching_cubes, not installable here).  Marching tetrahedra on the SDF grid: every cube is split into 6
tetrahedra around its main diagonal; each tetrahedron contributes 0, 1 or 2 triangles with vertices linearly
interpolated on the edges where the field crosses the threshold.  Plain torch ops (host-side plumbing around the HIP
SDF queries), watertight by construction because neighbouring cubes split their shared faces identically."""
from __future__ import annotations

import numpy as np
import torch

# cube corners (x,y,z bits) and the 6 tetrahedra sharing the diagonal 0-7
_CORNERS = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]])
_TETS = torch.tensor([[0, 1, 3, 7], [0, 3, 2, 7], [0, 2, 6, 7], [0, 6, 4, 7], [0, 4, 5, 7], [0, 5, 1, 7]])


# the dense weld key min * N^3 + max of two linear grid indices (< N^3 each) is below N^6: 1448^6 < 2^63 < 1449^6
MAX_DENSE_RESOLUTION = 1448


def _check_weld_key_range(fn, N):
    if N > MAX_DENSE_RESOLUTION:
        raise ValueError(f"{fn}: resolution {N} > {MAX_DENSE_RESOLUTION}: the edge keys min * N^3 + max overflow int64 (vertices would be "
                         "welded by wrapped keys); use the sparse extraction mode (dynhor_amd/mesh_extract.py), whose keys fit at any N")


def marching_tetrahedra(u: torch.Tensor, threshold: float, bound_min, bound_max):
    """u [N,N,N] scalar field (upstream convention: u = -sdf, inside > threshold).  Returns (vertices [V,3] float32 in
    world units, triangles [T,3] int64).  A surface vertex lies on a grid EDGE and is identified by that edge (the pair of corner
    indices): every tetrahedron sharing the edge computes the same position from the same end, and vertices are welded by that
    key -- the mesh is watertight by construction (round 4: welding by quantised positions left a few cracks where the two ends'
    roundings differed; tests/test_cpu_mesh.py).  N <= 1448 (MAX_DENSE_RESOLUTION): the key min * N^3 + max must fit int64."""
    dev = u.device
    N = u.shape[0]
    _check_weld_key_range("marching_tetrahedra", N)
    bmin = torch.as_tensor(bound_min, dtype=torch.float32, device=dev)
    bmax = torch.as_tensor(bound_max, dtype=torch.float32, device=dev)
    # active cells first (8 shifted views of the grid: no per-cell index tensors for the empty 99 % of the volume)
    f = u - threshold
    sl = (slice(0, N - 1), slice(1, N))
    vmax = torch.full((N - 1, N - 1, N - 1), -float("inf"), device=dev)
    vmin = torch.full((N - 1, N - 1, N - 1), float("inf"), device=dev)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                c = f[sl[dx], sl[dy], sl[dz]]
                vmax = torch.maximum(vmax, c)
                vmin = torch.minimum(vmin, c)
    base = ((vmax > 0) & (vmin <= 0)).nonzero().reshape(-1, 1, 3)              # [C,1,3] active cells only
    corners = base + _CORNERS.to(dev).reshape(1, 8, 3)                          # [C,8,3]
    vals = f[corners[..., 0], corners[..., 1], corners[..., 2]]               # [C,8]
    lin = (corners[..., 0] * N + corners[..., 1]) * N + corners[..., 2]        # [C,8] linear index of every corner
    tets = _TETS.to(dev)
    tv = vals[:, tets].reshape(-1, 4)                                          # [C*6,4]
    tp = corners[:, tets].float().reshape(-1, 4, 3)                            # [C*6,4,3]
    ti = lin[:, tets].reshape(-1, 4)                                           # [C*6,4]
    inside = tv > 0
    n_in = inside.sum(dim=1)
    tris, keys = [], []
    NN = N * N * N

    def edge_vertex(p, v, idx, ar, a, b):
        """Crossing of edge (a, b) (per-row corner slots): position computed from the lower corner index, and the edge's key."""
        pa, pb, va, vb, ia, ib = p[ar, a], p[ar, b], v[ar, a], v[ar, b], idx[ar, a], idx[ar, b]
        sw = ia > ib
        p0, p1 = torch.where(sw[:, None], pb, pa), torch.where(sw[:, None], pa, pb)
        v0, v1 = torch.where(sw, vb, va), torch.where(sw, va, vb)
        t = (v0 / (v0 - v1)).clamp(0, 1).unsqueeze(-1)
        return p0 + t * (p1 - p0), torch.minimum(ia, ib) * NN + torch.maximum(ia, ib)

    def emit(pts, ks, ref, ref_inside):
        """One triangle per row from three (position, key) pairs, oriented so that its normal points away from `ref` if
        ref_inside (ref lies on the inside), towards it otherwise."""
        tri = torch.stack(pts, dim=1)
        key = torch.stack(ks, dim=1)
        n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        s = (n * (ref - tri.mean(dim=1))).sum(-1)
        wrong = (s > 0) if ref_inside else (s < 0)
        tri[wrong] = tri[wrong][:, [0, 2, 1]]
        key[wrong] = key[wrong][:, [0, 2, 1]]
        tris.append(tri); keys.append(key)

    # one corner inside (or one outside): a single triangle on the three edges leaving that corner
    for count in (1, 3):
        sel = n_in == count
        if sel.any():
            v, p, ins, idx = tv[sel], tp[sel], inside[sel], ti[sel]
            lone = (ins if count == 1 else ~ins).float().argmax(dim=1)          # slot of the lone corner
            ar = torch.arange(v.shape[0], device=dev)
            ev = [edge_vertex(p, v, idx, ar, lone, (lone + k) % 4) for k in (1, 2, 3)]
            emit([e[0] for e in ev], [e[1] for e in ev], p[ar, lone], ref_inside=(count == 1))
    # two inside / two outside: a quad (two triangles) across the four mixed edges
    sel = n_in == 2
    if sel.any():
        v, p, ins, idx = tv[sel], tp[sel], inside[sel], ti[sel]
        order = torch.argsort(ins.int(), dim=1, descending=True, stable=True)   # [in0, in1, out0, out1]
        ar = torch.arange(v.shape[0], device=dev)
        i0, i1, o0, o1 = order[:, 0], order[:, 1], order[:, 2], order[:, 3]
        q00, q01 = edge_vertex(p, v, idx, ar, i0, o0), edge_vertex(p, v, idx, ar, i0, o1)
        q10, q11 = edge_vertex(p, v, idx, ar, i1, o0), edge_vertex(p, v, idx, ar, i1, o1)
        ref = 0.5 * (p[ar, i0] + p[ar, i1])
        emit([q00[0], q01[0], q11[0]], [q00[1], q01[1], q11[1]], ref, ref_inside=True)
        emit([q00[0], q11[0], q10[0]], [q00[1], q11[1], q10[1]], ref, ref_inside=True)
    if not tris:
        return torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev)
    flat = torch.cat(tris, dim=0).reshape(-1, 3)                                # positions in grid units
    key = torch.cat(keys, dim=0).reshape(-1)
    uniq, inv = torch.unique(key, return_inverse=True)
    verts = torch.zeros(uniq.shape[0], 3, device=dev).index_copy_(0, inv, flat)
    faces = inv.reshape(-1, 3)
    # a crossing that falls exactly on a grid corner makes a triangle collapse onto one vertex KEYED by different edges: such
    # zero-area triangles are dropped only when two of their indices coincide after welding (never by area: that opened holes)
    ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    faces = faces[ok]
    verts = verts / (N - 1) * (bmax - bmin) + bmin
    return verts, faces


# ---------------------------------------------------------------------------------------------------- marching cubes
# Upstream's extract_geometry calls mcubes.marching_cubes.  The 256-case table is GENERATED here from the cube's
# topology instead of typed in: corner / edge numbering of the classic table (Lorensen & Cline; P. Bourke's layout), every cube face
# contributes one directed segment per maximal run of inside corners along its boundary (counter-clockwise seen from outside the cube:
# from the cut edge where the run is entered to the one where it is left), the segments of the six faces chain into closed loops, and
# every loop is fanned into triangles.  Because the rule is a FACE rule, two cubes always agree on the face they share -- ambiguous
# faces (diagonal corners inside) always separate the inside corners -- so the mesh is closed without the case-13 style repairs the
# hand-made tables need; for the unambiguous cases the polygons are the classic ones.  Normals point from inside (u > threshold)
# to outside, as marching_tetrahedra's.
_MC_CORNERS = torch.tensor([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]])
_MC_EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
_MC_FACES = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)]      # CCW seen from outside
_MC_TABLE = None


def _same_face(e0, e1):
    """Do cube edges e0, e1 lie on a common face?  (A triangle edge between two such crossings lies IN that face, where the
    neighbouring cube may put the same edge: four triangles around one edge.)"""
    for face in _MC_FACES:
        fe = {frozenset((face[k], face[(k + 1) % 4])) for k in range(4)}
        if frozenset(_MC_EDGES[e0]) in fe and frozenset(_MC_EDGES[e1]) in fe:
            return True
    return False


def _triangulate_loop(loop):
    """All triangulations of the (ordered) polygon `loop`, the first one none of whose DIAGONALS lies in a cube face; orientation kept."""
    n = len(loop)
    best = None

    def rec(idx):
        # triangulations of the sub-polygon with vertex indices idx (in order): lists of triangles
        if len(idx) < 3:
            yield []
            return
        if len(idx) == 3:
            yield [tuple(idx)]
            return
        a, b = idx[0], idx[-1]
        for k in range(1, len(idx) - 1):
            for left in rec(idx[:k + 1]):
                for right in rec(idx[k:]):
                    yield left + [(a, idx[k], b)] + right

    for tri in rec(list(range(n))):
        bad = 0
        for t in tri:
            for i, j in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                if (j - i) % n not in (1, n - 1) and _same_face(loop[i], loop[j]):
                    bad += 1
        if best is None or bad < best[0]:
            best = (bad, tri)
            if bad == 0:
                break
    assert best is not None and best[0] == 0, ("no face-diagonal-free triangulation", loop)
    return [(loop[a], loop[b], loop[c]) for a, b, c in best[1]]


def marching_cubes_table():
    """(tri [256, 5, 3] int64 edge ids, -1 padded; n_tri [256]).  Bit i of the case index = corner i inside."""
    global _MC_TABLE
    if _MC_TABLE is not None:
        return _MC_TABLE
    edge_id = {}
    for i, (a, b) in enumerate(_MC_EDGES):
        edge_id[(a, b)] = edge_id[(b, a)] = i
    tri = torch.full((256, 5, 3), -1, dtype=torch.int64)
    n_tri = torch.zeros(256, dtype=torch.int64)
    for case in range(256):
        inside = [(case >> i) & 1 for i in range(8)]
        nxt = {}
        for face in _MC_FACES:
            ins = [inside[c] for c in face]
            if all(ins) or not any(ins):
                continue
            for k in range(4):
                # a run of inside corners starts at corner k (its predecessor is outside) ...
                if ins[k] and not ins[k - 1]:
                    j = k
                    while ins[(j + 1) % 4]:
                        j += 1
                    # ... and ends at corner j: the segment runs from the edge entering the run to the edge leaving it
                    e_in = edge_id[(face[k - 1], face[k])]
                    e_out = edge_id[(face[j % 4], face[(j + 1) % 4])]
                    assert e_in not in nxt
                    nxt[e_in] = e_out
        tris = []
        todo = set(nxt)
        while todo:
            start = min(todo)
            loop, e = [], start
            while True:
                loop.append(e); todo.discard(e)
                e = nxt[e]
                if e == start:
                    break
            tris += _triangulate_loop(loop)
        assert len(tris) <= 5, (case, tris)
        n_tri[case] = len(tris)
        for t, abc in enumerate(tris):
            tri[case, t] = torch.tensor(abc)
    _MC_TABLE = (tri, n_tri)
    return _MC_TABLE


def marching_cubes(u: torch.Tensor, threshold: float, bound_min, bound_max):
    """Table-driven marching cubes on u [N,N,N] (u = -sdf, inside > threshold): same interface, vertex welding (by grid edge) and
    orientation as marching_tetrahedra; about a third of its triangles.  N <= 1448 (MAX_DENSE_RESOLUTION: the weld key min * N^3 +
    max of an edge's two linear indices must fit int64; ValueError beyond).  mesh_extract.sparse_marching_cubes builds the same mesh
    from the blocks near the surface with a key that fits at any N."""
    dev = u.device
    N = u.shape[0]
    _check_weld_key_range("marching_cubes", N)
    bmin = torch.as_tensor(bound_min, dtype=torch.float32, device=dev)
    bmax = torch.as_tensor(bound_max, dtype=torch.float32, device=dev)
    f = u - threshold
    sl = (slice(0, N - 1), slice(1, N))
    case = torch.zeros((N - 1, N - 1, N - 1), dtype=torch.int64, device=dev)
    for i, (dx, dy, dz) in enumerate(_MC_CORNERS.tolist()):
        case |= (f[sl[dx], sl[dy], sl[dz]] > 0).to(torch.int64) << i
    tri_t, n_t = marching_cubes_table()
    tri_t, n_t = tri_t.to(dev), n_t.to(dev)
    base = ((case != 0) & (case != 255)).nonzero()                                # [C,3] active cells
    if base.shape[0] == 0:
        return torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev)
    ccase = case[base[:, 0], base[:, 1], base[:, 2]]
    ea = torch.tensor([e[0] for e in _MC_EDGES], device=dev)
    eb = torch.tensor([e[1] for e in _MC_EDGES], device=dev)
    corners = _MC_CORNERS.to(dev)
    NN = N * N * N
    pos_all, key_all = [], []
    for t in range(5):
        sel = n_t[ccase] > t
        if not bool(sel.any()):
            break
        cell = base[sel]                                                          # [M,3]
        edges = tri_t[ccase[sel], t]                                              # [M,3] edge ids
        ca = cell[:, None, :] + corners[ea[edges]]                                # [M,3,3] corner a of each edge
        cb = cell[:, None, :] + corners[eb[edges]]
        ia = (ca[..., 0] * N + ca[..., 1]) * N + ca[..., 2]
        ib = (cb[..., 0] * N + cb[..., 1]) * N + cb[..., 2]
        va = f[ca[..., 0], ca[..., 1], ca[..., 2]]
        vb = f[cb[..., 0], cb[..., 1], cb[..., 2]]
        # the crossing is computed from the corner with the lower linear index, whichever cell asks (identical bits everywhere)
        sw = ia > ib
        p0 = torch.where(sw[..., None], cb, ca).float(); p1 = torch.where(sw[..., None], ca, cb).float()
        v0 = torch.where(sw, vb, va); v1 = torch.where(sw, va, vb)
        tt = (v0 / (v0 - v1)).clamp(0, 1).unsqueeze(-1)
        pos_all.append(p0 + tt * (p1 - p0))
        key_all.append(torch.minimum(ia, ib) * NN + torch.maximum(ia, ib))
    flat = torch.cat(pos_all, dim=0).reshape(-1, 3)
    key = torch.cat(key_all, dim=0).reshape(-1)
    uniq, inv = torch.unique(key, return_inverse=True)
    verts = torch.zeros(uniq.shape[0], 3, device=dev).index_copy_(0, inv, flat)
    faces = inv.reshape(-1, 3)
    ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    faces = faces[ok]
    verts = verts / (N - 1) * (bmax - bmin) + bmin
    return verts, faces


def write_ply(path: str, verts: torch.Tensor, faces: torch.Tensor, colors=None):
    """Binary little-endian PLY: float x y z per vertex, then the triangles.  colors: u8 [V,3] per-vertex red, green, blue (vertex
    element gains `property uchar red/green/blue`); None writes geometry only."""
    v = verts.detach().cpu().numpy().astype(np.float32)
    f = faces.detach().cpu().numpy().astype(np.int32)
    if colors is not None:
        c = colors.detach().cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors)
        if c.dtype != np.uint8 or c.shape != (len(v), 3):
            raise ValueError(f"write_ply: colors must be uint8 [{len(v)},3], got {c.dtype} {c.shape}")
    with open(path, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                  "property float z\n%selement face %d\nproperty list uchar int vertex_indices\nend_header\n"
                  % (len(v), "" if colors is None else "property uchar red\nproperty uchar green\nproperty uchar blue\n",
                     len(f))).encode())
        if colors is None:
            fh.write(v.tobytes())
        else:
            rec = np.empty(len(v), dtype=[("p", "<f4", (3,)), ("c", "u1", (3,))])
            rec["p"] = v
            rec["c"] = c
            fh.write(rec.tobytes())
        rec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        rec["n"] = 3
        rec["i"] = f
        fh.write(rec.tobytes())
