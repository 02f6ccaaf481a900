"""Geometry metrics: a reconstructed mesh scored against a ground-truth surface (Chamfer distance, F-score, normal consistency).

The definitions are those of the NeuS / HHOR line of papers, on point samples of the two surfaces:

  * sample n points on each mesh (``sample_surface``: area-weighted, uniform inside each triangle, each with its face normal);
  * P->G = every prediction sample's distance to its nearest ground-truth sample, G->P the reverse (``nearest_sqdist``: exact
    brute force in HIP, csrc/nn.hip -- about 10^12 point pairs at n = 10^6; there is no CPU path);
  * accuracy = mean P->G, completeness = mean G->P, chamfer_l1 = (accuracy + completeness) / 2,
    chamfer_l2 = mean (P->G)^2 + mean (G->P)^2;
  * for every threshold tau: precision@tau = fraction of P->G < tau, recall@tau = fraction of G->P < tau,
    fscore@tau = 2 P R / (P + R), and 0 when both are 0;
  * normal_consistency = mean over both directions of |n . n_nn|, n_nn the normal of the nearest sample on the other mesh.

Distances are in the frame the meshes are given in -- for this project the canonical object frame (the object inside the
radius-0.5 ball; dataset.py ``_load_from_disk``).  ``normalize_like_reference`` brings a ground-truth mesh in its own units into
that frame the way the reference normalises its shape prior; the metrics then carry ``gt_scale``, the factor from canonical
back to ground-truth units.  That fixes no rotation and depends on the scan's tessellation: ``mesh_metrics(gt_align=...)`` registers
the ground truth to the prediction by trimmed similarity ICP first (dynhor_amd/mesh_align.py; off by default).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib


# ------------------------------------------------------------------------------------------------ nearest neighbour (HIP)
def nearest_sqdist(q: torch.Tensor, ref: torch.Tensor, return_index: bool = False):
    """d2[i] = min_j |q[i] - ref[j]|^2 for device tensors q [N,3], ref [M,3] float32 (dh_nearest_sqdist: exact fp32 difference
    form, bitwise reproducible).  With return_index also idx[i] (int64), the smallest j that attains it.  A CPU tensor raises
    DynhorHipError: there is no fallback."""
    for name, t in (("q", q), ("ref", ref)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.DynhorHipError(f"nearest_sqdist: {name} must be a device tensor (the HIP kernel has no CPU fallback)")
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"nearest_sqdist: {name} must be float32 [N,3], got {t.dtype} {tuple(t.shape)}")
    if q.device != ref.device:
        raise ValueError(f"nearest_sqdist: q on {q.device}, ref on {ref.device}")
    q, ref = q.contiguous(), ref.contiguous()
    nq, nr = q.shape[0], ref.shape[0]
    L = _lib.lib()
    with torch.cuda.device(q.device):
        d2 = torch.empty(nq, device=q.device)
        idx = torch.empty(nq, dtype=torch.int32, device=q.device) if return_index else None
        nbytes = int(L.dh_nearest_sqdist_workspace(nq, nr))
        if nbytes < 0:
            _lib.check(nbytes)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if nbytes > 0 else None
        _lib.check(L.dh_nearest_sqdist(_lib.ptr(q), nq, _lib.ptr(ref), nr, _lib.ptr(d2), _lib.ptr(idx) if idx is not None else None,
                                       _lib.ptr(ws) if ws is not None else None, _lib.stream()))
    return (d2, idx.long()) if return_index else d2


# ------------------------------------------------------------------------------------------------ mesh files
def load_mesh(path: str):
    """(verts [V,3] float32, faces [F,3] int64) CPU tensors from a .obj (``v`` and ``f`` lines; faces ``a``, ``a/b``, ``a//c``
    or ``a/b/c``, negative = relative indices; polygons fan-triangulated; everything else ignored) or a .ply (ASCII or binary
    little-endian; triangles and polygons, fan-triangulated).  Other formats raise ValueError."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".obj":
        return _load_obj(path)
    if ext == ".ply":
        return _load_ply(path)
    raise ValueError(f"load_mesh: unsupported mesh format {ext!r} ({path}); use .obj or .ply")


def _fan(polys):
    """Fan triangulation of index lists: (i0, i_k, i_k+1)."""
    tris = [(p[0], p[k], p[k + 1]) for p in polys for k in range(1, len(p) - 1)]
    return torch.tensor(tris, dtype=torch.int64).reshape(-1, 3)


def _load_obj(path):
    verts, polys = [], []
    with open(path, "r") as fh:
        for line in fh:
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(x) for x in tok[1:4]])
            elif tok[0] == "f":
                poly = []
                for t in tok[1:]:
                    i = int(t.split("/", 1)[0])
                    poly.append(i - 1 if i > 0 else len(verts) + i)
                polys.append(poly)
    v = torch.tensor(verts, dtype=torch.float32).reshape(-1, 3)
    f = _fan(polys)
    _check_indices(f, v.shape[0], path)
    return v, f


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def load_ply_colors(path: str):
    """u8 [V,3] CPU tensor of the red / green / blue vertex properties of a .ply (the file mesh.write_ply writes for a coloured mesh), in
    load_mesh's vertex order; None when the file has none."""
    return _load_ply(path, with_colors=True)[2]


def _load_ply(path, with_colors=False):
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"load_mesh: {path} is not a PLY file")
    body = data.index(b"\n", end) + 1
    fmt, elements = None, []           # elements: [name, count, [(prop, type) or (prop, (count_type, item_type))]]
    for line in data[:end].decode("ascii", "replace").splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if tok[1] == "list":
                elements[-1][2].append((tok[4], (_PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]])))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"load_mesh: PLY format {fmt!r} of {path} is not supported (ascii or binary_little_endian)")
    reader = _PlyAscii(data[body:]) if fmt == "ascii" else _PlyBinary(data, body)
    verts, polys, colors = None, [], None
    for name, count, props in elements:
        rows = reader.element(count, props)
        if name == "vertex":
            if with_colors and all(c in rows for c in ("red", "green", "blue")):
                colors = torch.from_numpy(np.stack([np.asarray(rows[c], np.float64) for c in ("red", "green", "blue")], axis=1)
                                          .round().clip(0, 255).astype(np.uint8))
            verts = np.stack([np.asarray(rows["x"], np.float64), np.asarray(rows["y"], np.float64),
                              np.asarray(rows["z"], np.float64)], axis=1)
        elif name == "face":
            key = "vertex_indices" if "vertex_indices" in rows else "vertex_index"
            polys = rows[key]
    if verts is None:
        raise ValueError(f"load_mesh: {path} has no vertex element")
    v = torch.from_numpy(verts.astype(np.float32)).reshape(-1, 3)
    if isinstance(polys, np.ndarray):                      # every face a triangle: read as one block
        f = torch.from_numpy(polys.astype(np.int64)).reshape(-1, 3)
    else:
        f = _fan([[int(i) for i in p] for p in polys])
    _check_indices(f, v.shape[0], path)
    return (v, f, colors) if with_colors else (v, f)


class _PlyBinary:
    def __init__(self, data, pos):
        self.data, self.pos = data, pos

    def element(self, count, props):
        """dict prop -> array (scalars) or [count, k] array / list of arrays (lists)."""
        if all(isinstance(t, str) for _, t in props):
            dt = np.dtype([(n, "<" + t) for n, t in props])
            a = np.frombuffer(self.data, dtype=dt, count=count, offset=self.pos)
            self.pos += dt.itemsize * count
            return {n: a[n] for n, _ in props}
        if len(props) == 1 and count > 0:
            # one list per row (the usual face element): try the uniform-length block first
            name, (ct, it) = props[0]
            k = int(np.frombuffer(self.data, dtype="<" + ct, count=1, offset=self.pos)[0])
            dt = np.dtype([("n", "<" + ct), ("i", "<" + it, (k,))])
            if self.pos + dt.itemsize * count <= len(self.data):
                a = np.frombuffer(self.data, dtype=dt, count=count, offset=self.pos)
                if (a["n"] == k).all():
                    self.pos += dt.itemsize * count
                    return {name: a["i"] if k == 3 else list(a["i"])}
        out = {n: [] for n, _ in props}
        for _ in range(count):
            for n, t in props:
                if isinstance(t, str):
                    v = np.frombuffer(self.data, dtype="<" + t, count=1, offset=self.pos)[0]
                    self.pos += np.dtype(t).itemsize
                else:
                    k = int(np.frombuffer(self.data, dtype="<" + t[0], count=1, offset=self.pos)[0])
                    self.pos += np.dtype(t[0]).itemsize
                    v = np.frombuffer(self.data, dtype="<" + t[1], count=k, offset=self.pos)
                    self.pos += np.dtype(t[1]).itemsize * k
                out[n].append(v)
        return out


class _PlyAscii:
    def __init__(self, body):
        self.lines = iter(body.decode("ascii", "replace").splitlines())

    def element(self, count, props):
        out = {n: [] for n, _ in props}
        for _ in range(count):
            tok = next(self.lines).split()
            while not tok:
                tok = next(self.lines).split()
            p = 0
            for n, t in props:
                if isinstance(t, str):
                    out[n].append(float(tok[p])); p += 1
                else:
                    k = int(tok[p])
                    out[n].append([int(x) for x in tok[p + 1:p + 1 + k]]); p += 1 + k
        return out


def _check_indices(f, n_verts, path):
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= n_verts):
        raise ValueError(f"load_mesh: {path} has face indices outside its {n_verts} vertices")


def normalize_like_reference(verts: torch.Tensor):
    """The stage-1 canonical frame of the reference (its shape prior's normalisation): subtract the vertex mean, then scale so
    that the largest vertex norm is 0.5.  Returns (verts', center [3], scale) with verts' = (verts - center) * scale, so
    verts = verts' / scale + center."""
    v = verts.double()
    center = v.mean(dim=0)
    scale = 0.5 / float((v - center).norm(dim=1).max())
    return ((v - center) * scale).to(verts.dtype), center.to(verts.dtype), scale


def check_align_args(fn, gt_align, gt_align_init):
    """ValueError unless gt_align is none | rigid | similarity and gt_align_init is identity | global."""
    if gt_align not in ("none", "rigid", "similarity"):
        raise ValueError(f"{fn}: gt_align must be 'none', 'rigid' or 'similarity', got {gt_align!r}")
    if gt_align_init not in ("identity", "global"):
        raise ValueError(f"{fn}: gt_align_init must be 'identity' or 'global', got {gt_align_init!r}")


def aligned_ground_truth(gt_v: torch.Tensor, res: dict, gt_normalize: str = "none") -> torch.Tensor:
    """The ground-truth vertices in the prediction's frame, from the file's vertices and a mesh_metrics result that carries an
    alignment: normalize_like_reference first when gt_normalize is "reference", then align_scale align_R x + align_t (fp64)."""
    from .mesh_align import apply_transform
    if gt_normalize == "reference":
        gt_v = normalize_like_reference(gt_v)[0]
    return apply_transform(gt_v, res["align_scale"], res["align_R"], res["align_t"])


# ------------------------------------------------------------------------------------------------ surface sampling
def sample_surface(verts: torch.Tensor, faces: torch.Tensor, n: int, generator, return_faces: bool = False):
    """n points on the mesh, on the device of `verts`: a triangle is drawn with probability proportional to its area (CDF in
    fp64; zero-area triangles are never drawn), a point uniformly inside it (barycentric sqrt(r1) rule).  Returns (points [n,3]
    float32, normals [n,3] float32 unit face normals[, face index [n] int64]).  generator: a torch.Generator on that device, or
    an int seed; the same seed gives the same samples."""
    dev = verts.device
    if not isinstance(generator, torch.Generator):
        generator = torch.Generator(device=dev).manual_seed(int(generator))
    faces = faces.to(dev).long()
    if faces.shape[0] == 0:
        raise ValueError("sample_surface: the mesh has no faces")
    tri = verts.double()[faces]                                                   # [F,3,3]
    cr = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = 0.5 * cr.norm(dim=1)
    cdf = torch.cumsum(area, 0)
    total = float(cdf[-1])
    if not (total > 0.0):
        raise ValueError("sample_surface: the mesh has no area (every triangle is degenerate)")
    cdf = cdf / cdf[-1]
    u = torch.rand(n, dtype=torch.float64, device=dev, generator=generator)
    # first triangle whose CDF exceeds u: a zero-area triangle repeats its predecessor's CDF and can never be that one
    fi = torch.searchsorted(cdf, u, right=True).clamp_(max=faces.shape[0] - 1)
    r = torch.rand(n, 2, dtype=torch.float64, device=dev, generator=generator)
    s = r[:, 0].sqrt()
    w = torch.stack([1.0 - s, s * (1.0 - r[:, 1]), s * r[:, 1]], dim=1)          # barycentric weights
    t = tri[fi]
    pts = (w[:, :, None] * t).sum(dim=1)
    nrm = cr[fi] / cr[fi].norm(dim=1, keepdim=True)
    out = (pts.float().contiguous(), nrm.float().contiguous())
    return out + (fi,) if return_faces else out


# ------------------------------------------------------------------------------------------------ metrics
def _key(name, tau):
    return f"{name}@{tau:g}"


def distance_metrics(d2_pg: torch.Tensor, d2_gp: torch.Tensor, taus=(0.005, 0.01, 0.02)) -> dict:
    """The distance metrics of the module docstring from the squared nearest distances P->G [n] and G->P [m] (any device)."""
    if d2_pg.numel() == 0 or d2_gp.numel() == 0:
        raise ValueError("distance_metrics: empty distance arrays")
    a2, c2 = d2_pg.double(), d2_gp.double()
    a, c = a2.sqrt(), c2.sqrt()
    acc, comp = float(a.mean()), float(c.mean())
    out = {"accuracy": acc, "completeness": comp, "chamfer_l1": 0.5 * (acc + comp), "chamfer_l2": float(a2.mean()) + float(c2.mean())}
    for tau in taus:
        p, r = float((a < tau).double().mean()), float((c < tau).double().mean())
        out[_key("precision", tau)] = p
        out[_key("recall", tau)] = r
        out[_key("fscore", tau)] = 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0
    return out


def mesh_metrics(pred_v, pred_f, gt_v, gt_f, n_samples: int = 1_000_000, taus=(0.005, 0.01, 0.02), seed: int = 0,
                 gt_normalize: str = "none", device=None, gt_align: str = "none", gt_align_init: str = "identity",
                 align_opts: dict | None = None) -> dict:
    """Score the predicted mesh (pred_v [V,3], pred_f [F,3]) against the ground truth (gt_v, gt_f); the metric definitions are in
    the module docstring.  n_samples points on each mesh, drawn from one generator seeded with `seed` (prediction first).
    gt_normalize "reference": the ground truth is first brought into the canonical frame by normalize_like_reference, and the
    result carries gt_scale (canonical -> ground-truth units) besides the metrics, n_samples, n_pred_faces and n_gt_faces.
    The sampling and the nearest-neighbour search run on `device` (default: the device of pred_v if it is one, else the current
    one).  An empty predicted (or ground-truth) mesh raises ValueError.
    gt_align "rigid" | "similarity": the ground truth (after gt_normalize, which is then simply the initial guess) is first registered
    to the prediction by trimmed ICP (mesh_align.align_meshes; gt_align_init "identity" starts there, "global" searches the rotations;
    align_opts over mesh_align.ALIGN_DEFAULTS, n_align included) on samples of a generator of its own, so the scoring samples of the
    prediction are the ones drawn without it.  The dict then gains gt_align, gt_align_init, align_scale, align_R (row-major list of
    9), align_t (x' = align_scale align_R x + align_t takes the normalised ground truth into the prediction's frame), the registration's
    stats prefixed align_, and gt_scale = 1 / (align_scale x normalisation scale), the total factor from canonical back to
    ground-truth units.  With "none" (the default) nothing of this runs and the dict is what it always was."""
    if gt_normalize not in ("none", "reference"):
        raise ValueError(f"mesh_metrics: gt_normalize must be 'none' or 'reference', got {gt_normalize!r}")
    check_align_args("mesh_metrics", gt_align, gt_align_init)
    if pred_f.shape[0] == 0 or pred_v.shape[0] == 0:
        raise ValueError("mesh_metrics: the predicted mesh is empty (no faces): the reconstruction has no surface to score "
                         "(is the zero level set inside the extraction box?)")
    if gt_f.shape[0] == 0 or gt_v.shape[0] == 0:
        raise ValueError("mesh_metrics: the ground-truth mesh is empty (no faces)")
    if device is None:
        device = pred_v.device if pred_v.is_cuda else torch.device("cuda", torch.cuda.current_device())
    extra = {}
    gt_v = gt_v.to(device, torch.float32)
    if gt_normalize == "reference":
        gt_v, _, scale = normalize_like_reference(gt_v)
        extra["gt_scale"] = 1.0 / scale
    if gt_align != "none":
        from . import mesh_align
        a_s, a_R, a_t, st = mesh_align.align_meshes(gt_v, gt_f, pred_v, pred_f, mode=gt_align, init=gt_align_init, seed=seed,
                                                    device=device, **(align_opts or {}))
        gt_v = mesh_align.apply_transform(gt_v, a_s, a_R, a_t)
        extra.update(gt_align=gt_align, gt_align_init=gt_align_init, align_scale=a_s, align_R=[float(x) for x in a_R.reshape(-1)],
                     align_t=[float(x) for x in a_t], gt_scale=extra.get("gt_scale", 1.0) / a_s,
                     **{"align_" + k: v for k, v in st.items()})
    g = torch.Generator(device=device).manual_seed(int(seed))
    p, pn = sample_surface(pred_v.to(device, torch.float32), pred_f, n_samples, g)
    q, qn = sample_surface(gt_v, gt_f, n_samples, g)
    d2_pg, i_pg = nearest_sqdist(p, q, return_index=True)
    d2_gp, i_gp = nearest_sqdist(q, p, return_index=True)
    out = distance_metrics(d2_pg, d2_gp, taus)
    nc = 0.5 * (float((pn * qn[i_pg]).sum(dim=1).abs().double().mean()) + float((qn * pn[i_gp]).sum(dim=1).abs().double().mean()))
    out["normal_consistency"] = nc
    out.update(n_samples=int(n_samples), n_pred_faces=int(pred_f.shape[0]), n_gt_faces=int(gt_f.shape[0]), **extra)
    return out
