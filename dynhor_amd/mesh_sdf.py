"""Signed distance from arbitrary points to a triangle mesh (csrc/mesh_sdf.hip; include/dynhor_hip.h dh_mesh_sdf_*).

    m = MeshSDF(verts, faces)                 # one record per face, prepared once on the device
    sdf, face, wind = m.query(pts)            # [N] fp32 signed distance, [N] int64 nearest face, [N] fp32 winding number

The distance is exact brute force over every (point, face) pair (closest point on the triangle by regions, the distance in the
difference form); the sign comes from the generalised winding number: inside (negative, the SDF networks' convention) where
wind >= 0.5.  That rule needs no closed manifold -- a mesh with seams or small holes (a Meshlab export) still has wind ~ 1 inside and
~ 0 outside away from the hole -- but next to a hole wind passes 0.5 on a surface that merely spans the rim, and for a mesh whose
faces are not oriented consistently the winding number means nothing.  The cost is N x F pairs: a template beyond about 10^5 faces
should be simplified first (dynhor_amd/mesh_simplify.py, --mesh_simplify).  Device tensors only: there is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib

DEFAULT_CHUNK = 1 << 16        # points per launch of query(): bounds the slab scratch (16 bytes x slabs x chunk)


class MeshSDF:
    """The face records of one mesh (dh_mesh_sdf_prepare).  verts [V,3] float, faces [F,3] integer, device tensors.  The index range
    is validated here, once per mesh (one device read); the kernel itself skips a face it cannot read."""

    def __init__(self, verts: torch.Tensor, faces: torch.Tensor):
        for name, t in (("verts", verts), ("faces", faces)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise _lib.DynhorHipError(f"MeshSDF: {name} must be a device tensor (the HIP kernel has no CPU fallback)")
            if t.dim() != 2 or t.shape[1] != 3:
                raise ValueError(f"MeshSDF: {name} must be [N,3], got {tuple(t.shape)}")
        if verts.device != faces.device:
            raise ValueError(f"MeshSDF: verts on {verts.device}, faces on {faces.device}")
        if faces.dtype.is_floating_point or faces.dtype == torch.bool:
            raise ValueError(f"MeshSDF: faces must be integers, got {faces.dtype}")
        if faces.shape[0] == 0:
            raise ValueError("MeshSDF: the mesh has no faces")
        nv = int(verts.shape[0])
        if bool(((faces < 0) | (faces >= nv)).any()):
            raise ValueError(f"MeshSDF: face indices outside [0, {nv})")
        self._prepare(verts, faces)

    @classmethod
    def unchecked(cls, verts: torch.Tensor, faces: torch.Tensor):
        """The records without the index check (tests of the kernel's own handling of a face it cannot read)."""
        self = cls.__new__(cls)
        self._prepare(verts, faces)
        return self

    def _prepare(self, verts, faces):
        L = _lib.lib()
        self.device = verts.device
        v = verts.detach().to(torch.float32).contiguous()
        f = faces.detach().to(torch.int32).contiguous()
        self.n_verts, self.n_faces = int(v.shape[0]), int(f.shape[0])
        with torch.cuda.device(self.device):
            self.rec = torch.empty(self.n_faces, int(L.dh_mesh_sdf_record_floats()), device=self.device, dtype=torch.float32)
            _lib.check(L.dh_mesh_sdf_prepare(_lib.ptr(v) if self.n_verts else None, self.n_verts, _lib.ptr(f), self.n_faces,
                                             _lib.ptr(self.rec), _lib.stream()))
        self._ws = None

    def _workspace(self, n: int):
        nbytes = int(_lib.lib().dh_mesh_sdf_query_workspace(n, self.n_faces))
        if nbytes < 0:
            _lib.check(nbytes)
        if nbytes == 0:
            return None
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def query_raw(self, pts: torch.Tensor, chunk: int | None = None, want_face: bool = True, want_wind: bool = True):
        """(sqdist [N] fp32, face [N] int32 or None, wind [N] fp32 or None) as dh_mesh_sdf_query returns them, the points in launches
        of `chunk` (the results do not depend on it, bit for bit).  No host synchronisation."""
        if not torch.is_tensor(pts) or not pts.is_cuda:
            raise _lib.DynhorHipError("MeshSDF.query: pts must be a device tensor (the HIP kernel has no CPU fallback)")
        if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"MeshSDF.query: pts must be float32 [N,3], got {pts.dtype} {tuple(pts.shape)}")
        if pts.device != self.device:
            raise ValueError(f"MeshSDF.query: pts on {pts.device}, the mesh on {self.device}")
        chunk = DEFAULT_CHUNK if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError(f"MeshSDF.query: chunk must be positive, got {chunk}")
        pts = pts.contiguous()
        n = int(pts.shape[0])
        L = _lib.lib()
        with torch.cuda.device(self.device):
            d2 = torch.empty(n, device=self.device)
            face = torch.empty(n, dtype=torch.int32, device=self.device) if want_face else None
            wind = torch.empty(n, device=self.device) if want_wind else None
            ws = self._workspace(min(n, chunk))
            for s in range(0, n, chunk):
                m = min(chunk, n - s)
                _lib.check(L.dh_mesh_sdf_query(_lib.ptr(self.rec), self.n_faces, _lib.ptr(pts[s:s + m]), m, _lib.ptr(d2[s:s + m]),
                                               _lib.ptr(face[s:s + m]) if want_face else None,
                                               _lib.ptr(wind[s:s + m]) if want_wind else None,
                                               _lib.ptr(ws) if ws is not None else None, _lib.stream()))
        return d2, face, wind

    def query(self, pts: torch.Tensor, chunk: int | None = None):
        """(sdf [N] fp32, face [N] int64, wind [N] fp32): sdf = sqrt(sqdist), negated where wind >= 0.5 (inside is negative).  A
        non-finite point has sdf = +inf, face = -1, wind = 0."""
        d2, face, wind = self.query_raw(pts, chunk)
        d = torch.sqrt(d2)
        return torch.where(wind >= 0.5, -d, d), face.long(), wind


def mesh_signed_distance(pts: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor):
    """MeshSDF(verts, faces).query(pts) in one call."""
    return MeshSDF(verts, faces).query(pts)
