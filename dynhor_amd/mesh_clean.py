"""Mesh cleaning before evaluation, as the NeuS line of papers does it: cull the mesh with the object masks of every view, then keep
the largest connected component.

  * ``dilate_labels``: keep map u8 [F,H,W] = 1 where a (2r+1)^2 window holds an object OR hand pixel (csrc/mesh_clean.hip,
    dh_label_dilate).  A hand pixel hides whatever lies behind it, so it never removes a vertex: the keep-mask rule of the losses
    (label >= 0 is "not hand-occluded"); geometry the hand occludes in one frame is judged by the frames where it is visible.
  * ``mask_votes``: per vertex, the frames that see it (in front of the camera, inside the image) and, of those, the frames whose
    keep map is 0 at its pixel (dh_mesh_mask_votes); ``cull_by_masks`` removes the vertices with at least ``min_bg_votes`` such
    background votes and every face that touches one.
  * ``vertex_components`` (dh_mesh_components): the component of every vertex, labelled by its smallest vertex index;
    ``keep_components`` keeps the component of largest total face area (or every component of at least ``min_area_frac`` of it).

Every removal ends with a stable compaction: unreferenced vertices are dropped, the survivors keep their relative order and the faces
are re-indexed, so a cleaned mesh is an exact sub-mesh of its input.  The kernels run on the current stream; there is no CPU path, and
nothing is read back from the device except the sizes of the compacted mesh (and the counts ``clean_mesh`` reports).
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import check_faces, check_poses, device_tensor

MODES = ("none", "mask", "largest", "mask+largest")


def dilate_labels(label: torch.Tensor, radius: int) -> torch.Tensor:
    """keep u8 [F,H,W] from a label map i8 [F,H,W] (1 object / 0 background / -1 hand): 1 where the square window of half-width
    `radius` (clipped to the image) holds a label != 0.  radius 0 = (label != 0)."""
    label = device_tensor("dilate_labels", "label", label, torch.int8, lambda s: len(s) == 3, "[F,H,W]")
    if int(radius) < 0:
        raise ValueError(f"dilate_labels: radius must be >= 0, got {radius}")
    F, H, W = label.shape
    keep = torch.empty(label.shape, dtype=torch.uint8, device=label.device)
    if label.numel() == 0:
        return keep
    with torch.cuda.device(label.device):
        tmp = torch.empty_like(keep)
        _lib.check(_lib.lib().dh_label_dilate(_lib.ptr(label), F, H, W, int(radius), _lib.ptr(tmp), _lib.ptr(keep), _lib.stream()))
    return keep


def mask_votes(verts: torch.Tensor, keep: torch.Tensor, R: torch.Tensor, T: torch.Tensor, K: torch.Tensor):
    """(bg_votes, seen), int32 [V]: for every vertex, the frames in which it projects inside the image in front of the camera (x_cam =
    R_f v + T_f, pixel round(K x_cam / z)), and of those the frames whose keep map is 0 at its pixel.  keep u8 [F,H,W]
    (dilate_labels), R [F,3,3], T [F,3], K [3,3] float32 (Dataset.R / T / K)."""
    verts = device_tensor("mask_votes", "verts", verts, torch.float32, lambda s: len(s) == 2 and s[1] == 3, "[V,3]")
    keep, R, T, K = check_poses("mask_votes", keep, R, T, K)
    if verts.device != keep.device:
        raise ValueError(f"mask_votes: verts on {verts.device}, keep on {keep.device}")
    F, H, W = keep.shape
    if H == 0 or W == 0:
        raise ValueError(f"mask_votes: empty images {H}x{W}")
    nv = verts.shape[0]
    bg = torch.empty(nv, dtype=torch.int32, device=verts.device)
    seen = torch.empty(nv, dtype=torch.int32, device=verts.device)
    with torch.cuda.device(verts.device):
        _lib.check(_lib.lib().dh_mesh_mask_votes(_lib.ptr(verts), nv, _lib.ptr(keep), _lib.ptr(R), _lib.ptr(T), _lib.ptr(K), F, H, W,
                                                 _lib.ptr(bg), _lib.ptr(seen), _lib.stream()))
    return bg, seen


def vertex_components(n_verts: int, faces: torch.Tensor) -> torch.Tensor:
    """labels int32 [n_verts]: the smallest vertex index of each vertex's connected component (edges: the three edges of every face;
    a vertex in no face is its own component).  Bitwise reproducible."""
    faces = check_faces("vertex_components", faces)
    n_verts = int(n_verts)
    if n_verts < 0:
        raise ValueError(f"vertex_components: n_verts must be >= 0, got {n_verts}")
    labels = torch.empty(n_verts, dtype=torch.int32, device=faces.device)
    with torch.cuda.device(faces.device):
        _lib.check(_lib.lib().dh_mesh_components(_lib.ptr(faces), faces.shape[0], n_verts, _lib.ptr(labels), _lib.stream()))
    return labels


def _compact(verts, faces, face_keep):
    """The sub-mesh of the kept faces: vertices no kept face references are dropped, the others keep their order."""
    f = faces[face_keep]
    used = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
    used[f.reshape(-1)] = True
    new_index = torch.cumsum(used, 0) - 1
    return verts[used], new_index[f]


def cull_by_masks(verts, faces, keep, R, T, K, min_bg_votes: int = 1):
    """Removes every vertex with at least `min_bg_votes` background votes (mask_votes) and every face that touches one, then compacts."""
    faces = check_faces("cull_by_masks", faces)
    if int(min_bg_votes) < 1:
        raise ValueError(f"cull_by_masks: min_bg_votes must be >= 1, got {min_bg_votes}")
    bg, _ = mask_votes(verts, keep, R, T, K)
    gone = bg >= int(min_bg_votes)
    return _compact(verts, faces, ~gone[faces].any(dim=1))


def _component_areas(verts, faces, labels):
    """(component label of every face, total face area per label [V] float64).  The per-label sums are a segment reduction over the
    faces sorted by label (stable sort): a fixed order, no float atomics."""
    lab = labels[faces[:, 0]].long()
    v = verts.double()
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    area = 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1)
    order = torch.sort(lab, stable=True).indices
    counts = torch.bincount(lab, minlength=verts.shape[0])
    comp = torch.segment_reduce(area[order], "sum", lengths=counts, unsafe=True)
    return lab, comp


def _count_components(n_verts, faces, labels):
    """Components that hold at least one face."""
    roots = torch.zeros(n_verts, dtype=torch.bool, device=faces.device)
    roots[labels[faces.reshape(-1)].long()] = True
    return int(roots.sum())


def keep_components(verts, faces, min_area_frac=None):
    """Keeps the connected component of largest total face area (ties: the smaller label), or, with min_area_frac = f, every
    component whose area is at least f x the largest; then compacts."""
    verts = device_tensor("keep_components", "verts", verts, torch.float32, lambda s: len(s) == 2 and s[1] == 3, "[V,3]")
    faces = check_faces("keep_components", faces)
    if faces.shape[0] == 0:
        return _compact(verts, faces, torch.zeros(0, dtype=torch.bool, device=faces.device))
    labels = vertex_components(verts.shape[0], faces)
    lab, comp = _component_areas(verts, faces, labels)
    best = torch.argmax(comp)                               # the first maximum: the smaller label on a tie
    if min_area_frac is None:
        face_keep = lab == best
    else:
        face_keep = comp[lab] >= float(min_area_frac) * comp[best]
    return _compact(verts, faces, face_keep)


def keep_map(dataset, radius: int) -> torch.Tensor:
    """The dataset's dilated keep maps at `radius`, cached on the dataset: one u8 copy of the labels at most (a new radius replaces
    the cached one)."""
    cached = getattr(dataset, "_clean_keep", None)
    if cached is None or cached[0] != int(radius):
        dataset._clean_keep = None
        dataset._clean_keep = (int(radius), dilate_labels(dataset.label, int(radius)))
    return dataset._clean_keep[1]


def clean_mesh(verts, faces, dataset, mode: str = "mask+largest", dilate_px: int = 2, min_bg_votes: int = 1, min_area_frac=None):
    """The cleaning pipeline on an extracted mesh: "none" | "mask" | "largest" | "mask+largest".  Mask culling runs first, with the
    dataset's labels and its current poses (Dataset.R / T: refined in place when pose refinement is on), so that a floater joined to
    the object only through background space is cut off before the component pass.  Returns (verts, faces, stats): the vertices and
    faces each stage removed and the number of connected components of the mesh the component stage sees."""
    if mode not in MODES:
        raise ValueError(f"clean_mesh: mode must be one of {MODES}, got {mode!r}")
    verts = device_tensor("clean_mesh", "verts", verts, torch.float32, lambda s: len(s) == 2 and s[1] == 3, "[V,3]")
    faces = check_faces("clean_mesh", faces)
    stats = {"mode": mode, "verts_in": int(verts.shape[0]), "faces_in": int(faces.shape[0])}
    v, f = verts, faces
    if mode == "none":
        stats.update(removed_verts=0, removed_faces=0)
        return v, f, stats
    if "mask" in mode:
        v1, f1 = cull_by_masks(v, f, keep_map(dataset, dilate_px), dataset.R, dataset.T, dataset.K, min_bg_votes)
        stats.update(mask_removed_verts=int(v.shape[0] - v1.shape[0]), mask_removed_faces=int(f.shape[0] - f1.shape[0]))
        v, f = v1, f1
    stats["components"] = _count_components(v.shape[0], f, vertex_components(v.shape[0], f)) if f.shape[0] else 0
    if "largest" in mode:
        v1, f1 = keep_components(v, f, min_area_frac)
        stats.update(components_removed_verts=int(v.shape[0] - v1.shape[0]), components_removed_faces=int(f.shape[0] - f1.shape[0]))
        v, f = v1, f1
    stats.update(removed_verts=int(verts.shape[0] - v.shape[0]), removed_faces=int(faces.shape[0] - f.shape[0]))
    return v, f, stats
