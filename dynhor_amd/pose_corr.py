"""A correspondence term for the mesh pose refinement (dynhor_amd/pose_sil.py): dense matches between frames tie two poses directly.

The silhouette cannot see a rotation the outline does not show, and the photometric term needs colours on the mesh.  A match (pixel p
of frame i, position q in frame j, confidence c: Dataset.set_correspondences, --mode match_frames) needs neither.  The rule
(csrc/pose_corr.hip, include/dynhor_hip.h; fp64 from fp32 inputs):
  * the ray of p, d = K^-1 (p, 1), is cut with the plane of the mesh face that frame i's z-buffer (mesh_color.raster_depth at the
    current poses; only the face index is used) shows at p: o = -R_i^T T_i, e = R_i^T d, s = n.(a - o) / (n.e), X = o + s e;
  * X goes into frame j: Y = R_j X + T_j, (u, w) its projection, r = (u, w) - q, rho = huber(|r|; delta_px), weight c (constant);
  * a match counts when p lies in the image, the z-buffer holds a face there, the face has an area, |n.e| >= min_cos |n| |e|,
    s > 1e-3, Y_z > 1e-3, c > 0 and every input is finite.
``corr_sums`` (dh_pose_corr_sums) reduces every frame PAIR to 28 numbers: sum c rho, sum c, d/dR_i (9), d/dT_i (3), d/dR_j (9), d/dT_j
(3), the counted matches and those inside the Huber band; one lane per match, block-ordered fp64 sums, bitwise the same for every
order of the pairs and every split of them into calls.  ``frame_grads`` (dh_pose_corr_frames) folds the pairs' rows into per-frame
gradients in the fixed order of a list built once on the host.  ``CorrespondenceTerm`` holds the matches, the pair table and that list
on the device and rasterises the z-buffers of the source frames in chunks; bound to a ``SilhouettePoseOptimizer`` (``corr=``) it adds
lw_corr / n_live_pairs * rows / max(sum c, TINY) to the pose gradient (n_live_pairs = the pairs with a counted match); L_corr = the
mean over the live pairs of sum c rho / max(sum c, TINY).

Limits: matches alone leave one common rotation of the object frame free (keep a frame fixed, or compare relative rotations); one plane
per match, so on a coarse mesh the normal is a facet's; Huber is the only outlier handling; the matches are not refreshed while the
poses move.

The kernels run on the current stream; there is no CPU path.
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import check_cams, check_faces, check_verts, device_tensor
from .mesh_color import raster_depth

# defaults of the YAML's pose_corr: block; DESIGN_NEXT_ROWS.md section 24 says where each comes from
DEFAULTS = {"mode": "none", "lw_corr": 1e-3, "delta_px": 2.0, "min_cos": 0.1, "min_conf": 0.0}
MODES = ("none", "dataset", "match")
TINY = 1e-12


def corr_sums(verts, faces, R, T, K, zbuf, matches, pairs, max_count: int, delta_px: float = DEFAULTS["delta_px"],
              min_cos: float = DEFAULTS["min_cos"], resid=None) -> torch.Tensor:
    """float64 [n_pairs,28] on the device, the layout of dh_pose_corr_sums: [0] sum c rho, [1] sum c, [2..10] d/dR_i row-major,
    [11..13] d/dT_i, [14..22] d/dR_j, [23..25] d/dT_j, [26] counted matches, [27] those with |r| <= delta_px.  R, T: ALL frames; zbuf:
    raster_depth of the mesh at the poses of the source frames the pairs' slots name; matches f32 [M,5] = (p_x, p_y, q_x, q_y, c); pairs
    int64 [n_pairs,5] = (slot, i, j, first, count); max_count: a host-side bound on the counts.  resid f32 [M] (optional) receives |r|
    per match of these pairs, -1 where it does not count.  Nothing is read back."""
    fn = "corr_sums"
    verts = check_verts(fn, verts)
    faces = check_faces(fn, faces)
    zbuf = device_tensor(fn, "zbuf", zbuf, torch.int64, lambda s: len(s) == 3, "[n_z,H,W]")
    n_z, H, W = zbuf.shape
    if H == 0 or W == 0:
        raise ValueError(f"{fn}: empty images {H}x{W}")
    F = R.shape[0] if torch.is_tensor(R) and R.dim() >= 1 else -1
    R, T, K = check_cams(fn, F, R, T, K, zbuf.device)
    matches = device_tensor(fn, "matches", matches, torch.float32, lambda s: len(s) == 2 and s[1] == 5, "[M,5]")
    pairs = device_tensor(fn, "pairs", pairs, torch.int64, lambda s: len(s) == 2 and s[1] == 5, "[n_pairs,5]")
    M, n_pairs = matches.shape[0], pairs.shape[0]
    if resid is not None:
        resid = device_tensor(fn, "resid", resid, torch.float32, lambda s: s == (M,), f"[{M}]")
        if not resid.is_contiguous():
            raise ValueError(f"{fn}: resid must be contiguous")
    if any(t.device != zbuf.device for t in (verts, faces, matches, pairs) + (() if resid is None else (resid,))):
        raise ValueError(f"{fn}: every tensor must be on {zbuf.device}")
    max_count, delta_px, min_cos = int(max_count), float(delta_px), float(min_cos)
    if max_count < 0 or not delta_px > 0 or not 0.0 <= min_cos <= 1.0:
        raise ValueError(f"{fn}: max_count >= 0, delta_px > 0 and min_cos in [0, 1]; got {max_count}, {delta_px}, {min_cos}")
    L = _lib.lib()
    out = torch.empty(n_pairs, int(L.dh_pose_corr_width()), dtype=torch.float64, device=zbuf.device)
    if n_pairs == 0:
        return out
    with torch.cuda.device(zbuf.device):
        ws = torch.empty(max(16, int(L.dh_pose_corr_sums_workspace(n_pairs, max_count))), dtype=torch.uint8, device=zbuf.device)
        _lib.check(L.dh_pose_corr_sums(_lib.ptr(verts), verts.shape[0], _lib.ptr(faces), faces.shape[0], _lib.ptr(R), _lib.ptr(T),
                                       _lib.ptr(K), F, _lib.ptr(zbuf), n_z, H, W, _lib.ptr(matches), M, _lib.ptr(pairs), n_pairs, max_count,
                                       delta_px, min_cos, _lib.ptr(out), _lib.ptr(resid) if resid is not None else None, _lib.ptr(ws),
                                       _lib.stream()))
    return out


def frame_grads(rows, scale, start, entries):
    """(gR float64 [F,3,3], gT float64 [F,3]) on the device: frame f's sum, in list order, of scale[pair] * rows[pair, 2..13] (entry
    2 pair: f is the pair's i) or scale[pair] * rows[pair, 14..25] (entry 2 pair + 1: f is its j) over entries[start[f] : start[f+1]];
    rows float64 [n_pairs,28], scale float64 [n_pairs], start int64 [F+1], entries int64 [E].  Nothing is read back."""
    fn = "frame_grads"
    L = _lib.lib()
    width = int(L.dh_pose_corr_width())
    rows = device_tensor(fn, "rows", rows, torch.float64, lambda s: len(s) == 2 and s[1] == width, f"[n_pairs,{width}]")
    n_pairs = rows.shape[0]
    scale = device_tensor(fn, "scale", scale, torch.float64, lambda s: s == (n_pairs,), f"[{n_pairs}]")
    start = device_tensor(fn, "start", start, torch.int64, lambda s: len(s) == 1 and s[0] >= 1, "[F+1]")
    entries = device_tensor(fn, "entries", entries, torch.int64, lambda s: len(s) == 1, "[E]")
    if any(t.device != rows.device for t in (scale, start, entries)):
        raise ValueError(f"{fn}: every tensor must be on {rows.device}")
    F = start.shape[0] - 1
    gR = torch.empty(F, 3, 3, dtype=torch.float64, device=rows.device)
    gT = torch.empty(F, 3, dtype=torch.float64, device=rows.device)
    if F == 0:
        return gR, gT
    with torch.cuda.device(rows.device):
        _lib.check(L.dh_pose_corr_frames(_lib.ptr(rows), _lib.ptr(scale), n_pairs, _lib.ptr(start), _lib.ptr(entries), entries.shape[0], F,
                                         _lib.ptr(gR), _lib.ptr(gT), _lib.stream()))
    return gR, gT


def frame_list(pair_i, pair_j, n_frames: int):
    """(start [F+1], entries [E]) as Python lists: frame f's entries are 2 p (f == pair_i[p]) and 2 p + 1 (f == pair_j[p]) over the
    pairs p in ascending order; a pair with i == j gives both."""
    per = [[] for _ in range(int(n_frames))]
    for p, (i, j) in enumerate(zip(pair_i, pair_j)):
        per[int(i)].append(2 * p)
        per[int(j)].append(2 * p + 1)
    start, entries = [0], []
    for lst in per:
        entries.extend(sorted(lst))
        start.append(len(entries))
    return start, entries


class CorrespondenceTerm:
    """The matches (f32 [M,5] = (p_x, p_y, q_x, q_y, c) on the device, a pair's matches consecutive), the frame pairs (host lists
    pair_i, pair_j, pair_first, pair_count) and the settings, for images of H x W over n_frames frames.  active (bool [F] or None =
    all): a pair is kept when at least one of its frames is active (the inactive one anchors the other).  The kept pairs keep their
    order; sums(...) returns their rows, chunked over the source frames in groups of frame_chunk z-buffers.  bind(opt, weight) attaches
    the term to a SilhouettePoseOptimizer, which then calls sums / add_grads / stats; settings() is its share of refine_poses' result."""

    def __init__(self, matches, pair_i, pair_j, pair_first, pair_count, n_frames: int, H: int, W: int, active=None,
                 delta_px=DEFAULTS["delta_px"], min_cos=DEFAULTS["min_cos"], frame_chunk: int = 16):
        fn = "CorrespondenceTerm"
        self.matches = device_tensor(fn, "matches", matches, torch.float32, lambda s: len(s) == 2 and s[1] == 5, "[M,5]")
        dev = self.device = self.matches.device
        M = self.matches.shape[0]
        self.F, self.H, self.W, self.frame_chunk = int(n_frames), int(H), int(W), int(frame_chunk)
        if self.F < 1 or self.H < 1 or self.W < 1 or self.frame_chunk < 1:
            raise ValueError(f"{fn}: n_frames, H, W and frame_chunk must be >= 1, got {n_frames}, {H}, {W}, {frame_chunk}")
        if not float(delta_px) > 0 or not 0.0 <= float(min_cos) <= 1.0:
            raise ValueError(f"{fn}: delta_px > 0 and min_cos in [0, 1], got {delta_px}, {min_cos}")
        self.delta_px, self.min_cos = float(delta_px), float(min_cos)
        lists = [[int(x) for x in lst] for lst in (pair_i, pair_j, pair_first, pair_count)]
        if len({len(lst) for lst in lists}) != 1:
            raise ValueError(f"{fn}: pair_i, pair_j, pair_first and pair_count must have one length")
        act = [True] * self.F if active is None else [bool(x) for x in torch.as_tensor(active).reshape(-1).tolist()]
        if len(act) != self.F:
            raise ValueError(f"{fn}: active must name {self.F} frames, got {len(act)}")
        kept = []
        for i, j, first, count in zip(*lists):
            # the indices are checked here, once: the kernel zeroes the row of a pair it cannot use and nothing is read back per call
            if not (0 <= i < self.F and 0 <= j < self.F):
                raise ValueError(f"{fn}: pair ({i}, {j}) names a frame outside 0..{self.F - 1}")
            if first < 0 or count < 0 or first + count > M:
                raise ValueError(f"{fn}: pair ({i}, {j}) names matches {first}..{first + count - 1} outside 0..{M - 1}")
            if act[i] or act[j]:
                kept.append((i, j, first, count))
        self.pair_i, self.pair_j = [k[0] for k in kept], [k[1] for k in kept]
        self.pair_first, self.pair_count = [k[2] for k in kept], [k[3] for k in kept]
        self.n_pairs = len(kept)
        # chunks of at most frame_chunk source frames, filled in pair order: the chunks' rows, concatenated, are the kept pairs' rows
        self.chunks = []               # (frames int64 [n_z] on the device, pairs int64 [n,5] on the device, max_count)
        slot_of, frames, table = {}, [], []
        def close():
            if table:
                self.chunks.append((torch.tensor(frames, dtype=torch.int64, device=dev), torch.tensor(table, dtype=torch.int64, device=dev),
                                    max(r[4] for r in table)))
        for i, j, first, count in kept:
            if i not in slot_of:
                if len(frames) == self.frame_chunk:
                    close()
                    slot_of, frames, table = {}, [], []
                slot_of[i] = len(frames)
                frames.append(i)
            table.append([slot_of[i], i, j, first, count])
        close()
        start, entries = frame_list(self.pair_i, self.pair_j, self.F)
        self.start = torch.tensor(start, dtype=torch.int64, device=dev)
        self.entries = torch.tensor(entries, dtype=torch.int64, device=dev)

    def sums(self, verts, faces, R, T, K, resid=None) -> torch.Tensor:
        """corr_sums of the kept pairs, float64 [n_pairs,28] in their order, at the poses R f32 [F,3,3], T f32 [F,3] of all frames."""
        width = int(_lib.lib().dh_pose_corr_width())
        if not self.chunks:
            return torch.zeros(0, width, dtype=torch.float64, device=self.device)
        out = []
        for frames, pairs, max_count in self.chunks:
            zbuf = raster_depth(verts, faces, R[frames].contiguous(), T[frames].contiguous(), K, self.H, self.W)
            out.append(corr_sums(verts, faces, R, T, K, zbuf, self.matches, pairs, max_count, self.delta_px, self.min_cos, resid=resid))
            del zbuf
        return torch.cat(out)

    def grads(self, rows, scale):
        """frame_grads of the rows of sums() with the per-pair factors `scale`."""
        return frame_grads(rows, scale, self.start, self.entries)

    def bind(self, opt, weight: float):
        """Attach the term at weight `weight` to the optimiser `opt` (the moving frames were given as `active` at construction)."""
        if (self.F, self.H, self.W) != (opt.F, opt.H, opt.W) or self.device != opt.device:
            raise ValueError(f"SilhouettePoseOptimizer: corr holds frames {(self.F, self.H, self.W)} on {self.device}, the labels are "
                             f"{(opt.F, opt.H, opt.W)} on {opt.device}")
        self.weight = float(weight)

    def add_grads(self, rows, gR, gT):
        """gR [F,3,3], gT [F,3] (float64) += weight / n_live_pairs * the frames' share of rows / max(sum c, TINY).  No host read."""
        live = (rows[:, 26] > 0).sum().clamp(min=1).to(torch.float64)
        cR, cT = self.grads(rows, (self.weight / live) / rows[:, 1].clamp(min=TINY))
        gR += cR
        gT += cT

    def stats(self, rows):
        """(L_corr, the stats' extra keys) of the rows of sums() on the CPU."""
        live = rows[:, 26] > 0
        loss = float((rows[live, 0] / rows[live, 1].clamp(min=TINY)).sum() / max(1, int(live.sum())))
        return loss, {"loss_corr": loss, "corr_matches": int(rows[:, 26].sum().round()),
                      "corr_inliers": float(rows[:, 27].sum() / rows[:, 26].sum().clamp(min=1.0))}

    def settings(self) -> dict:
        return {"pairs": self.n_pairs, "matches": int(sum(self.pair_count)), "lw_corr": self.weight, "delta_px": self.delta_px,
                "min_cos": self.min_cos}

    @torch.no_grad()
    def residuals(self, verts, faces, R, T, K):
        """Per frame i (host read; outside the iteration loop only): the median |r| in pixels of the counted matches of the kept pairs
        whose source frame it is, None where there is none."""
        resid = torch.full((self.matches.shape[0],), -1.0, dtype=torch.float32, device=self.device)
        self.sums(verts, faces, R, T, K, resid=resid)
        r = resid.cpu()
        per = [[] for _ in range(self.F)]
        for i, first, count in zip(self.pair_i, self.pair_first, self.pair_count):
            x = r[first:first + count]
            per[i].append(x[x >= 0])
        return [float(torch.cat(x).median()) if x and sum(t.numel() for t in x) > 0 else None for x in per]


def dataset_pairs(dataset, min_conf: float = DEFAULTS["min_conf"]):
    """(matches f32 [M,5] on the dataset's device, pair_i, pair_j, pair_first, pair_count) from Dataset.corr / corr_pair / corr_conf0
    (set_correspondences: sorted by (i, j)); the confidence is the matcher's (corr_conf0), and a match below min_conf gets c = 0."""
    if getattr(dataset, "corr", None) is None:
        raise ValueError("pose_corr: the dataset holds no correspondences; point data_info.correspondence_infos at a folder of "
                         "<stem_i>_<stem_j>.npz files, or run --mode match_frames (or --pose_corr match) first")
    corr, pid = dataset.corr.detach().cpu(), dataset.corr_pair.detach().cpu()
    conf = dataset.corr_conf0.detach().cpu().clone()
    conf[conf < float(min_conf)] = 0.0
    fi = torch.zeros(corr.shape[0], dtype=torch.int64)
    for f, (lo, hi) in dataset._corr_range.items():
        fi[lo:hi] = int(f)
    _, counts = torch.unique_consecutive(pid, return_counts=True)
    first = torch.cumsum(counts, 0) - counts
    pair_i, pair_j = fi[first].tolist(), corr[first, 5].long().tolist()
    matches = torch.cat([corr[:, :4], conf[:, None]], 1).to(torch.float32).contiguous().to(dataset.corr.device)
    return matches, pair_i, pair_j, first.tolist(), counts.tolist()


def make_term(dataset, active=None, delta_px=DEFAULTS["delta_px"], min_cos=DEFAULTS["min_cos"], min_conf=DEFAULTS["min_conf"],
              frame_chunk: int = 16) -> CorrespondenceTerm:
    """A CorrespondenceTerm over the correspondences the dataset holds."""
    matches, pi, pj, first, count = dataset_pairs(dataset, min_conf)
    return CorrespondenceTerm(matches, pi, pj, first, count, dataset.n_images, dataset.H, dataset.W, active=active, delta_px=delta_px,
                              min_cos=min_cos, frame_chunk=frame_chunk)
