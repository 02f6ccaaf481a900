"""Record tests/golden/pose_refine.json: what pose_sil.refine_poses returns, bit for bit, on four small scenes -- the silhouette alone
(A), with the photometric term (B), with the correspondence term and a fixed frame (C), and with both terms on a subset of the frames
(D).  tests/test_gpu_pose_terms.py replays the file.

    python tests/golden/make_golden_pose_refine.py [--out path]

It needs an MI355X and calls only entry points that outlive a reorganisation of the pose terms: refine_poses, PhotometricTerm,
surface_points, CorrespondenceTerm and mesh_color.usable_map, on scenes the tests' helpers build on the CPU.  Run it at the commit
BEFORE a change that must not move a bit, twice, and keep the file only when both runs wrote the same bytes; a difference in the test is
a finding to explain, never a reason to run this again.

Every case runs 6 iterations and reports each one.  Recorded per case: R and T as int32 bit patterns, the whole curve, iou_before /
iou_after, settings and, where the run has them, photo_pairs, corr_resid_before / corr_resid_after and corr_worst.  json keeps a Python
float exactly, so the replay compares without a tolerance."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

ITERS = 6
KEYS = ("curve", "iou_before", "iou_after", "settings", "photo_pairs", "corr_resid_before", "corr_resid_after", "corr_worst")


def _f32(t, dev):
    return t.to(dev, torch.float32).contiguous()


def _dataset(sc, n, dev, rgb=None):
    rgb = torch.zeros(n, sc["H"], sc["W"], 3, dtype=torch.uint8, device=dev) if rgb is None else rgb
    return SimpleNamespace(label=sc["label"].to(dev), rgb=rgb, R=_f32(sc["R0"], dev), T=_f32(sc["T0"], dev), K=_f32(sc["K"], dev),
                           H=sc["H"], W=sc["W"], n_images=n, stems=None)


def _photo_term(verts, faces, ds, n, dev):
    from dynhor_amd.mesh_color import usable_map
    from dynhor_amd.pose_photo import PhotometricTerm, surface_points
    from tests import mesh_texture_util as TU
    g = torch.Generator().manual_seed(1)
    pts, nrm, col = surface_points(verts, faces, 1000, 3, vertex_colors=torch.rand(verts.shape[0], 3, generator=g).to(dev))
    ds.rgb = TU.smooth_noisy_frames(n, ds.H, ds.W, seed=8, device=dev)
    return PhotometricTerm(pts, nrm, col, ds.rgb, usable_map(ds.label, 1), levels=(1.0, 0.0))


def _corr_term(sc, dev):
    from dynhor_amd.pose_corr import CorrespondenceTerm
    return lambda active: CorrespondenceTerm(sc["matches"].to(dev), sc["pair_i"], sc["pair_j"], sc["pair_first"], sc["pair_count"], 5,
                                             sc["H"], sc["W"], active=active, frame_chunk=2)


def _record(res):
    out = {"R": res["R"].cpu().contiguous().view(torch.int32).tolist(), "T": res["T"].cpu().contiguous().view(torch.int32).tolist()}
    out.update({k: res[k] for k in KEYS if k in res})
    return json.loads(json.dumps(out))


def run_cases(device="cuda:0"):
    """{case: the recorded part of refine_poses' result} of the four cases."""
    from dynhor_amd.pose_sil import refine_poses
    from tests import mesh_texture_util as TU
    from tests import pose_corr_util as CU
    from tests import pose_sil_util as SU
    dev = torch.device(device)
    out = {}
    sc = SU.small_scene()                                              # 4 frames of 96 x 96; chunks of 3 + 1
    verts, faces = _f32(sc["verts"], dev), sc["faces"].to(dev)
    ds = _dataset(sc, 4, dev)
    out["A_silhouette"] = _record(refine_poses(verts, faces, ds, iters=ITERS, report_freq=1, frame_chunk=3, lw_smooth=0.1))
    ds = _dataset(sc, 4, dev)
    term = _photo_term(verts, faces, ds, 4, dev)                       # the blur level changes at iteration 3
    out["B_photo"] = _record(refine_poses(verts, faces, ds, iters=ITERS, report_freq=1, frame_chunk=3, lw_smooth=0.1, photo=term))
    sc = CU.corr_scene(10.0, n_per_pair=300)                           # 5 frames of 96 x 128, frame 0 at the truth
    verts, faces = TU.sphere_mesh((0.0, 0.0, 0.0), TU.SPHERE_R, N=12)
    verts, faces = _f32(verts, dev), faces.to(dev)
    ds = _dataset(sc, 5, dev)
    out["C_corr_fixed_frame"] = _record(refine_poses(verts, faces, ds, iters=ITERS, report_freq=1, frame_chunk=3, lw_smooth=0.1,
                                                     frames=[1, 2, 3, 4], corr=_corr_term(sc, dev)))
    ds = _dataset(sc, 5, dev)
    term = _photo_term(verts, faces, ds, 5, dev)
    out["D_all_terms_subset"] = _record(refine_poses(verts, faces, ds, iters=ITERS, report_freq=1, frame_chunk=3, lw_smooth=0.1,
                                                     frames=[1, 3], photo=term, corr=_corr_term(sc, dev)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "pose_refine.json"))
    args = ap.parse_args()
    out = run_cases()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases -> {args.out}: " + ", ".join(f"{k} ({len(v['curve'])} curve entries, keys {sorted(v)})" for k, v in out.items()))


if __name__ == "__main__":
    main()
