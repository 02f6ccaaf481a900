"""Timing and quality of the mesh simplification (dynhor_amd/mesh_simplify.py) on the analytic scene's mesh.  One JSON line per
measurement:

  * stages: cell keys (box reduction, dh_simplify_cells), the record sort (gather + stable sort + runs), dh_simplify_quadrics, the
    face stage (rank lookup, dh_simplify_faces) and the de-duplication (sort, compaction, edge counts), each timed on the stream with
    events, and the wall time of a whole simplify_mesh, for --pairs RESOLUTION:CELLS (default 512:128 1024:256);
  * --quality: Chamfer / F-score / normal consistency (metrics.mesh_metrics) against the surface extracted at --gt_resolution of
    the mesh extracted at --fine, of that mesh simplified to each of --cells, and of the meshes extracted directly at those resolutions,
    for the synthetic scene and for the three-box fixture of the tests;
  * --pose: the wall time of one refine_poses of 16 frames of 256 x 256 against extract@--fine + faces:12000 and against extract@128.

Kernel times proper come from a profiler run:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d <out> -o msimp -- python scripts/bench_mesh_simplify.py
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def sdf_mesh(sdf, N, dev, bound=0.55):
    """The zero level set of `sdf` over [-bound, bound]^3 at N grid points per axis (block-sparse extraction at lipschitz 1)."""
    from dynhor_amd.mesh_extract import sparse_marching_cubes
    v, f = sparse_marching_cubes(lambda p: -sdf(p), int(N), [-bound] * 3, [bound] * 3, lipschitz=1.0, device=dev)[:2]
    return v.contiguous(), f.contiguous()


def stage_times(v, f, cells, reps, dev):
    """Seconds per call of every stage of one simplification, as mesh_simplify._simplify_cells issues them."""
    import torch
    from bench_mesh_clean import _timed
    from dynhor_amd import _lib, mesh_simplify as M
    L = _lib.lib()
    nv, nf = v.shape[0], f.shape[0]
    out = {}
    out["cells_s"] = _timed(lambda: M._cell_keys("bench", v, cells), reps, dev)
    keys, g = M._cell_keys("bench", v, cells)

    def records():
        rkey, order = torch.sort(keys[f.reshape(-1)], stable=True)
        run_key, run_len = torch.unique_consecutive(rkey, return_counts=True)
        run_start = torch.zeros(run_key.shape[0] + 1, dtype=torch.int64, device=dev)
        torch.cumsum(run_len, 0, out=run_start[1:])
        return order, run_key, run_len, run_start

    out["record_sort_s"] = _timed(records, reps, dev)
    order, run_key, run_len, run_start = records()
    n_runs = int(run_key.shape[0])
    rep = torch.empty(n_runs, 3, device=dev)
    clamped = torch.empty(n_runs, dtype=torch.int32, device=dev)
    out["quadrics_s"] = _timed(lambda: _lib.check(L.dh_simplify_quadrics(
        _lib.ptr(v), nv, _lib.ptr(f), nf, _lib.ptr(order), _lib.ptr(run_start), _lib.ptr(run_key), n_runs, g.lo, g.h, g.dims, 1e-3, 1,
        _lib.ptr(rep), _lib.ptr(clamped), None, _lib.stream())), reps, dev)
    tri = torch.empty(nf, 3, dtype=torch.int64, device=dev)
    keep = torch.empty(nf, dtype=torch.uint8, device=dev)
    key = torch.empty(nf, dtype=torch.int64, device=dev)

    def faces():
        vrank = torch.searchsorted(run_key, keys).to(torch.int32)
        _lib.check(L.dh_simplify_faces(_lib.ptr(f), nf, _lib.ptr(vrank), nv, n_runs, _lib.ptr(tri), _lib.ptr(keep), _lib.ptr(key),
                                       _lib.stream()))

    out["faces_s"] = _timed(faces, reps, dev)

    def dedupe():
        idx = torch.nonzero(keep).reshape(-1)
        k, perm = torch.sort(key[idx] * n_runs + tri[idx, 2], stable=True)
        first = torch.ones_like(k, dtype=torch.bool)
        first[1:] = k[1:] != k[:-1]
        t = tri[torch.sort(idx[perm[first]])[0]]
        used = torch.zeros(n_runs, dtype=torch.bool, device=dev)
        used[t.reshape(-1)] = True
        return M.edge_counts((torch.cumsum(used, 0) - 1)[t])

    if n_runs < (1 << 21):
        out["dedupe_s"] = _timed(dedupe, reps, dev)
    out.update(records=3 * nf, runs=n_runs, longest_run=int(run_len.max()), record_bytes=3 * nf * (8 + 3 * 8 + 9 * 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=str, nargs="*", default=["512:128", "1024:256"], help="RESOLUTION:CELLS to time")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--fine", type=int, default=512)
    ap.add_argument("--cells", type=int, nargs="*", default=[128, 64])
    ap.add_argument("--gt_resolution", type=int, default=1024)
    ap.add_argument("--n_samples", type=int, default=1_000_000)
    ap.add_argument("--pose", action="store_true")
    args = ap.parse_args()
    import torch
    from dynhor_amd.mesh_simplify import simplify_mesh
    from dynhor_amd.scene import scene_sdf
    assert torch.cuda.is_available(), "bench_mesh_simplify needs a GPU"
    dev = torch.device("cuda:0")

    for pair in args.pairs:
        N, cells = (int(x) for x in pair.split(":"))
        v, f = sdf_mesh(scene_sdf, N, dev)
        st = stage_times(v, f, cells, args.reps, dev)
        simplify_mesh(v, f, cells=cells)
        torch.cuda.synchronize(dev)
        wall = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sv, sf, stats = simplify_mesh(v, f, cells=cells)
            torch.cuda.synchronize(dev)
            wall.append(time.perf_counter() - t0)
        print(json.dumps({"bench": "mesh_simplify", "mesh": f"scene@{N}", "cells": cells, "verts": v.shape[0], "faces": f.shape[0],
                          **st, "simplify_mesh_wall_s": sorted(wall)[len(wall) // 2], "stats": stats}), flush=True)
        del v, f, sv, sf
        torch.cuda.empty_cache()

    if args.quality:
        from dynhor_amd.metrics import mesh_metrics
        from tests.mesh_align_util import three_box_sdf
        keys = ("chamfer_l1", "chamfer_l2", "fscore@0.005", "precision@0.005", "recall@0.005", "normal_consistency", "n_pred_faces")
        for name, sdf in (("scene", scene_sdf), ("three_box", three_box_sdf)):
            gt_v, gt_f = sdf_mesh(sdf, args.gt_resolution, dev)
            fv, ff = sdf_mesh(sdf, args.fine, dev)
            variants = [(f"extract@{args.fine}", fv, ff, None)]
            for c in args.cells:
                sv, sf, st = simplify_mesh(fv, ff, cells=c)
                variants.append((f"extract@{args.fine} -> cells:{c}", sv, sf, st))
                variants.append((f"extract@{c}", *sdf_mesh(sdf, c, dev), None))
            for label, pv, pf, st in variants:
                res = mesh_metrics(pv, pf, gt_v, gt_f, n_samples=args.n_samples, taus=(0.005, 0.01, 0.02), seed=0, device=dev)
                row = {"bench": "mesh_simplify_quality", "shape": name, "gt": f"extract@{args.gt_resolution}", "variant": label,
                       **{k: res[k] for k in keys if k in res}}
                if st is not None:
                    row.update({k: st[k] for k in ("cell_size", "n_verts_out", "n_clamped", "n_boundary_edges", "n_nonmanifold_edges")})
                print(json.dumps(row), flush=True)
            del gt_v, gt_f, fv, ff, variants
            torch.cuda.empty_cache()

    if args.pose:
        from dynhor_amd.dataset import Dataset
        from dynhor_amd.pose_sil import refine_poses
        meshes = {"extract@128": sdf_mesh(scene_sdf, 128, dev)}
        fv, ff = sdf_mesh(scene_sdf, args.fine, dev)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        sv, sf, st = simplify_mesh(fv, ff, target_faces=12000)
        torch.cuda.synchronize(dev)
        t_simplify = time.perf_counter() - t0
        meshes[f"extract@{args.fine} -> faces:12000"] = (sv, sf)
        for rep in range(2):                                                  # the first round warms both up
            for label, (mv, mf) in meshes.items():
                ds = Dataset.from_synthetic(n_frames=16, H=256, W=256, seed=4321, device=dev)
                for fr in range(0, 16, 8):
                    ds.T[fr, 0] += 0.05
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                res = refine_poses(mv.contiguous(), mf.contiguous(), ds)
                torch.cuda.synchronize(dev)
                if rep:
                    print(json.dumps({"bench": "mesh_simplify_pose", "mesh": label, "faces": mf.shape[0], "frames": 16, "H": 256, "W": 256,
                                      "refine_poses_s": time.perf_counter() - t0, "simplify_s": t_simplify if "faces:" in label else None,
                                      "cells": st["cells"] if "faces:" in label else None, "iou_mean_before": res["iou_mean_before"],
                                      "iou_mean_after": res["iou_mean_after"], "iou_min_after": res["iou_min_after"]}), flush=True)


if __name__ == "__main__":
    main()
