"""Mesh extraction, dense against block-sparse (dynhor_amd/mesh_extract.py), on the SDF network of a synthetic Runner trained as
scripts/bench_inference.py trains it (20 iterations, --family neus | hash) and on the analytic scene (lipschitz 1).  Dense and sparse
run alternately in one process, --reps times after a warm-up, each call between device synchronises; sparse alone at --sparse_only,
dense once at --dense_once when memory allows.  One JSON line per measurement (times in seconds).  Kernel times come from a profiler
run of one path alone (--only), so that the SDF kernel's statistics are that path's:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \\
        python scripts/bench_mesh_extract.py --fields network --only sparse --resolutions 512

--lipschitz_record prints instead the L_min values behind mesh_extract.DEFAULT_LIPSCHITZ: configs/synthetic.yaml, both families, at
initialisation and after --iters iterations, resolution 512."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENE_BOX = ([-0.55] * 3, [0.55] * 3)
QUIET = {"batch_size": 2048, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0}


def _timed(fn, N, dev):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn(N)
    torch.cuda.synchronize(dev)
    return round(time.perf_counter() - t0, 6), out


def _line(**kw):
    print(json.dumps(kw, separators=(",", ":")), flush=True)


def fields(runner, dev, block):
    """name -> (dense(N) -> (verts, faces), sparse(N) -> (verts, faces, stats), lipschitz)."""
    from dynhor_amd.mesh_extract import DEFAULT_LIPSCHITZ, sparse_marching_cubes
    from dynhor_amd.scene import scene_sdf
    rd = runner.renderer
    box = runner.dataset.object_bbox_min, runner.dataset.object_bbox_max
    scene = lambda p: -scene_sdf(p)

    def net_sparse(N):
        return (*rd.extract_geometry(*box, N, mode="sparse", block=block), rd.last_extract_stats)

    def scene_dense(N):
        runner.__dict__.pop("_gt_meshes", None)                               # (its cache)
        return runner._scene_gt_mesh(N)

    return {"network": (lambda N: rd.extract_geometry(*box, N), net_sparse, DEFAULT_LIPSCHITZ),
            "scene": (scene_dense, lambda N: sparse_marching_cubes(scene, N, *SCENE_BOX, lipschitz=1.0, block=block, device=dev), 1.0)}


def bench(args, dev):
    import torch
    from dynhor_amd.runner import Runner
    conf = {"seq_name": "mx", "exp_name": args.family, "data_info": {"synthetic": {"n_frames": 4, "H": 512, "W": 512, "seed": 1}},
            "train": QUIET, "model": {"family": args.family}}
    with tempfile.TemporaryDirectory() as tmp:
        r = Runner(conf=conf, device="cuda:0", exp_root=tmp)
        for _ in range(20):
            r.train_iteration()
        for name, (dense, sparse, lip) in fields(r, dev, args.block).items():
            if name not in args.fields:
                continue
            base = {"bench": "mesh_extract", "field": name, "family": args.family if name == "network" else None, "lipschitz": lip}
            count = lambda st: dict({k: st[k] for k in ("dense_samples", "blocks", "active_blocks", "verts", "faces")}, sparse_samples=st["samples"])
            for N in args.resolutions:
                if args.only:
                    fn = dense if args.only == "dense" else sparse
                    fn(N)
                    _line(**base, resolution=N, only=args.only, s=[_timed(fn, N, dev)[0] for _ in range(args.reps)])
                    continue
                dense(N); sparse(N)                                           # warm-up: code objects, allocator
                td, ts = [], []
                for _ in range(args.reps):
                    t, dm = _timed(dense, N, dev); td.append(t)
                    t, (sv, sf, st) = _timed(sparse, N, dev); ts.append(t)
                _line(**base, resolution=N, dense_s=td, sparse_s=ts, sparse_over_dense=round(sorted(ts)[len(ts) // 2] / sorted(td)[len(td) // 2], 4),
                      **count(st), same_vertices=bool(torch.equal(sv, dm[0])) and sf.shape == dm[1].shape)
                del dm, sv, sf
            for N in () if args.only else args.sparse_only:
                sparse(N)
                runs = [_timed(sparse, N, dev) for _ in range(args.reps)]
                _line(**base, resolution=N, sparse_s=[t for t, _ in runs], **count(runs[-1][1][2]))
                del runs
            N = 0 if args.only else args.dense_once
            if N and torch.cuda.mem_get_info(dev)[0] > 48 * N ** 3:             # the dense path's int64 case tensor and shifted views
                t, dm = _timed(dense, N, dev)
                _line(**base, resolution=N, dense_once_s=t, verts=dm[0].shape[0], faces=dm[1].shape[0],
                      peak_GiB=round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2))
                del dm
        r.close()


def lipschitz_record(args, dev):
    import torch
    import yaml
    from dynhor_amd.mesh_extract import block_grid, grid_axes, min_safe_lipschitz
    from dynhor_amd.runner import Runner
    N, B = 512, args.block
    with tempfile.TemporaryDirectory() as tmp:
        for family in ("neus", "hash"):
            conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "synthetic.yaml")))
            conf.setdefault("model", {})["family"] = family
            conf["train"].update(report_freq=10 ** 9, save_freq=10 ** 9, val_freq=0)
            r = Runner(conf=conf, device="cuda:0", exp_root=tmp)
            axes = grid_axes(N, r.dataset.object_bbox_min, r.dataset.object_bbox_max, dev)
            _, c, rad = block_grid(axes, B)
            for what in ("initialisation", f"{args.iters} iterations"):
                if what != "initialisation":
                    r.train(args.iters)
                u = torch.empty(N, N, N, device=dev)
                for xi in range(0, N, 64):
                    g = torch.stack(torch.meshgrid(axes[0][xi:xi + 64], axes[1], axes[2], indexing="ij"), dim=-1)
                    u[xi:xi + 64] = -r.renderer.sdf(g.reshape(-1, 3).contiguous()).reshape(g.shape[:3])
                _line(bench="mesh_extract_l_min", family=family, checkpoint=what, iter=r.iter_step, resolution=N,
                      l_min=round(min_safe_lipschitz(u, -r.renderer.sdf(c).reshape(-1), rad, 0.0, B), 6))
            r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", default="neus", choices=["neus", "hash"])
    ap.add_argument("--resolutions", type=int, nargs="*", default=[256, 512], help="dense and sparse, alternately")
    ap.add_argument("--sparse_only", type=int, nargs="*", default=[1024, 2048])
    ap.add_argument("--dense_once", type=int, default=1024, help="one dense run at this resolution when memory allows (0: none)")
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fields", nargs="*", default=["network", "scene"], choices=["network", "scene"])
    ap.add_argument("--only", default=None, choices=["dense", "sparse"], help="time this path alone at --resolutions (profiler runs)")
    ap.add_argument("--lipschitz_record", action="store_true")
    ap.add_argument("--iters", type=int, default=2000)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_mesh_extract needs a GPU"
    (lipschitz_record if args.lipschitz_record else bench)(args, torch.device("cuda:0"))


if __name__ == "__main__":
    main()
