"""Timing of the mesh distance (dynhor_amd/mesh_sdf.py) and of the SDF warm start built on it (dynhor_amd/sdf_init.py).  One JSON line
per measurement:

  * dh_mesh_sdf_query for 65,536 random points against closed tori of 5,000 and 49,000 faces: hip events around every call, warm-up
    calls first, the median (and the fastest and slowest) of the repetitions;
  * one fit iteration at the default sizes against the 5,000-face torus, for both model families, split into sampling, mesh query,
    network forward, loss and adjoints plus network backward, Adam (events around each phase, medians), and the share of the
    iteration the colour stage takes (the renderer's per-stage timer: the colour network runs although its adjoint is zero);
  * with --full_fit FAMILY: the wall time of a whole fit at the defaults (2,000 iterations of 65,536 points).

    timeout -k 10 600 python scripts/bench_mesh_sdf.py [--full_fit neus]
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torus(n_u, n_v, R=0.32, r=0.13, device="cpu"):
    """(verts [n_u n_v, 3] float32, faces [2 n_u n_v, 3] int64): a closed torus about the z axis, faces wound counter-clockwise seen
    from outside."""
    import torch
    u = torch.arange(n_u, dtype=torch.float64) * (2 * math.pi / n_u)
    v = torch.arange(n_v, dtype=torch.float64) * (2 * math.pi / n_v)
    uu, vv = torch.meshgrid(u, v, indexing="ij")
    verts = torch.stack([(R + r * vv.cos()) * uu.cos(), (R + r * vv.cos()) * uu.sin(), r * vv.sin()], dim=-1).reshape(-1, 3)
    i, j = torch.meshgrid(torch.arange(n_u), torch.arange(n_v), indexing="ij")
    a, b = i * n_v + j, ((i + 1) % n_u) * n_v + j
    c, d = ((i + 1) % n_u) * n_v + (j + 1) % n_v, i * n_v + (j + 1) % n_v
    faces = torch.cat([torch.stack([a, b, c], -1).reshape(-1, 3), torch.stack([a, c, d], -1).reshape(-1, 3)])
    return verts.float().to(device), faces.to(device)


def _median_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t), min(t), max(t)


def time_query(n, n_u, n_v, warmup, reps, dev):
    import torch
    from dynhor_amd.mesh_sdf import MeshSDF
    verts, faces = torus(n_u, n_v, device=dev)
    m = MeshSDF(verts, faces)
    g = torch.Generator(device=dev).manual_seed(n + n_u)
    pts = (torch.rand(n, 3, device=dev, generator=g) * 2 - 1) * 0.6
    med, lo, hi = _median_ms(lambda: m.query_raw(pts), warmup, reps)
    sdf, _, wind = m.query(pts)
    return {"bench": "mesh_sdf_query", "points": n, "faces": int(faces.shape[0]), "warmup": warmup, "reps": reps, "ms_median": med,
            "ms_min": lo, "ms_max": hi, "pairs_per_s": n * float(faces.shape[0]) / (med * 1e-3),
            "inside_fraction": float((sdf < 0).float().mean()), "wind_min": float(wind.min()), "wind_max": float(wind.max())}


def _runner(family, tmp, dev):
    from dynhor_amd.runner import Runner
    conf = {"seq_name": "bench_mesh_sdf", "exp_name": family, "data_info": {"synthetic": {"n_frames": 3, "H": 64, "W": 64, "seed": 5}},
            "train": {"report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0}, "model": {"family": family}}
    return Runner(conf=conf, device=str(dev), exp_root=tmp)


def time_fit_iteration(family, warmup, reps, dev):
    import torch
    from dynhor_amd import sdf_init as S
    from dynhor_amd.mesh_sdf import MeshSDF
    c = S.SDF_INIT_DEFAULTS
    mix = {k: c[k] for k in ("share_near", "share_far", "sigma_near", "sigma_far")}
    verts, faces = torus(50, 50, device=dev)
    mesh = MeshSDF(verts, faces)
    phases = ("sample", "query", "forward", "backward", "adam")
    with tempfile.TemporaryDirectory() as tmp:
        r = _runner(family, tmp, dev)
        ren = r.renderer
        gen = torch.Generator(device=dev).manual_seed(0)
        rec = {k: [] for k in phases}
        stage = {}
        for it in range(warmup + reps):
            ren.timer.enabled = it >= warmup
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(phases) + 1)]
            ev[0].record()
            pts = S.draw_samples(verts, faces, c["points"], gen, **mix)
            ev[1].record()
            target = mesh.query(pts)[0]
            ev[2].record()
            s = S.fit_forward(ren, pts, c["ray_points"])
            ev[3].record()
            S.fit_backward(ren, s, target, c["eik_weight"])
            ev[4].record()
            ren.store.adam_step(c["lr"])
            ev[5].record()
            torch.cuda.synchronize()
            if it >= warmup:
                for k, name in enumerate(phases):
                    rec[name].append(ev[k].elapsed_time(ev[k + 1]))
        for name, (ms, _) in ren.timer.summary().items():
            stage[name] = ms
        r.close()
    med = {k: statistics.median(v) for k, v in rec.items()}
    total = sum(med.values())
    colour = sum(ms for name, ms in stage.items() if "color" in name)
    return {"bench": "sdf_init_iteration", "family": family, "points": c["points"], "faces": int(faces.shape[0]), "warmup": warmup,
            "reps": reps, "ms_median": med, "ms_total": total, "stage_ms_mean": stage, "colour_stage_ms": colour,
            "colour_stage_share": colour / total}


def time_full_fit(family, dev):
    import torch
    from dynhor_amd.sdf_init import fit_sdf_to_mesh
    verts, faces = torus(50, 50, device=dev)
    with tempfile.TemporaryDirectory() as tmp:
        r = _runner(family, tmp, dev)
        res = fit_sdf_to_mesh(r.renderer, verts, faces)
        r.close()
    return {"bench": "sdf_init_full_fit", "family": family, "iters": res["iters"], "points": res["points"], "faces": res["faces"],
            "seconds": res["seconds"], "heldout_before": res["heldout_before"], "heldout_after": res["heldout_after"],
            "loss_first": res["loss"][0], "loss_last": res["loss"][-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip_fit", action="store_true")
    ap.add_argument("--full_fit", type=str, default=None, choices=["neus", "hash"])
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_mesh_sdf needs a GPU"
    dev = torch.device("cuda:0")
    for n_u, n_v in ((50, 50), (175, 140)):
        print(json.dumps(time_query(args.points, n_u, n_v, args.warmup, args.reps, dev)), flush=True)
    if not args.skip_fit:
        for family in ("neus", "hash"):
            print(json.dumps(time_fit_iteration(family, args.warmup, args.reps, dev)), flush=True)
    if args.full_fit:
        print(json.dumps(time_full_fit(args.full_fit, dev)), flush=True)


if __name__ == "__main__":
    main()
