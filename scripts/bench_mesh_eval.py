"""Timing of the mesh evaluation (dynhor_amd/metrics.py): dh_nearest_sqdist at 10^4 / 10^5 / 10^6 queries x 10^6 references, and one
full Runner.evaluate_mesh at resolution 512 (geometric initialisation of a synthetic Runner against the analytic scene, 10^6 samples per
mesh).  One JSON line per measurement.  Kernel times proper come from a profiler run over this script:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d <out> -o nn -- python scripts/bench_mesh_eval.py

Measured on one MI355X: 154 ms of nn_sqdist_kernel at 10^6 x 10^6 (0.74 of the estimate's rate); evaluate_mesh at resolution 512 0.65 s
(0.84 s with the analytic ground truth's extraction).

The kernel's work estimate: 9 VALU operations per pair (3 subtractions, 1 multiply, 2 fma, compare, 2 selects) at the non-packed fp32
issue rate of 256 CUs x 128 lanes per clock x 2.4 GHz."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIR_OPS = 9
VALU_LANE_OPS_PER_S = 256 * 128 * 2.4e9


def time_nn(nq, nr, reps, dev):
    import torch
    from dynhor_amd.metrics import nearest_sqdist
    g = torch.Generator(device=dev).manual_seed(nq)
    q = torch.rand(nq, 3, device=dev, generator=g) - 0.5
    ref = torch.rand(nr, 3, device=dev, generator=g) - 0.5
    nearest_sqdist(q, ref, return_index=True)                    # warm-up: code object load, allocator
    torch.cuda.synchronize(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        nearest_sqdist(q, ref, return_index=True)
    ev[1].record()
    torch.cuda.synchronize(dev)
    s = ev[0].elapsed_time(ev[1]) / 1e3 / reps
    pairs = float(nq) * nr
    return {"bench": "nearest_sqdist", "nq": nq, "nr": nr, "reps": reps, "s_per_call": s, "pairs_per_s": pairs / s,
            "estimate_s": pairs * PAIR_OPS / VALU_LANE_OPS_PER_S}


def time_evaluate(resolution, n_samples, dev):
    import torch
    from dynhor_amd.runner import Runner
    conf = {"seq_name": "bench_mesh_eval", "exp_name": "geo_init",
            "data_info": {"synthetic": {"n_frames": 3, "H": 64, "W": 64, "seed": 5}},
            "train": {"report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0}}
    with tempfile.TemporaryDirectory() as tmp:
        r = Runner(conf=conf, device=str(dev), exp_root=tmp)
        r.validate_mesh(resolution=64, save=False)               # warm-up of the SDF kernels and marching cubes
        torch.cuda.synchronize(dev)
        t = []
        for _ in range(2):                                       # first call: with the analytic ground truth's extraction; second: cached
            t0 = time.perf_counter()
            m = r.evaluate_mesh(resolution=resolution, gt_resolution=resolution, n_samples=n_samples, save=False)
            torch.cuda.synchronize(dev)
            t.append(time.perf_counter() - t0)
    return {"bench": "evaluate_mesh", "resolution": resolution, "n_samples": n_samples, "s_wall_first": t[0],
            "s_wall_gt_cached": t[1], "metrics": m}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, nargs="*", default=[10 ** 4, 10 ** 5, 10 ** 6])
    ap.add_argument("--refs", type=int, default=10 ** 6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--n_samples", type=int, default=10 ** 6)
    ap.add_argument("--skip_evaluate", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_mesh_eval needs a GPU"
    dev = torch.device("cuda:0")
    for nq in args.queries:
        print(json.dumps(time_nn(nq, args.refs, args.reps, dev)), flush=True)
    if not args.skip_evaluate:
        print(json.dumps(time_evaluate(args.resolution, args.n_samples, dev)), flush=True)


if __name__ == "__main__":
    main()
