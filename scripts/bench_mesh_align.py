"""Timing of the mesh alignment (dynhor_amd/mesh_align.py): dh_icp_correspond and dh_icp_moments (point and plane) at the refinement's
size (n_align x n_align samples, 1 and 4 hypotheses) and at the coarse level's (1024 x 4096, n_seeds hypotheses) under HIP events, and
the wall time of whole alignments of the three-box shape (marching cubes at 128 / 192, the ground truth moved by a known similarity):
local (15 degrees off, both methods) and global (130 degrees off).  One JSON line per measurement.  Kernel times proper come from a
profiler run over this script:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d <out> -o icp -- python scripts/bench_mesh_align.py

The estimate for the correspondence search is scripts/bench_mesh_eval.py's: 9 VALU operations per pair at the non-packed fp32 issue rate,
i.e. the measured pair rate of nn_sqdist_kernel (10^12 pairs in 0.154 s) gives 1.5 ms per hypothesis and iteration at 10^5 x 10^5."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIR_OPS = 9
VALU_LANE_OPS_PER_S = 256 * 128 * 2.4e9
BOXES = (((0.15, 0.0, 0.0), (0.25, 0.05, 0.05)), ((0.0, 0.09, 0.0), (0.05, 0.14, 0.05)), ((0.0, 0.0, 0.04), (0.05, 0.05, 0.09)))


def _timed(fn, reps, dev):
    import torch
    fn()                                                         # warm-up: code object load, allocator
    torch.cuda.synchronize(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize(dev)
    return ev[0].elapsed_time(ev[1]) / 1e3 / reps


def time_kernels(n, m, h, reps, dev):
    import torch
    from dynhor_amd.mesh_align import icp_correspond, icp_moments, pack_transforms, rotation_seeds
    g = torch.Generator(device=dev).manual_seed(n + h)
    src = torch.rand(n, 3, device=dev, generator=g) - 0.5
    tgt = torch.rand(m, 3, device=dev, generator=g) - 0.5
    nrm = torch.nn.functional.normalize(torch.randn(m, 3, device=dev, generator=g), dim=1).contiguous()
    xf = pack_transforms(torch.ones(h, dtype=torch.float64), rotation_seeds(h), torch.zeros(h, 3, dtype=torch.float64)).to(dev)
    s_corr = _timed(lambda: icp_correspond(src, tgt, xf), reps, dev)
    d2, idx = icp_correspond(src, tgt, xf)
    thr = torch.kthvalue(d2, max(1, int(0.9 * n)), dim=1).values
    o_s, o_t = src.mean(0), tgt.mean(0)
    s_trim = _timed(lambda: torch.kthvalue(d2, max(1, int(0.9 * n)), dim=1), reps, dev)
    s_point = _timed(lambda: icp_moments(src, tgt, None, xf, idx, d2, thr, o_s, o_t), reps, dev)
    s_plane = _timed(lambda: icp_moments(src, tgt, nrm, xf, idx, d2, thr, o_s, o_t), reps, dev)
    pairs = float(n) * m * h
    return {"bench": "icp_kernels", "n": n, "m": m, "hypotheses": h, "reps": reps, "s_correspond": s_corr, "pairs_per_s": pairs / s_corr,
            "estimate_s_correspond": pairs * PAIR_OPS / VALU_LANE_OPS_PER_S, "s_kthvalue": s_trim, "s_moments_point": s_point,
            "s_moments_plane": s_plane}


def _three_box_mesh(resolution, dev):
    import torch
    from dynhor_amd.mesh import marching_cubes
    ax = torch.linspace(-0.5, 0.5, resolution, device=dev)
    p = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)
    sdf = None
    for c, hw in BOXES:
        q = (p - torch.tensor(c, device=dev)).abs() - torch.tensor(hw, device=dev)
        d = q.clamp(min=0).norm(dim=-1) + q.max(dim=-1).values.clamp(max=0)
        sdf = d if sdf is None else torch.minimum(sdf, d)
    return marching_cubes((-sdf).view(resolution, resolution, resolution), 0.0, [-0.5] * 3, [0.5] * 3)


def time_alignment(deg, init, method, n_align, dev):
    import torch
    from dynhor_amd.mesh_align import align_meshes, rotvec_to_matrix
    from dynhor_amd.metrics import normalize_like_reference
    pv, pf = _three_box_mesh(128, dev)
    gv, gf = _three_box_mesh(192, dev)
    axis = torch.tensor([0.3, -0.5, 0.8], dtype=torch.float64)
    Rm = rotvec_to_matrix(axis / axis.norm() * math.radians(deg))
    mv = (7.3 * (gv.double().cpu() @ Rm.T) + torch.tensor([2.0, -3.0, 1.5], dtype=torch.float64)).float()
    scale = 1.0
    if init == "identity":
        mv, _, scale = normalize_like_reference(mv)
    out = None
    t = []
    for _ in range(2):                                           # first call warms the kernels up
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = align_meshes(mv, gf, pv, pf, mode="similarity", init=init, device=dev, method=method, n_align=n_align)
        torch.cuda.synchronize(dev)
        t.append(time.perf_counter() - t0)
    s, R, _, st = out
    tr = float((R * Rm.T).sum())
    err = math.degrees(math.acos(max(-1.0, min(1.0, (tr - 1.0) / 2.0))))
    return {"bench": "align_meshes", "rotation_deg": deg, "init": init, "method": method, "n_align": n_align, "s_wall_first": t[0],
            "s_wall": t[1], "rotation_error_deg": err, "total_scale_x_7.3": s * scale * 7.3, "stats": st}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_align", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip_alignments", action="store_true")
    args = ap.parse_args()
    import torch
    from dynhor_amd.mesh_align import ALIGN_DEFAULTS as D
    assert torch.cuda.is_available(), "bench_mesh_align needs a GPU"
    dev = torch.device("cuda:0")
    for n, m, h in ((args.n_align, args.n_align, 1), (args.n_align, args.n_align, 4), (args.n_align, 2 * args.n_align, 1),
                    (D["coarse_src"], D["coarse_tgt"], D["n_seeds"])):
        print(json.dumps(time_kernels(n, m, h, args.reps, dev)), flush=True)
    if not args.skip_alignments:
        for deg, init, method in ((15.0, "identity", "plane"), (15.0, "identity", "point"), (130.0, "global", "plane")):
            print(json.dumps(time_alignment(deg, init, method, args.n_align, dev)), flush=True)


if __name__ == "__main__":
    main()
