"""Pose refinement of the hash-grid family (DESIGN_NEXT_ROWS.md section 28): what it costs and a first look at whether it descends.

  * step time: one fused training step at --batch rays on both samplers with ray_grads off and on, alternating in one process, HIP event
    times, median of --reps; the stage times of the same steps (StageTimer) next to them -- hash_geo_backward_rays minus
    hash_geo_backward is the point adjoint's gather and its level sum, hash_geo_forward holds hash_encode7_kernel, the gather it was
    estimated against.  --lib PATH runs another build of the library (scripts/build_variant.sh), for an A/B of two forms.
  * --descent N: on the synthetic scene with every pose perturbed by --perturb_deg degrees and --perturb_t units, N iterations with
    train.refine_poses for the MLP family, hash hierarchical and hash occgrid: mean rotation / translation error before and after,
    and the rotation error of every frame relative to frame 0 (a rigid motion of the object is not observable).

One JSON line per part."""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _conf(family, sampler, batch, refine=True, **train):
    return {"seq_name": "bench_hash_pose", "exp_name": f"{family}_{sampler}",
            "train": dict({"batch_size": batch, "normal_weight": 0.05, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0,
                           "warm_up_end": 50, "end_iter": 10 ** 6, "refine_poses": refine}, **train),
            "model": {"family": family, "hash_renderer": {"sampler": sampler}}}


def step_times(args, torch):
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.runner import Runner
    ds = Dataset.from_synthetic(n_frames=8, H=256, W=256, seed=3, device="cuda:0")
    for sampler in ("hierarchical", "occgrid"):
        with tempfile.TemporaryDirectory() as tmp:
            r = Runner(conf=_conf("hash", sampler, args.batch, pose_start_iter=10 ** 9), dataset=ds, device="cuda:0", exp_root=tmp)
            r.train(args.settle)                             # the occupancy grid prunes, the surface forms
            ren = r.renderer
            rays = ds.gen_random_rays_at(0, args.batch, generator=r.ray_gen)
            near, far = ds._last_near_far
            t_rand = torch.rand(args.batch, 1, device="cuda:0", generator=r.ray_gen)
            ren._march_iter = 1

            def step(rg):
                if sampler == "occgrid":
                    ren._march_iter = 1                      # no grid update inside a timed step
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ren.train_step_core(rays, near, far, ds.R[0], 0.5, 0.1, 0.1, 0.05, t_rand=t_rand, ray_grads=rg)
                b.record()
                torch.cuda.synchronize()
                return a.elapsed_time(b)

            for _ in range(args.warmup):
                step(False); step(True)
            ms = {False: [], True: []}
            for _ in range(args.reps):
                for rg in (False, True):
                    ms[rg].append(step(rg))
            ren.timer.enabled = True
            for _ in range(args.reps):
                step(False); step(True)
            stages = {k: round(v[0], 4) for k, v in ren.timer.summary().items()}
            ren.timer.enabled = False; ren.timer.reset()
            lm = ren.last_march if sampler == "occgrid" else None
            print(json.dumps({"bench": "hash_pose_step", "sampler": sampler, "batch": args.batch, "reps": args.reps, "lib": args.lib,
                              "off_ms_median": round(statistics.median(ms[False]), 4), "off_ms": [round(x, 4) for x in ms[False]],
                              "on_ms_median": round(statistics.median(ms[True]), 4), "on_ms": [round(x, 4) for x in ms[True]],
                              "samples": lm["samples"] if lm else args.batch * (ren.n_samples + ren.n_importance),
                              "stage_ms_mean": stages}), flush=True)


def descent(args, torch):
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.runner import Runner

    def errors(ds, R_true, T_true):
        rel = ds.R @ R_true.transpose(1, 2)
        ang = torch.acos(((rel.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).clamp(-1, 1)) * 180 / math.pi
        # (a rigid motion of the object moves every pose alike and leaves the images alone: the rotation of frame i relative to frame 0
        # does not see it)
        rr = (ds.R @ ds.R[:1].transpose(1, 2)) @ (R_true @ R_true[:1].transpose(1, 2)).transpose(1, 2)
        rang = torch.acos(((rr.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).clamp(-1, 1)) * 180 / math.pi
        return ang.mean().item(), (ds.T - T_true).norm(dim=1).mean().item(), rang[1:].mean().item()

    for family, sampler in (("neus", "hierarchical"), ("hash", "hierarchical"), ("hash", "occgrid")):
        ds = Dataset.from_synthetic(n_frames=args.frames, H=128, W=128, seed=3, device="cuda:0")
        R_true, T_true = ds.R.clone(), ds.T.clone()
        g = torch.Generator(device="cpu").manual_seed(1)
        ax = torch.nn.functional.normalize(torch.randn(args.frames, 3, generator=g), dim=1) * math.radians(args.perturb_deg)
        K = torch.zeros(args.frames, 3, 3)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
        ds.R.copy_(torch.matrix_exp(K).cuda() @ R_true)
        ds.T.copy_(T_true + args.perturb_t * torch.nn.functional.normalize(torch.randn(args.frames, 3, generator=g), dim=1).cuda())
        before = errors(ds, R_true, T_true)
        with tempfile.TemporaryDirectory() as tmp:
            r = Runner(conf=_conf(family, sampler, 512, pose_lr=args.pose_lr, pose_start_iter=args.pose_start, learning_rate=5e-3 if family == "hash" else 5e-4),
                       dataset=ds, device="cuda:0", exp_root=tmp)
            r.train(args.descent)
        after = errors(ds, R_true, T_true)
        print(json.dumps({"bench": "hash_pose_descent", "family": family, "sampler": sampler, "frames": args.frames, "iterations": args.descent,
                          "batch": 512, "pose_lr": args.pose_lr, "pose_start_iter": args.pose_start, "perturb_deg": args.perturb_deg,
                          "perturb_t": args.perturb_t, "rot_err_deg_before": round(before[0], 4), "rot_err_deg_after": round(after[0], 4),
                          "trans_err_before": round(before[1], 5), "trans_err_after": round(after[1], 5),
                          "rot_err_rel_frame0_deg_before": round(before[2], 4), "rot_err_rel_frame0_deg_after": round(after[2], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=int, default=64, help="training iterations before the timed steps")
    ap.add_argument("--lib", default=None, help="another build of the library, relative to the repository root")
    ap.add_argument("--descent", type=int, default=0, help="iterations of the descent check (0: skip)")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--perturb_deg", type=float, default=3.0)
    ap.add_argument("--perturb_t", type=float, default=0.02)
    ap.add_argument("--pose_lr", type=float, default=1e-3)
    ap.add_argument("--pose_start", type=int, default=100)
    ap.add_argument("--no_step", action="store_true")
    args = ap.parse_args()
    import torch
    from dynhor_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.join(ROOT, args.lib)
    assert torch.cuda.is_available(), "bench_hash_pose needs a GPU"
    if not args.no_step:
        step_times(args, torch)
    if args.descent > 0:
        descent(args, torch)


if __name__ == "__main__":
    main()
