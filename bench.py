"""bench.py -- training rays/s of the NeuS reconstruction hot path on N MI355X (contract in the task brief).

One "step" = one full training iteration on 2048 rays x (64 coarse + 64 importance) samples of a synthetic 512x512
sequence (BASELINE.json configs[1]): HIP ray gather -> hierarchical up-sampling -> SDF/colour MLPs
-> volume rendering -> losses -> backward -> (N>1: RCCL all-reduce of the flat gradient) -> fused Adam.  Frames shard
data-parallel over ranks (weak scaling: 2048 rays per rank).  Prints ONE JSON line on rank 0.

    python bench.py                          # cfg2, N = 1: the headline line only (set-up, warm-up, the K timed steps)
    python bench.py --full                   # the same, plus `kernels`, `roofline`, `cpu_baseline`, `parity_check`, "secondary" (cfg4,
                                             # cfg4 + marcher, cfg5's loss stack: 20 steps each) and "psnr_at_2k" (the committed record)
    python bench.py --family hash            # BASELINE.json configs[3]: hash-grid encoding + shallow MLPs, same batch
    python bench.py --arithmetic fp32_mfma   # every GEMM on native fp32 MFMA (the independent, exact-fp32 arithmetic)
    python bench.py --full --psnr            # "psnr_at_2k" measured now: HIP vs oracle at equal iterations (minutes per seed)
    python bench.py --dump-outputs DIR       # also write what the last timed step computed as DIR/<name>.npy

Timing protocol: W untimed warm-up steps, then EXACTLY K steps between barrier + synchronize on both sides with NO per-stage
timers (the headline `value`).  With --full, a separate short loop (--kernel-steps, default 20) with the per-stage HIP-event timers
on then fills `kernels` and `roofline`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

# algorithmic MACs per sample point of each MLP stage (DESIGN.md "Algorithmic work")
MACS = {
    "sdf_forward": 524544, "sdf_gradient": 459008, "color_forward": 271360, "color_backward": 271360,
    "sdf_tangent": 458752, "sdf_backward": 514560, "weight_grads_gemm": 1254656,
    "sdf_nograd_coarse": 459008, "sdf_nograd_fine": 459008,
}
# algorithmic HBM bytes per launch of each MLP stage = the saved tiles ("native" [64 x 256] fp32 tiles) it must
# read or write ONCE, as (main tiles, aux [64 x 64] tiles) per 64 sample points: forward writes act[8] + feat and the embedding;
# the reverse chain reads act[8], writes a[8]; ...; the weight-gradient GEMMs read 40 distinct main + 3 aux tiles (dw.hip job table)
STAGE_TILES = {"sdf_forward": (9, 1), "sdf_gradient": (16, 0), "color_forward": (5, 1), "color_backward": (9, 0),
               "sdf_tangent": (31, 1), "sdf_backward": (25, 0), "weight_grads_gemm": (40, 3)}
FP32_MFMA_PEAK_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md, Chip-level parameters
BF16_MFMA_PEAK_TFLOPS = 2500.0     # same table: bf16 dense
HBM_PEAK_GBPS = 8000.0             # same table: HBM3E spec
HBM_ACHIEVABLE_GBPS = 6290.0       # same guide: measured float4 copy
FLOAT_ATOMIC_PEAK_GBPS = 1300.0    # same guide, "Global float atomics": chip-wide rate of added bytes
FLOP_PER_RAY_TRAIN = 1081270272


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(rays, R, n_samples, n_importance, normal_weight, family="neus", like_runner=None):
    """The oracle (PyTorch restatement, oracle/ -- the CHECKER, timed here as the reported CPU baseline only) on the host
    cores: one warm-up + two timed full training iterations on rays of the synthetic sequence the GPU path trains on.
    The thread count is chosen by calibration (the GPU boxes advertise far more logical CPUs than an eager-PyTorch run of this
    size can use: 256 threads ran >100x slower than 8): every candidate on 128 rays, then the two fastest again on 512 rays
    (GEMMs 4x larger scale further with threads), the faster of those runs the timed iterations."""
    from oracle import neus_oracle as O
    try:
        ncpu = len(os.sched_getaffinity(0))
    except AttributeError:
        ncpu = os.cpu_count() or 1
    rays, R = rays.detach().cpu(), R.detach().cpu()
    g = torch.Generator().manual_seed(0)
    t_rand = torch.rand(rays.shape[0], 1, generator=g)

    def build():
        if family == "hash":
            from oracle import hashgrid_oracle as HO
            sdf, col = HO.build_models(seed=1234, device="cpu")
            var = O.SingleVarianceNetwork(0.3)
            lr = 5e-3
        else:
            sdf, col, var = O.build_models(seed=1234, device="cpu")
            lr = 5e-4
        r = O.NeuSRenderer(None, sdf, var, col, n_samples, n_importance, 0, 4, 1.0)
        opt = torch.optim.Adam(list(sdf.parameters()) + list(var.parameters()) + list(col.parameters()), lr=lr)
        return r, opt

    def time_once(nt, n):
        torch.set_num_threads(nt)
        r, opt = build()
        O.train_step(r, opt, rays[:max(n // 2, 16)], 0.5, 0.1, 0.1, normal_weight, R=R, t_rand=t_rand[:max(n // 2, 16)])
        t0 = time.perf_counter()
        O.train_step(r, opt, rays[:n], 0.5, 0.1, 0.1, normal_weight, R=R, t_rand=t_rand[:n])
        return time.perf_counter() - t0

    if family == "hash":
        # an iteration of this oracle carries ~6 s of fixed cost on 8 cores (dense 12 M-parameter table gradient + Adam), so a
        # thread sweep would take minutes: the count the NeuS sweep settles on on these hosts (16) is used as is
        calib, calib2, best = {}, {}, min(16, ncpu)
    else:
        n_small = min(128, rays.shape[0])
        calib = {nt: time_once(nt, n_small) for nt in sorted({t for t in (4, 8, 16, 32, 64) if t <= ncpu} or {1})}
        finalists = sorted(calib, key=calib.get)[:2]
        n_mid = min(512, rays.shape[0])
        calib2 = {nt: time_once(nt, n_mid) for nt in finalists} if n_mid > n_small else {}
        best = min(calib2, key=calib2.get) if calib2 else finalists[0]
    torch.set_num_threads(best)
    r, opt = build()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        O.train_step(r, opt, rays, 0.5, 0.1, 0.1, normal_weight, R=R, t_rand=t_rand)
        times.append(time.perf_counter() - t0)
    dt = sum(times[1:]) / 2
    n = rays.shape[0]
    return {"value": n / dt, "unit": "rays/s", "cores": torch.get_num_threads(), "kind": "port",
            "host": {"os_cpu_count": os.cpu_count(), "affinity": ncpu, "model": _cpu_model(),
                     "thread_calibration_s_per_128_rays": {str(k): round(v, 3) for k, v in calib.items()},
                     "thread_calibration_s_per_512_rays_two_fastest": {str(k): round(v, 3) for k, v in calib2.items()}},
            "sample": f"{n} rays x {n_samples}+{n_importance} samples of one synthetic frame"
                      + (" (the GPU path's own batch)" if n == 2048 else f" (1/{2048 // n} of the GPU path's batch)" if n < 2048 else "")
                      + f", full training iteration of the {'hash-grid' if family == 'hash' else 'NeuS'} oracle (render, losses, "
                      f"backward, Adam), 1 warm-up + 2 timed, fp32, {dt:.2f} s/iter"}


def _delta_stats(w):
    ps = w.get("per_seed") or []
    return {"mean": round(w["mean_db"], 4), "se": round(w["se_db"], 4), "seeds": w["n"],
            "median": round(w["median_db"], 4) if "median_db" in w else None,
            "worst_seed": round(min(ps), 4) if ps else None, "best_seed": round(max(ps), 4) if ps else None}


def committed_psnr_record():
    """`psnr_at_2k` of the default line: the pooled paired-seed record committed under profiles/ (measuring it costs ~4 GPU-minutes
    per seed: `--psnr` does that instead).  The newest round's file wins.  Both statistics of the record are carried: the WINDOW of
    checkpoints at 1800..2000 iterations (`delta` / `se`: the protocol's headline) and the FINAL checkpoint at exactly 2000."""
    import glob
    for pat in ("psnr_parity_r06_neus_hip_vs_oracle_f16_pooled.json", "psnr_parity_r05_neus_hip_vs_oracle_f16_pooled.json",
                "psnr_parity_r04_neus_hip_vs_oracle_f16_pooled.json",
                "psnr_parity_r03_neus_hip_vs_oracle_59seeds.json"):
        for path in sorted(glob.glob(os.path.join(ROOT, "profiles", pat))):
            d = json.load(open(path))
            w = d.get("window_delta") or d.get("all_seeds") or d.get("all_59_seeds")
            out = {"measured_in_this_run": False,
                   "label": "COMMITTED record quoted from profiles/ (not measured by this run; --psnr measures fresh pairs; this run's own "
                            "parity measurement is `parity_check`)",
                   "source": "profiles/" + os.path.basename(path), "delta": round(w["mean_db"], 4), "se": round(w["se_db"], 4),
                   "seeds": w["n"], "median": round(w.get("median_db", float("nan")), 4) if "median_db" in w else None,
                   "window": _delta_stats(w),
                   "final_checkpoint": _delta_stats(d["final_delta"]) if "final_delta" in d else None,
                   "what": d.get("what", "HIP minus oracle, paired seeds, PSNR over all 64 frames in a window of checkpoints at 1800..2000 "
                                         "iterations (scripts/psnr_parity.py)"),
                   "arithmetic": d.get("arithmetic", "split_bf16 (rounds 2-3)")}
            nf = sorted(glob.glob(os.path.join(ROOT, "profiles", "psnr_r05_hip_noise_floor_*.json")))
            if nf:
                n = json.load(open(nf[-1]))
                out["hip_noise_floor"] = {"source": "profiles/" + os.path.basename(nf[-1]),
                                          "window": _delta_stats(n["window_delta"]), "final_checkpoint": _delta_stats(n["final_delta"]),
                                          "what": n.get("what")}
            return out
    return None


def parity_check_in_this_run(runner, device, iters=50):
    """`parity_check` of the default line (VERDICT r5 next #5a): ONE lock-step segment HIP path vs the GPU-eager oracle, MEASURED IN THIS
    RUN, after the timed region (never inside it).  The oracle (the checker, never the thing measured) copies the bench runner's current
    weights, the HIP arm takes the oracle's (fresh) Adam state, and both train `iters` iterations on the same rays, the same
    perturbations and the same learning rates.  first_step_loss_diff is pure kernel error (same weights, same rays); a biased kernel
    would show as a one-sided signed_segment_mean; param_rel_divergence_at_end is the chaotic drift of `iters` steps."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import psnr_parity as PP
    from dynhor_amd import schedules
    PP.LOG = sys.stderr
    t0 = time.perf_counter()
    ds = runner.dataset
    B = PP.OracleArm("neus", runner, 5e-4, device)
    runner.store.load_optimizer_state_dict(B.opt.state_dict())
    runner.store.bump()
    A = PP.HipArm(runner)
    gen = torch.Generator(device=device); gen.manual_seed(20261004)
    fp = schedules.FramePermutation(ds.n_images, 97)
    it0 = int(runner.iter_step)
    dl, la0, lb0 = [], None, None
    n = runner.batch_size
    for i in range(iters):
        it = it0 + i
        frame = fp.frame(i)
        car = schedules.cos_anneal_ratio(it, PP.ANNEAL_END)
        lr = 5e-4 * schedules.lr_factor(it, PP.WARM_UP, PP.END_ITER, PP.LR_ALPHA)
        px = torch.randint(0, ds.W, [n], device=device, generator=gen)
        py = torch.randint(0, ds.H, [n], device=device, generator=gen)
        tr = torch.rand([n, 1], device=device, generator=gen)
        rays = ds.gen_rays_at_pixels(frame, px, py)
        near, far = ds._last_near_far
        la, _ = A.step(rays, near, far, ds.R[frame], car, lr, tr)
        lb, _ = B.step(rays, near, far, ds.R[frame], car, lr, tr)
        dl.append(float(la) - float(lb))
        if i == 0:
            la0, lb0 = float(la), float(lb)
    fa, fb = A.flat(), B.flat()
    d = torch.tensor(dl, dtype=torch.float64)
    return {"measured_in_this_run": True, "what": f"lock-step, {iters} training iterations from this run's weights (iteration {it0}): "
            "HIP path vs the GPU-eager PyTorch oracle on the same rays; loss differences HIP - oracle",
            "iters": iters, "rays_per_iter": n, "loss_hip_first_step": round(la0, 7), "loss_oracle_first_step": round(lb0, 7),
            "first_step_loss_diff": float(d[0]), "signed_segment_mean": float(d.mean()),
            "signed_segment_se": float(d.std() / len(dl) ** 0.5) if len(dl) > 1 else None, "abs_max": float(d.abs().max()),
            "param_rel_divergence_at_end": float((fa - fb).norm() / fb.norm()),
            "tolerance": "first step |diff| <= 5e-6 (committed lock-steps: <= 7.2e-7); see DESIGN.md section 4",
            "pass": bool(abs(float(d[0])) <= 5e-6), "seconds": round(time.perf_counter() - t0, 1),
            "oracle": "oracle/neus_oracle.py (this repo's restatement of upstream NeuS: parity unpinned at the reference)"}


def occgrid_quality_record():
    """PSNR at 2k iterations of the occupancy-grid sampler minus the hierarchical sampler (hash family, 8 paired seeds; committed)."""
    path = os.path.join(ROOT, "profiles", "psnr_r05_hash_occgrid_vs_hierarchical.json")
    try:
        w = json.load(open(path))["window_delta"]
        return {"mean": round(w["mean_db"], 3), "se": round(w["se_db"], 3), "seeds": w["n"], "measured_in_this_run": False,
                "source": "profiles/" + os.path.basename(path),
                "note": "equal iterations; the marcher is faster per step and learns less per step (nerfacc's refresh schedule: -0.69 +- 0.09)"}
    except (OSError, KeyError, ValueError):
        return None


def lib_identity():
    """Which library bytes ran: sha256 of the loaded .so and the stamp build() left beside it."""
    import hashlib
    from dynhor_amd import _lib
    h = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    stamp = os.path.join(os.path.dirname(_lib.LIB_PATH), "libdynhor_hip.build.json")
    build = None
    if os.path.exists(stamp):
        try:
            st = json.load(open(stamp))
            build = ({"mode": st.get("last_build_call"), "sources_sha16": st.get("sources_sha16"),
                      "hipcc": st.get("hipcc"), "flags": st.get("flags")} if st.get("lib_sha16") == h
                     else {"mode": "unknown (the stamp beside the library is of another build)"})
        except (OSError, ValueError):
            build = None
    return h, build


DUMP_MAX_FLOATS = 1 << 22          # per array (16 MB of float32): the hash family's 12.2 M-entry vectors are sampled


def dump_outputs(out_dir, stats, store):
    """--dump-outputs: what the last timed step computed, as float32 .npy files -- the loss statistics train_iteration returned, the
    flat parameters after its Adam step and the flat gradient it applied.  A vector longer than DUMP_MAX_FLOATS is written as a fixed,
    seeded sample of its entries (the same indices in every run), so that all files stay well under 64 MB."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    for name, t in (("stats", stats), ("params", store.flat), ("grad", store.grad_flat)):
        t = t.detach().reshape(-1).float().cpu()
        if t.numel() > DUMP_MAX_FLOATS:
            t = t[torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))[:DUMP_MAX_FLOATS].sort().values]
        np.save(os.path.join(out_dir, f"{name}.npy"), t.numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernel-steps", type=int, default=20, help="steps of the second loop, with per-stage HIP-event timers on")
    ap.add_argument("--no-secondary", action="store_true", help="skip the secondary lines (cfg4, cfg4 + occupancy grid, cfg5 loss stack)")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--family", choices=["neus", "hash"], default="neus",
                    help="neus = BASELINE.json configs[1] (the headline); hash = configs[3] (hash-grid encoding + shallow MLPs)")
    ap.add_argument("--arithmetic", choices=["split_f16", "split_bf16", "fp32_mfma"], default="split_f16",
                    help="split_f16 = two fp16 pieces / three MFMA products per fp32 product (shipping); split_bf16 = three bf16 "
                         "pieces / six products (rounds 1-3); fp32_mfma = the native fp32-MFMA twins")
    ap.add_argument("--loss", choices=["cfg2", "full"], default="cfg2",
                    help="cfg2 = rgb + eikonal + mask + mono-normal (the headline config); full = BASELINE.json configs[4]'s loss "
                         "stack: additionally the dense-correspondence reprojection term on a quarter of the rays")
    ap.add_argument("--hash-sampler", choices=["hierarchical", "occgrid"], default="hierarchical",
                    help="hash family only: NeuS 64+64 sampler or instant-nsr-pl occupancy-grid marching (packed rays)")
    ap.add_argument("--float-atomic-table-grad", action="store_true",
                    help="hash family: the table scatter by float atomics instead of the default fixed-point integer atomics "
                         "(dh_hash_weight_grads_parts, parts bit 4 clear)")
    ap.add_argument("--serial-weight-grads", action="store_true",
                    help="DEVELOPMENT, hash family: the table scatter and the small weight-gradient GEMMs on one stream (default: two streams)")
    ap.add_argument("--rays-per-rank", type=int, default=2048,
                    help="2048 = throughput mode (weak scaling, the headline); 2048/N = fixed global batch (PSNR-parity mode)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-rays", type=int, default=None, help="rays of the cpu_baseline sample (default 2048; hash family 128)")
    ap.add_argument("--psnr", action="store_true", help="add psnr_at_2k: HIP path vs oracle at equal iterations (scripts/psnr_parity.py)")
    ap.add_argument("--no-parity-check", action="store_true",
                    help="skip parity_check (one 50-iteration lock-step segment HIP vs GPU-eager oracle after the timed region, ~10 s)")
    ap.add_argument("--parity-iters", type=int, default=50)
    ap.add_argument("--psnr-seeds", type=int, default=2)
    ap.add_argument("--psnr-iters", type=int, default=2000)
    ap.add_argument("--backend", type=str, default="nccl", help="torch.distributed backend (nccl == RCCL; gloo for tests)")
    ap.add_argument("--share-gpu", action="store_true", help="TEST ONLY: every rank uses cuda:0 (with --backend gloo)")
    ap.add_argument("--check-sync", action="store_true", help="(default at N > 1) verify all ranks hold identical parameters at the end")
    ap.add_argument("--no-check-sync", action="store_true")
    ap.add_argument("--force-dist", action="store_true", help="TEST ONLY: initialise the process group even for one rank")
    ap.add_argument("--lib", type=str, default=None, help="DEVELOPMENT: another build of the library (scripts/build_variant.sh), for same-box A/Bs")
    ap.add_argument("--full", action="store_true",
                    help="beyond the headline: the per-stage timer loop (kernels, roofline), the all-reduce diagnostics (comm), "
                         "cpu_baseline, parity_check, the secondary lines and psnr_at_2k (their --no-* / --psnr options apply here)")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="write what the last timed step computed (loss statistics, updated parameters, flat gradient) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.psnr and not args.full:
        ap.error("--psnr is a measurement of --full: pass both")

    from dynhor_amd import launch
    if args.gpus > 1 and not launch.launched_by_torchrun():
        # `python bench.py --gpus N`: nobody started the ranks for us, so start them -- as CHILD processes, before anything in
        # this process touches the GPU (the parent makes no HIP call at all); rank 0's JSON line reaches our stdout unchanged
        # and we leave with the ranks' exit code.  Under `python -m torch.distributed.run ... bench.py --gpus N` (the
        # driver's form) WORLD_SIZE is set and this branch is not taken.
        # (no device query here: the parent makes NO call that could initialise the HIP runtime -- ADVICE r3; a rank whose GPU does
        # not exist fails in torch.cuda.set_device and the launcher relays its non-zero exit code)
        sys.exit(launch.spawn_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but the launcher set WORLD_SIZE={world}; pass the same N to both", file=sys.stderr,
              flush=True)
        sys.exit(2)
    if args.share_gpu:
        local_rank = 0
    use_dist = world > 1 or args.force_dist
    saved_stdout = None
    if use_dist:
        # RCCL prints a version banner on STDOUT when its communicator comes up (first collective); this program's stdout is
        # ONE JSON line, so everything native code writes to fd 1 until the collectives have run goes to stderr instead
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if not launch.launched_by_torchrun():          # --force-dist with one self-started rank: a private rendezvous
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(launch.free_port()), RANK="0", WORLD_SIZE="1",
                              LOCAL_RANK="0")
        torch.cuda.set_device(local_rank)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
        else:
            dist.init_process_group(args.backend)
    device = torch.device(f"cuda:{local_rank}")
    torch.cuda.set_device(device)

    from dynhor_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.join(ROOT, args.lib)
    from dynhor_amd.runner import Runner

    def bench_line(args, restore_stdout):
        """One measured line (rank 0 returns the dict, the others None).  restore_stdout: give fd 1 back once the collectives have run."""
        nonlocal saved_stdout
        arith = _lib.ARITH_NAMES[args.arithmetic]
        hash_family = args.family == "hash"
        full = args.loss == "full"
        conf = {"seq_name": "bench_synth", "exp_name": f"r{rank}",
                "data_info": {"synthetic": {"n_frames": args.frames, "H": 512, "W": 512, "seed": 4321,
                                            "correspondences": 2048 if full else 0}},
                "train": {"batch_size": args.rays_per_rank, "normal_weight": 0.05, "report_freq": 10 ** 9, "save_freq": 10 ** 9,
                          "val_freq": 0, "corr_weight": 0.1 if full else 0.0, "corr_fraction": 0.25},
                "model": {"family": args.family, "arithmetic": args.arithmetic, "hash_renderer": {"sampler": args.hash_sampler, "reproducible_table_grad": not args.float_atomic_table_grad}}}
        runner = Runner(conf=conf, device=device, exp_root=os.path.join("/tmp", "dynhor_bench_exps"))
        if args.serial_weight_grads:
            runner.renderer.concurrent_weight_grads = False
        B = runner.batch_size
        n_samples = runner.renderer.n_samples + runner.renderer.n_importance

        def sync():
            torch.cuda.synchronize()
            if use_dist:
                dist.barrier()
            torch.cuda.synchronize()

        for _ in range(args.warmup):
            runner.train_iteration()
        runner.renderer.timer.enabled = False
        sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            stats = runner.train_iteration()
        sync()
        dt_local = dt = time.perf_counter() - t0
        if use_dist:
            t = torch.tensor([dt], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, stats, runner.store)
        kern, kern_steps = {}, max(args.kernel_steps, 1)
        if args.full:
            # second, short loop with the per-stage HIP-event timers on (on the launch stream): the `kernels` block and the roofline's
            # launch duration -- kept out of the headline loop above
            runner.renderer.timer.enabled = True
            runner.renderer.timer.reset()
            for _ in range(kern_steps):
                runner.train_iteration()
            torch.cuda.synchronize()
            runner.renderer.timer.enabled = False
            kern = runner.renderer.timer.summary()

        comm = None
        if use_dist and args.full:
            # self-diagnosis for the first real multi-GPU run: what the process group reports, and the cost of the one collective
            # on this path in isolation (the flat gradient bucket; 20 back-to-back all-reduces, HIP events)
            g = runner.store.grad_bucket()           # the very buffer the training loop reduces (same registered address)
            for _ in range(3):
                dist.all_reduce(g)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                dist.all_reduce(g)
            b.record()
            torch.cuda.synchronize()
            ar_ms = a.elapsed_time(b) / 20
            t = torch.tensor([ar_ms], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            nccl_ver = None
            try:
                nccl_ver = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:
                pass
            # per-rank step time and device (a straggler or a mis-bound rank would otherwise be invisible behind the MAX)
            mine = torch.tensor([dt_local / args.steps * 1e3], device=device, dtype=torch.float64)
            every = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(every, mine)
            rank_ms = [float(x.item()) for x in every]
            prop = torch.cuda.get_device_properties(device)
            devs = [None] * world
            dist.all_gather_object(devs, {"rank": rank, "local_rank": local_rank, "name": prop.name,
                                          "arch": getattr(prop, "gcnArchName", None), "cus": prop.multi_processor_count})
            comm = {"backend": dist.get_backend(), "nranks": dist.get_world_size(), "rccl_version": nccl_ver,
                    "rank_ms_per_step": {"min": round(min(rank_ms), 3), "max": round(max(rank_ms), 3),
                                         "rank_of_max": int(max(range(world), key=lambda i: rank_ms[i])),
                                         "all": [round(x, 3) for x in rank_ms]},
                    "devices": devs,
                    "bucket_bytes": g.numel() * 4, "bucket_persistent": runner.store.grad_flat.data_ptr() == g.data_ptr(),
                    "allreduce_only_ms": round(float(t.item()), 4),
                    "allreduce_frac_of_step": round(float(t.item()) / (dt / args.steps * 1e3), 4),
                    "collectives_per_step": 2 if getattr(runner, "overlap_table_reduce", False) else 1}
            if getattr(runner, "overlap_table_reduce", False):
                tf = runner.store.table_floats
                comm["collective_bytes"] = {"table_gradient (side stream, overlapped with the small weight-gradient GEMMs)": tf * 4,
                                            "mlp_gradients": (g.numel() - tf) * 4}
        if saved_stdout is not None:
            torch.cuda.synchronize()
            sys.stdout.flush()
            import ctypes
            ctypes.CDLL(None).fflush(None)          # RCCL printf()s into libc's stdout buffer: empty it while fd 1 still is stderr
            os.dup2(saved_stdout, 1)
            os.close(saved_stdout)
            saved_stdout = None
        if world > 1 and not args.no_check_sync:        # on by default: the first multi-GPU contact must not pass with diverged ranks
            ref = runner.store.flat.clone()
            dist.broadcast(ref, src=0)
            assert torch.equal(ref, runner.store.flat), f"rank {rank}: parameters diverged from rank 0"
            frames = torch.tensor([float(runner.image_perm[(i * world + rank) % runner.dataset.n_images]) for i in range(4)],
                                  device=device)
            allf = [torch.empty_like(frames) for _ in range(world)]
            dist.all_gather(allf, frames)
            flat = torch.stack(allf).reshape(-1).tolist()
            assert len(set(flat)) == len(flat), "ranks must draw disjoint frames"
            if comm is not None:
                comm["check_sync"] = "identical parameters on all ranks, disjoint frames"
            if rank == 0:
                print("check-sync ok: identical parameters on all ranks, disjoint frames", file=sys.stderr, flush=True)

        if rank == 0:
            ms = dt / args.steps * 1e3
            value = world * B * args.steps / dt
            P = B * n_samples
            pts = {"sdf_nograd_coarse": B * runner.renderer.n_samples,
                   "sdf_nograd_fine": B * (runner.renderer.n_importance // max(runner.renderer.up_sample_steps, 1))}
            per_kernel = {}
            for k, (mean_ms, cnt) in kern.items():
                per_kernel[k] = {"ms": round(mean_ms, 4), "launches_per_step": cnt / kern_steps}
                if k in MACS and not hash_family:
                    npts = pts.get(k, P)
                    per_kernel[k]["tflops"] = round(2.0 * MACS[k] * npts / (mean_ms * 1e-3) / 1e12, 2)
            traffic_path = os.path.join(ROOT, "profiles", "pmc_traffic_hash.json" if hash_family else "pmc_traffic.json")
            traffic_table = json.load(open(traffic_path)) if os.path.exists(traffic_path) else {}

            def offline_traffic(stage, kernel):
                """HBM bytes per launch from the committed rocprofv3 PMC passes -- only if they were taken on THIS kernel."""
                e = traffic_table.get(stage)
                if e and e.get("kernel") == kernel:
                    return e.get("hbm_bytes_per_launch"), f"profiles/{os.path.basename(traffic_path)} (offline rocprofv3 PMC passes: FETCH_SIZE x2 + WRITE_SIZE)"
                return None, None

            if hash_family:
                workload = (f"instant-nsr-pl-shaped hash-grid family (BASELINE.json configs[3]): 16-level x 2-feature hash grid (T = 2^19) + "
                            f"1x64 geometry MLP with finite-difference normals + SH-4 2x64 colour MLP, custom_shoes-shaped synthetic seq, "
                            f"512x512, {B} rays x " + ("(64+64) samples" if args.hash_sampler == "hierarchical" else
                                                         "occupancy-grid marching (packed rays: fixed capacity of 128 samples per ray on average, "
                                                         "per-ray cap up to 1024 chosen on the device)")
                            + " per rank, full training iteration; 'LDS-resident grid tiles' of the config's wording: built (levels 0-1, the "
                            "only ones that fit 160 KB), measured slower (0.48 vs 0.44 ms per forward), not shipped")
                arithmetic = ("fp32 everywhere (VALU / fp32 MFMA for the small dW GEMMs); table gradient by "
                              + ("2^-48 fixed-point integer atomics (bitwise reproducible)" if not args.float_atomic_table_grad else "float atomics"))
            else:
                workload = (f"custom_shoes-shaped synthetic seq, 512x512, {B} rays x (64+64) samples per rank, "
                            "NeuS SDF(8x256, skip 4, softplus100) + colour(4x256) MLP, full training iteration")
                arithmetic = {"fp32_mfma": "fp32 everywhere, every GEMM on v_mfma_f32_32x32x2_f32 (--arithmetic fp32_mfma)",
                              "split_bf16": "fp32 in / fp32 out everywhere; GEMMs as 3-way bf16 split of both operands (6 MFMA "
                                            "products, fp32 accumulate: 2^-24 relative = fp32 accuracy; --arithmetic split_bf16)",
                              "split_f16": "fp32 in / fp32 out everywhere; GEMMs as 2-way fp16 split of both operands scaled by powers of two "
                                           "(3 MFMA products, fp32 accumulate: fp32 accuracy, measured 1.9e-7 vs fp64 against 2.3e-7 for "
                                           "the exact fp32 MFMA)"}[args.arithmetic]
            if not args.full:
                roof = None          # the per-stage timer loop did not run
            elif hash_family:
                # dominant stage of this family: the table-gradient scatter of dh_hash_weight_grads_parts (memory-side-atomic bound; the
                # five small dW reductions of the same entry point run beside it on a second stream: hash_weight_grads_mlp).
                # Algorithmic bytes per launch = every add the per-evaluation scatter defines (7 evaluations x 16 levels x 8 corners x
                # 2 features x 4 B per sample); dw_operands = one read of the small GEMMs' operands (the concurrent stage).
                dom = "hash_weight_grads"
                Pk = runner.renderer.last_march["samples"] if args.hash_sampler == "occgrid" else P     # packed rays: the last step's count
                add_bytes = 7 * Pk * 16 * 8 * 2 * 4
                dw_bytes = 7 * Pk * (64 + 36 + 13 + 64) * 4 + Pk * (64 + 32 + 64 + 64 + 3 + 64) * 4
                tsec = per_kernel[dom]["ms"] * 1e-3
                kernel = _lib.HASH_STAGE_KERNELS[dom]
                traffic, tsrc = offline_traffic(dom, kernel)
                scale = 1.0
                if args.hash_sampler == "occgrid" and traffic is not None:
                    # the committed counters are of the 262,144-sample launch: a packed launch touches the table and the dW operands
                    # in proportion to its sample count
                    scale = Pk / float(P)
                    traffic = traffic * scale
                    tsrc = tsrc + f", scaled by this launch's sample count ({Pk} / {P})"
                # the stage is bound by the table scatter: float atomics execute at the memory side at ~1.3 TB/s of added bytes chip-wide
                # (MI355X_MICROARCH.md, Global float atomics), not at the HBM rate -- that is the ceiling it is priced against.
                # achieved = ALGORITHMIC added bytes (what the per-evaluation scatter defines) / stage time: the kernel merges ~85 %
                # of them in registers / across lanes before they reach memory, so it can exceed the physical atomic rate.
                te = traffic_table.get(dom, {}) if traffic is not None else {}
                # like for like: PHYSICAL atomic bytes (what reaches memory after the in-register / cross-lane
                # merge; committed PMC pass, WRITE_SIZE of the scatter kernel) against the 1.3 TB/s float-atomic ceiling, and counter
                # HBM bytes against the 6.29 TB/s the guide measures as achievable; `frac` = the larger of the two.  The ALGORITHMIC
                # adds (what the per-evaluation scatter defines) over the physical ones is the merge ratio.  Neither bound explains
                # the stage's time: it is latency / contention bound (DESIGN_NEXT_ROWS.md section 7).
                phys = te.get("atomic_bytes_per_launch")
                phys = None if phys is None else phys * scale
                f_atomic = None if phys is None else phys / tsec / 1e9 / FLOAT_ATOMIC_PEAK_GBPS
                f_hbm = None if traffic is None else traffic / tsec / 1e9 / HBM_ACHIEVABLE_GBPS
                fracs = [f for f in (f_atomic, f_hbm) if f is not None]
                roof = {"bound": "hbm", "kernel": kernel + " (+ hash_fix_to_float_kernel; small_dw_kernel and its reductions run concurrently on a second stream)", "stage": dom,
                        "achieved": None if phys is None else round(phys / tsec / 1e9, 1), "peak": FLOAT_ATOMIC_PEAK_GBPS, "unit": "GB/s",
                        "frac": round(max(fracs), 4) if fracs else None,
                        "peak_basis": "physical atomic request bytes (64 B each) / time against the memory-side atomic rate the guide measures "
                                      "for float atomics, 1.3 TB/s (Global float atomics; the int64 atomics of the fixed-point scatter "
                                      "run at the same request rate: profiles/r05_hash_reproducible_scatter.json); frac = max(that, "
                                      "counter HBM bytes / time / 6.29 TB/s)",
                        "frac_atomic": None if f_atomic is None else round(f_atomic, 4),
                        "frac_hbm_counters": None if f_hbm is None else round(f_hbm, 4),
                        "merge_ratio_algorithmic_over_physical_adds": None if phys is None else round(add_bytes / phys, 2),
                        "traffic": traffic, "traffic_source": tsrc,
                        "physical_atomic_bytes_per_launch": phys,
                        "avg_launch_ms": per_kernel[dom]["ms"],
                        "algorithmic_bytes": {"scatter_adds": add_bytes, "dw_operands_of_the_concurrent_stage": dw_bytes},
                        "algorithmic_adds_GBps": round(add_bytes / tsec / 1e9, 1)}
                if args.hash_sampler == "occgrid":
                    lm = runner.renderer.last_march
                    per_kernel["march"] = {"samples_per_ray_last_step": round(lm["samples_per_ray"], 2), "per_ray_cap": lm["per_ray_cap"],
                                           "rays_at_cap": lm["rays_at_cap"], "rays_truncated": lm["rays_truncated"],
                                           "capacity": lm["capacity"]}
            else:
                names = _lib.STAGE_KERNELS[arith]
                dom = max((k for k in per_kernel if per_kernel[k]["launches_per_step"] <= 1.01 and "tflops" in per_kernel[k]),
                          key=lambda k: per_kernel[k]["ms"])
                # peak of the dominant kernel's own instruction mix: every GEMM runs each fp32 product as 6 bf16 products (3-way
                # split of both operands, fp32 accumulate: 2^-24 relative) on v_mfma_f32_32x32x16_bf16, so the ceiling in
                # ALGORITHMIC (fp32-product) FLOP/s is the dense bf16 peak / 6; fp32_mfma runs v_mfma_f32_32x32x2_f32 (157.3 TFLOP/s)
                split = arith != _lib.ARITH_FP32_MFMA
                nprod = {_lib.ARITH_SPLIT_F16: 3.0, _lib.ARITH_SPLIT_BF16: 6.0}.get(arith, 1.0)
                peak = BF16_MFMA_PEAK_TFLOPS / nprod if split else FP32_MFMA_PEAK_TFLOPS
                traffic, tsrc = offline_traffic(dom, names[dom])
                ntile = (P + 63) // 64
                for k, v in per_kernel.items():
                    if "tflops" in v:
                        v["kernel"] = names.get(k)
                        v["frac_of_peak"] = round(v["tflops"] / peak, 4)
                    if k in STAGE_TILES:
                        nbytes = ntile * (STAGE_TILES[k][0] * 65536 + STAGE_TILES[k][1] * 16384)
                        v["algorithmic_hbm_bytes"] = nbytes
                        v["hbm_gbps"] = round(nbytes / (v["ms"] * 1e-3) / 1e9, 1)
                        v["frac_of_hbm_peak"] = round(nbytes / (v["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
                # the roofline that bounds this path is the MATRIX pipe (> 99 % of the algorithmic FLOPs are the MLP
                # GEMMs; fused, the algorithmic HBM traffic is ~23 MB per step) -- so `frac` = algorithmic fp32-product FLOP/s of the
                # dominant kernel / the ceiling of its instruction mix.  The save-everything data flow of THIS design
                #  puts the large kernels on an HBM floor of their own: that engineering view rides along as
                # `design_floor` (design_bytes = the saved tiles the stage must read or write once; NOT section 8(d)'s algorithmic bytes).
                d = per_kernel[dom]
                t_mfma = 2.0 * MACS[dom] * pts.get(dom, P) / (peak * 1e12)
                t_hbm = d.get("algorithmic_hbm_bytes", 0) / (HBM_PEAK_GBPS * 1e9)
                roof = {"bound": "mfma", "bound_in_this_design": "hbm" if t_hbm > t_mfma else "mfma",
                        "kernel": names[dom], "stage": dom, "achieved": d["tflops"], "peak": round(peak, 1),
                        "unit": "TFLOP/s", "frac": round(d["tflops"] / peak, 4),
                        "bound_basis": "`bound` is SURVEY.md section 8(d)'s (the path, fused, is matrix-bound: `frac` is priced against the "
                                       "matrix ceiling); `bound_in_this_design` says which ceiling the dominant launch needs longer at "
                                       "peak rates in THIS save-everything data flow (design_floor.why) -- where that is hbm, `frac` is "
                                       "measured against a ceiling the kernel cannot reach without changing the data flow",
                        "peak_basis": (f"dense fp16 / bf16 MFMA 2500 TFLOP/s / {int(nprod)} matrix products per fp32 product "
                                       f"(the {'three' if nprod == 3 else 'six'}-product ceiling of this arithmetic)" if split
                                       else "fp32 MFMA v_mfma_f32_32x32x2_f32"),
                        "algorithmic_flop": 2 * MACS[dom] * pts.get(dom, P),
                        "frac_of_six_product_peak": round(d["tflops"] / (BF16_MFMA_PEAK_TFLOPS / 6.0), 4),
                        "frac_of_fp32_mfma_peak": round(d["tflops"] / FP32_MFMA_PEAK_TFLOPS, 4),
                        "design_floor": {"design_bytes": d.get("algorithmic_hbm_bytes"), "achieved_gbps": d.get("hbm_gbps"),
                                         "frac_of_hbm_peak_8000": d.get("frac_of_hbm_peak"),
                                         "frac_of_achievable_6290": None if d.get("hbm_gbps") is None else round(d["hbm_gbps"] / HBM_ACHIEVABLE_GBPS, 4),
                                         "why": f"at peak rates this launch needs {t_hbm * 1e3:.2f} ms of HBM time for its saved tiles against "
                                                f"{t_mfma * 1e3:.2f} ms of matrix time: within this data flow it is "
                                                + ("HBM-bound" if t_hbm > t_mfma else "matrix-bound")}}
                step_tf = value / world * FLOP_PER_RAY_TRAIN / 1e12
                step_bytes = sum(v.get("algorithmic_hbm_bytes", 0) for v in per_kernel.values())
                # counter HBM bytes of one whole step (every committed per-stage PMC entry that was taken on the kernel this run used)
                # over section 8(d)'s algorithmic bytes per step: fused Adam (7 words per parameter) + the ray gather
                s8d_bytes = 802491 * 7 * 4 + B * (8 + 56)
                counter_step = 0.0
                for k, v in per_kernel.items():
                    tb, _ = offline_traffic(k, names.get(k))
                    if tb is not None:
                        counter_step += tb * v["launches_per_step"]
                roof.update({"traffic": traffic, "traffic_source": tsrc, "avg_launch_ms": d["ms"],
                             "traffic_ratio": None if counter_step == 0 else round(counter_step / s8d_bytes, 1),
                             "traffic_ratio_basis": f"counter HBM bytes of one step ({counter_step / 1e9:.2f} GB over the MLP stages) / SURVEY.md "
                                                    f"section 8(d) algorithmic bytes per step ({s8d_bytes / 1e6:.1f} MB: Adam + ray gather)",
                             "whole_step_tflops": round(step_tf, 2), "whole_step_frac_of_peak": round(step_tf / peak, 4),
                             "whole_step_frac_of_six_product_peak": round(step_tf / (BF16_MFMA_PEAK_TFLOPS / 6.0), 4),
                             "whole_step_frac_of_fp32_mfma_peak": round(step_tf / FP32_MFMA_PEAK_TFLOPS, 4),
                             "whole_step_design_hbm_gbps": round(step_bytes / (ms * 1e-3) / 1e9, 1),
                             "whole_step_design_frac_of_hbm_peak": round(step_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)})
            # which matrix pipe ran: `dtype` is the I/O, accumulate and optimizer type
            mfma_dtype = ("f32 (v_mfma_f32_32x32x2_f32, small weight-gradient GEMMs only; the MLPs run on the vector ALU)" if hash_family else
                          {"split_f16": "f16 (2-piece split, 3 products per fp32 product, fp32 accumulate)",
                           "split_bf16": "bf16 (3-piece split, 6 products per fp32 product, fp32 accumulate)",
                           "fp32_mfma": "f32 (v_mfma_f32_32x32x2_f32)"}[args.arithmetic])
            out = {"metric": "training rays/sec", "value": round(value, 1), "unit": "rays/s", "n_gpus": world,
                   "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True,
                   "scaling": "weak" if args.rays_per_rank == 2048 else "strong", "vs_baseline": None, "dtype": "f32", "mfma_dtype": mfma_dtype,
                   "data": "synthetic",
                   "config": {"workload": workload, "family": args.family, "frames": args.frames, "rays_per_rank": B,
                              "samples_per_ray": n_samples, "parallelism": f"dp{world}",
                              "loss": "rgb L1 + 0.1 eikonal + 0.1 mask BCE + 0.05 mono-normal"
                                      + (" + 0.1 dense-correspondence reprojection (Huber 4 px) on 25 % of the rays" if full else ""),
                              "arithmetic": arithmetic},
                   **({"roofline": roof, "kernels": per_kernel} if args.full else {}),
                   "lib_sha16": lib_identity()[0], "build": lib_identity()[1],
                   "final_stats": {"loss": round(float(stats[0]), 5), "psnr": round(float(stats[5]), 3)}}
            if comm is not None:
                out["comm"] = comm
            if args.full and world == 1 and not args.no_cpu_baseline:
                frame = int(runner.image_perm[0])
                g = torch.Generator(device=device); g.manual_seed(99)
                n_cpu = args.cpu_rays if args.cpu_rays is not None else (128 if hash_family else 2048)
                rays = runner.dataset.gen_random_rays_at(frame, n_cpu, generator=g)
                out["cpu_baseline"] = cpu_baseline(rays, runner.dataset.R[frame], runner.renderer.n_samples,
                                                   runner.renderer.n_importance, runner.normal_weight, family=args.family)
            if (args.full and world == 1 and not hash_family and not args.no_parity_check and args.rays_per_rank == 2048 and restore_stdout
                    and args.loss == "cfg2"):
                # measured by THIS run, outside the timed region; last, because it replaces the runner's optimizer state
                try:
                    out["parity_check"] = parity_check_in_this_run(runner, device, args.parity_iters)
                except Exception as e:          # noqa: BLE001 -- the check must never take the measured line down; it says so instead
                    out["parity_check"] = {"measured_in_this_run": False, "error": repr(e)}
            if args.psnr and world == 1:
                # the oracle is the checker here (never the thing measured): PSNR of both arms on all frames at equal iterations
                sys.path.insert(0, os.path.join(ROOT, "scripts"))
                import psnr_parity
                psnr_parity.LOG = sys.stderr          # this program prints ONE JSON line on stdout
                seeds = ",".join(str(11 * (i + 1)) for i in range(args.psnr_seeds))
                res = psnr_parity.run_parity(["--mode", "hip_vs_oracle", "--family", args.family, "--seeds", seeds,
                                              "--iters", str(args.psnr_iters)])
                w = res["window_delta"]
                out["psnr_at_2k"] = {"hip": round(res["window_mean_a"], 3), "oracle": round(res["window_mean_b"], 3),
                                     "delta": round(w["mean_db"], 4), "se": None if w["n"] < 2 else round(w["se_db"], 4),
                                     "seeds": w["n"], "per_seed_delta": [round(x, 4) for x in w["per_seed"]],
                                     "iters": res["iters"], "protocol": res["protocol"],
                                     "committed_runs": "profiles/psnr_parity_r02*.json + psnr_parity_r03*.json (43 paired seeds neus, oracle / HIP noise floors, lock-step; hash: 6 seeds + sampler reports)"}
            return out
        return None

    out = bench_line(args, True)
    if rank == 0:
        if (args.full and world == 1 and args.family == 'neus' and args.loss == 'cfg2' and args.arithmetic == 'split_f16' and not args.no_secondary
                and args.rays_per_rank == 2048):
            # the other configurations BASELINE.json names, made visible in the one line the driver records:
            # 20 steps each, same schema, no CPU baseline of their own
            import copy
            sec = {}
            for name, over in (('hash', dict(family='hash')), ('hash_occgrid', dict(family='hash', hash_sampler='occgrid')),
                               ('full_loss', dict(loss='full'))):
                a2 = copy.copy(args)
                a2.steps, a2.warmup, a2.kernel_steps, a2.no_cpu_baseline, a2.psnr, a2.dump_outputs = 20, 5, 10, True, False, None
                for k, v in over.items():
                    setattr(a2, k, v)
                try:
                    line = bench_line(a2, False)
                    sec[name] = {k: line[k] for k in ('value', 'unit', 'ms_per_step', 'steps', 'warmup', 'config', 'roofline', 'kernels', 'final_stats')}
                    if name == 'hash_occgrid':
                        # a throughput number on a sampler that learns LESS per iteration: never read it without this
                        sec[name]['psnr_vs_hierarchical_db'] = occgrid_quality_record()
                except Exception as e:          # noqa: BLE001 -- a secondary line must never take the headline down
                    sec[name] = {'error': repr(e)}
            out['secondary'] = sec
            if 'psnr_at_2k' not in out:
                out['psnr_at_2k'] = committed_psnr_record()
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
