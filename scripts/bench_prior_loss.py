"""Timing of the depth / masked normal priors (dynhor_amd/renderer.py: prior_loss -> dh_prior_loss, dh_prior_loss_packed;
DESIGN_NEXT_ROWS.md section 27).

  kernel   the entry alone (its three launches) on a dense batch of 2048 x 128 and on a packed batch of 2048 rays with ragged counts
           (mean about 64, a few at 1024), depth and normal term on; next to dh_corr_loss on the same dense batch, in alternating runs.
  step     the MLP family's training step (Runner.train_iteration without the all-reduce: one rank) at batch 2048 on the synthetic
           scene with analytic depth maps, with the terms off and on, in alternating runs; then the hash family's occupancy-grid step.

Every time is taken with device events around --reps calls after a warm-up, and the median of --rounds alternating rounds is reported
with the spread (min, max).  One JSON line per measurement.  Kernel times proper come from a profiler run of this script:

    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <out> -o prior -- python scripts/bench_prior_loss.py --only kernel
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    """milliseconds per call: device events around `reps` calls."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(variants, reps, rounds, warmup):
    """{name: [ms per call, one per round]} with the variants run in turn inside every round."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(timed(fn, reps))
    return out


def line(name, ms, **kw):
    print(json.dumps({"bench": "prior_loss", "name": name, "ms_median": round(statistics.median(ms), 5), "ms_min": round(min(ms), 5),
                      "ms_max": round(max(ms), 5), "rounds": len(ms), **kw}), flush=True)


def kernel_inputs(B, n, dev, seed=0):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    R = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    dc = torch.nn.functional.normalize(torch.cat([0.4 * torch.randn(B, 2, generator=g), torch.ones(B, 1)], -1), dim=-1)
    rays = torch.zeros(B, 14)
    rays[:, 3:6] = dc @ R
    rays[:, 0:3] = -2.5 * rays[:, 3:6]
    rays[:, 9] = (torch.rand(B, generator=g) < 0.5).float()
    rays[:, 10] = (torch.rand(B, generator=g) < 0.9).float()
    mono = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1)
    mono[torch.rand(B, generator=g) < 0.7] = 128.0 / 255.0 * 2.0 - 1.0           # an MVS normal map is mostly holes
    rays[:, 11:14] = mono
    z = 1.5 + torch.sort(torch.rand(B, n, generator=g) * 2.0, dim=-1).values
    w = torch.rand(B, n, generator=g) ** 4
    w = w / w.sum(-1, keepdim=True)
    prior = 2.5 + 0.1 * torch.randn(B, generator=g)
    prior[torch.rand(B, generator=g) < 0.5] = float("inf")
    nmap = torch.randn(B, 3, generator=g)
    return [t.to(dev).contiguous() for t in (rays, R.reshape(9), z, w, prior, nmap)]


def bench_kernel(args, dev):
    import torch
    from dynhor_amd import _lib
    from dynhor_amd.renderer import _p, prior_loss
    B, n = args.rays, args.samples
    rays, R, z, w, prior, nmap = kernel_inputs(B, n, dev)
    dw, dn = torch.empty(B, n, device=dev), torch.empty(B, 3, device=dev)
    sd = 2.0 / 64
    dense = lambda: prior_loss(rays, R, z, w, nmap, prior, sd, 0.1, 0.02, 0.05, False, dw, dn)
    depth_only = lambda: prior_loss(rays, R, z, w, None, prior, sd, 0.1, 0.02, 0.0, False, dw, None)
    # dh_corr_loss on the same batch: every ray matched into one of 8 frames
    g = torch.Generator(device="cpu").manual_seed(1)
    F = 8
    R_all = torch.linalg.qr(torch.randn(F, 3, 3, generator=g))[0].to(dev).contiguous()
    T_all = (torch.randn(F, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, 2.3])).to(dev).contiguous()
    K = torch.tensor([[614.4, 0, 256.0], [0, 614.4, 256.0], [0, 0, 1]], device=dev)
    corr = torch.stack([torch.rand(B, generator=g) * 511, torch.rand(B, generator=g) * 511, torch.rand(B, generator=g),
                        torch.randint(0, F, (B,), generator=g).float()], -1).to(dev).contiguous()
    o, d = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous()
    cst, res = torch.empty(4, device=dev), torch.empty(B, device=dev)
    L = _lib.lib()
    corr_fn = lambda: _lib.check(L.dh_corr_loss(_p(o), _p(d), _p(z), _p(w), _p(corr), _p(R_all), _p(T_all), F, _p(K), B, n, sd, 4.0, 0.1,
                                                _p(cst), _p(res), _p(dw), None, _lib.stream()))
    # packed: ragged counts, mean about 64, a few rays at the cap
    cnt = torch.randint(0, 129, (B,), generator=g)
    cnt[torch.rand(B, generator=g) < 0.01] = 1024
    off = (torch.cumsum(cnt, 0) - cnt).to(dev)
    N = int(cnt.sum())
    t_start = (1.5 + torch.rand(N, generator=g)).to(dev)
    wp = (torch.rand(N, generator=g) * 0.02).to(dev)
    dwp = torch.empty(N, device=dev)
    cnt32 = cnt.to(torch.int32).to(dev)
    packed = lambda: prior_loss(rays, R, t_start, wp, nmap, prior, 1.0 / 256, 0.1, 0.02, 0.05, False, dwp, dn, packed=(off, cnt32, 1024))
    t = alternate({"dense": dense, "dense_depth_only": depth_only, "corr_loss": corr_fn, "packed": packed}, args.reps, args.rounds, args.warmup)
    byt = B * n * 4 * 5 + B * (14 * 4 * 2 + 3 * 4 * 2 + 4 + 8)      # z, w read twice / once, d_weights written; the per-ray rows
    line(f"dh_prior_loss dense {B} x {n}, depth + normal (3 launches, incl. the workspace allocation)", t["dense"], bytes_moved=byt)
    line(f"dh_prior_loss dense {B} x {n}, depth only", t["dense_depth_only"])
    line(f"dh_corr_loss dense {B} x {n} (one workgroup), same process", t["corr_loss"])
    line(f"dh_prior_loss_packed {B} rays, {N} samples, depth + normal", t["packed"], samples=N)


def bench_step(args, dev):
    import torch
    from dynhor_amd.runner import Runner
    import tempfile
    tmp = tempfile.mkdtemp(prefix="bench_prior_")
    for family, sampler in (("neus", None), ("hash", "occgrid")):
        conf = {"seq_name": "bench", "exp_name": family,
                "data_info": {"synthetic": {"n_frames": 16, "H": 256, "W": 256, "seed": 4321, "depth": True}},
                "train": {"batch_size": args.rays, "normal_weight": 0.05, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0},
                "model": {"family": family}}
        if sampler:
            conf["model"]["hash_renderer"] = {"sampler": sampler}
        r = Runner(conf=conf, device=dev, exp_root=tmp)

        def step(on):
            def fn():
                r.depth_weight, r.normal_skip_missing = (0.1, True) if on else (0.0, False)
                r.train_iteration()
            return fn
        t = alternate({"off": step(False), "on": step(True)}, args.step_reps, args.rounds, args.warmup)
        name = f"{family}{' ' + sampler if sampler else ''} training step, batch {args.rays}"
        line(name + ", terms off", t["off"])
        line(name + ", depth term + masked normal term on", t["on"])
        del r
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step_reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=("kernel", "step"), default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    if args.only != "step":
        bench_kernel(args, dev)
    if args.only != "kernel":
        bench_step(args, dev)


if __name__ == "__main__":
    main()
