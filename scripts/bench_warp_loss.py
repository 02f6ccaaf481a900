"""Timing of the multi-view photometric term (dynhor_amd/warp_loss.py -> dh_ray_depth, dh_warp_loss, dh_ray_depth_bwd;
DESIGN_NEXT_ROWS.md section 30).

  kernel   the three new launches one by one at 2048 rays (P 5, 8 neighbours) on 1080 x 1920 frames: dh_ray_depth / dh_ray_depth_bwd on
           a dense batch of 2048 x 128 and on 2048 packed rays with ragged counts, dh_warp_loss (its ray kernel, the block-order sum and
           the stats kernel) on a fronto-parallel textured plane seen by 9 cameras 2 cm apart -- every ray counts, every neighbour is
           valid: the most work the kernel can have.
  step     the MLP family's training step (Runner.train_iteration on one rank) at batch 2048 on the synthetic scene with the term off
           and on, in alternating runs; then the hash family's occupancy-grid step.
  tables   the one-time build of the grey tables (warp_loss.frames_for) at --table_frames frames of 1080 x 1920, timed once.

Every time is taken with device events around --reps calls after a warm-up, and the median of --rounds alternating rounds is reported
with the spread (min, max).  One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_prior_loss import alternate  # noqa: E402


def line(name, ms, **kw):
    print(json.dumps({"bench": "warp_loss", "name": name, "ms_median": round(statistics.median(ms), 5), "ms_min": round(min(ms), 5),
                      "ms_max": round(max(ms), 5), "rounds": len(ms), **kw}), flush=True)


def plane_frames(F, H, W, dev, seed=0):
    """gray, valid u8 [F,H,W], R [F,9], T [F,3], K, Kinv [9]: the plane z = 1 of the object frame, textured, seen by F cameras that look
    along +z from (0.02 (i - F // 2), 0, 0)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    f = 1500.0
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=torch.float64)
    ph = (torch.rand(4, generator=g) * 6.0).tolist()
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    grays, Ts = [], []
    for i in range(F):
        cx = 0.02 * (i - F // 2)
        X, Y = (xs - W / 2) / f + cx, (ys - H / 2) / f                       # the plane point a pixel sees
        tex = 128 + 45 * torch.sin(400.0 * X + ph[0]) * torch.cos(330.0 * Y + ph[1]) + 35 * torch.sin(190.0 * X + 270.0 * Y + ph[2]) \
            + 25 * torch.cos(610.0 * X - 130.0 * Y + ph[3])
        grays.append(torch.floor(tex + 0.5).clamp(0, 255).to(torch.uint8))
        Ts.append([-cx, 0.0, 0.0])
    gray = torch.stack(grays).contiguous()
    R = torch.eye(3).reshape(1, 9).repeat(F, 1).to(dev).contiguous()
    T = torch.tensor(Ts, dtype=torch.float32, device=dev).contiguous()
    return (gray, torch.ones_like(gray), R, T, K.float().reshape(9).to(dev).contiguous(),
            torch.inverse(K).float().reshape(9).to(dev).contiguous())


def bench_kernel(args, dev):
    import torch
    from dynhor_amd import warp_loss as WL
    from dynhor_amd.mvs import neighbours
    from scripts.bench_prior_loss import kernel_inputs
    B, n, F, H, W = args.rays, args.samples, 9, 1080, 1920
    gray, valid, R_all, T_all, K, Kinv = plane_frames(F, H, W, dev)
    nbr = neighbours(F, (1, 2, 3, 4)).to(dev).contiguous()
    st = WL.kernel_settings(WL.check_settings({}))
    g = torch.Generator(device="cpu").manual_seed(2)
    frame = F // 2
    pix = torch.stack([torch.randint(200, W - 200, (B,), generator=g), torch.randint(50, H - 50, (B,), generator=g)], 1).int().to(dev)
    zc = (1.0 + 0.002 * torch.randn(B, generator=g)).to(dev)
    nrm = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.05 * torch.randn(B, 3, generator=g), dim=1).to(dev).contiguous()
    wsum = torch.ones(B, device=dev)
    out_f, out_i, stats = WL.warp_loss(gray, valid, R_all, T_all, K, Kinv, nbr, frame, pix, zc, wsum, nrm, st, 0.5)
    torch.cuda.synchronize()
    counted, nvalid = int(stats[1]), float(out_i[:, 0].float().mean())
    rays, R, z, w, _, _ = kernel_inputs(B, n, dev)
    dw, dn = torch.empty(B, n, device=dev), torch.empty(B, 3, device=dev)
    sd = 2.0 / 64
    t, ws_, zz = WL.ray_depth(rays, R, z, w, sd)
    cnt = torch.randint(0, 129, (B,), generator=g)
    cnt[torch.rand(B, generator=g) < 0.01] = 1024
    off = (torch.cumsum(cnt, 0) - cnt).to(dev)
    N = int(cnt.sum())
    t_start = (1.5 + torch.rand(N, generator=g)).to(dev)
    wp = (torch.rand(N, generator=g) * 0.02).to(dev)
    dwp = torch.empty(N, device=dev)
    pk = (off, cnt.to(torch.int32).to(dev), 1024)
    tp, wsp, zp = WL.ray_depth(rays, R, t_start, wp, 1.0 / 256, packed=pk)
    variants = {
        "warp": lambda: WL.warp_loss(gray, valid, R_all, T_all, K, Kinv, nbr, frame, pix, zc, wsum, nrm, st, 0.5),
        "depth_dense": lambda: WL.ray_depth(rays, R, z, w, sd),
        "bwd_dense": lambda: WL.ray_depth_bwd(rays, R, z, t, ws_, out_f, stats, sd, 0.5, dw, dn),
        "depth_packed": lambda: WL.ray_depth(rays, R, t_start, wp, 1.0 / 256, packed=pk),
        "bwd_packed": lambda: WL.ray_depth_bwd(rays, R, t_start, tp, wsp, out_f, stats, 1.0 / 256, 0.5, dwp, dn, packed=pk),
    }
    tm = alternate(variants, args.reps, args.rounds, args.warmup)
    taps = counted * nvalid * (2 * st.patch + 1) ** 2
    line(f"dh_warp_loss {B} rays, P {st.patch}, 8 neighbours, {H} x {W} frames (3 launches, incl. the output allocation)", tm["warp"],
         rays_counted=counted, mean_valid_neighbours=round(nvalid, 2), taps=int(taps))
    line(f"dh_ray_depth dense {B} x {n}", tm["depth_dense"])
    line(f"dh_ray_depth_bwd dense {B} x {n}", tm["bwd_dense"])
    line(f"dh_ray_depth_packed {B} rays, {N} samples", tm["depth_packed"], samples=N)
    line(f"dh_ray_depth_bwd_packed {B} rays, {N} samples", tm["bwd_packed"], samples=N)


def bench_step(args, dev):
    import tempfile

    import torch
    from dynhor_amd.runner import Runner
    tmp = tempfile.mkdtemp(prefix="bench_warp_")
    for family, sampler in (("neus", None), ("hash", "occgrid")):
        conf = {"seq_name": "bench", "exp_name": family,
                "data_info": {"synthetic": {"n_frames": 16, "H": 256, "W": 256, "seed": 4321}},
                "train": {"batch_size": args.rays, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "warp_weight": 0.5,
                          "warp_min_views": 1},
                "model": {"family": family}}
        if sampler:
            conf["model"]["hash_renderer"] = {"sampler": sampler}
        r = Runner(conf=conf, device=dev, exp_root=tmp)

        def step(on):
            def fn():
                r.warp_weight = 0.5 if on else 0.0
                r.train_iteration()
            return fn
        t = alternate({"off": step(False), "on": step(True)}, args.step_reps, args.rounds, args.warmup)
        name = f"{family}{' ' + sampler if sampler else ''} training step, batch {args.rays}"
        line(name + ", term off", t["off"])
        line(name + ", term on", t["on"], rays_counted_last=int(r.renderer.last_warp_stats[1]))
        del r
        torch.cuda.empty_cache()


def bench_tables(args, dev):
    import torch
    from types import SimpleNamespace
    from dynhor_amd import warp_loss as WL
    F, H, W = args.table_frames, 1080, 1920
    g = torch.Generator(device=dev).manual_seed(3)
    rgb = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    label = torch.zeros(F, H, W, dtype=torch.int8, device=dev)
    label[:, 200:880, 400:1500] = 1
    ds = SimpleNamespace(rgb=rgb, label=label, n_images=F, K=torch.tensor([[1500.0, 0, W / 2], [0, 1500.0, H / 2], [0, 0, 1]], device=dev))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tb = WL.frames_for(ds, range(F))
    torch.cuda.synchronize()
    print(json.dumps({"bench": "warp_loss", "name": f"frames_for, {F} frames of {H} x {W} (once)", "seconds": round(time.perf_counter() - t0, 3),
                      "resident_bytes": int(tb.gray.numel() + tb.valid.numel())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--step_reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--table_frames", type=int, default=300)
    ap.add_argument("--only", choices=("kernel", "step", "tables"), default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    if args.only in (None, "kernel"):
        bench_kernel(args, dev)
    if args.only in (None, "step"):
        bench_step(args, dev)
    if args.only in (None, "tables"):
        bench_tables(args, dev)


if __name__ == "__main__":
    main()
