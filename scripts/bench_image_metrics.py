"""Time dh_ssim (csrc/image_metrics.hip) against its fp64 torch restatement on the same GPU, and its share of Runner.evaluate_views.

    python scripts/bench_image_metrics.py                       # 16 frames of 1080 x 1920, radius 5
    rocprofv3 --kernel-trace --stats -d prof_im -- python scripts/bench_image_metrics.py --no_share
        (alone, no counters in the run: ssim_kernel and sum64_reduce_kernel in the stats are one call's two kernels)

Random pictures (b = a plus noise) with a disc mask per frame, not zeros.  The kernel and the restatement (tests/image_metrics_util.py
ssim_torch: the same integer sums and fp64 operations as tensor expressions) alternate in one process, `--reps` times each after a
warm-up; the medians of the event times are reported, and the two must agree (map bit for bit, integer sums exactly).  The share is
taken on a synthetic run (--share_frames frames of --share_size^2, untrained networks: the sphere of the geometric initialisation is
what gets drawn): wall time inside image_metrics.ssim_frames over the wall time of evaluate_views, both with the device synchronised.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=1.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no_share", action="store_true")
    ap.add_argument("--share_frames", type=int, default=16)
    ap.add_argument("--share_size", type=int, default=512)
    args = ap.parse_args()

    import torch
    from dynhor_amd import image_metrics as im
    from tests import image_metrics_util as U
    dev = torch.device("cuda:0")
    F, H, W = args.frames, args.height, args.width
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    a = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    noise = torch.randint(-40, 41, (F, H, W, 3), dtype=torch.int16, device=dev, generator=g)
    b = (a.to(torch.int16) + noise).clamp(0, 255).to(torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    cy = torch.randint(H // 3, 2 * H // 3, (F, 1, 1), device=dev, generator=g)
    cx = torch.randint(W // 3, 2 * W // 3, (F, 1, 1), device=dev, generator=g)
    usable = (((yy - cy) ** 2 + (xx - cx) ** 2) < (min(H, W) // 3) ** 2).to(torch.uint8).contiguous()
    taps = im.gaussian_taps_q16(args.sigma, args.radius)
    w_min = im.weight_threshold(0.5)

    def kernel():
        return im.ssim_frames(a, b, usable, sigma=args.sigma, radius=args.radius, want_map=True, chunk=F)

    def restatement():
        return U.ssim_torch(a, b, usable, taps, w_min)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    _, k = timed(kernel)
    _, (rmap, rout) = timed(restatement)
    agree = bool(torch.equal(k["map"], rmap)) and bool(torch.equal(k["sums"][:, 1:5], rout[:, 1:5].cpu()))
    tk, tr = [], []
    for _ in range(args.reps):
        tk.append(timed(kernel)[0])
        tr.append(timed(restatement)[0])
    res = {"frames": F, "height": H, "width": W, "radius": args.radius, "usable_share": float(usable.float().mean()),
           "agree": agree, "kernel_ms_per_frame": statistics.median(tk) / F, "restatement_ms_per_frame": statistics.median(tr) / F,
           "kernel_ms_all": sorted(tk), "restatement_ms_all": sorted(tr)}
    res["ratio"] = res["restatement_ms_per_frame"] / res["kernel_ms_per_frame"]
    del rmap, rout, k

    if not args.no_share:
        import tempfile
        from dynhor_amd.runner import Runner
        conf = {"seq_name": "bench", "exp_name": "im", "model": {"family": "neus"},
                "data_info": {"synthetic": {"n_frames": args.share_frames, "H": args.share_size, "W": args.share_size, "seed": 17}}}
        with tempfile.TemporaryDirectory() as tmp:
            r = Runner(conf=conf, device=str(dev), exp_root=tmp)
            spent = [0.0]
            inner = im.ssim_frames

            def wrapped(*a_, **k_):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = inner(*a_, **k_)
                torch.cuda.synchronize()
                spent[0] += time.perf_counter() - t0
                return out

            im.ssim_frames = wrapped
            try:
                r.evaluate_views(frames="all", save=False)          # warm-up
                spent[0] = 0.0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r.evaluate_views(frames="all", save=False)
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
            finally:
                im.ssim_frames = inner
        res.update(share_frames=args.share_frames, share_size=args.share_size, evaluate_views_s=total, metric_s=spent[0],
                   metric_share=spent[0] / total)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
