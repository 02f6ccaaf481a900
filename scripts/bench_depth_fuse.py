"""Timing of the depth fusion's kernel (dynhor_amd/depth_fuse.py: dh_tsdf_integrate) over 300 frames on orbit poses
(bench_mesh_clean.sequence) with analytic depth maps of a sphere of radius 0.35, of 270 x 480 (1080p at mvs step_px 4) and of 1080 x
1920, in chunks of 16 frames as fuse_field issues them, against a 128^3 and a 256^3 grid over [-0.6, 0.6]^3 at trunc = 4 cells.  The
points go in plain grid order and in 4 x 4 x 4-brick order (visual_hull.brick_points), in alternating runs inside one process; every
time is taken with device events around the whole set of calls, and the median of --rounds runs is reported with the pairs (point x
frame) per second.  The same rule in float32 torch ops is timed on a subset (--torch_frames frames against 64^3 points) and its state
compared.  One JSON line per measurement.  Kernel times proper come from a profiler run:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d <out> -o fuse -- python scripts/bench_depth_fuse.py
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

RADIUS = 0.35


def sphere_depth(R, T, K, H, W, chunk=16):
    """(depth f32 [F,H,W] camera z of the sphere of RADIUS about the origin, inf where the ray misses; weight u8: 255 max(0, cos) of the
    hit, at least 1, 0 without one), formed on the device."""
    import torch
    dev = R.device
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    e = torch.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], torch.ones_like(xs)], -1)       # camera rays with z = 1
    depth = torch.empty(R.shape[0], H, W, device=dev)
    weight = torch.empty(R.shape[0], H, W, dtype=torch.uint8, device=dev)
    for f in range(R.shape[0]):
        c = T[f]                                                     # the origin in the camera frame
        a = (e * e).sum(-1)
        b = (e * c).sum(-1)
        disc = b * b - a * ((c * c).sum() - RADIUS * RADIUS)
        t = (b - disc.clamp_min(0).sqrt()) / a
        hit = (disc > 0) & (t > 0)
        depth[f] = torch.where(hit, t, torch.full_like(t, float("inf")))
        nrm = (t[..., None] * e - c) / RADIUS
        cos = (-(nrm * e).sum(-1) / a.sqrt()).clamp(0, 1)
        weight[f] = torch.where(hit, (255.0 * cos + 0.5).floor().clamp(1, 255), torch.zeros_like(cos)).to(torch.uint8)
    return depth, weight


def torch_integrate(pts, depth, weight, R, T, K, trunc):
    """(num int64 [n], den int64 [n], obs int64 [n]) of dh_tsdf_integrate's rule in float32 torch ops (no fma: the last bit of a
    projection may differ)."""
    import torch
    F, H, W = depth.shape
    c = torch.einsum("frc,nc->fnr", R, pts) + T[:, None, :]
    z = c[..., 2]
    u = (K[0, 0] * c[..., 0] + K[0, 1] * c[..., 1] + K[0, 2] * z) / z
    w = (K[1, 0] * c[..., 0] + K[1, 1] * c[..., 1] + K[1, 2] * z) / z
    xf, yf = torch.floor(u + 0.5), torch.floor(w + 0.5)
    inside = (z > 1e-3) & (xf >= 0) & (xf <= W - 1) & (yf >= 0) & (yf <= H - 1)
    x = torch.where(inside, xf, torch.zeros_like(xf)).long()
    y = torch.where(inside, yf, torch.zeros_like(yf)).long()
    at = torch.arange(F, device=pts.device)[:, None] * (H * W) + y * W + x
    zd, wt = depth.reshape(-1)[at], weight.reshape(-1)[at].long()
    d = zd - z
    ok = inside & (wt != 0) & torch.isfinite(zd) & (zd > 1e-3) & ~(d < -trunc)
    q = torch.round(torch.clamp_max(torch.where(ok, d, torch.zeros_like(d)) / trunc, 1.0) * 65536.0).long()
    wt = torch.where(ok, wt, torch.zeros_like(wt))
    return (wt * q).sum(0), wt.sum(0), ok.long().sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--sizes", type=str, nargs="*", default=["270x480", "1080x1920"])
    ap.add_argument("--resolutions", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--rounds", type=int, default=3, help="alternating (grid order, brick order) runs, at least 3")
    ap.add_argument("--torch_frames", type=int, default=16, help="frames of the float32 torch comparison against 64^3 points (0: skip)")
    args = ap.parse_args()
    import torch
    from bench_mesh_clean import _timed, sequence
    from dynhor_amd.depth_fuse import integrate
    from dynhor_amd.visual_hull import brick_points, grid_points
    assert torch.cuda.is_available(), "bench_depth_fuse needs a GPU"
    assert args.rounds >= 3
    dev = torch.device("cuda:0")
    F, C = args.frames, args.chunk
    lo, hi = [-0.6] * 3, [0.6] * 3
    for size in args.sizes:
        H, W = (int(v) for v in size.split("x"))
        _, R, T, K = sequence(F, H, W, dev)
        depth, weight = sphere_depth(R, T, K, H, W)
        for N in args.resolutions:
            trunc = 4 * 1.2 / (N - 1)
            pts = {"grid": grid_points(lo, hi, N, dev)[0]}
            brick, grid_order = brick_points(lo, hi, N, dev)
            pts["brick"] = brick
            state = {k: (torch.empty(p.shape[0], dtype=torch.int64, device=dev), torch.empty(p.shape[0], dtype=torch.int32, device=dev),
                         torch.empty(p.shape[0], dtype=torch.int32, device=dev)) for k, p in pts.items()}

            def run(k):
                for s in state[k]:
                    s.zero_()
                for f0 in range(0, F, C):
                    integrate(pts[k], depth[f0:f0 + C], weight[f0:f0 + C], R[f0:f0 + C], T[f0:f0 + C], K, trunc, *state[k])

            times = {k: [] for k in pts}
            for _ in range(args.rounds):
                for k in pts:
                    times[k].append(_timed(lambda: run(k), 1, dev))
            same = all(torch.equal(a, grid_order(b)) for a, b in zip(state["grid"], state["brick"]))
            assert same, "the order of the points changed a result"
            n = N ** 3
            row = {"bench": "depth_fuse_integrate", "H": H, "W": W, "resolution": N, "points": n, "brick_points": int(brick.shape[0]),
                   "frames": F, "chunk": C, "trunc": trunc, "pairs": n * F, "observed": int((state["grid"][1] > 0).sum()),
                   "bytes_maps": 5 * F * H * W}
            for k, v in times.items():
                med = sorted(v)[len(v) // 2]
                row[k + "_s"] = sorted(v)
                row[k + "_median_s"] = med
                row[k + "_pairs_per_s"] = pts[k].shape[0] * F / med
            row["brick_speedup"] = row["grid_median_s"] / row["brick_median_s"]
            print(json.dumps(row), flush=True)
            del pts, state, brick
        if args.torch_frames > 0:
            Ft, N = min(args.torch_frames, F), 64
            trunc = 4 * 1.2 / (N - 1)
            p = brick_points(lo, hi, N, dev)[0]
            st = (torch.zeros(p.shape[0], dtype=torch.int64, device=dev), torch.zeros(p.shape[0], dtype=torch.int32, device=dev),
                  torch.zeros(p.shape[0], dtype=torch.int32, device=dev))

            def hip():
                for s in st:
                    s.zero_()
                integrate(p, depth[:Ft], weight[:Ft], R[:Ft], T[:Ft], K, trunc, *st)

            ref = []

            def eager():
                ref[:] = torch_integrate(p, depth[:Ft], weight[:Ft], R[:Ft], T[:Ft], K, trunc)

            th = sorted(_timed(hip, 1, dev) for _ in range(args.rounds))
            tt = sorted(_timed(eager, 1, dev) for _ in range(args.rounds))
            differ = int(((st[1].long() != ref[1]) | (st[2].long() != ref[2])).sum())
            dq = int((st[0] - ref[0])[(st[1].long() == ref[1]) & (st[2].long() == ref[2])].abs().max())
            print(json.dumps({"bench": "depth_fuse_vs_torch_f32", "H": H, "W": W, "resolution": N, "points": int(p.shape[0]), "frames": Ft,
                              "pairs": int(p.shape[0]) * Ft, "hip_s": th, "torch_s": tt, "hip_median_s": th[len(th) // 2],
                              "torch_median_s": tt[len(tt) // 2], "speedup": tt[len(tt) // 2] / th[len(th) // 2],
                              "points_with_another_verdict": differ, "max_abs_num_difference_elsewhere": dq}), flush=True)
        del depth, weight
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
