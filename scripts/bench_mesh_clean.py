"""Timing of the mesh cleaning (dynhor_amd/mesh_clean.py): silhouette votes for 10^6 vertices x 300 frames of 1080 x 1920 labels and
the dilation of those labels (labels, poses and vertices made on the device), and the connected components of the analytic scene's
mesh at marching-cubes resolution 512 and 1024.  One JSON line per measurement.  Kernel times proper come from a profiler run:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d <out> -o mc -- python scripts/bench_mesh_clean.py

The vote kernel's work: one byte gathered and ~25 fp32 operations per (vertex, frame) pair, 3 x 10^8 pairs."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def scene_mesh(N, dev, chunk=1 << 22):
    import torch
    from dynhor_amd.mesh import marching_cubes
    from dynhor_amd.scene import scene_sdf
    ax = torch.linspace(-0.55, 0.55, N, device=dev)
    u = torch.empty(N * N * N, device=dev)
    for s in range(0, N * N * N, chunk):
        i = torch.arange(s, min(s + chunk, N * N * N), device=dev)
        p = torch.stack([ax[i // (N * N)], ax[(i // N) % N], ax[i % N]], dim=-1)
        u[s:s + i.shape[0]] = -scene_sdf(p)
    return marching_cubes(u.view(N, N, N), 0.0, [-0.55] * 3, [0.55] * 3)


def sequence(n_frames, H, W, dev):
    """Orbit poses as scene.make_sequence draws them, and label maps made on the device: the object's projected disc (1) with a hand
    ellipse (-1) on it, background 0."""
    import torch
    from dynhor_amd.scene import look_at_pose
    g = torch.Generator().manual_seed(0)
    f = 1.2 * min(H, W)
    K = torch.tensor([[f, 0, W // 2], [0, f, H // 2], [0, 0, 1]], dtype=torch.float32)
    Rs, Ts = [], []
    for i in range(n_frames):
        az = 2 * math.pi * (i + torch.rand(1, generator=g).item() * 0.5) / n_frames
        el = (torch.rand(1, generator=g).item() - 0.5) * 1.2
        pos = torch.tensor([2.2 * math.cos(el) * math.cos(az), 2.2 * math.cos(el) * math.sin(az), 2.2 * math.sin(el)])
        R, T = look_at_pose(pos)
        Rs.append(R); Ts.append(T)
    R, T = torch.stack(Rs).float().to(dev), torch.stack(Ts).float().to(dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing="ij")
    label = torch.zeros(n_frames, H, W, dtype=torch.int8, device=dev)
    rad = 0.35 * f / 2.2
    for i in range(n_frames):
        obj = (xs - W // 2) ** 2 + (ys - H // 2) ** 2 < rad ** 2
        hand = ((xs - W // 2 - 0.6 * rad) / (0.5 * rad)) ** 2 + ((ys - H // 2) / (0.25 * rad)) ** 2 < 1.0
        label[i] = torch.where(hand, -1, obj.to(torch.int8))
    return label, R, T, K.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--verts", type=int, default=10 ** 6)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--resolutions", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from dynhor_amd.mesh_clean import dilate_labels, mask_votes, vertex_components
    assert torch.cuda.is_available(), "bench_mesh_clean needs a GPU"
    dev = torch.device("cuda:0")

    label, R, T, K = sequence(args.frames, args.H, args.W, dev)
    s = _timed(lambda: dilate_labels(label, args.radius), args.reps, dev)
    print(json.dumps({"bench": "dilate_labels", "frames": args.frames, "H": args.H, "W": args.W, "radius": args.radius,
                      "s_per_call": s, "GB_per_s": 2 * 2 * label.numel() / s / 1e9}), flush=True)
    keep = dilate_labels(label, args.radius)
    # vertices in marching-cubes order (the order the votes see in use): the scene's mesh, cut or repeated to --verts
    v, _ = scene_mesh(384, dev)
    verts = v.repeat((args.verts + v.shape[0] - 1) // v.shape[0], 1)[:args.verts].contiguous()
    s = _timed(lambda: mask_votes(verts, keep, R, T, K), args.reps, dev)
    bg, seen = mask_votes(verts, keep, R, T, K)
    print(json.dumps({"bench": "mask_votes", "verts": args.verts, "frames": args.frames, "H": args.H, "W": args.W, "s_per_call": s,
                      "pairs_per_s": args.verts * args.frames / s, "mean_seen": float(seen.double().mean()),
                      "mean_bg_votes": float(bg.double().mean())}), flush=True)
    del keep, label
    for N in args.resolutions:
        mv, mf = scene_mesh(N, dev)
        s = _timed(lambda: vertex_components(mv.shape[0], mf), args.reps, dev)
        lab = vertex_components(mv.shape[0], mf)
        print(json.dumps({"bench": "vertex_components", "resolution": N, "verts": mv.shape[0], "faces": mf.shape[0], "s_per_call": s,
                          "components": int((lab == torch.arange(mv.shape[0], device=dev, dtype=torch.int32)).sum())}), flush=True)
        del mv, mf, lab


if __name__ == "__main__":
    main()
