"""Timing of the photometric pose term (dynhor_amd/pose_photo.py): the masked Gaussian of the frames (dh_image_blur, once per blur level)
and the loss / gradient reduction (dh_photo_loss_grad, with the z-buffer it reads: dh_mesh_raster_depth) over 300 frames of 1080 x 1920
for 20,000 coloured points of the analytic scene's mesh at marching-cubes resolution 128, at blur sigma 4 (radius 12) and 0, in chunks
of 16 frames as SilhouettePoseOptimizer issues them.  One JSON line per measurement.  Kernel times proper come from a profiler run of
its own:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d <out> -o pphoto -- python scripts/bench_pose_photo.py
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--sigmas", type=float, nargs="*", default=[4.0, 0.0])
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    from bench_mesh_clean import _timed, scene_mesh, sequence
    from dynhor_amd.mesh_color import raster_depth, usable_map
    from dynhor_amd.pose_photo import blur_frames, photo_sums, surface_points
    assert torch.cuda.is_available(), "bench_pose_photo needs a GPU"
    dev = torch.device("cuda:0")
    label, R, T, K = sequence(args.frames, args.H, args.W, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rgb = torch.randint(0, 256, (args.frames, args.H, args.W, 3), dtype=torch.uint8, device=dev, generator=g)
    mv, mf = scene_mesh(args.resolution, dev)
    mv, mf = mv.float().contiguous(), mf.long().contiguous()
    pts, nrm, col = surface_points(mv, mf, args.points, 0, vertex_colors=torch.rand(mv.shape[0], 3, device=dev, generator=g))
    chunks = [(f0, min(args.frames, f0 + args.chunk)) for f0 in range(0, args.frames, args.chunk)]
    usable = [usable_map(label[f0:f1].contiguous(), 1) for f0, f1 in chunks]
    for sigma in args.sigmas:
        def blur_all():
            for (f0, f1), us in zip(chunks, usable):
                blur_frames(rgb[f0:f1], us, sigma)

        def raster_all():
            for f0, f1 in chunks:
                raster_depth(mv, mf, R[f0:f1].contiguous(), T[f0:f1].contiguous(), K, args.H, args.W)

        def loss_all():
            # the blurred frames of all 300 frames do not fit next to each other: one chunk's image stands in for every chunk's
            for f0, f1 in chunks:
                Rc, Tc = R[f0:f1].contiguous(), T[f0:f1].contiguous()
                zbuf = raster_depth(mv, mf, Rc, Tc, K, args.H, args.W)
                photo_sums(pts, nrm, col, img[:f1 - f0], zbuf, Rc, Tc, K)

        s_blur = _timed(blur_all, args.reps, dev)
        img = blur_frames(rgb[:args.chunk], usable[0], sigma)
        s_raster = _timed(raster_all, args.reps, dev)
        s_both = _timed(loss_all, args.reps, dev)
        pairs = photo_sums(pts, nrm, col, img, raster_depth(mv, mf, R[:args.chunk].contiguous(), T[:args.chunk].contiguous(), K, args.H,
                                                            args.W), R[:args.chunk].contiguous(), T[:args.chunk].contiguous(), K)[:, 14]
        print(json.dumps({"bench": "pose_photo", "mesh": f"scene@{args.resolution}", "faces": mf.shape[0], "points": args.points,
                          "frames": args.frames, "chunk": args.chunk, "H": args.H, "W": args.W, "sigma": sigma,
                          "blur_s": s_blur, "blur_ms_per_chunk": 1e3 * s_blur / len(chunks), "raster_s": s_raster,
                          "loss_grad_s": s_both - s_raster, "loss_grad_ms_per_chunk": 1e3 * (s_both - s_raster) / len(chunks),
                          "pairs_per_frame_first_chunk": float(pairs.mean())}), flush=True)
        del img


if __name__ == "__main__":
    main()
