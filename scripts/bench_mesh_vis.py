"""Timing of the mesh overlay (dynhor_amd/mesh_vis.py): the shade kernel (dh_mesh_shade, with frames and labels, alpha 0.6) over one
frame chunk (16 frames, the default of overlay_frames) of 1080 x 1920 for the analytic scene's mesh at marching-cubes resolution 512
and 1024, over 300 such frames for a ~10^6-vertex mesh in one launch, and one full Runner.visualize_mesh split into its GPU part
(overlay_frames without writing) and the rest (JPEG encoding and writing, the turntable).  One JSON line per measurement.  Kernel
times proper come from a profiler run:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d <out> -o mvis -- python scripts/bench_mesh_vis.py

The shade streams 15 bytes per pixel (z-buffer 8, frame 3, label 1, output 3) and gathers face and vertex data for covered pixels
only; bytes_per_s below is those 15 bytes per pixel over the measured time."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--big_resolution", type=int, default=816, help="marching-cubes resolution of the ~10^6-vertex mesh")
    ap.add_argument("--resolutions", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runner_frames", type=int, default=64, help="synthetic frames (512 x 512) of the Runner.visualize_mesh run")
    args = ap.parse_args()
    import torch
    from bench_mesh_clean import _timed, scene_mesh, sequence
    from dynhor_amd.mesh_color import raster_depth, vertex_normals
    from dynhor_amd.mesh_vis import shade
    assert torch.cuda.is_available(), "bench_mesh_vis needs a GPU"
    dev = torch.device("cuda:0")

    label, R, T, K = sequence(args.frames, args.H, args.W, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rgb = torch.randint(0, 256, (args.frames, args.H, args.W, 3), dtype=torch.uint8, device=dev, generator=g)

    def run(verts, faces, F):
        Rc, Tc = R[:F].contiguous(), T[:F].contiguous()
        normals = vertex_normals(verts, faces)
        zbuf = raster_depth(verts, faces, Rc, Tc, K, args.H, args.W)
        s = _timed(lambda: shade(verts, faces, zbuf, Rc, Tc, K, normals=normals, rgb=rgb[:F], label=label[:F], alpha=0.6), args.reps,
                   dev)
        covered = int((zbuf != -1).sum())
        del zbuf
        return s, covered

    for N in args.resolutions:
        mv, mf = scene_mesh(N, dev)
        s, covered = run(mv, mf, args.chunk)
        px = args.chunk * args.H * args.W
        print(json.dumps({"bench": "mesh_vis", "mesh": f"scene@{N}", "verts": mv.shape[0], "faces": mf.shape[0], "frames": args.chunk,
                          "H": args.H, "W": args.W, "shade_s": s, "covered_px": covered, "bytes_per_s": 15 * px / s}), flush=True)
        del mv, mf
    mv, mf = scene_mesh(args.big_resolution, dev)
    s, covered = run(mv, mf, args.frames)
    px = args.frames * args.H * args.W
    print(json.dumps({"bench": "mesh_vis", "mesh": f"scene@{args.big_resolution}", "verts": mv.shape[0], "faces": mf.shape[0],
                      "frames": args.frames, "H": args.H, "W": args.W, "shade_s": s, "covered_px": covered,
                      "bytes_per_s": 15 * px / s}), flush=True)
    del mv, mf, rgb, label
    torch.cuda.empty_cache()

    # one whole Runner.visualize_mesh of the scene mesh on the synthetic sequence
    from dynhor_amd.mesh import write_ply
    from dynhor_amd.mesh_vis import overlay_frames
    from dynhor_amd.runner import Runner
    with tempfile.TemporaryDirectory() as tmp:
        conf = {"seq_name": "bench_mvis", "exp_name": "vis",
                "data_info": {"synthetic": {"n_frames": args.runner_frames, "H": 512, "W": 512, "seed": 4321}}}
        r = Runner(conf=conf, device="cuda:0", exp_root=tmp)
        v, f = r._scene_gt_mesh(512)
        ply = os.path.join(tmp, "scene.ply")
        write_ply(ply, v, f)
        vd, fd = v.contiguous(), f.contiguous()
        overlay_frames(vd, fd, r.dataset)                      # warm-up
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        overlay_frames(vd, fd, r.dataset)
        torch.cuda.synchronize(dev)
        t_gpu = time.perf_counter() - t0
        t0 = time.perf_counter()
        res = r.visualize_mesh(mesh=ply, turntable=36)
        torch.cuda.synchronize(dev)
        t_all = time.perf_counter() - t0
        r.close()
        print(json.dumps({"bench": "mesh_vis_runner", "frames": args.runner_frames, "H": 512, "W": 512, "verts": v.shape[0],
                          "overlay_gpu_s": t_gpu, "visualize_mesh_s": t_all, "host_s": t_all - t_gpu, "turntable": 36,
                          "iou_mean": res["iou_mean"]}), flush=True)


if __name__ == "__main__":
    main()
