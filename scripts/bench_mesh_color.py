"""Timing of the mesh colouring kernels (dynhor_amd/mesh_color.py): the z-buffer (dh_mesh_raster_depth) and the colour gather
(dh_mesh_bake_colors) for the analytic scene's mesh at marching-cubes resolution 512 and 1024 over one frame chunk (16 frames, the
default of bake_vertex_colors), and for a ~10^6-vertex mesh over 300 frames of 1080 x 1920 in one launch each (poses, labels, images
and meshes made on the device).  One JSON line per measurement.  Kernel times proper come from a profiler run:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d <out> -o mcol -- python scripts/bench_mesh_color.py

The raster's work: per (frame, face) pair one projection of three vertices, then per covered pixel centre one 64-bit atomic minimum;
the bake's: per (vertex, frame) pair one projection and a gather of 1 + 8 (+ 3 when it contributes) bytes."""
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
    ap.add_argument("--big_resolution", type=int, default=816, help="marching-cubes resolution of the ~10^6-vertex mesh")
    ap.add_argument("--resolutions", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from bench_mesh_clean import _timed, scene_mesh, sequence
    from dynhor_amd import _lib
    from dynhor_amd.mesh_color import raster_depth, usable_map, vertex_normals
    assert torch.cuda.is_available(), "bench_mesh_color needs a GPU"
    dev = torch.device("cuda:0")

    label, R, T, K = sequence(args.frames, args.H, args.W, dev)
    usable = usable_map(label, 1)
    del label
    g = torch.Generator(device=dev).manual_seed(0)
    rgb = torch.randint(0, 256, (args.frames, args.H, args.W, 3), dtype=torch.uint8, device=dev, generator=g)

    def run(verts, faces, F):
        Rc, Tc = R[:F].contiguous(), T[:F].contiguous()
        normals = vertex_normals(verts, faces)
        zbuf = [None]

        def raster():
            zbuf[0] = None
            zbuf[0] = raster_depth(verts, faces, Rc, Tc, K, args.H, args.W)

        s_r = _timed(raster, args.reps, dev)
        nv = verts.shape[0]
        acc = torch.zeros(nv, 4, device=dev)
        n_views = torch.zeros(nv, dtype=torch.int32, device=dev)

        def bake():
            _lib.check(_lib.lib().dh_mesh_bake_colors(_lib.ptr(verts), _lib.ptr(normals), nv, _lib.ptr(rgb[:F]), _lib.ptr(usable[:F]),
                                                      _lib.ptr(zbuf[0]), _lib.ptr(Rc), _lib.ptr(Tc), _lib.ptr(K), F, args.H, args.W,
                                                      0.01, 0.1, _lib.ptr(acc), _lib.ptr(n_views), _lib.stream()))

        s_b = _timed(bake, args.reps, dev)
        covered = int((zbuf[0] != -1).sum())
        n_views.zero_()
        bake()
        return s_r, s_b, covered, float(n_views.double().mean())

    for N in args.resolutions:
        mv, mf = scene_mesh(N, dev)
        s_r, s_b, covered, mean_views = run(mv, mf, args.chunk)
        print(json.dumps({"bench": "mesh_color", "mesh": f"scene@{N}", "verts": mv.shape[0], "faces": mf.shape[0], "frames": args.chunk,
                          "H": args.H, "W": args.W, "raster_s": s_r, "bake_s": s_b, "covered_px": covered, "mean_views": mean_views}),
              flush=True)
        del mv, mf
    mv, mf = scene_mesh(args.big_resolution, dev)
    s_r, s_b, covered, mean_views = run(mv, mf, args.frames)
    print(json.dumps({"bench": "mesh_color", "mesh": f"scene@{args.big_resolution}", "verts": mv.shape[0], "faces": mf.shape[0],
                      "frames": args.frames, "H": args.H, "W": args.W, "raster_s": s_r, "bake_s": s_b, "covered_px": covered,
                      "mean_views": mean_views, "bake_pairs_per_s": mv.shape[0] * args.frames / s_b}), flush=True)


if __name__ == "__main__":
    main()
