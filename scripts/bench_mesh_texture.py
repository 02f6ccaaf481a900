"""Timing of the texture kernels (dynhor_amd/mesh_texture.py): the bake (dh_texture_bake) of the analytic scene's mesh, simplified to
5,000 and to 50,000 faces, over 300 frames of 1080 x 1920 in one launch on atlases of 1024, 2048 and 4096 texels per side, and the
textured shade (dh_mesh_shade_tex, with the error sums) over one frame chunk (poses, labels, images and meshes made on the device).
One JSON line per measurement.  Kernel times proper come from a profiler run of its own:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d <out> -o mtex -- python scripts/bench_mesh_texture.py

The bake's work: per (owned texel, frame) pair one projection, then for a pair that passes the tests up to there one usable byte, one
8-byte z-buffer key and, when the frame contributes, four 3-byte colour gathers.  `gather_bytes_per_s` is the byte rate of the work
estimate S^2 F (8 + 4 * 3) against the measured time: an upper bound of the rate achieved, since unowned texels, texels outside a
frame and hidden or back-facing ones stop before some or all of those loads (`contributions` counts the pairs that went all the way)."""
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
    ap.add_argument("--resolution", type=int, default=512, help="marching-cubes resolution of the mesh that is simplified")
    ap.add_argument("--faces", type=int, nargs="*", default=[5000, 50000])
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 2048, 4096])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from bench_mesh_clean import _timed, scene_mesh, sequence
    from dynhor_amd import _lib
    from dynhor_amd.mesh_color import raster_depth, usable_map, vertex_normals
    from dynhor_amd.mesh_simplify import simplify_by_mode
    from dynhor_amd.mesh_texture import atlas_capacity, face_atlas, render_textured
    assert torch.cuda.is_available(), "bench_mesh_texture needs a GPU"
    dev = torch.device("cuda:0")
    F, H, W = args.frames, args.H, args.W

    label, R, T, K = sequence(F, H, W, dev)
    usable = usable_map(label, 1)
    del label
    g = torch.Generator(device=dev).manual_seed(0)
    rgb = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    fine_v, fine_f = scene_mesh(args.resolution, dev)

    for target in args.faces:
        verts, faces, _ = simplify_by_mode(fine_v.float().contiguous(), fine_f.long().contiguous(), f"faces:{target}")
        nv, nf = verts.shape[0], faces.shape[0]
        normals = vertex_normals(verts, faces)
        zbuf = raster_depth(verts, faces, R, T, K, H, W)
        shaded = False
        for S in args.sizes:
            row = {"bench": "mesh_texture", "kernel": "dh_texture_bake", "faces": nf, "verts": nv, "size": S, "frames": F, "H": H, "W": W}
            if nf > atlas_capacity(S):
                print(json.dumps(dict(row, skipped=f"{nf} faces do not fit: at most {atlas_capacity(S)}")), flush=True)
                continue
            uv, owner, info = face_atlas(nf, S, device=dev)
            acc = torch.zeros(S, S, 4, device=dev)
            n_views = torch.zeros(S, S, dtype=torch.int32, device=dev)

            def bake():
                _lib.check(_lib.lib().dh_texture_bake(_lib.ptr(verts), _lib.ptr(normals), nv, _lib.ptr(faces), nf, _lib.ptr(uv),
                                                      _lib.ptr(owner), S, _lib.ptr(rgb), _lib.ptr(usable), _lib.ptr(zbuf), _lib.ptr(R),
                                                      _lib.ptr(T), _lib.ptr(K), F, H, W, 0.01, 0.1, 2, _lib.ptr(acc), _lib.ptr(n_views),
                                                      _lib.stream()))

            s = _timed(bake, args.reps, dev)
            n_views.zero_()
            bake()
            print(json.dumps(dict(row, cell=info["cell"], owned_frac=info["owned_frac"], bake_s=s, texel_frames_per_s=S * S * F / s,
                                  gather_bytes_per_s=S * S * F * 20 / s, contributions=int(n_views.long().sum()),
                                  unseen_texels=int(((owner >= 0) & (n_views == 0)).sum()))), flush=True)
            if not shaded:                                       # once per mesh, at the first atlas that holds it
                shaded = True
                n = min(args.chunk, F)
                tex = torch.randint(0, 256, (S, S, 3), dtype=torch.uint8, device=dev, generator=g)
                zc, Rc, Tc = zbuf[:n].contiguous(), R[:n].contiguous(), T[:n].contiguous()
                rc, uc = rgb[:n].contiguous(), usable[:n].contiguous()
                s2 = _timed(lambda: render_textured(verts, faces, zc, Rc, Tc, K, uv, tex, normals=normals, rgb=rc, usable=uc), args.reps, dev)
                print(json.dumps({"bench": "mesh_texture", "kernel": "dh_mesh_shade_tex", "faces": nf, "size": S, "frames": n, "H": H,
                                  "W": W, "shade_s": s2, "pixels_per_s": n * H * W / s2, "covered_px": int((zc != -1).sum())}), flush=True)
            del uv, owner, acc, n_views
        del zbuf


if __name__ == "__main__":
    main()
