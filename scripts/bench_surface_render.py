"""Frames of the synthetic sequence drawn by the sphere tracer (dynhor_amd/surface_render.py, csrc/trace.hip) and by the volume
renderer (Runner.render_image: the existing path and the yardstick -- the new path is not measured against itself), on the same
machine, alternating, median of --repeats:

    python scripts/bench_surface_render.py --size 512 --family neus --iters 300
    timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d <out> -o srender -- python scripts/bench_surface_render.py --size 512

One JSON line: frames per second end to end for `volume`, `surface` with compact_every 1 and 4, the tracer's queries per ray, rounds
and count reads, the time of one 4-byte device read times the reads as a share of a surface frame, and the PSNR between the two
methods' pictures over the object's pixels.  Kernel times of trace_init / trace_step / trace_compact / trace_scan / trace_compose come
from the profiler run (a run of its own: the script times nothing inside a kernel).  --iters trains the networks first (the PSNR
between the methods means something only on a trained surface; configs/synthetic.yaml's full training is --iters 20000)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=str, default="512", help="512 (512 x 512) or 1080 (1080 x 1920), or HxW")
    ap.add_argument("--family", type=str, default="neus", choices=["neus", "hash"])
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--volume_level", type=int, default=1, help="pixel stride of the volume yardstick (its fps is scaled to full frames)")
    args = ap.parse_args()
    import torch
    from dynhor_amd import surface_render as sr
    from dynhor_amd.runner import Runner
    assert torch.cuda.is_available(), "bench_surface_render needs a GPU"
    H, W = {"512": (512, 512), "1080": (1080, 1920)}.get(args.size) or tuple(int(v) for v in args.size.split("x"))
    conf = {"seq_name": "bench", "exp_name": "surface_render", "data_info": {"synthetic": {"n_frames": args.frames, "H": H, "W": W, "seed": 17}},
            "train": {"report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0}, "model": {"family": args.family}}
    with tempfile.TemporaryDirectory() as root:
        r = Runner(conf=conf, device="cuda:0", exp_root=root)
        for _ in range(args.iters):
            r.train_iteration()
        ds = r.dataset
        sync = torch.cuda.synchronize

        def surface(k, every):
            return sr.render_surface(r.renderer, ds.R[k:k + 1], ds.T[k:k + 1], ds.K, H, W, compact_every=every)

        def volume(k):
            return r.render_image(k, resolution_level=args.volume_level)[0]

        surface(0, 1); volume(0); sync()                                           # warm-up: workspaces, code objects
        times = {"volume": [], "surface_1": [], "surface_4": []}
        stats = None
        for rep in range(args.repeats):
            k = rep % args.frames
            for name, fn in (("volume", lambda: volume(k)), ("surface_1", lambda: surface(k, 1)), ("surface_4", lambda: surface(k, 4))):
                sync(); t0 = time.perf_counter()
                out = fn()
                sync(); times[name].append(time.perf_counter() - t0)
                if name == "surface_1":
                    stats = out["stats"]
        word = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        sync(); t0 = time.perf_counter()
        for _ in range(100):
            int(word.item())
        read_s = (time.perf_counter() - t0) / 100
        med = {k: statistics.median(v) for k, v in times.items()}
        scale = float(args.volume_level ** 2)
        img_v = volume(0)
        out_s = surface(0, 1)
        L = args.volume_level
        m = (ds.label[0, ::L, ::L] > 0)[..., None].float()
        a, b = out_s["rgb"][0, ::L, ::L].float() / 255.0, img_v.clamp(0, 1)
        mse = float((((a - b) ** 2) * m).sum() / (m.sum() * 3.0 + 1e-5))
        print(json.dumps({"bench": "surface_render", "family": args.family, "H": H, "W": W, "iters": args.iters, "repeats": args.repeats,
                          "volume_level": L, "fps_volume": 1.0 / (med["volume"] * scale), "fps_surface_compact1": 1.0 / med["surface_1"],
                          "fps_surface_compact4": 1.0 / med["surface_4"], "queries_per_ray": stats["queries_mean"],
                          "queries_max": stats["queries_max"], "rounds": stats["rounds"], "count_reads": stats["count_reads"],
                          "count_read_s": read_s, "count_read_share": read_s * stats["count_reads"] / med["surface_1"],
                          "scanned": stats["scanned"], "capped": stats["capped"], "hits": stats["hit"],
                          "psnr_surface_vs_volume_db": 10.0 * __import__("math").log10(1.0 / max(mse, 1e-12))}), flush=True)


if __name__ == "__main__":
    main()
