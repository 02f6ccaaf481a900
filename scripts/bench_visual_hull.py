"""Timing of the visual hull (dynhor_amd/visual_hull.py) over 300 frames of 1080 x 1920 (labels made of discs with a hand blob:
bench_mesh_clean.sequence), in chunks of 16 frames as hull_field issues them: the three distance transforms (dh_label_edt), the
signed map formed from them (torch elementwise ops), the carving (dh_hull_accumulate, m = 2) of a 128^3 and a 256^3 grid over
[-0.6, 0.6]^3, and the whole of visual_hull() with bound "auto".  The carving is timed with the points in plain grid order and in
4 x 4 x 4-brick order (a wave's 64 points form one brick, whose projections cover a compact patch of pixels), in alternating runs
inside one process.  One JSON line per measurement.  Kernel times proper come from a profiler run:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d <out> -o vhull -- python scripts/bench_visual_hull.py
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def brick_order(pts, N, b=4):
    """The N^3 grid points (x-major) reordered so that every b^3 brick is contiguous."""
    n = N // b
    return pts.view(n, b, n, b, n, b, 3).permute(0, 2, 4, 1, 3, 5, 6).reshape(-1, 3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--resolutions", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--band_px", type=float, default=16)
    ap.add_argument("--rounds", type=int, default=3, help="alternating (grid order, brick order) runs of the carving")
    ap.add_argument("--whole", type=int, default=1, help="also time visual_hull() as a whole (0: skip)")
    args = ap.parse_args()
    import math
    import torch
    from bench_mesh_clean import _timed, sequence
    from dynhor_amd.pose_sil import label_edt
    from dynhor_amd.visual_hull import grid_points, hull_accumulate, signed_label_distance, visual_hull
    assert torch.cuda.is_available(), "bench_visual_hull needs a GPU"
    dev = torch.device("cuda:0")
    label, R, T, K = sequence(args.frames, args.H, args.W, dev)
    F, C = args.frames, args.chunk
    rmax = int(math.ceil(args.band_px)) + 1

    def edt_all():
        for f0 in range(0, F, C):
            for value in (1, -1, 0):
                label_edt(label[f0:f0 + C], value, rmax)

    def signed_all():
        for f0 in range(0, F, C):
            signed_label_distance(label[f0:f0 + C], args.band_px)

    s_edt = _timed(edt_all, 1, dev)
    s_signed = _timed(signed_all, 1, dev)
    print(json.dumps({"bench": "visual_hull_signed_map", "frames": F, "chunk": C, "H": args.H, "W": args.W, "band_px": args.band_px,
                      "rmax": rmax, "label_edt_s": s_edt, "elementwise_s": s_signed - s_edt, "signed_map_s": s_signed}), flush=True)

    sd = [signed_label_distance(label[f0:f0 + C], args.band_px) for f0 in range(0, F, C)]       # 4 bytes per pixel: 2.5 GB at the defaults
    for N in args.resolutions:
        pts = {"grid": grid_points([-0.6] * 3, [0.6] * 3, N, dev)[0]}
        if N % 4 == 0:
            pts["brick"] = brick_order(pts["grid"], N)
        n = N ** 3
        state = (torch.empty(n, 2, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))

        def carve(p):
            state[0].fill_(float("-inf")); state[1].fill_(-1); state[2].zero_()
            for k, f0 in enumerate(range(0, F, C)):
                hull_accumulate(p, sd[k], R[f0:f0 + C], T[f0:f0 + C], K, f0, *state)

        times = {k: [] for k in pts}
        inside = {}
        for _ in range(args.rounds):
            for k, p in pts.items():
                times[k].append(_timed(lambda: carve(p), 1, dev))
                inside[k] = int((state[0][:, 0] <= 0).sum())
        assert len(set(inside.values())) == 1, inside                       # the order of the points changes nothing
        row = {"bench": "visual_hull_accumulate", "resolution": N, "points": n, "frames": F, "chunk": C, "m": 2, "pairs": n * F,
               "inside": inside["grid"]}
        for k, v in times.items():
            row[k + "_s"] = sorted(v)
            row[k + "_median_s"] = sorted(v)[len(v) // 2]
            row[k + "_pairs_per_s"] = n * F / sorted(v)[len(v) // 2]
        print(json.dumps(row), flush=True)
        del pts, state
    del sd
    torch.cuda.empty_cache()

    if args.whole:
        ds = SimpleNamespace(label=label, R=R, T=T, K=K, n_images=F, H=args.H, W=args.W, stems=None)
        for N in args.resolutions:
            visual_hull(ds, resolution=min(N, 64), frame_chunk=C, band_px=args.band_px)           # warm-up
            timer = {}
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            v, f, st = visual_hull(ds, resolution=N, frame_chunk=C, band_px=args.band_px, timer=timer)
            torch.cuda.synchronize(dev)
            print(json.dumps({"bench": "visual_hull", "resolution": N, "frames": F, "H": args.H, "W": args.W, "seconds": time.perf_counter() - t0,
                              "phases": timer, "verts": st["verts"], "faces": st["faces"], "cell": st["cell"], "volume": st["volume"],
                              "touches_bound": st["touches_bound"], "sole_carved_max": st["sole_carved"]["share_max"]}), flush=True)


if __name__ == "__main__":
    main()
