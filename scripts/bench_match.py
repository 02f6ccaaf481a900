"""Timing of the dense frame matcher (dynhor_amd/match.py): 16 frames of 1080 x 1920 smooth-noisy input (every pixel usable), grey
frames (dh_image_blur + dh_match_gray), query selection, and the forward search of every pair i -> i + 1 at P 4, R 16 with 4,096
queries per pair and the guess moved off the truth by a few pixels (dh_match_search; the frames are shifted copies of one picture, so
the search finds something).  One JSON line.  Kernel times proper come from a profiler run of its own:

    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <out> -o match -- python scripts/bench_match.py

To compare v_dot4_u32_u8 against plain integer multiply-adds build csrc/match.hip with -DDH_MATCH_NO_DOT4 and run this again on the
same machine.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--patch", type=int, default=4)
    ap.add_argument("--range", type=int, default=16)
    ap.add_argument("--per_pair", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from bench_mesh_clean import _timed
    from mesh_texture_util import smooth_noisy_frames
    from dynhor_amd.match import gray_frames, search, select_queries, usable_sources
    assert torch.cuda.is_available(), "bench_match needs a GPU"
    dev = torch.device("cuda:0")
    F, H, W = args.frames, args.H, args.W
    base = smooth_noisy_frames(1, H + 4 * F, W + 4 * F, seed=0, device=dev)[0]
    rgb = torch.stack([base[3 * f:3 * f + H, 2 * f:2 * f + W] for f in range(F)]).contiguous()     # frame f + 1 = frame f moved by (-2, -3)
    usable = torch.ones(F, H, W, dtype=torch.uint8, device=dev)
    s_gray = _timed(lambda: gray_frames(rgb, usable, 1.0, 0.5), args.reps, dev)
    gray, valid = gray_frames(rgb, usable, 1.0, 0.5)
    src = usable_sources(gray, valid, args.patch)
    pix, steps = select_queries(src, 1, args.per_pair)
    keep = pix[:, 0] < F - 1
    p = pix[keep].long()
    g = torch.Generator(device=dev).manual_seed(1)
    off = torch.randint(-5, 6, (p.shape[0], 2), device=dev, generator=g)
    q = torch.stack([p[:, 0], p[:, 0] + 1, p[:, 1], p[:, 2], p[:, 1] - 2 + off[:, 0], p[:, 2] - 3 + off[:, 1]], 1).to(torch.int32).contiguous()
    s_search = _timed(lambda: search(gray, valid, q, args.patch, args.range), args.reps, dev)
    oi, of = search(gray, valid, q, args.patch, args.range)
    found = ((oi[:, 0] == q[:, 2] - 2) & (oi[:, 1] == q[:, 3] - 3) & (oi[:, 2] == 0)).float().mean()
    cand = (2 * args.range + 1) ** 2
    prod = q.shape[0] * cand * (2 * args.patch + 1) ** 2
    print(json.dumps({"bench": "match", "frames": F, "H": H, "W": W, "patch": args.patch, "range": args.range, "queries": int(q.shape[0]),
                      "steps": steps, "gray_s": s_gray, "search_s": s_search, "search_us_per_query": 1e6 * s_search / max(1, q.shape[0]),
                      "byte_products": prod, "byte_products_per_s": prod / s_search, "found_share": float(found),
                      "mean_s1": float(of[:, 0].mean())}), flush=True)


if __name__ == "__main__":
    main()
