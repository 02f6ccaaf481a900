"""Timing of the dense frame matcher (dynhor_amd/match.py): 16 frames of 1080 x 1920 smooth-noisy input (every pixel usable), grey
frames (dh_image_blur + dh_match_gray), query selection, and the forward search of every pair i -> i + 1 at P 4, R 16 with 4,096
queries per pair and the guess moved off the truth by a few pixels (dh_match_search; the frames are shifted copies of one picture, so
the search finds something).  A second arm ("warp") alternates dh_match_search and dh_match_search_warp on the same queries in this
process, with a random affine map within warp_max per query and with the identity.  One JSON line.  Kernel times proper come from a profiler run of its own:

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
    ap.add_argument("--warp_rounds", type=int, default=7, help="rounds of the arm that alternates search and search_warp (0: skip it)")
    ap.add_argument("--warp_max", type=float, default=3.0)
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
    out = {"bench": "match", "frames": F, "H": H, "W": W, "patch": args.patch, "range": args.range, "queries": int(q.shape[0]),
           "steps": steps, "gray_s": s_gray, "search_s": s_search, "search_us_per_query": 1e6 * s_search / max(1, q.shape[0]),
           "byte_products": prod, "byte_products_per_s": prod / s_search, "found_share": float(found), "mean_s1": float(of[:, 0].mean())}
    if args.warp_rounds > 0:
        out["warp"] = warp_arm(gray, valid, q, args, dev)
    print(json.dumps(out), flush=True)


def warp_arm(gray, valid, q, args, dev):
    """dh_match_search and dh_match_search_warp on the same queries, alternating in this process (plain, warp, plain, warp, ...), the
    warp with a random map per query: rotation over the circle, both singular values within [1 / warp_max, warp_max].  Per arm the
    median and the spread of the rounds; the identity map as a third arm (the cost of the staging alone, same memory footprint)."""
    import statistics
    import torch
    from dynhor_amd.match import search, search_warp
    n = q.shape[0]
    g = torch.Generator(device=dev).manual_seed(2)
    rnd = lambda: torch.rand(n, device=dev, generator=g, dtype=torch.float64)
    ta, tb = rnd() * 6.283185307179586, rnd() * 6.283185307179586
    lw = torch.log(torch.tensor(float(args.warp_max), dtype=torch.float64, device=dev))
    s1, s2 = torch.exp((2 * rnd() - 1) * lw), torch.exp((2 * rnd() - 1) * lw)
    rot = lambda t: torch.stack([torch.cos(t), -torch.sin(t), torch.sin(t), torch.cos(t)], 1).reshape(n, 2, 2)
    A = rot(ta) @ torch.diag_embed(torch.stack([s1, s2], 1)) @ rot(tb)                              # U S V^T: det > 0
    a = torch.floor(A.reshape(n, 4) * 65536.0 + 0.5).to(torch.int32)
    eye = torch.tensor([65536, 0, 0, 65536], dtype=torch.int32, device=dev).expand(n, 4)
    arms = {"plain": lambda: search(gray, valid, q, args.patch, args.range),
            "warp": lambda q10=torch.cat([q, a], 1).contiguous(): search_warp(gray, valid, q10, args.patch, args.range),
            "warp_identity": lambda q10=torch.cat([q, eye], 1).contiguous(): search_warp(gray, valid, q10, args.patch, args.range)}
    times = {k: [] for k in arms}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize(dev)
    for _ in range(args.warp_rounds):
        for k, fn in arms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize(dev)
            times[k].append(ev[0].elapsed_time(ev[1]) / 1e3)
    oi, _ = arms["warp"]()
    res = {"rounds": args.warp_rounds, "warp_max": args.warp_max, "searched_share_warp": float((oi[:, 2] != 1).float().mean())}
    for k, t in times.items():
        res[k + "_s"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    res["warp_over_plain"] = res["warp_s"]["median"] / res["plain_s"]["median"]
    res["identity_over_plain"] = res["warp_identity_s"]["median"] / res["plain_s"]["median"]
    return res


if __name__ == "__main__":
    main()
