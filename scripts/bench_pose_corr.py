"""Timing of the correspondence pose term (dynhor_amd/pose_corr.py) over 300 frames of 1080 x 1920, frame i matched to i + 1, i + 2 and
i + 5 with 1,000 matches per pair, on the analytic scene's mesh at marching-cubes resolution 128:
  * both kernels by event times: dh_pose_corr_sums (all chunks of 16 source frames, the z-buffers made beforehand and kept) and
    dh_pose_corr_frames;
  * the z-buffers the term rasterises per step (dh_mesh_raster_depth), for scale;
  * one iteration of SilhouettePoseOptimizer with and without the term, in alternating runs in this one process.
The matches are synthetic: pixels of frame i on the object, q their reprojection through the mesh at the true poses plus 0.5 px of noise
(the term's own lift; a pixel that sees no face of the mesh gets c = 0).  One JSON line per measurement.  Kernel times proper come from a profiler
run of its own:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d <out> -o pcorr -- python scripts/bench_pose_corr.py
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
    ap.add_argument("--offsets", type=int, nargs="*", default=[1, 2, 5])
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="alternating with / without rounds of the whole-iteration timing")
    args = ap.parse_args()
    import torch
    from bench_mesh_clean import _timed, scene_mesh, sequence
    from dynhor_amd.mesh_color import raster_depth
    from dynhor_amd.pose_corr import CorrespondenceTerm, corr_sums
    from dynhor_amd.pose_sil import SilhouettePoseOptimizer
    assert torch.cuda.is_available(), "bench_pose_corr needs a GPU"
    dev = torch.device("cuda:0")
    F, H, W = args.frames, args.H, args.W
    label, R, T, K = sequence(F, H, W, dev)
    mv, mf = scene_mesh(args.resolution, dev)
    mv, mf = mv.float().contiguous(), mf.long().contiguous()
    g = torch.Generator(device=dev).manual_seed(0)
    # matches: random object pixels of frame i (the label's disc), q filled in below from the term's own residual-free lift
    pi, pj, first, count, rows = [], [], [], [], []
    for i in range(F):
        ys, xs = (label[i] == 1).nonzero(as_tuple=True)
        for off in args.offsets:
            if i + off >= F:
                continue
            sel = torch.randint(0, ys.shape[0], (args.matches,), device=dev, generator=g)
            m = torch.zeros(args.matches, 5, device=dev)
            m[:, 0], m[:, 1], m[:, 4] = xs[sel].float(), ys[sel].float(), 1.0
            pi.append(i); pj.append(i + off); first.append(len(rows) * args.matches); count.append(args.matches); rows.append(m)
    matches = torch.cat(rows).contiguous()
    # q = the reprojection the kernel itself finds, recovered from two residuals: |(u, w)| at q = 0 and |(u - 1e4, w)| at q = (1e4, 0)
    # (u, w > 0 inside the image), plus noise
    a = matches[:, 2].clone()
    probe = matches.clone()
    probe[:, 2:4] = 0.0
    resid_a = torch.full((matches.shape[0],), -1.0, device=dev)
    CorrespondenceTerm(probe, pi, pj, first, count, F, H, W, frame_chunk=args.chunk, delta_px=1e6).sums(mv, mf, R, T, K, resid=resid_a)
    probe[:, 2] = 1e4
    resid_b = torch.full((matches.shape[0],), -1.0, device=dev)
    CorrespondenceTerm(probe, pi, pj, first, count, F, H, W, frame_chunk=args.chunk, delta_px=1e6).sums(mv, mf, R, T, K, resid=resid_b)
    ok = (resid_a >= 0) & (resid_b >= 0)
    ra, rb = resid_a.double(), resid_b.double()
    u = (ra * ra - rb * rb + 1e8) / 2e4
    w = (ra * ra - u * u).clamp(min=0).sqrt()
    noise = 0.5 * torch.randn(matches.shape[0], 2, device=dev, generator=g)
    matches[:, 2] = torch.where(ok, u.float() + noise[:, 0], torch.zeros_like(a))
    matches[:, 3] = torch.where(ok, w.float() + noise[:, 1], torch.zeros_like(a))
    matches[:, 4] = ok.float()
    del a, probe, resid_a, resid_b
    term = CorrespondenceTerm(matches, pi, pj, first, count, F, H, W, frame_chunk=args.chunk)
    zbufs = [raster_depth(mv, mf, R[fr].contiguous(), T[fr].contiguous(), K, H, W) for fr, _, _ in term.chunks]

    def sums_all():
        return torch.cat([corr_sums(mv, mf, R, T, K, zb, term.matches, pairs, mc, term.delta_px, term.min_cos)
                          for zb, (_, pairs, mc) in zip(zbufs, term.chunks)])

    def raster_all():
        for fr, _, _ in term.chunks:
            raster_depth(mv, mf, R[fr].contiguous(), T[fr].contiguous(), K, H, W)

    rows = sums_all()
    scale = (1.0 / term.n_pairs) / rows[:, 1].clamp(min=1e-12)
    s_sums = _timed(sums_all, args.reps, dev)
    s_frames = _timed(lambda: term.grads(rows, scale), args.reps, dev)
    s_raster = _timed(raster_all, args.reps, dev)
    del zbufs
    base = {"bench": "pose_corr", "mesh": f"scene@{args.resolution}", "faces": mf.shape[0], "frames": F, "chunk": args.chunk, "H": H, "W": W,
            "pairs": term.n_pairs, "matches": int(matches.shape[0])}
    print(json.dumps(dict(base, what="kernels", corr_sums_ms=1e3 * s_sums, corr_sums_calls=len(term.chunks), corr_frames_ms=1e3 * s_frames,
                          raster_ms=1e3 * s_raster, counted=float(rows[:, 26].sum()), inlier_share=float(rows[:, 27].sum() / rows[:, 26].sum()))),
          flush=True)
    # a whole iteration, with and without the term, alternating
    opts = {False: SilhouettePoseOptimizer(mv, mf, label, R, T, K, frame_chunk=args.chunk),
            True: SilhouettePoseOptimizer(mv, mf, label, R, T, K, frame_chunk=args.chunk, corr=term, lw_corr=1e-3)}
    times = {False: [], True: []}
    for _ in range(args.rounds):
        for with_term in (False, True):
            times[with_term].append(_timed(lambda: opts[with_term].step(6.0), args.reps, dev))
    print(json.dumps(dict(base, what="iteration", without_ms=[1e3 * t for t in times[False]], with_ms=[1e3 * t for t in times[True]],
                          added_ms_median=1e3 * (sorted(times[True])[len(times[True]) // 2] - sorted(times[False])[len(times[False]) // 2]))),
          flush=True)


if __name__ == "__main__":
    main()
