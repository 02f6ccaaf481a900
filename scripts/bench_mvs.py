"""Timing of the multi-view stereo kernels (dynhor_amd/mvs.py): 16 frames of 1080 x 1920 smooth-noisy input (every pixel usable), each
frame the one before moved by (-96, -8) px -- a fronto-parallel plane at depth 1.5 seen by cameras that slide sideways by 0.096, so
that one depth step of the sweep moves a patch by 0.16 px in the nearest neighbours.  dh_mvs_sweep at
P 4, D 33, four neighbours on a grid of --step_px with the guide off the plane by up to a third of the range, and dh_mvs_check on the 16
full depth maps; event times, the median of --reps.  The rate is pixel x hypothesis x neighbour per second (neighbours that exist).  The
comparison is the same rule in torch on the same GPU (torch_sweep below: the homography, the taps, the bilinear fetch with validity, the
fp32 sums, the mean score and the argmax, vectorised over pixels x hypotheses x taps) on --torch_pixels of the same pixels.  One JSON
line.  Kernel times proper come from a profiler run of its own:

    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <out> -o mvs -- python scripts/bench_mvs.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _events(fn, reps, dev):
    import torch
    fn()
    torch.cuda.synchronize(dev)
    t = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize(dev)
        t.append(ev[0].elapsed_time(ev[1]) / 1e3)
    return statistics.median(t)


def torch_sweep(gray, valid, R, T, K, Kinv, pix, guide, nbr, D, step, P, min_vb, min_views, chunk=2048):
    """k_best int64 [n] (-1: none) and c_best f32 [n] by dh_mvs_sweep's rule in float32 torch (the sums by torch.sum, not sequential)."""
    import torch
    F, H, W = gray.shape
    S = 2 * P + 1
    N = S * S
    offs = torch.arange(-P, P + 1, device=gray.device)
    cc, rr = offs.repeat(S).float(), offs.repeat_interleave(S).float()
    gflat, vflat = gray.reshape(F, -1).float(), valid.reshape(F, -1)
    kb, cb = [], []
    for a0 in range(0, pix.shape[0], chunk):
        p, g = pix[a0:a0 + chunk].long(), guide[a0:a0 + chunk]
        n = p.shape[0]
        fi = p[:, 0]
        ys, xs = p[:, 2, None] + offs.repeat_interleave(S)[None], p[:, 1, None] + offs.repeat(S)[None]
        a = gflat[fi[:, None], ys * W + xs]                                                            # the bench's pixels lie inside
        sa, va = a.sum(1), N * (a * a).sum(1) - a.sum(1) ** 2
        ph = torch.stack([p[:, 1].float(), p[:, 2].float(), torch.ones(n, device=p.device)], 1)
        e = ph @ Kinv.reshape(3, 3).T
        zk = g[:, 0, None] + (torch.arange(D, device=p.device) - (D - 1) // 2).float()[None] * step    # [n,D]
        X = zk[..., None] * e[:, None]
        s = g[:, None, 1:] / (X * g[:, None, 1:]).sum(-1, keepdim=True)
        csum = torch.zeros(n, D, device=p.device)
        views = torch.zeros(n, D, device=p.device)
        Ri, Ti = R.reshape(F, 3, 3)[fi], T[fi]
        for jn in range(nbr.shape[1]):
            j = nbr[fi, jn].long()
            jok = j >= 0
            jc = j.clamp(min=0)
            Rij = R.reshape(F, 3, 3)[jc] @ Ri.transpose(1, 2)
            t = T[jc] - (Rij @ Ti[..., None])[..., 0]
            M = Rij[:, None] + t[:, None, :, None] * s[:, :, None, :]                                  # [n,D,3,3]
            Hm = K.reshape(3, 3) @ M @ Kinv.reshape(3, 3)
            h = (Hm @ ph[:, None, :, None])[..., 0]
            ok = jok[:, None] & (zk > 1e-3) & (h[..., 2] > 1e-3)
            q = h[..., :2] / h[..., 2:]
            A = (Hm[..., :2, :2] - q[..., None] * Hm[..., 2:, :2]) / h[..., 2, None, None]
            tx = q[..., 0, None] + A[..., 0, 0, None] * cc + A[..., 0, 1, None] * rr                   # [n,D,N]
            ty = q[..., 1, None] + A[..., 1, 0, None] * cc + A[..., 1, 1, None] * rr
            inb = (tx >= 0) & (tx < W - 1) & (ty >= 0) & (ty < H - 1)
            x0, y0 = torch.where(inb, tx, torch.zeros_like(tx)).floor(), torch.where(inb, ty, torch.zeros_like(ty)).floor()
            at = y0.long() * W + x0.long()
            jj = jc[:, None, None].expand_as(at)
            v = inb & (vflat[jj, at] != 0) & (vflat[jj, at + 1] != 0) & (vflat[jj, at + W] != 0) & (vflat[jj, at + W + 1] != 0)
            wx, wy = tx - x0, ty - y0
            top = gflat[jj, at] + wx * (gflat[jj, at + 1] - gflat[jj, at])
            bot = gflat[jj, at + W] + wx * (gflat[jj, at + W + 1] - gflat[jj, at + W])
            b = torch.where(v, top + wy * (bot - top), torch.zeros_like(tx))
            sb, sb2, sab = b.sum(-1), (b * b).sum(-1), (a[:, None] * b).sum(-1)
            vb = N * sb2 - sb * sb
            ok = ok & v.all(-1) & (vb >= min_vb)
            score = (N * sab - sa[:, None] * sb) / torch.sqrt(va[:, None] * vb.clamp(min=1e-30))
            csum = csum + torch.where(ok, score, torch.zeros_like(score))
            views = views + ok.float()
        c = torch.where(views >= min_views, csum / views.clamp(min=1), torch.full_like(csum, -2.0))
        best, k = c.max(1)
        kb.append(torch.where(best > -1.5, k, torch.full_like(k, -1)))
        cb.append(best)
    return torch.cat(kb), torch.cat(cb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--patch", type=int, default=4)
    ap.add_argument("--depths", type=int, default=33)
    ap.add_argument("--range", type=float, default=0.04)
    ap.add_argument("--step_px", type=int, default=4)
    ap.add_argument("--torch_pixels", type=int, default=1 << 14)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from mesh_texture_util import smooth_noisy_frames
    from dynhor_amd import mvs
    from dynhor_amd.match import default_min_va, gray_frames
    assert torch.cuda.is_available(), "bench_mvs needs a GPU"
    dev = torch.device("cuda:0")
    F, H, W, P, D = args.frames, args.H, args.W, args.patch, args.depths
    base = smooth_noisy_frames(1, H + 8 * F, W + 96 * F, seed=0, device=dev)[0]
    rgb = torch.stack([base[8 * f:8 * f + H, 96 * f:96 * f + W] for f in range(F)]).contiguous()   # frame f + 1 = frame f moved by (-96, -8)
    usable = torch.ones(F, H, W, dtype=torch.uint8, device=dev)
    gray, valid = gray_frames(rgb, usable, 1.0, 0.5)
    focal, Z = 1500.0, 1.5
    K = torch.tensor([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], device=dev)
    R = torch.eye(3, device=dev).expand(F, 3, 3).contiguous()
    T = torch.stack([torch.tensor([-96.0 * f * Z / focal, -8.0 * f * Z / focal, 0.0]) for f in range(F)]).to(dev)
    nbr = mvs.neighbours(F).to(dev)
    m = 32                                                                                          # a margin: the bench's patches lie inside
    ys, xs = torch.meshgrid(torch.arange(m, H - m, args.step_px, device=dev), torch.arange(m, W - m, args.step_px, device=dev), indexing="ij")
    per = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    pix = torch.cat([torch.cat([torch.full((per.shape[0], 1), f, device=dev), per], 1) for f in range(F)]).to(torch.int32).contiguous()
    n = pix.shape[0]
    g = torch.Generator(device=dev).manual_seed(1)
    z0 = Z + (torch.rand(n, device=dev, generator=g) * 2 - 1) * args.range / 3
    guide = torch.stack([z0, torch.zeros_like(z0), torch.zeros_like(z0), -torch.ones_like(z0)], 1).contiguous()
    step = 2.0 * args.range / (D - 1)
    min_va = default_min_va(P)
    run = lambda: mvs.sweep(gray, valid, R, T, K, pix, guide, nbr, D, step, P, min_va, float(min_va), 2, 0.2)
    s_sweep = _events(run, args.reps, dev)
    of, oi = run()
    pairs = int((nbr[pix[:, 0].long()] >= 0).sum())                                                 # pixel x existing neighbour
    found = ((of[:, 0] - Z).abs() <= step) & (oi[:, 2] == 0)
    depth = torch.full((F, H, W), float("nan"), device=dev)
    depth[:] = Z
    s_check = _events(lambda: mvs.check(depth, R, T, K, nbr, 0.01), args.reps, dev)
    count = mvs.check(depth, R, T, K, nbr, 0.01)
    out = {"bench": "mvs", "frames": F, "H": H, "W": W, "patch": P, "depths": D, "neighbours": int(nbr.shape[1]), "step_px": args.step_px,
           "pixels": n, "sweep_s": s_sweep, "pixel_hyp_nbr": pairs * D, "pixel_hyp_nbr_per_s": pairs * D / s_sweep,
           "taps_per_s": pairs * D * (2 * P + 1) ** 2 / s_sweep, "flags0_share": float((oi[:, 2] == 0).float().mean()),
           "found_share": float(found.float().mean()), "mean_c_best": float(of[oi[:, 2] == 0, 1].mean()),
           "check_s": s_check, "check_pixels_per_s": F * H * W / s_check, "check_mean_count": float(count.float().mean())}
    if args.torch_pixels > 0:
        sel = torch.randperm(n, device=dev, generator=g)[:args.torch_pixels]
        tp, tg = pix[sel].contiguous(), guide[sel].contiguous()
        Kinv = mvs._kinv(K)
        trun = lambda: torch_sweep(gray, valid, R, T, K, Kinv, tp, tg, nbr, D, step, P, float(min_va), 2)
        s_torch = _events(trun, max(1, args.reps - 1), dev)
        kb, _ = trun()
        tpairs = int((nbr[tp[:, 0].long()] >= 0).sum())
        rate = tpairs * D / s_torch
        out["torch"] = {"pixels": int(tp.shape[0]), "sweep_s": s_torch, "pixel_hyp_nbr_per_s": rate,
                        "same_k_best_share": float((kb == torch.where(oi[sel, 2] & 11 == 0, oi[sel, 0].long(), torch.full_like(kb, -1))).float().mean()),
                        "kernel_over_torch": out["pixel_hyp_nbr_per_s"] / rate}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
