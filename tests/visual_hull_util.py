"""The visual hull's rule (dynhor_amd/visual_hull.py, include/dynhor_hip.h: dh_hull_accumulate) restated in numpy, in fp64 by default
and in any other dtype (float32: to price the rounding of the device's arithmetic).  Built on a brute-force windowed distance
transform: no scipy, no torch ops beyond the conversion of the inputs."""
import math

import numpy as np


def as_np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def brute_edt(label, value, rmax):
    """f64 [F,H,W]: min over |dx|, |dy| <= rmax (window clipped to the image) with label[y + dy, x + dx] == value of dx^2 + dy^2, +inf
    where the window holds none: every shift of the match mask, one after the other."""
    label = as_np(label)
    F, H, W = label.shape
    far = np.int32(1 << 30)
    cost = np.where(label == value, np.int32(0), far)
    out = np.full((F, H, W), far, dtype=np.int32)
    r = int(rmax)
    for dy in range(-min(r, H - 1), min(r, H - 1) + 1):
        ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))      # source rows y + dy, destination rows y
        for dx in range(-min(r, W - 1), min(r, W - 1) + 1):
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            view = out[:, yd, xd]
            np.minimum(view, cost[:, ys, xs] + np.int32(dx * dx + dy * dy), out=view)
    return np.where(out >= far, np.inf, out.astype(np.float64))


def signed_label_distance(label, band_px, dtype=np.float64):
    """s [F,H,W]: solid = label != 0; on solid pixels -(sqrt(d2_bg) - 0.5), elsewhere sqrt(min(d2_obj, d2_hand)) - 0.5; clamped to
    [-band_px, band_px]; rmax = ceil(band_px) + 1."""
    label = as_np(label)
    rmax = int(math.ceil(band_px)) + 1
    d_bg = brute_edt(label, 0, rmax).astype(dtype)
    d_solid = np.minimum(brute_edt(label, 1, rmax), brute_edt(label, -1, rmax)).astype(dtype)
    half = dtype(0.5)
    s = np.where(label != 0, -(np.sqrt(d_bg) - half), np.sqrt(d_solid) - half)
    return np.clip(s, dtype(-band_px), dtype(band_px)).astype(dtype)


def frame_values(points, sd, R, T, K, dtype=np.float64, with_uv=False):
    """(g [F,n], seen bool [F,n]) of points [n,3] in every frame: c = R_f p + T_f, u = (K0 . c) / z, w = (K1 . c) / z, seen when
    z > 1e-6 and 0 <= u <= W - 1 and 0 <= w <= H - 1; the four taps at x0 = min(floor(u), W - 2), y0 = min(floor(w), H - 2)
    interpolated along x, then along y; g = bilinear z / K00.  with_uv: also (u, w, z) [F,n] each."""
    p = as_np(points).astype(dtype)
    sd = as_np(sd).astype(dtype)
    R = as_np(R).astype(dtype).reshape(-1, 3, 3)
    T = as_np(T).astype(dtype).reshape(-1, 3)
    K = as_np(K).astype(dtype).reshape(3, 3)
    F, H, W = sd.shape
    g = np.zeros((F, p.shape[0]), dtype=dtype)
    seen = np.zeros((F, p.shape[0]), dtype=bool)
    us, ws, zs = (np.zeros_like(g) for _ in range(3))
    with np.errstate(all="ignore"):
        for f in range(F):
            c = [R[f, r, 2] * p[:, 2] + (R[f, r, 1] * p[:, 1] + R[f, r, 0] * p[:, 0]) + T[f, r] for r in range(3)]
            z = c[2]
            u = (K[0, 2] * c[2] + (K[0, 1] * c[1] + K[0, 0] * c[0])) / z
            w = (K[1, 2] * c[2] + (K[1, 1] * c[1] + K[1, 0] * c[0])) / z
            ok = (z > dtype(1e-6)) & (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1)
            x0 = np.where(ok, np.minimum(np.floor(u), W - 2), 0).astype(np.int64)
            y0 = np.where(ok, np.minimum(np.floor(w), H - 2), 0).astype(np.int64)
            fx, fy = u - x0.astype(dtype), w - y0.astype(dtype)
            s00, s01, s10, s11 = sd[f, y0, x0], sd[f, y0, x0 + 1], sd[f, y0 + 1, x0], sd[f, y0 + 1, x0 + 1]
            top, bot = s00 + fx * (s01 - s00), s10 + fx * (s11 - s10)
            val = top + fy * (bot - top)
            g[f] = np.where(ok, (val * z) / K[0, 0], 0)
            seen[f] = ok
            us[f], ws[f], zs[f] = u, w, z
    return (g, seen, us, ws, zs) if with_uv else (g, seen)


def state_from_values(g, seen, m, frame_index=None):
    """(topk [n,m] descending, -inf padded; arg int64 [n], the frame of the largest value, the lowest frame on equal values, -1 when no
    frame sees the point; seen int64 [n]).  frame_index: the global index of every row of g (default 0 .. F-1)."""
    F, n = g.shape
    fi = np.arange(F) if frame_index is None else np.asarray(frame_index)
    order = np.argsort(fi, kind="stable")
    v = np.where(seen, g, -np.inf)[order]
    topk = np.full((n, m), -np.inf, dtype=g.dtype)
    srt = -np.sort(-v, axis=0)[:m]
    topk[:, :srt.shape[0]] = srt.T
    count = seen.sum(axis=0)
    arg = np.where(count > 0, fi[order][np.argmax(v, axis=0)], -1) if F else np.full(n, -1)
    return topk, arg.astype(np.int64), count.astype(np.int64)


def field_from_state(topk, seen, n_frames, min_carve_votes=1, min_seen=0.5, outside_value=1.0):
    k = int(min_carve_votes)
    need = max(k, int(math.ceil(min_seen * n_frames)))
    return np.where(seen >= need, topk[:, k - 1], topk.dtype.type(outside_value))


def hull_state(points, label, R, T, K, m=2, band_px=16, dtype=np.float64, sd=None):
    """(topk, arg, seen) of the points against every frame (sd: a signed map formed earlier, to share it)."""
    sd = signed_label_distance(label, band_px, dtype) if sd is None else sd
    g, ok = frame_values(points, sd, R, T, K, dtype)
    return state_from_values(g, ok, m)


def sole_carved_share(topk, arg, seen, n_frames, min_seen=0.5):
    """share [F]: the points frame f alone carves (topk0 > 0, topk1 <= 0, arg = f) over the points of the k = 2 hull."""
    need = max(2, int(math.ceil(min_seen * n_frames)))
    judged = seen >= need
    hull2 = int((judged & (topk[:, 1] <= 0)).sum())
    sole = judged & (topk[:, 0] > 0) & (topk[:, 1] <= 0)
    return np.bincount(arg[sole], minlength=n_frames) / max(hull2, 1), hull2


def grid_points(lo, hi, N):
    """f32 [N^3,3], x-major, the axes as float32 linspace (np.linspace in fp64, then rounded: the values torch.linspace gives may
    differ in the last bit, so a test that compares against the device passes the device's points instead)."""
    ax = [np.linspace(lo[a], hi[a], N).astype(np.float32) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
