"""Restatements of dh_ssim (include/dynhor_hip.h) for the tests and scripts/bench_image_metrics.py:
  * ssim_ref: numpy, int64 window sums formed separably and the fp64 formula in the kernel's operation order -- the map must match the
    kernel's bit for bit, the integer sums exactly, the two float sums up to the order of addition;
  * ssim_plain: an independent plain-float SSIM (dense 2-D window, weights t t' / 2^32) for interior pixels of a fully usable image;
  * ssim_torch: the same rule as ssim_ref in torch (int64 / float64 tensors on any device), the yardstick of the timing.
"""
import math

import numpy as np

K1, K2 = 0.01 * 255.0, 0.03 * 255.0
C1, C2 = K1 * K1, K2 * K2
ROW_LIMIT, COL_LIMIT = 1 << 32, 1 << 48


def _window(q, taps, check=True):
    """q int64 [F,H,W] -> sum over the window of taps[dx + r] taps[dy + r] q (0 outside the image): rows, then columns."""
    r = len(taps) // 2
    F, H, W = q.shape
    p = np.pad(q, ((0, 0), (0, 0), (r, r)))
    rows = np.zeros_like(q)
    for k in range(2 * r + 1):
        rows += int(taps[k]) * p[:, :, k:k + W]
    if check:
        assert rows.size == 0 or int(rows.max()) < ROW_LIMIT, "a row sum must fit 32 bits"
    p = np.pad(rows, ((0, 0), (r, r), (0, 0)))
    cols = np.zeros_like(q)
    for k in range(2 * r + 1):
        cols += int(taps[k]) * p[:, k:k + H, :]
    if check:
        assert cols.size == 0 or int(cols.max()) < COL_LIMIT, "a column sum must stay below 2^48"
    return cols, (int(rows.max()) if rows.size else 0)


def ssim_ref(a, b, usable, taps, w_min):
    """a, b u8 [F,H,W,3], usable u8 [F,H,W] or None, taps ints (sum 65536), w_min int.  Returns a dict: map f32 [F,H,W], out f64 [F,6]
    (the float sums [0], [5] by math.fsum: correctly rounded), s f64 [F,H,W] (0 where not counted), counted bool [F,H,W], abs0 / abs5:
    sum |terms| of the two float sums per frame (for the reordering bound), max_row: the largest row sum met."""
    a = np.asarray(a)
    b = np.asarray(b)
    F, H, W, _ = a.shape
    u = np.ones((F, H, W), np.int64) if usable is None else (np.asarray(usable) != 0).astype(np.int64)
    wt, _ = _window(u, taps)
    counted = (u == 1) & (wt >= int(w_min))
    wd = np.where(counted, wt, 1).astype(np.float64)
    ssum = np.zeros((F, H, W), np.float64)
    max_row = 0
    for c in range(3):
        A = a[..., c].astype(np.int64) * u
        B = b[..., c].astype(np.int64) * u
        sums = []
        for q in (A, B, A * A, B * B, A * B):
            s, m = _window(q, taps)
            max_row = max(max_row, m)
            sums.append(s.astype(np.float64))
        sx, sy, sxx, syy, sxy = sums
        mx = sx / wd
        my = sy / wd
        mxx = mx * mx
        myy = my * my
        mxy = mx * my
        vx = sxx / wd - mxx
        vy = syy / wd - myy
        cxy = sxy / wd - mxy
        num = ((2.0 * mx) * my + C1) * (2.0 * cxy + C2)
        den = ((mxx + myy) + C1) * ((vx + vy) + C2)
        ssum = ssum + num / den
    s = np.where(counted, ssum / 3.0, 0.0)
    d = (a.astype(np.int64) - b.astype(np.int64)) * u[..., None]
    out = np.zeros((F, 6), np.float64)
    abs0, abs5 = np.zeros(F), np.zeros(F)
    for f in range(F):
        sf = s[f][counted[f]]
        out[f] = (math.fsum(sf.tolist()), float(counted[f].sum()), float((d[f] * d[f]).sum()), float(np.abs(d[f]).sum()),
                  float(u[f].sum()), math.fsum((sf * sf).tolist()))
        abs0[f] = math.fsum(np.abs(sf).tolist())
        abs5[f] = out[f, 5]
    return {"map": s.astype(np.float32), "out": out, "s": s, "counted": counted, "abs0": abs0, "abs5": abs5, "max_row": max_row,
            "wt": wt}


def ssim_plain(a, b, taps):
    """Plain float SSIM of fully usable images at the interior pixels (whole window inside the image): f64 [F, H - 2r, W - 2r].  Dense
    2-D window with the weights t t' / 2^32, means and (co)variances as expectations; no integers, no separable passes."""
    a = np.asarray(a).astype(np.float64)
    b = np.asarray(b).astype(np.float64)
    t = np.asarray(taps, np.float64) / 65536.0
    r = len(t) // 2
    F, H, W, _ = a.shape
    h, w = H - 2 * r, W - 2 * r
    total = np.zeros((F, h, w))
    for c in range(3):
        x, y = a[..., c], b[..., c]
        e = {k: np.zeros((F, h, w)) for k in ("x", "y", "xx", "yy", "xy")}
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                wgt = t[dy] * t[dx]
                xs, ys = x[:, dy:dy + h, dx:dx + w], y[:, dy:dy + h, dx:dx + w]
                e["x"] += wgt * xs
                e["y"] += wgt * ys
                e["xx"] += wgt * (xs * xs)
                e["yy"] += wgt * (ys * ys)
                e["xy"] += wgt * (xs * ys)
        mx, my = e["x"], e["y"]
        vx, vy, cxy = e["xx"] - mx * mx, e["yy"] - my * my, e["xy"] - mx * my
        total = total + ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return total / 3.0


def ssim_torch(a, b, usable, taps, w_min):
    """ssim_ref's rule in torch on a's device: (map f32 [F,H,W], out f64 [F,6]); the float sums by torch.sum."""
    import torch
    import torch.nn.functional as Fn
    F, H, W, _ = a.shape
    t = [int(x) for x in taps]
    r = len(t) // 2
    u = torch.ones(F, H, W, dtype=torch.int64, device=a.device) if usable is None else (usable != 0).to(torch.int64)

    def window(q):
        p = Fn.pad(q, (r, r))
        rows = torch.zeros_like(q)
        for k in range(2 * r + 1):
            rows += t[k] * p[:, :, k:k + W]
        p = Fn.pad(rows, (0, 0, r, r))
        cols = torch.zeros_like(q)
        for k in range(2 * r + 1):
            cols += t[k] * p[:, k:k + H, :]
        return cols

    wt = window(u)
    counted = (u == 1) & (wt >= int(w_min))
    wd = torch.where(counted, wt, torch.ones_like(wt)).double()
    ssum = torch.zeros(F, H, W, dtype=torch.float64, device=a.device)
    for c in range(3):
        A = a[..., c].to(torch.int64) * u
        B = b[..., c].to(torch.int64) * u
        sx, sy, sxx, syy, sxy = (window(q).double() for q in (A, B, A * A, B * B, A * B))
        mx, my = sx / wd, sy / wd
        mxx, myy, mxy = mx * mx, my * my, mx * my
        vx, vy, cxy = sxx / wd - mxx, syy / wd - myy, sxy / wd - mxy
        num = ((2.0 * mx) * my + C1) * (2.0 * cxy + C2)
        den = ((mxx + myy) + C1) * ((vx + vy) + C2)
        ssum = ssum + num / den
    s = torch.where(counted, ssum / 3.0, torch.zeros_like(ssum))
    d = (a.to(torch.int64) - b.to(torch.int64)) * u[..., None]
    out = torch.stack([s.sum(dim=(1, 2)), counted.sum(dim=(1, 2)).double(), (d * d).sum(dim=(1, 2, 3)).double(),
                       d.abs().sum(dim=(1, 2, 3)).double(), u.sum(dim=(1, 2)).double(), (s * s).sum(dim=(1, 2))], dim=1)
    return s.float(), out


def disc_mask(H, W, cy, cx, radius):
    """u8 [H,W]: 1 where (y - cy)^2 + (x - cx)^2 < radius^2 (the open disc: 697 pixels at radius 15)."""
    y, x = np.mgrid[0:H, 0:W]
    return (((y - cy) ** 2 + (x - cx) ** 2) < radius * radius).astype(np.uint8)
