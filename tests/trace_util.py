"""A restatement of the sphere tracer (include/dynhor_hip.h: dh_trace_init, dh_trace_step; dynhor_amd/surface_render.trace) in plain
tensor expressions, written from the specification and sharing no code with the product: fp64 by default (the reference the tests
measure against), fp32 for the lock-step comparison of one step (every operation rounded on its own, as the kernel's are).  Also
the dense first-crossing check the end-to-end tests use.  Runs on any device."""
import math

import torch

MARCH, REFINE, HIT, MISS, FAIL = 0, 1, 2, 3, 4
INSIDE, CAPPED, SCANNED = 1, 2, 4
PARAMS = dict(eps=2e-4, relax=0.8, min_step=1e-3, max_step=0.1, refine_steps=8)


def reference_camera(pos=(2.0, 0.9, 0.7), H=96, W=96):
    """(R [1,3,3], T [1,3], K [3,3]) float32 on the CPU: a camera at `pos` looking at the origin, the reference intrinsics."""
    from dynhor_amd.scene import look_at_pose
    R, T = look_at_pose(torch.tensor(pos, dtype=torch.float64))
    f = 1.2 * min(H, W)
    K = torch.tensor([[f, 0, W // 2], [0, f, H // 2], [0, 0, 1]], dtype=torch.float32)
    return R.float()[None], T.float()[None], K


def sphere_bounds(o, d, bound=1.0):
    """(near, far, disc) fp64 of rays o [N,3], d [N,3] with the sphere |x| = bound: b = o.d, disc = b^2 - (|o|^2 - bound^2)."""
    o, d = o.double(), d.double()
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - bound * bound)
    sq = disc.clamp(min=0.0).sqrt()
    return -b - sq, -b + sq, disc


def new_arrays(N, dtype=torch.float64, device="cpu"):
    z = lambda dt: torch.zeros(N, dtype=dt, device=device)
    return dict(t=z(dtype), t_far=z(dtype), t_lo=z(dtype), s_lo=z(dtype), t_hi=z(dtype), s_hi=z(dtype), state=z(torch.int64),
                nq=z(torch.int64), nref=z(torch.int64), flags=z(torch.int64))


def trace_init_ref(R, T, K, H, W, level=1, bound=1.0, dtype=torch.float64, device="cpu"):
    """Arrays of the N = F h w rays (pixels 0, level, ...): o [F,3], d [N,3], near / far / disc [N] and the state-machine arrays."""
    R = R.reshape(-1, 3, 3).to(device, dtype)
    T = T.reshape(-1, 3).to(device, dtype)
    Kinv = torch.inverse(K.to("cpu", torch.float32)).to(device, dtype)
    F = R.shape[0]
    ys = torch.arange(0, H, level, device=device)
    xs = torch.arange(0, W, level, device=device)
    yy, xx = torch.meshgrid(ys, xs, indexing="ij")
    pix = torch.stack([xx.reshape(-1), yy.reshape(-1), torch.ones_like(xx.reshape(-1))], -1).to(dtype)
    dcam = pix @ Kinv.T
    dcam = dcam / dcam.norm(dim=-1, keepdim=True)
    d = torch.einsum("fji,pj->fpi", R, dcam).reshape(-1, 3)                  # R^T dcam
    o = -torch.einsum("fji,fj->fi", R, T)
    hw = ys.numel() * xs.numel()
    near, far, disc = sphere_bounds(o.repeat_interleave(hw, dim=0), d, bound)
    a = new_arrays(F * hw, dtype, device)
    ok = (disc > 0) & (far > 0)
    a.update(o=o, d=d, near=near, far=far, disc=disc, F=F, h=ys.numel(), w=xs.numel(), rays_per_view=hw)
    a["t"] = torch.where(disc > 0, near.clamp(min=0.0), torch.zeros_like(near)).to(dtype)
    a["t_far"] = torch.where(disc > 0, far, torch.zeros_like(far)).to(dtype)
    a["state"] = torch.where(ok, MARCH, MISS).to(torch.int64)
    return a


def trace_step_ref(a, idx, s, eps=2e-4, relax=0.8, min_step=1e-3, max_step=0.1, refine_steps=8):
    """One step for the rays idx (long [n]) with s [n] = sdf(o + t d), in the dtype of a["t"]; updates `a` in place.  Returns tie [n]:
    the rays whose deciding comparison (|s| against eps, t' against t_far, the bracket width against eps) is between unequal numbers
    within 4 ulp of each other -- an implementation that rounds differently may decide those the other way."""
    dt, dev = a["t"].dtype, a["t"].device
    c = lambda v: torch.tensor(v, dtype=dt, device=dev)
    ulp = torch.finfo(dt).eps

    def near_tie(x, y):
        return (x != y) & ((x - y).abs() <= 4 * ulp * torch.maximum(x.abs(), y.abs()))

    s = s.to(dt)
    g = {k: a[k][idx] for k in ("t", "t_far", "t_lo", "s_lo", "t_hi", "s_hi", "state", "nq", "nref", "flags")}
    t, state, nq = g["t"], g["state"], g["nq"]
    live = (state == MARCH) | (state == REFINE)
    fin = torch.isfinite(s)
    small = s.abs() <= c(eps)
    m_fail = live & ~fin
    m_hit = live & fin & small
    rest = live & fin & ~small
    mm, mr = rest & (state == MARCH), rest & (state == REFINE)
    m_inside = mm & (s < 0) & (nq == 0)
    m_enter = mm & (s < 0) & (nq > 0)
    m_adv = mm & ~(s < 0)
    stp = c(relax) * s
    stp = torch.where(stp < c(min_step), c(min_step), torch.where(stp > c(max_step), c(max_step), stp))
    tn = t + stp
    m_miss = m_adv & (tn > g["t_far"])
    pos, neg = mr & (s > 0), mr & ~(s > 0)
    t_lo = torch.where(m_adv | pos, t, g["t_lo"])
    s_lo = torch.where(m_adv | pos, s, g["s_lo"])
    t_hi = torch.where(m_enter | neg, t, g["t_hi"])
    s_hi = torch.where(m_enter | neg, s, g["s_hi"])
    nref = torch.where(mr, (g["nref"] + 1).clamp(max=255), g["nref"])
    m_cap = mr & (g["nref"] + 1 >= refine_steps)
    width = t_hi - t_lo
    m_w = mr & ~m_cap & (width <= c(eps))
    sec = m_enter | (mr & ~m_cap & ~m_w)
    m = c(0.1) * width
    lo, hi = t_lo + m, t_hi - m
    ts = t_lo + width * (s_lo / (s_lo - s_hi))
    ts = torch.where(ts >= lo, ts, lo)
    ts = torch.where(ts <= hi, ts, hi)
    t_new = torch.where(m_adv & ~m_miss, tn, t)
    t_new = torch.where(sec, ts, t_new)
    st = state.clone()
    st[m_fail] = FAIL
    st[m_hit | m_inside | m_cap | m_w] = HIT
    st[m_enter] = REFINE
    st[m_miss] = MISS
    fl = g["flags"] | torch.where(m_inside, INSIDE, 0) | torch.where(m_cap, CAPPED, 0)
    a["t"][idx] = t_new
    a["t_lo"][idx], a["s_lo"][idx], a["t_hi"][idx], a["s_hi"][idx] = t_lo, s_lo, t_hi, s_hi
    a["state"][idx], a["flags"][idx], a["nref"][idx] = st, fl, nref
    a["nq"][idx] = torch.where(live, (nq + 1).clamp(max=65535), nq)
    return live & fin & (near_tie(s.abs(), c(eps).expand_as(s)) | (m_adv & near_tie(tn, g["t_far"]))
                         | (mr & ~m_cap & near_tie(width, c(eps).expand_as(width))))


def points(a, idx):
    return a["o"][idx // a["rays_per_view"]] + a["t"][idx, None] * a["d"][idx]


def trace_ref(sdf_fn, R, T, K, H, W, level=1, bound=1.0, max_steps=48, scan_step=0.01, dtype=torch.float64, device="cpu", **params):
    """The whole tracer: init, max_steps rounds of one query and one step over the live rays, the chord scan of the rays still
    marching (samples t, t + scan_step, ... clipped to t_far; the first with s <= eps is stepped on, the sample before it becoming the
    last positive one), the remaining REFINE steps.  sdf_fn: [n,3] -> [n] or [n,1] in `dtype`.  Returns the arrays; a["scan_q"] holds
    the chord-scan queries per ray."""
    p = dict(PARAMS)
    p.update(params)
    a = trace_init_ref(R, T, K, H, W, level, bound, dtype, device)
    a["scan_q"] = torch.zeros_like(a["nq"])
    live = lambda: ((a["state"] == MARCH) | (a["state"] == REFINE)).nonzero().reshape(-1)
    for _ in range(max_steps):
        idx = live()
        if idx.numel() == 0:
            break
        trace_step_ref(a, idx, sdf_fn(points(a, idx)).reshape(-1), **p)
    rr = (a["state"] == MARCH).nonzero().reshape(-1)
    if rr.numel():
        t0, tf = a["t"][rr], a["t_far"][rr]
        m = int(math.ceil(float((tf - t0).max()) / scan_step)) + 1
        ts = torch.minimum(t0[:, None] + scan_step * torch.arange(m, device=device, dtype=dtype)[None], tf[:, None])
        pts = a["o"][rr // a["rays_per_view"]][:, None] + ts[..., None] * a["d"][rr][:, None]
        s = sdf_fn(pts.reshape(-1, 3)).reshape(-1, m).to(dtype)
        found = (s <= p["eps"]) | ~torch.isfinite(s)
        has = found.any(dim=1)
        first = found.float().argmax(dim=1)
        a["flags"][rr] |= SCANNED
        a["scan_q"][rr] = torch.where(has, first, torch.full_like(first, m))
        a["state"][rr[~has]] = MISS
        rh, jf, ar = rr[has], first[has], torch.arange(int(has.sum()), device=device)
        prev = (jf - 1).clamp(min=0)
        a["t_lo"][rh] = torch.where(jf > 0, ts[has][ar, prev], a["t_lo"][rh])
        a["s_lo"][rh] = torch.where(jf > 0, s[has][ar, prev], a["s_lo"][rh])
        a["t"][rh] = ts[has][ar, jf]
        trace_step_ref(a, rh, s[has][ar, jf], **p)
    for _ in range(p["refine_steps"] + 1):
        idx = live()
        if idx.numel() == 0:
            break
        trace_step_ref(a, idx, sdf_fn(points(a, idx)).reshape(-1), **p)
    assert live().numel() == 0
    return a


def dense_check(sdf_fn, o, d, t0, t_far, state, t_hit, scan_step=0.01, n=4097, chunk=512):
    """Dense first-crossing check of traced rays (o [N,3] per ray, fp64 tensors): n samples over each chord [t0, t_far].
    Returns (missed, earlier): missed = rays in state MISS with a negative sample; earlier = rays in state HIT with a run of negative
    samples longer than scan_step that ends before the hit (samples at or beyond t_hit do not count)."""
    dev = o.device
    missed = torch.zeros(o.shape[0], dtype=torch.bool, device=dev)
    earlier = torch.zeros_like(missed)
    lin = torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev)
    for c0 in range(0, o.shape[0], chunk):
        sl = slice(c0, c0 + chunk)
        ts = t0[sl, None] + (t_far[sl] - t0[sl])[:, None] * lin[None]
        s = sdf_fn((o[sl, None] + ts[..., None] * d[sl, None]).reshape(-1, 3)).reshape(-1, n)
        neg = s < 0
        missed[sl] = (state[sl] == MISS) & neg.any(dim=1)
        before = neg & (ts < t_hit[sl, None])
        run = torch.zeros(ts.shape[0], dtype=torch.int64, device=dev)
        longest = torch.zeros_like(run)
        for j in range(n):
            run = (run + 1) * before[:, j]
            longest = torch.maximum(longest, run)
        h = (t_far[sl] - t0[sl]) / (n - 1)
        earlier[sl] = (state[sl] == HIT) & ((longest - 1).clamp(min=0) * h > scan_step)
    return missed, earlier


def check_sphere_depth(o, d, t, state, radius, eps):
    """Depth of the hits against the ray-sphere root to eps / cos(theta); rays with cos(theta) < 0.2 are left out (fewer than 10 %).
    o [N,3] per ray, all fp64.  Returns (hits, left out, largest error / bound)."""
    near, _, disc = sphere_bounds(o, d, radius)
    hit = state == HIT
    assert bool((disc[hit] > -1e-3).all()), "a hit on a ray that passes the sphere by more than its tolerance"
    assert bool(hit[disc > 4 * eps].all()), "a ray that crosses the sphere well inside its rim is no hit"
    x = o + near[:, None] * d
    cos = ((x / radius) * d).sum(-1).abs()
    use = hit & (disc > 0) & (cos >= 0.2)
    left = int(hit.sum()) - int(use.sum())
    assert left < 0.1 * int(hit.sum()), (left, int(hit.sum()))
    ratio = ((t[use] - near[use]).abs() * cos[use] / eps)
    assert float(ratio.max()) <= 1.0, float(ratio.max())
    return int(hit.sum()), left, float(ratio.max())
