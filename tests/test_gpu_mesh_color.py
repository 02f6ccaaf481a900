"""Mesh colouring on the GPU: the z-buffer against an fp64 brute force and under face permutation, the colour gather against an fp64
restatement of its rule (on the GPU's own z-buffer) and across frame chunkings, occlusion in a two-sphere scene, hand pixels on the
synthetic sequence, the network colours of both model families against the oracles, and Runner.validate_mesh / the CLI."""
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
EDGE_TOL_PX = 1e-4


def _cameras(n, H, W, radius=2.5, seed=0):
    """n look-at cameras on a sphere of `radius` (Fibonacci directions, jittered), reference intrinsics f = 1.2 min(H,W)."""
    from dynhor_amd.scene import look_at_pose
    Rs, Ts = [], []
    g = torch.Generator().manual_seed(seed)
    for i in range(n):
        z = 1 - 2 * (i + 0.5) / n
        phi = i * math.pi * (3 - math.sqrt(5)) + float(torch.rand(1, generator=g))
        d = torch.tensor([math.sqrt(1 - z * z) * math.cos(phi), math.sqrt(1 - z * z) * math.sin(phi), z])
        R, T = look_at_pose(d * radius, up=torch.tensor([0.0, 0.0, 1.0]) if abs(z) < 0.95 else torch.tensor([1.0, 0.0, 0.0]))
        Rs.append(R); Ts.append(T)
    f = 1.2 * min(H, W)
    K = torch.tensor([[f, 0, W // 2], [0, f, H // 2], [0, 0, 1]], dtype=torch.float32)
    return torch.stack(Rs).float().to(DEV), torch.stack(Ts).float().to(DEV), K.to(DEV)


def _sphere_mesh(center, r, N=48):
    from dynhor_amd.mesh import marching_cubes
    lo, hi = [c - r * 1.2 for c in center], [c + r * 1.2 for c in center]
    ax = [torch.linspace(lo[i], hi[i], N, device=DEV) for i in range(3)]
    gx, gy, gz = torch.meshgrid(*ax, indexing="ij")
    p = torch.stack([gx, gy, gz], -1)
    return marching_cubes(r - torch.linalg.norm(p - torch.tensor(center, device=DEV), dim=-1), 0.0, lo, hi)


# ------------------------------------------------------------------------------------------------ 1. raster vs fp64
def _raster_fp64(verts, faces, R, T, K, H, W):
    """Per frame: (depth [H,W] fp64 min over strictly covering faces, inf if none; ambiguous [H,W]: some face has the pixel centre
    within EDGE_TOL_PX of one of its edges without being strictly outside another)."""
    v = verts.double()
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float64), torch.arange(W, device=DEV, dtype=torch.float64),
                            indexing="ij")
    px, py = xs.reshape(-1, 1), ys.reshape(-1, 1)
    out = []
    for f in range(R.shape[0]):
        c = v @ R[f].double().T + T[f].double()
        z = c[:, 2]
        u = (c @ K[0].double()) / z
        w = (c @ K[1].double()) / z
        a, b, cc = faces[:, 0], faces[:, 1], faces[:, 2]
        ua, wa, ub, wb, uc, wc = u[a], w[a], u[b], w[b], u[cc], w[cc]
        area = (ub - ua) * (wc - wa) - (wb - wa) * (uc - ua)
        ok = (z[a] > 1e-3) & (z[b] > 1e-3) & (z[cc] > 1e-3) & (area != 0)
        sgn = torch.sign(area)

        def sdist(au, aw, bu, bw):                     # signed distance of the pixel centres to edge (a, b), inside > 0
            e = (bu - au) * (py - aw) - (bw - aw) * (px - au)
            return e * sgn / torch.sqrt((bu - au) ** 2 + (bw - aw) ** 2)

        d0, d1, d2 = sdist(ub, wb, uc, wc), sdist(uc, wc, ua, wa), sdist(ua, wa, ub, wb)     # [HW, nf]
        dmin = torch.minimum(torch.minimum(d0, d1), d2)
        inside = (dmin > EDGE_TOL_PX) & ok
        amb = ((dmin.abs() <= EDGE_TOL_PX) & ok).any(dim=1)
        e0 = d0 * torch.sqrt((uc - ub) ** 2 + (wc - wb) ** 2)
        e1 = d1 * torch.sqrt((ua - uc) ** 2 + (wa - wc) ** 2)
        e2 = d2 * torch.sqrt((ub - ua) ** 2 + (wb - wa) ** 2)
        depth = (e0 + e1 + e2) / (e0 / z[a] + e1 / z[b] + e2 / z[cc])
        depth = torch.where(inside, depth, torch.full_like(depth, float("inf")))
        dm, arg = depth.min(dim=1)
        out.append((dm.view(H, W), amb.view(H, W), depth, arg.view(H, W)))
    return out


def _random_triangles(n_small=400, n_large=12, seed=0):
    """Small triangles about random centres, and large ones (vertices 1.4 from the origin: tens of pixels wide); every vertex lies
    within 2 of the origin, so at least 0.5 in front of cameras at distance 2.5."""
    g = torch.Generator().manual_seed(seed)
    c = (torch.rand(n_small, 1, 3, generator=g) * 2 - 1) * 0.6
    small = c + (0.02 + 0.15 * torch.rand(n_small, 1, 1, generator=g)) * torch.randn(n_small, 3, 3, generator=g).clamp(-2, 2)
    large = 1.4 * torch.nn.functional.normalize(torch.randn(n_large, 3, 3, generator=g), dim=2)
    v = torch.cat([small, large]).reshape(-1, 3)
    return v.to(DEV), torch.arange(v.shape[0], device=DEV).view(-1, 3)


def _scenes():
    H, W = 64, 96
    R, T, K = _cameras(3, H, W, seed=1)
    tv, tf = _random_triangles()
    sv, sf = _sphere_mesh((0.05, -0.02, 0.03), 0.4, N=20)
    return H, W, R, T, K, [(tv, tf), (sv.contiguous(), sf.contiguous())]


def test_raster_matches_fp64_brute_force():
    from dynhor_amd.mesh_color import raster_depth, zbuf_depth
    H, W, R, T, K, meshes = _scenes()
    n_big = 0
    for verts, faces in meshes:
        zb = raster_depth(verts, faces, R, T, K, H, W)
        assert zb.dtype == torch.int64 and zb.shape == (3, H, W)
        d = zbuf_depth(zb)
        fid = (zb & 0xFFFFFFFF)
        ref = _raster_fp64(verts, faces, R, T, K, H, W)
        for f, (dm, amb, depth_all, _) in enumerate(ref):
            ok = ~amb
            empty = zb[f] == -1
            assert torch.equal(empty[ok], torch.isinf(dm)[ok]), int((empty[ok] != torch.isinf(dm)[ok]).sum())
            cov = ok & ~empty
            assert int(cov.sum()) > 200
            rel = ((d[f][cov].double() - dm[cov]) / dm[cov]).abs()
            assert float(rel.max()) < 1e-5, float(rel.max())
            # the stored face covers the pixel centre, at the minimum depth
            stored = depth_all.view(H, W, -1).gather(2, torch.where(empty, 0, fid[f]).unsqueeze(-1)).squeeze(-1)
            assert bool(torch.isfinite(stored[cov]).all())
            assert float(((stored[cov] - dm[cov]) / dm[cov]).abs().max()) < 1e-5
            assert int(amb.sum()) < 0.02 * H * W, int(amb.sum())
        # faces whose clipped pixel box exceeds 32 px (the wave phase) are among the stored faces
        v = verts.double()
        for f in range(3):
            c = v @ R[f].double().T + T[f].double()
            uw = (c @ K.double().T)[:, :2] / c[:, 2:3]
            tri = uw[faces]
            lo = torch.stack([tri[..., 0].min(1).values.clamp(min=0), tri[..., 1].min(1).values.clamp(min=0)], 1)
            hi = torch.stack([tri[..., 0].max(1).values.clamp(max=W - 1), tri[..., 1].max(1).values.clamp(max=H - 1)], 1)
            big = torch.zeros(faces.shape[0], dtype=torch.bool, device=DEV)
            big[((hi - lo) > 33).any(1)] = True
            n_big += int(big[fid[f][zb[f] != -1]].sum())
    assert n_big > 1000, n_big


def test_raster_is_reproducible_and_order_independent():
    from dynhor_amd.mesh_color import raster_depth
    H, W, R, T, K, meshes = _scenes()
    for verts, faces in meshes:
        a = raster_depth(verts, faces, R, T, K, H, W)
        assert torch.equal(a, raster_depth(verts, faces, R, T, K, H, W))
        perm = torch.randperm(faces.shape[0], generator=torch.Generator().manual_seed(5)).to(DEV)
        b = raster_depth(verts, faces[perm].contiguous(), R, T, K, H, W)
        assert torch.equal(a >> 32, b >> 32)
        hit = a != -1
        ida, idb = a & 0xFFFFFFFF, perm[(b & 0xFFFFFFFF).clamp(max=faces.shape[0] - 1)]
        diff = hit & (ida != idb)
        # only at exact depth ties, where the smaller index wins: each of the two faces alone gives the same depth there
        assert int(diff.sum()) < 0.01 * int(hit.sum())
        for f, y, x in diff.nonzero().tolist()[:20]:
            i, j = int(ida[f, y, x]), int(idb[f, y, x])
            assert i < j
            for k in (i, j):
                one = raster_depth(verts, faces[k:k + 1].contiguous(), R[f:f + 1].contiguous(), T[f:f + 1].contiguous(), K, H, W)
                assert int(one[0, y, x] >> 32) == int(a[f, y, x] >> 32)


# ------------------------------------------------------------------------------------------------ 2. bake vs fp64
def _bake_fp64(verts, normals, ds, zbuf, usable, depth_eps, min_cos, tol_px=1e-3):
    """(acc [V,4], n_views [V], ambiguous frames per vertex) in fp64 on the GPU z-buffer."""
    from dynhor_amd.mesh_color import zbuf_depth
    v, n = verts.double(), normals.double()
    F, H, W = usable.shape
    acc = torch.zeros(v.shape[0], 4, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(v.shape[0], dtype=torch.int64, device=DEV)
    amb = torch.zeros(v.shape[0], dtype=torch.int64, device=DEV)
    depth = zbuf_depth(zbuf).double()
    for f in range(F):
        Rf, Tf = ds.R[f].double(), ds.T[f].double()
        c = v @ Rf.T + Tf
        z = c[:, 2]
        u = (c @ ds.K[0].double()) / z + 0.5
        w = (c @ ds.K[1].double()) / z + 0.5
        near = lambda q: (q - q.round()).abs() < tol_px
        px, py = torch.floor(u), torch.floor(w)
        ins = (z > 1e-3) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
        pxi, pyi = torch.where(ins, px, 0).long(), torch.where(ins, py, 0).long()
        dz = depth[f, pyi, pxi]
        C = -(Rf.T @ Tf)
        dvec = C - v
        cs = (n * dvec).sum(1) / dvec.norm(dim=1)
        vis = ins & (usable[f, pyi, pxi] != 0) & (z <= dz + depth_eps) & (cs >= min_cos)
        a = (z.abs() < 1e-6) | ((z > 0) & (near(u) | near(w))) | (ins & ((z - dz - depth_eps).abs() < 1e-5)) | \
            ((cs - min_cos).abs() < 1e-6)
        rgb = ds.rgb[f, pyi, pxi].double() / 255.0
        acc[:, :3] += torch.where(vis[:, None], cs[:, None] * rgb, torch.zeros_like(rgb))
        acc[:, 3] += torch.where(vis, cs, torch.zeros_like(cs))
        cnt += vis
        amb += a
    return acc, cnt, amb


def test_bake_matches_fp64_and_chunking():
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.mesh_color import bake_vertex_colors, raster_depth, usable_map, vertex_normals
    from dynhor_amd import _lib
    from dynhor_amd.scene import scene_sdf
    ds = Dataset.from_synthetic(n_frames=7, H=96, W=128, seed=3, device=DEV, hand=True)
    verts, faces = _mesh_of(scene_sdf, N=96)
    normals = vertex_normals(verts, faces)
    zbuf = raster_depth(verts, faces, ds.R, ds.T, ds.K, ds.H, ds.W)
    usable = usable_map(ds.label, 1)
    assert torch.equal(usable.bool(), (ds.label == 1) & (torch.nn.functional.max_pool2d(
        (ds.label != 1).float()[:, None], 3, 1, 1)[:, 0] == 0))
    nv = verts.shape[0]
    acc = torch.zeros(nv, 4, device=DEV)
    cnt = torch.zeros(nv, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().dh_mesh_bake_colors(_lib.ptr(verts), _lib.ptr(normals), nv, _lib.ptr(ds.rgb), _lib.ptr(usable),
                                              _lib.ptr(zbuf), _lib.ptr(ds.R), _lib.ptr(ds.T), _lib.ptr(ds.K), ds.n_images, ds.H, ds.W,
                                              0.01, 0.1, _lib.ptr(acc), _lib.ptr(cnt), _lib.stream()))
    racc, rcnt, amb = _bake_fp64(verts, normals, ds, zbuf, usable, 0.01, 0.1)
    clear = amb == 0
    assert int(clear.sum()) > 0.9 * nv
    assert torch.equal(cnt.long()[clear], rcnt[clear]), int((cnt.long() != rcnt)[clear].sum())
    seen = clear & (rcnt > 0)
    assert int(seen.sum()) > 0.5 * nv
    got = acc[seen, :3].double() / acc[seen, 3:].double()
    ref = racc[seen, :3] / racc[seen, 3:]
    assert float((got - ref).abs().max()) < 1e-5
    assert float(((acc[seen, 3].double() - racc[seen, 3]) / racc[seen, 3]).abs().max()) < 1e-5
    # the wrapper: the same sums, and bitwise the same colours for every frame chunking
    runs = [bake_vertex_colors(verts, faces, ds, frame_chunk=k) for k in (1, 5, ds.n_images)]
    assert torch.equal(runs[0][2], cnt) and torch.equal(runs[0][1], acc[:, 3])
    for col, wt, nvw in runs[1:]:
        assert torch.equal(col.nan_to_num(-1), runs[0][0].nan_to_num(-1)) and torch.equal(wt, runs[0][1]) and torch.equal(nvw, cnt)
    assert bool(torch.isnan(runs[0][0][cnt == 0]).all()) and bool(torch.isfinite(runs[0][0][cnt > 0]).all())


def _mesh_of(sdf, N=128, lo=-0.55, hi=0.55):
    from dynhor_amd.mesh import marching_cubes
    ax = torch.linspace(lo, hi, N, device=DEV)
    gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
    p = torch.stack([gx, gy, gz], -1).reshape(-1, 3)
    return marching_cubes((-sdf(p)).view(N, N, N), 0.0, [lo] * 3, [hi] * 3)


# ------------------------------------------------------------------------------------------------ 3. occlusion
SPHERES = [((0.0, 0.0, 0.0), 0.28, (0.9, 0.1, 0.1)), ((0.45, 0.0, 0.0), 0.14, (0.1, 0.2, 0.9))]


def _two_sphere_dataset(n=40, H=96, W=96):
    """Ray-cast in torch: per pixel the nearest sphere hit, its constant colour, label 1; background 0 and grey."""
    from dynhor_amd.dataset import Dataset
    R, T, K = _cameras(n, H, W, seed=2)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, device=DEV)], -1).double()
    rgb = torch.zeros(n, H, W, 3, dtype=torch.uint8, device=DEV)
    label = torch.zeros(n, H, W, dtype=torch.int8, device=DEV)
    for f in range(n):
        d = torch.nn.functional.normalize(pix @ torch.inverse(K.double()).T, dim=1) @ R[f].double()
        o = -(R[f].double().T @ T[f].double())
        best = torch.full((H * W,), float("inf"), dtype=torch.float64, device=DEV)
        col = torch.full((H * W, 3), 0.05, dtype=torch.float64, device=DEV)
        for c, r, rgbc in SPHERES:
            oc = o - torch.tensor(c, dtype=torch.float64, device=DEV)
            b = d @ oc
            disc = b * b - (oc @ oc - r * r)
            t = -b - torch.sqrt(disc.clamp(min=0))
            hit = (disc > 0) & (t > 0) & (t < best)
            best = torch.where(hit, t, best)
            col[hit] = torch.tensor(rgbc, dtype=torch.float64, device=DEV)
        rgb[f] = (col * 255).round().to(torch.uint8).view(H, W, 3)
        label[f] = torch.isfinite(best).to(torch.int8).view(H, W)
    frames = {"rgb": rgb, "label": label, "normal": torch.full((n, H, W, 3), 128, dtype=torch.uint8, device=DEV), "R": R, "T": T, "K": K}
    return Dataset(frames=frames, device=DEV)


def test_occluded_vertices_take_no_front_colour():
    from dynhor_amd.mesh_color import bake_vertex_colors
    ds = _two_sphere_dataset()
    (ca, ra, col_a), (cb, rb, col_b) = SPHERES
    va, fa = _sphere_mesh(ca, ra, N=64)
    vb, fb = _sphere_mesh(cb, rb, N=48)
    verts = torch.cat([va, vb]).contiguous()
    faces = torch.cat([fa, fb + va.shape[0]]).contiguous()
    A, B = torch.tensor(col_a, device=DEV), torch.tensor(col_b, device=DEV)

    def closer_to_b(eps):
        col, _, n = bake_vertex_colors(verts, faces, ds, depth_eps=eps)
        ca_, na = col[:va.shape[0]], n[:va.shape[0]]
        seen = na > 0
        bad = seen & ((ca_ - B).norm(dim=1) < (ca_ - A).norm(dim=1))
        return int(seen.sum()), int(bad.sum())

    seen, bad = closer_to_b(0.01)
    assert seen > 0.8 * va.shape[0] and bad == 0, (seen, bad)
    seen_inf, bad_inf = closer_to_b(float("inf"))
    assert bad_inf > 50, bad_inf                          # without the depth test the same scene bleeds


# ------------------------------------------------------------------------------------------------ 4. hands
HAND = (0.85, 0.62, 0.50)


def test_hand_pixels_never_colour_the_object():
    """The synthetic sequence with and without hands (same cameras, same object pixels outside the hand) on the analytic mesh.
    Bound on how much a vertex's colour may differ between the two runs (or from the analytic diffuse colour), from scene.py's shading
    col = alb (0.25 + 0.75 lam) + 0.25 spec, clamped to [0, 1], with min_cos = 0.5:
      * the view-dependent specular term lies in [0, 0.25];
      * u8 rounding: 1/255 on each side;
      * the sampled surface point lies within half a pixel diagonal (0.71 px) of the vertex's projection; one pixel spans at most
        depth / f = 3.0 / 307.2 world units (cameras within 2.5 of the origin, object within 0.5), along the surface at most 1 / min_cos
        times that: rho = 0.71 * 3.0 / 307.2 / 0.5;  the diffuse part changes at most by rho (|grad alb| + 0.75 max(alb) kappa), with
        |grad alb| <= 0.35 * 21 and the curvature kappa <= 1 / 0.04 (the rounded box's edge radius)."""
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.mesh_color import bake_vertex_colors
    from dynhor_amd.runner import Runner
    from dynhor_amd.scene import _normal
    rho = 0.71 * 3.0 / (1.2 * 256) / 0.5
    bound = 0.25 + 2 / 255 + rho * (0.35 * 21 + 0.75 * 0.9 / 0.04)
    verts, faces = Runner._scene_gt_mesh(SimpleNamespace(device=DEV), 256)
    runs = {}
    for hand in (True, False):
        ds = Dataset.from_synthetic(n_frames=16, H=256, W=256, seed=21, device=DEV, hand=hand)
        runs[hand] = bake_vertex_colors(verts, faces, ds, min_cos=0.5)
    hcol = torch.tensor(HAND, device=DEV)
    near_hand = {h: int(((runs[h][0] - hcol).abs().max(dim=1).values < 0.05).sum()) for h in runs}
    assert near_hand[True] <= near_hand[False], near_hand
    both = (runs[True][2] > 0) & (runs[False][2] > 0)
    assert int(both.sum()) > 0.5 * verts.shape[0]
    diff = (runs[True][0][both] - runs[False][0][both]).abs().max()
    print(f"hand vs no hand: max |diff| {float(diff):.4f} (bound {bound:.4f}); vertices near the hand colour {near_hand}")
    assert float(diff) <= bound
    p = verts[both]
    alb = 0.55 + 0.35 * torch.sin(p * torch.tensor([21.0, 17.0, 13.0], device=DEV) + torch.tensor([0.0, 1.0, 2.0], device=DEV))
    light = torch.nn.functional.normalize(torch.tensor([0.4, -0.5, 0.8], device=DEV), dim=0)
    lam = (_normal(p) * light).sum(-1).clamp(min=0.0)[:, None]
    err = (runs[True][0][both] - alb * (0.25 + 0.75 * lam)).abs().max(dim=1).values
    print(f"median error against the analytic diffuse colour: {float(err.median()):.4f}")
    assert float(err.median()) <= bound


# ------------------------------------------------------------------------------------------------ 5. network mode
def _trained_runner(tmp_path, family):
    from dynhor_amd.runner import Runner
    conf = {"seq_name": "mcolor", "exp_name": family,
            "data_info": {"synthetic": {"n_frames": 3, "H": 64, "W": 64, "seed": 5}},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100},
            "model": {"family": family}}
    r = Runner(conf=conf, device="cuda:0", exp_root=str(tmp_path))
    r.train(3)
    return r


@pytest.mark.parametrize("family", ["neus", "hash"])
def test_network_colors_match_the_oracle(tmp_path, family):
    from dynhor_amd.mesh_color import network_vertex_colors
    from oracle import hashgrid_oracle as HO
    from oracle import neus_oracle as O
    r = _trained_runner(tmp_path, family)
    if family == "neus":
        o_sdf, o_col, _ = O.build_models(seed=1, device=r.device)
    else:
        o_sdf, o_col = HO.build_models(seed=1, device=r.device)
    o_sdf.load_state_dict(r.sdf_network.state_dict())
    o_col.load_state_dict(r.color_network.state_dict())
    g = torch.Generator().manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(3000, 3, generator=g), dim=1) * (0.2 + 0.3 * torch.rand(3000, 1, generator=g))
    verts = x.to(DEV).contiguous()
    got = network_vertex_colors(r.renderer, verts)

    def oracle(dtype):
        o_sdf.to(dtype); o_col.to(dtype)
        p = verts.to(dtype).clone()
        feat = o_sdf(p)[:, 1:].detach()
        grad = o_sdf.gradient(p).squeeze(1).detach()
        out = o_col(p.detach(), grad, -torch.nn.functional.normalize(grad, dim=1), feat).detach()
        o_sdf.float(); o_col.float()
        return out

    r64, r32 = oracle(torch.float64), oracle(torch.float32)
    e = float((got.double() - r64).abs().max())
    e32 = float((r32.double() - r64).abs().max())
    print(f"{family}: |hip-f64| {e:.3e}  |torch32-f64| {e32:.3e}")
    assert bool(torch.isfinite(got).all())
    if family == "neus":
        assert e < 2e-5 or e < 10 * e32                   # tests/test_gpu_mlp_forward.py, colour forward
    else:
        assert e < max(5e-4, 3 * e32)                     # tests/test_gpu_hash_family.py, finite-difference normals


# ------------------------------------------------------------------------------------------------ 6. Runner and CLI
def _conf(name):
    return {"seq_name": "mcolor", "exp_name": name,
            "data_info": {"synthetic": {"n_frames": 3, "H": 64, "W": 64, "seed": 5}},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100},
            "mesh_clean": {"dilate_px": 16}}


def test_runner_validate_mesh_with_colour(tmp_path):
    from dynhor_amd.mesh_color import bake_vertex_colors, network_vertex_colors
    from dynhor_amd.metrics import load_mesh
    from dynhor_amd.runner import Runner
    r = Runner(conf=_conf("runner"), device="cuda:0", exp_root=str(tmp_path))
    d = os.path.join(r.base_exp_dir, "meshes")
    r.validate_mesh(resolution=64, clean="mask+largest")
    raw, cleaned = (open(os.path.join(d, n), "rb").read() for n in ("00000000.ply", "00000000_clean.ply"))
    assert not os.path.exists(os.path.join(d, "00000000_color.ply")) and r.last_mesh_colors is None
    cv, cf = r.validate_mesh(resolution=64, clean="mask+largest", color="views+network")
    assert open(os.path.join(d, "00000000.ply"), "rb").read() == raw
    assert open(os.path.join(d, "00000000_clean.ply"), "rb").read() == cleaned
    lv, lf = load_mesh(os.path.join(d, "00000000_color.ply"))
    assert torch.equal(lv, cv.cpu()) and torch.equal(lf, cf.cpu())
    cols, st = r.last_mesh_colors, r.last_color_stats
    assert cols.dtype == torch.uint8 and cols.shape == cv.shape
    assert st["verts_in"] == cv.shape[0] and 0 <= st["unseen_verts"] < cv.shape[0] and st["mean_views"] >= 1.0
    # every vertex has a colour: the views where seen, the network elsewhere -- none NaN
    col, _, n = bake_vertex_colors(cv, cf, r.dataset)
    seen = n > 0
    assert int((~seen).sum()) == st["unseen_verts"]
    assert torch.equal(cols[seen], (col[seen].clamp(0, 1) * 255).round().to(torch.uint8))
    if st["unseen_verts"]:
        net = network_vertex_colors(r.renderer, cv[~seen].contiguous())
        assert bool(torch.isfinite(net).all())
        assert torch.equal(cols[~seen], (net.clamp(0, 1) * 255).round().to(torch.uint8))
    body = open(os.path.join(d, "00000000_color.ply"), "rb").read().split(b"end_header\n", 1)[1]
    rec = np.frombuffer(body, dtype=[("p", "<f4", (3,)), ("c", "u1", (3,))], count=cv.shape[0])
    np.testing.assert_array_equal(rec["c"], cols.cpu().numpy())
    r.close()


def test_cli_validate_mesh_prints_colour_stats(tmp_path):
    import yaml
    from dynhor_amd.runner import Runner
    conf = _conf("cli")
    r = Runner(conf=conf, device="cuda:0", exp_root=str(tmp_path))
    r.train(2)
    r.save_checkpoint()
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--mode", "validate_mesh", "--is_continue",
                        "--exp_root", str(tmp_path), "--mesh_clean", "mask+largest", "--mesh_color", "views+network"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("mesh_color views+network:")]
    assert len(lines) == 1, p.stdout
    assert os.path.exists(os.path.join(r.base_exp_dir, "meshes", "00000002_color.ply"))
