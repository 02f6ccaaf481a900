"""CPU: the fp64 restatement of the photometric pose term (tests/pose_photo_util.py) is licensed first -- the blur against closed
forms, the analytic gradient formulas against autograd, the Huber branches -- then measured: the share of ambiguous points on every
fixture and the convergence rows of DESIGN_NEXT_ROWS.md section 19 (a fine texture converges only coarse to fine).  Then the parts of
the feature that need no GPU: argument validation of both entry points through ctypes, the wrappers' refusal of CPU tensors, the point
sampler, the schedule, the config block and the CLI flag."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import mesh_texture_util as TU
from tests import pose_photo_util as U
from tests import pose_sil_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64

# DESIGN_NEXT_ROWS.md section 19: the largest final angle, in degrees, of the k = 30 scene refined coarse to fine by the restatement,
# as this file measures it (0.2737).  tests/test_gpu_pose_photo.py allows the product twice the value measured here.
K30_FINAL_DEG_RECORDED = 0.2737


def test_taps_sum_to_one_and_radius_zero_is_the_identity():
    from dynhor_amd.pose_photo import gaussian_taps
    for sigma in (0.0, 0.3, 1.0, 2.0, 4.0):
        g, r = U.taps(sigma)
        assert r == math.ceil(3 * sigma) and g.shape[0] == 2 * r + 1
        assert abs(float(g.double().sum()) - 1.0) < (2 * r + 1) * 2.0 ** -24
        assert torch.equal(g, g.flip(0)) and float(g[r]) == float(g.max())
        host, hr = gaussian_taps(sigma)
        assert hr == r and abs(math.fsum(host) - 1.0) < 1e-15
        assert torch.equal(torch.tensor(host, dtype=F64).float(), g)          # the host's taps are the restatement's
    rgb = TU.smooth_noisy_frames(2, 9, 13, seed=4)
    us = (torch.rand(2, 9, 13, generator=torch.Generator().manual_seed(1)) > 0.3).to(torch.uint8)
    out = U.blur(rgb, us, U.taps(0.0)[0])
    want = torch.cat([rgb.double() / 255.0 * us[..., None], us[..., None].double()], -1)
    assert torch.equal(out, want)


def test_blur_of_a_constant_image_is_that_constant_under_any_mask():
    g = torch.Generator().manual_seed(2)
    rgb = torch.empty(2, 11, 17, 3, dtype=torch.uint8)
    rgb[..., 0], rgb[..., 1], rgb[..., 2] = 37, 200, 255
    us = (torch.rand(2, 11, 17, generator=g) > 0.6).to(torch.uint8)
    us[1, :, :9] = 0
    for sigma in (0.5, 1.0, 4.0):                        # radius 12 exceeds the image height
        out = U.blur(rgb, us, U.taps(sigma)[0])
        a = out[..., 3]
        assert float(a.min()) >= 0 and float(a.max()) <= 1 + 1e-6
        want = torch.tensor([37, 200, 255], dtype=F64) / 255.0
        assert float((out[..., :3][a > 0] - want).abs().max()) < 1e-14
        assert float(out[..., :3][a == 0].abs().max() if bool((a == 0).any()) else 0.0) == 0.0
    # a one-pixel mask: a is the separable product of the taps around it
    us = torch.zeros(1, 11, 17, dtype=torch.uint8)
    us[0, 5, 8] = 1
    t, r = U.taps(1.0)
    out = U.blur(rgb[:1], us, t)
    assert torch.allclose(out[0, 5 - r:5 + r + 1, 8 - r:8 + r + 1, 3], torch.outer(t.double(), t.double()), rtol=0, atol=1e-16)


def test_huber_branches_are_continuous_and_the_derivative_is_the_clamp():
    d = 0.1
    for s in (-1.0, 1.0):
        x = torch.tensor([s * d * (1 - 1e-12), s * d, s * d * (1 + 1e-12)], dtype=F64)
        h = U.huber(x, d)
        assert float((h - 0.5 * d * d).abs().max()) < 1e-13
    x = torch.linspace(-0.5, 0.5, 1001, dtype=F64).requires_grad_(True)
    (g,) = torch.autograd.grad(U.huber(x, d).sum(), x)
    assert torch.allclose(g, U.huber_grad(x.detach(), d), rtol=0, atol=1e-16)
    assert float(U.huber(torch.tensor(0.3, dtype=F64), d)) == pytest.approx(d * (0.3 - d / 2), abs=1e-16)


def _bake_fixture(radius):
    verts, faces, ds = TU.bake_scene()
    from dynhor_amd.mesh_color import vertex_normals
    g = torch.Generator().manual_seed(11)
    pts = verts[torch.randint(0, verts.shape[0], (1500,), generator=g)] * (1 + 0.002 * torch.randn(1500, 1, generator=g))
    nrm = torch.nn.functional.normalize(pts - torch.tensor([0.05, -0.02, 0.03]), dim=1)
    col = torch.rand(1500, 3, generator=g)
    usable = TU.erode_object(ds.label, 1)
    sigma = radius / 3.0
    img = U.blur(ds.rgb, usable, U.taps(sigma)[0])
    zbuf = TU.raster_fp64(verts, faces, ds.R, ds.T, ds.K, ds.H, ds.W)
    return pts.float().contiguous(), nrm.float().contiguous(), col, img, zbuf, ds


@pytest.mark.parametrize("radius", [0, 3])
def test_analytic_gradient_equals_autograd_and_few_points_are_ambiguous(radius):
    pts, nrm, col, img, zbuf, ds = _bake_fixture(radius)
    amb = U.ambiguous(pts, nrm, img, zbuf, ds.R, ds.T, ds.K, 0.01, 0.2, 0.5)
    share = float(amb.double().mean())
    print(f"bake scene radius {radius}: ambiguous {int(amb.sum())} of {pts.shape[0]} ({100 * share:.3f} %)")
    assert share < U.AMBIGUOUS_CAP
    g = torch.Generator().manual_seed(3)
    R64 = torch.stack([ds.R[f].double() @ SU.axis_angle(torch.randn(3, generator=g, dtype=F64), 2.0) for f in range(ds.R.shape[0])])
    T64 = ds.T.double() + 0.01 * torch.randn(ds.T.shape, generator=g, dtype=F64)
    sums, absum = U.all_sums(pts, nrm, col, img, zbuf, R64, T64, ds.K)
    R64.requires_grad_(True); T64.requires_grad_(True)
    seen_kinds = 0
    for f in range(R64.shape[0]):
        num, den, n, inl = U.frame_loss(pts, nrm, col, img[f], zbuf[f], R64[f], T64[f], ds.K, 0.01, 0.2, 0.5, 0.1)
        assert n == int(sums[f, 14]) and inl == int(sums[f, 15]) and 0 <= inl <= n
        if n == 0:
            continue
        gR, gT = torch.autograd.grad(num, (R64, T64))
        got = sums[f, 2:14]
        want = torch.cat([gR[f].reshape(-1), gT[f]])
        assert float((got - want).abs().max()) <= 1e-12 * float(absum[f, 2:].max())
        assert abs(float(num.detach()) - float(sums[f, 0])) <= 1e-12 * float(absum[f, 0]) and abs(float(den) - float(sums[f, 1])) <= 1e-12 * n
        assert float(want.norm()) > 0
        seen_kinds += 1
    assert seen_kinds >= 4                                # the camera inside the sphere may see few points; the others all do
    # the scene reaches every reason for which a pair is dropped
    ok = torch.stack([U.decisions(pts, nrm, img[f], zbuf[f], ds.R[f].double(), ds.T[f].double(), ds.K, 0.01, 0.2, 0.5)[0]
                      for f in range(5)])
    assert 0 < int(ok.sum()) < ok.numel() and bool((~ok[4]).any())


def test_ambiguous_share_of_the_convergence_scene():
    sc = U.photo_scene(30, 10.0)
    verts, faces = TU.sphere_mesh((0.0, 0.0, 0.0), TU.SPHERE_R, N=20)
    zbuf = TU.raster_fp64(verts, faces, sc["R0"].float(), sc["T0"].float(), sc["K"], sc["H"], sc["W"])
    for sigma in (4.0, 0.0):
        img = U.blur(sc["rgb"], sc["usable"], U.taps(sigma)[0])
        amb = U.ambiguous(sc["pts"], sc["normals"], img, zbuf, sc["R0"], sc["T0"], sc["K"], 0.01, 0.2, 0.5)
        _, pairs = U.photo_loss(sc["pts"], sc["normals"], sc["colors"], img, zbuf, sc["R0"], sc["T0"], sc["K"])
        print(f"k = 30 scene sigma {sigma}: ambiguous {int(amb.sum())} of 4000, pairs per frame {pairs}")
        assert float(amb.double().mean()) < U.AMBIGUOUS_CAP
        assert min(pairs) > 500


ROWS = [  # (k, start angle, levels, iterations, converges)
    (0, 6.0, (2.0, 1.0, 0.0), 120, True),
    (12, 8.0, (4.0, 2.0, 1.0, 0.0), 160, True),
    (12, 8.0, (0.0,), 160, True),
    (30, 10.0, (4.0, 2.0, 1.0, 0.0), 160, True),
    (30, 10.0, (0.0,), 160, False),
]


@pytest.mark.parametrize("k,deg,levels,iters,converges", ROWS)
def test_convergence_rows_of_the_restatement(k, deg, levels, iters, converges):
    sc = U.photo_scene(k, deg)
    assert float((U.angles_deg(sc["R0"], sc["R_true"]) - deg).abs().max()) < 1e-3      # the true poses are fp32
    R, T = U.refine(sc, levels, iters)
    ang = U.angles_deg(R, sc["R_true"])
    dT = (T - sc["T_true"]).norm(dim=1)
    print(f"k {k} start {deg} levels {levels} x {iters}: final angles {[round(float(a), 4) for a in ang]} deg, "
          f"largest {float(ang.max()):.4f}, largest |dT| {float(dT.max()):.4f}")
    if converges:
        assert float(ang.max()) < 0.05 * deg                 # at least twenty times closer than the start
        if k == 30:
            assert float(ang.max()) == pytest.approx(K30_FINAL_DEG_RECORDED, abs=0.02)   # the number the GPU test's margin refers to
    else:
        assert float(ang.max()) > deg                        # the fine texture alone diverges


def test_entry_points_validate_their_arguments(hiplib):
    L = hiplib
    null, some, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    far = ctypes.c_void_p(1 << 40)
    # dh_image_blur(rgb, usable, n_frames, H, W, taps, radius, tmp, out, stream)
    assert L.dh_image_blur(null, null, 0, 4, 4, null, 1, null, null, null) == 0                     # n_frames == 0: a no-op
    assert L.dh_image_blur(null, null, 2, 4, 4, null, 1, null, null, null) == -1                    # null pointers
    assert L.dh_image_blur(some, some, 2, 4, 4, some, 1, null, far, null) == -1
    assert L.dh_image_blur(some, some, -1, 4, 4, some, 1, some, far, null) == -1
    assert L.dh_image_blur(some, some, 2, 0, 4, some, 1, some, far, null) == -1                     # H < 1
    assert L.dh_image_blur(some, some, 2, 4, 0, some, 1, some, far, null) == -1
    assert L.dh_image_blur(some, some, 2, 4, 4, some, -1, some, far, null) == -1
    assert L.dh_image_blur(some, some, 2, 4, 4, some, 1, odd, far, null) == -1                      # misaligned
    assert L.dh_image_blur(some, some, 2, 4, 4, some, 1, some, some, null) == -1                    # tmp overlaps out
    assert L.dh_image_blur(some, some, 2, 4, 4, some, 65, some, far, null) == -2                    # the row pass's LDS tile
    assert L.dh_image_blur(some, some, 1 << 30, 4, 4, some, 1, some, far, null) == -2
    # dh_photo_loss_grad(pts, normals, colors, n, img, zbuf, R, T, K, n_frames, H, W, depth_eps, min_cos, a_min, delta, out, ws, stream)
    assert L.dh_photo_loss_sums() == 16
    Wk = L.dh_photo_loss_grad_workspace
    assert Wk(3, 10) == 3 * 1 * 16 * 8 and Wk(2, 257) == 2 * 2 * 16 * 8 and Wk(2, 20000) == 2 * 64 * 16 * 8 and Wk(5, 0) == 5 * 16 * 8
    assert Wk(-1, 5) == -1 and Wk(5, -1) == -1 and Wk(5, 1 << 31) == -2 and Wk(70000, 5) == -2

    def call(n=10, frames=2, H=8, W=8, ptr=some, eps=0.01, mc=0.2, amin=0.5, delta=0.1, out=some, ws=some, img=some):
        return L.dh_photo_loss_grad(ptr, ptr, ptr, n, img, ptr, ptr, ptr, ptr, frames, H, W, eps, mc, amin, delta, out, ws, null)
    assert call(frames=0, ptr=null, out=null, ws=null, img=null) == 0                                 # n_frames == 0: a no-op
    assert call(ptr=null, img=null) == -1
    assert call(out=null) == -1 and call(ws=null) == -1 and call(ws=odd) == -1 and call(img=odd) == -1
    assert call(n=-1) == -1 and call(frames=-2) == -1 and call(H=0) == -1 and call(W=0) == -1
    assert call(eps=float("nan")) == -1 and call(eps=-0.1) == -1 and call(mc=float("nan")) == -1
    assert call(amin=float("nan")) == -1 and call(amin=-1.0) == -1 and call(delta=float("nan")) == -1 and call(delta=0.0) == -1
    assert call(n=1 << 31) == -2 and call(frames=70000) == -2 and call(H=(1 << 24) + 1) == -2


def test_wrappers_refuse_cpu_tensors():
    from dynhor_amd import _lib, pose_photo
    rgb, us = torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.ones(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(_lib.DynhorHipError):
        pose_photo.blur_frames(rgb, us, 1.0)
    p = torch.zeros(3, 3)
    with pytest.raises(_lib.DynhorHipError):
        pose_photo.photo_sums(p, p, p, torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), torch.eye(3)[None],
                              torch.zeros(1, 3), torch.eye(3))
    with pytest.raises(_lib.DynhorHipError):
        pose_photo.PhotometricTerm(p, p, p, rgb, us)
    with pytest.raises(ValueError):
        pose_photo.gaussian_taps(float("nan"))


def test_surface_points_interpolate_normals_and_colours():
    from dynhor_amd.pose_photo import surface_points
    verts, faces = TU.sphere_mesh((0.0, 0.0, 0.0), TU.SPHERE_R, N=16)
    vc = 0.5 + 0.4 * verts / TU.SPHERE_R
    pts, nrm, col = surface_points(verts, faces, 3000, 7, vertex_colors=vc)
    assert pts.shape == nrm.shape == col.shape == (3000, 3) and pts.dtype == nrm.dtype == col.dtype == torch.float32
    assert float((nrm.norm(dim=1) - 1).abs().max()) < 1e-6
    assert float((nrm * torch.nn.functional.normalize(pts, dim=1)).sum(1).min()) > 0.99       # the sphere's normal is radial
    assert float((col - (0.5 + 0.4 * pts / TU.SPHERE_R)).abs().max()) < 1e-5                  # a linear colour interpolates exactly
    again = surface_points(verts, faces, 3000, 7, vertex_colors=(vc * 255).round().to(torch.uint8))
    assert torch.equal(again[0], pts) and float((again[2] - col).abs().max()) <= 0.5 / 255 + 1e-6
    # a texture: every face's UV triangle lies in a texel of constant colour per face
    nf = faces.shape[0]
    S = 2 * math.isqrt(nf) + 4
    tex = torch.zeros(S, S, 3, dtype=torch.uint8)
    uv = torch.empty(nf, 3, 2)
    for i in range(nf):
        cx, cy = 1 + 2 * (i % (S // 2 - 1)), 1 + 2 * (i // (S // 2 - 1))
        tex[cy - 1:cy + 1, cx - 1:cx + 1] = torch.tensor([i % 251, (7 * i) % 251, 100], dtype=torch.uint8)
        uv[i] = torch.tensor([[cx, cy]] * 3, dtype=torch.float32)          # the corner shared by the four texels' centres' square
    tex = tex[:max(int(uv[..., 1].max()) + 2, 2)]
    p2, _, c2 = surface_points(verts, faces, 500, 9, uv=uv, texture=tex)
    from dynhor_amd.metrics import sample_surface
    fi = sample_surface(verts, faces, 500, 9, return_faces=True)[2]
    want = torch.stack([fi % 251, (7 * fi) % 251, torch.full_like(fi, 100)], 1).float() / 255.0
    assert float((c2 - want).abs().max()) < 1e-6
    with pytest.raises(ValueError):
        surface_points(verts, faces, 10, 0)
    with pytest.raises(ValueError):
        surface_points(verts, faces, 10, 0, vertex_colors=vc, uv=uv, texture=tex)


def test_level_schedule_and_config_block():
    import yaml
    from dynhor_amd.pose_photo import DEFAULTS, MODES, level_at
    from dynhor_amd.runner import DEFAULT_CONF, _merge
    lv = (4.0, 2.0, 1.0, 0.0)
    assert [level_at(k, 160, lv) for k in (0, 39, 40, 119, 120, 159)] == [4.0, 4.0, 2.0, 1.0, 0.0, 0.0]
    assert [level_at(k, 5, (2.0, 0.0)) for k in range(5)] == [2.0, 2.0, 2.0, 0.0, 0.0] and level_at(0, 1, (3.0,)) == 3.0
    assert all(level_at(k, 7, lv) == U.level_at(k, 7, lv) for k in range(7))
    assert set(DEFAULTS) == {"mode", "points", "levels", "lw_photo", "delta", "a_min", "min_cos", "depth_eps", "erode_px", "seed"}
    assert DEFAULTS["mode"] == "none" and DEFAULTS["points"] == 20000 and tuple(DEFAULTS["levels"]) == (2.0, 1.0, 0.0)
    assert (DEFAULTS["delta"], DEFAULTS["a_min"], DEFAULTS["min_cos"]) == (0.1, 0.5, 0.2)
    assert (DEFAULTS["depth_eps"], DEFAULTS["erode_px"]) == (0.01, 1)                    # bake_vertex_colors's
    assert MODES == ("none", "views", "mesh")
    assert DEFAULT_CONF["pose_photo"] == DEFAULTS
    conf = _merge(DEFAULT_CONF, yaml.safe_load(open(os.path.join(ROOT, "configs", "synthetic.yaml"))))
    assert conf["pose_photo"] == DEFAULTS
    assert _merge(DEFAULT_CONF, {"pose_photo": {"points": 7}})["pose_photo"]["points"] == 7


def test_cli_knows_the_flag():
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "--pose_photo" in p.stdout and "views" in p.stdout


def test_the_step_source_reads_nothing_back():
    """The source-level guard of tests/test_cpu_no_host_sync.py for what a step with the photometric term runs."""
    import inspect
    import re
    from dynhor_amd import pose_photo, pose_sil
    from tests.test_cpu_no_host_sync import FORBIDDEN
    for fn in (pose_photo.photo_sums, pose_photo.PhotometricTerm.sums, pose_photo.PhotometricTerm.add_grads, pose_sil.SilhouettePoseOptimizer.step,
               pose_sil.SilhouettePoseOptimizer.evaluate):
        src = re.sub(r'"""[\s\S]*?"""', "", inspect.getsource(fn))
        src = "\n".join(ln.split("#")[0] for ln in src.splitlines())
        for pat in FORBIDDEN:
            assert not re.search(pat, src), f"{fn.__qualname__} contains {pat}"
