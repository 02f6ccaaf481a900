"""Texture atlas on the GPU: dh_texture_bake against its fp64 restatement (tests/mesh_texture_util.py, on the GPU's own z-buffer) and
across frame chunkings, occlusion and hand labels, faces the kernel must leave alone, dh_mesh_shade_tex against fp64 with its integer
error sums, the end-to-end re-render PSNR on an analytic sphere, and Runner.validate_mesh / visualize_mesh / the CLI."""
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_texture_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def bake_case():
    """The bake scene on the device with its atlas, the GPU z-buffer and usable map, and the fp64 restatement of the bake: computed
    once, shared, never modified."""
    from dynhor_amd.mesh_color import raster_depth, usable_map, vertex_normals
    from dynhor_amd.mesh_texture import face_atlas
    verts, faces, ds = U.bake_scene(DEV)
    S = U.atlas_size_with_margin(faces.shape[0])
    uv, owner, info = face_atlas(faces.shape[0], S, device=DEV)
    normals = vertex_normals(verts, faces)
    zbuf = raster_depth(verts, faces, ds.R, ds.T, ds.K, ds.H, ds.W)
    usable = usable_map(ds.label, 1)
    ref = U.bake_fp64(verts, normals, faces, uv, owner, ds.rgb, usable, zbuf, ds.R, ds.T, ds.K)
    return dict(verts=verts, faces=faces, ds=ds, S=S, uv=uv, owner=owner, info=info, normals=normals, zbuf=zbuf, usable=usable, ref=ref)


# ------------------------------------------------------------------------------------------------ 1. bake vs fp64
def test_bake_matches_fp64(bake_case):
    """acc.rgb / acc.w within 1e-5 of the restatement: a texel's mean takes at most F + 8 fp32 roundings of values <= 1 (the fetch, the
    weight, one fma per frame, the division), below 2e-6 for the frames that can see one texel here (<= 3 of the 5), times a margin of
    5.  n_views equal.  Only the texels the restatement calls ambiguous (a decision within its tolerance of its threshold) are left
    out, fewer than 2 % of those worked on."""
    from dynhor_amd.mesh_texture import bake_texture_sums
    c = bake_case
    ds, S, owner = c["ds"], c["S"], c["owner"]
    assert c["faces"].shape[0] % 2 == 1 and c["info"]["cells_per_side"] * c["info"]["cell"] < S and (S * S) % 256 != 0
    assert torch.equal(c["usable"], U.erode_object(ds.label, 1))
    acc, cnt = bake_texture_sums(c["verts"], c["faces"], ds, c["uv"], owner, frame_chunk=ds.n_images)
    racc, rcnt, amb, worked = c["ref"]
    assert torch.equal(worked, owner >= 0)
    clear = worked & ~amb
    share = int((worked & amb).sum()) / int(worked.sum())
    seen = clear & (rcnt > 0)
    got = acc[seen][:, :3].double() / acc[seen][:, 3:].double()
    ref = racc[seen][:, :3] / racc[seen][:, 3:]
    err = float((got - ref).abs().max())
    werr = float(((acc[seen][:, 3].double() - racc[seen][:, 3]) / racc[seen][:, 3]).abs().max())
    wrong = int((cnt.long() != rcnt)[clear].sum())
    print(f"bake: S {S}, {int(worked.sum())} texels worked on, ambiguous {100 * share:.3f} %, seen {int(seen.sum())}, max |colour error| "
          f"{err:.3e}, max relative weight error {werr:.3e}, n_views differing on clear texels {wrong}")
    assert share < 0.02
    assert int(seen.sum()) > 0.5 * int(worked.sum())
    assert wrong == 0
    assert err < 1e-5
    assert werr < 1e-5
    # texels no face owns are never written
    assert bool((acc[~worked] == 0).all()) and bool((cnt[~worked] == 0).all())
    # the u8 texture is within one level
    tex = U.texture_from_sums(acc, cnt, owner)
    rtex = U.texture_from_sums(racc, rcnt, owner)
    assert int((tex.int() - rtex.int()).abs()[clear].max()) <= 1


# ------------------------------------------------------------------------------------------------ 2. bitwise
def test_bake_is_bitwise_identical_for_every_chunking(bake_case):
    from dynhor_amd.mesh_texture import bake_texture, bake_texture_sums
    c = bake_case
    ds = c["ds"]
    runs = [bake_texture_sums(c["verts"], c["faces"], ds, c["uv"], c["owner"], frame_chunk=k) for k in (1, 2, ds.n_images, ds.n_images)]
    for acc, cnt in runs[1:]:
        assert torch.equal(acc.view(torch.int32), runs[0][0].view(torch.int32)) and torch.equal(cnt, runs[0][1])
    texs = [bake_texture(c["verts"], c["faces"], ds, size=c["S"], frame_chunk=k) for k in (1, 2, ds.n_images, ds.n_images)]
    for tex, uv, owner, st in texs:
        assert torch.equal(tex, texs[0][0]) and torch.equal(uv, c["uv"]) and torch.equal(owner, c["owner"]) and st == texs[0][3]
    assert torch.equal(texs[0][0], U.texture_from_sums(runs[0][0], runs[0][1], c["owner"]))
    st = texs[0][3]
    seen = runs[0][1] > 0
    assert st["unseen_texels"] == int(((c["owner"] >= 0) & ~seen).sum()) and st["mean_views"] == pytest.approx(
        float(runs[0][1][seen].double().mean()))
    assert st["size"] == c["S"] and st["faces"] == c["faces"].shape[0] and st["mode"] == "views"


# ------------------------------------------------------------------------------------------------ 3. occlusion and labels
FRONT = ((0.0, 0.0, 0.0), 0.28)
BACK = ((0.6, 0.0, 0.0), 0.12)


def _two_sphere_case():
    """A large sphere at the origin and a small one beside it.  Four cameras look across the axis through both centres and see the two
    side by side, 6 px of background apart; one camera looks along the axis, from where the large sphere hides the small one entirely.
    Frames by ray casting: red where the large (front) sphere is seen, blue where the small (back) one is; a band of hand pixels (-1)
    across the frames of the side views is painted pure green.  (The views are chosen so that no frame shows the back sphere partly hidden: the depth
    test is made at the nearest pixel, and the bilinear fetch of a texel within a pixel of an occlusion boundary takes up to 3/4 of
    its weight from the occluder's pixels -- DESIGN_NEXT_ROWS.md states that limit.)"""
    H, W = 64, 96
    K = U.cameras(1, H, W)[2].to(DEV)
    poses = [U.camera_at(p, DEV) for p in ((0.3, 2.5, 0.0), (0.3, -2.5, 0.0), (0.3, 0.0, 2.5), (0.3, 0.1, -2.5), (-2.5, 0.0, 0.0))]
    R, T = torch.cat([p[0] for p in poses]).contiguous(), torch.cat([p[1] for p in poses]).contiguous()
    F = R.shape[0]
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, device=DEV)], -1).double()
    rgb = torch.zeros(F, H, W, 3, dtype=torch.uint8, device=DEV)
    label = torch.zeros(F, H, W, dtype=torch.int8, device=DEV)
    for f in range(F):
        d = torch.nn.functional.normalize(pix @ torch.inverse(K.double()).T, dim=1) @ R[f].double()
        o = -(R[f].double().T @ T[f].double())
        best = torch.full((H * W,), float("inf"), dtype=torch.float64, device=DEV)
        col = torch.zeros(H * W, 3, dtype=torch.uint8, device=DEV)
        for (cen, r), c in ((FRONT, (230, 0, 25)), (BACK, (25, 0, 230))):
            oc = o - torch.tensor(cen, dtype=torch.float64, device=DEV)
            b = d @ oc
            disc = b * b - (oc @ oc - r * r)
            t = -b - torch.sqrt(disc.clamp(min=0))
            hit = (disc > 0) & (t > 0) & (t < best)
            best = torch.where(hit, t, best)
            col[hit] = torch.tensor(c, dtype=torch.uint8, device=DEV)
        rgb[f] = col.view(H, W, 3)
        label[f] = torch.isfinite(best).to(torch.int8).view(H, W)
    hand = torch.zeros(F, H, W, dtype=torch.bool, device=DEV)
    hand[:4, 25:28, :] = True
    rgb[hand] = torch.tensor((0, 255, 0), dtype=torch.uint8, device=DEV)
    label[hand] = -1
    va, fa = U.sphere_mesh(*FRONT, N=20, device=DEV)
    vb, fb = U.sphere_mesh(*BACK, N=20, device=DEV)
    verts = torch.cat([va, vb]).contiguous()
    faces = torch.cat([fa, fb + va.shape[0]]).contiguous()
    return verts, faces, fa.shape[0], U.Frames(rgb, label, R, T, K)


def test_occluded_texels_take_no_front_colour_and_hands_no_green():
    from dynhor_amd.mesh_texture import bake_texture
    verts, faces, n_front, ds = _two_sphere_case()
    assert int((ds.label == -1).sum()) > 500

    def back_texels(eps):
        tex, _, owner, st = bake_texture(verts, faces, ds, size=U.atlas_size_with_margin(faces.shape[0], cell=8), depth_eps=eps,
                                         sharpen=0)
        seen = (owner >= n_front) & (tex != 128).any(-1)
        red_above_blue = seen & (tex[..., 0] > tex[..., 2])
        return tex, owner, int(seen.sum()), int(red_above_blue.sum())

    tex, owner, seen, bad = back_texels(0.01)
    assert seen > 0.3 * int((owner >= n_front).sum()) and bad == 0, (seen, bad)
    front = (owner >= 0) & (owner < n_front) & (tex != 128).any(-1)
    assert int(front.sum()) > 0.5 * int(((owner >= 0) & (owner < n_front)).sum())
    assert bool((tex[front][:, 0] > tex[front][:, 2]).all())
    # hand pixels are pure green and nothing else has any: no texel gains green (unseen texels are 0.5 grey, unowned ones 0)
    assert int(tex[..., 1][(tex != 128).any(-1)].max()) == 0
    # without the depth test the hidden sphere turns red in the view along the axis: the test can fail
    _, _, _, bad_inf = back_texels(float("inf"))
    assert bad_inf > 50, bad_inf


def test_bad_faces_and_owners_leave_their_texels_untouched(bake_case):
    from dynhor_amd import _lib
    from dynhor_amd.mesh_color import raster_depth
    c = bake_case
    ds, S = c["ds"], c["S"]
    nv, nf = c["verts"].shape[0], c["faces"].shape[0]
    faces, uv, owner = c["faces"].clone(), c["uv"].clone(), c["owner"].clone()
    faces[5, 1] = nv + 7                                         # an index out of range
    faces[6, 0] = -1
    uv[9] = uv[9, 0]                                             # a UV triangle without area
    uv[10, 2] = 2 * uv[10, 1] - uv[10, 0]                        # ... and a collinear one
    own11 = owner == 11
    owner[own11] = nf + 3                                        # an owner that is no face
    dead = (c["owner"] == 5) | (c["owner"] == 6) | (c["owner"] == 9) | (c["owner"] == 10) | own11
    zbuf = raster_depth(c["verts"], faces, ds.R, ds.T, ds.K, ds.H, ds.W)
    acc = torch.full((S, S, 4), 7.0, device=DEV)
    cnt = torch.full((S, S), 3, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().dh_texture_bake(_lib.ptr(c["verts"]), _lib.ptr(c["normals"]), nv, _lib.ptr(faces), nf, _lib.ptr(uv),
                                          _lib.ptr(owner), S, _lib.ptr(ds.rgb), _lib.ptr(c["usable"]), _lib.ptr(zbuf), _lib.ptr(ds.R),
                                          _lib.ptr(ds.T), _lib.ptr(ds.K), ds.n_images, ds.H, ds.W, 0.01, 0.1, 2, _lib.ptr(acc),
                                          _lib.ptr(cnt), _lib.stream()))
    torch.cuda.synchronize()
    untouched = (acc == 7.0).all(-1) & (cnt == 3)
    assert bool(untouched[dead].all()) and bool(untouched[c["owner"] < 0].all())
    live = (c["owner"] >= 0) & ~dead
    assert int((cnt[live] > 3).sum()) > 0.5 * int(live.sum())
    assert bool(torch.isfinite(acc).all())


# ------------------------------------------------------------------------------------------------ 4. textured shade vs fp64
def test_shade_tex_matches_fp64_with_exact_sums(bake_case):
    """Every output byte within one level of the fp64 restatement (on the GPU's z-buffer) for lit 0 / 1 and alpha 1 / 0.6, with UV
    triangles that reach the texture's border (the clamp); sums equal to the integer sums of the kernel's own output; coverage
    identical to dh_mesh_shade's."""
    from dynhor_amd.mesh_texture import render_textured
    from dynhor_amd.mesh_vis import shade
    c = bake_case
    ds, S, verts, faces, normals, zbuf = c["ds"], c["S"], c["verts"], c["faces"], c["normals"], c["zbuf"]
    tex = U.smooth_noisy_frames(1, S, S, seed=11, device=DEV)[0].contiguous()
    uv = c["uv"].clone()
    big = torch.tensor([[[0.0, 0.0], [S, 0.0], [0.0, S]], [[S, S], [0.0, S], [S, 0.0]]], device=DEV)
    uv[0::7] = big[0]
    uv[3::7] = big[1]
    usable = c["usable"]
    for lit in (False, True):
        for alpha in (1.0, 0.6):
            out, sums = render_textured(verts, faces, zbuf, ds.R, ds.T, ds.K, uv, tex, normals=normals, rgb=ds.rgb, usable=usable,
                                        alpha=alpha, lit=lit)
            ref, cov = U.shade_tex_fp64(verts, normals, faces, uv, tex, zbuf, ds.R, ds.T, ds.K, rgb=ds.rgb, alpha=alpha, lit=lit)
            diff = (out.double() - torch.floor(ref + 0.5).clamp(0, 255)).abs()
            frac = (out.double() - ref).abs()
            print(f"shade_tex lit {int(lit)} alpha {alpha}: covered {int(cov.sum())}, max byte difference {int(diff.max())}, "
                  f"max |byte - 255 o| {float(frac.max()):.4f}")
            assert int(cov.sum()) > 2000
            assert int(diff.max()) <= 1
            assert torch.equal(out[~cov], ds.rgb[~cov])
            m = cov & (usable != 0)
            d = out.long() - ds.rgb.long()
            exp = torch.stack([((d * d).sum(-1) * m).sum((1, 2)), m.sum((1, 2))], 1)
            assert torch.equal(sums, exp) and int(exp[:, 1].sum()) > 1000
            out2, sums2 = render_textured(verts, faces, zbuf, ds.R, ds.T, ds.K, uv, tex, normals=normals, rgb=ds.rgb, usable=usable,
                                          alpha=alpha, lit=lit)
            assert torch.equal(out, out2) and torch.equal(sums, sums2)
    # coverage: dh_mesh_shade over black frames leaves exactly the uncovered pixels black, and counts them against all-object labels
    black = torch.zeros_like(ds.rgb)
    ones = torch.ones_like(ds.label)
    base, counts = shade(verts, faces, zbuf, ds.R, ds.T, ds.K, normals=normals, rgb=black, label=ones, alpha=1.0)
    white = torch.full((4, 4, 3), 255, dtype=torch.uint8, device=DEV)
    mine, msums = render_textured(verts, faces, zbuf, ds.R, ds.T, ds.K, uv, white, normals=normals, rgb=black,
                                  usable=torch.ones_like(usable))
    assert torch.equal(mine.any(-1), base.any(-1)) and torch.equal(mine.any(-1), cov)
    assert torch.equal(msums[:, 1], counts[:, 0])
    # without frames the background is white; without faces nothing is covered
    plain = render_textured(verts, faces, zbuf, ds.R, ds.T, ds.K, uv, tex, normals=normals)[0]
    assert bool((plain[~cov] == 255).all())
    none = render_textured(verts, faces[:0].contiguous(), zbuf, ds.R, ds.T, ds.K, uv[:0].contiguous(), tex, rgb=ds.rgb)[0]
    assert torch.equal(none, ds.rgb)


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_end_to_end_psnr():
    """A sphere whose colour is linear in position, 0.5 + 0.4 p / r, seen by five analytic frames; bake at S = 512, re-render unlit,
    PSNR over the covered usable pixels.

    Why the fp64 restatement must reach 40 dB (rms error 2.55 levels).  Three roundings to u8 lie between the analytic colour and
    the re-rendered byte (the frame, the texture, the output), each uniform within half a level: variance 3 / 12 level^2.  The N = 20
    marching-cubes sphere has edges of at most sqrt(3) h, h = 2.4 r / 19, so its faces lie at most (3 h^2 / 4) / (2 r) = 0.006 r
    inside the sphere (chordal sag); seen along a ray at cosine c to the normal the surface point moves by at most 0.006 r / c, and
    the colour, whose gradient is 0.4 / r per unit length, by 0.0024 / c = 0.61 / c levels: at most 6.1 levels at the bake's
    min_cos = 0.1 and, with the cos^4 weights and the one-pixel erosion of the labels, below one level rms.  The bilinear fetches add
    the curvature of a linear function over a sphere, (1/8) |second derivative| per pixel or texel squared, again below a level
    away from the eroded limb.  Together: rms below sqrt(0.25 + 1 + 1) = 1.5 levels, 44.6 dB; 40 dB leaves a factor 1.7.
    tests/test_cpu_mesh_texture.py confirms the bound for the restatement with an fp64 z-buffer (measured 58.7 dB).
    The GPU result must lie within 0.1 dB of the restatement on the GPU's z-buffer, and a constant grey texture at least 10 dB lower.
    Measured on MI355X: see DESIGN_NEXT_ROWS.md."""
    from dynhor_amd.mesh_color import raster_depth
    from dynhor_amd.mesh_texture import bake_texture, texture_psnr
    verts, faces, ds = U.e2e_scene(DEV)
    tex, uv, owner, st = bake_texture(verts, faces, ds, size=512)
    got = texture_psnr(verts, faces, ds, uv, tex)
    zbuf = raster_depth(verts, faces, ds.R, ds.T, ds.K, ds.H, ds.W)
    rtex, rimg, mask = U.e2e_restatement(verts, faces, ds, uv, owner, zbuf)
    ref, rsse, rcount = U.psnr(rimg, ds.rgb, mask)
    grey = texture_psnr(verts, faces, ds, uv, torch.full_like(tex, 128))
    print(f"end to end: GPU {got['pooled']:.3f} dB (sse {got['sse']}, {got['count']} pixels), fp64 restatement {ref:.3f} dB (sse {rsse}), "
          f"grey texture {grey['pooled']:.3f} dB; per frame {[round(x, 2) for x in got['frames']]}; texture bytes differing from the "
          f"restatement {int((tex != rtex).any(-1).sum())}, unseen texels {st['unseen_texels']}, views per seen texel {st['mean_views']:.2f}")
    assert got["count"] == rcount > 5000
    assert ref >= 40.0
    assert abs(got["pooled"] - ref) <= 0.1
    assert grey["pooled"] <= got["pooled"] - 10.0
    assert len(got["frames"]) == ds.n_images and all(p is not None for p in got["frames"])


# ------------------------------------------------------------------------------------------------ 6. Runner and CLI
def _conf(name):
    import yaml
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "synthetic.yaml")))
    conf.update(seq_name="mtex", exp_name=name)
    conf["data_info"]["synthetic"] = {"n_frames": 3, "H": 64, "W": 64, "seed": 5}
    conf["train"].update(batch_size=256, report_freq=10 ** 9, save_freq=10 ** 9, val_freq=0, end_iter=100)
    return conf


def test_cli_writes_the_textured_asset_and_it_loads_back(tmp_path):
    import yaml
    from dynhor_amd.mesh_color import raster_depth
    from dynhor_amd.mesh_texture import load_textured_obj, render_textured
    from dynhor_amd.runner import Runner
    conf = _conf("cli")
    r = Runner(conf=conf, device="cuda:0", exp_root=str(tmp_path))
    r.save_checkpoint()
    d = os.path.join(r.base_exp_dir, "meshes")
    # without the option: exactly the files as before
    r.validate_mesh(resolution=64, simplify="cells:16")
    assert sorted(os.listdir(d)) == ["00000000.ply", "00000000_simple.ply"] and r.last_texture is None
    before = {n: open(os.path.join(d, n), "rb").read() for n in os.listdir(d)}
    sv, sf = r.validate_mesh(resolution=64, simplify="cells:16", texture="views", texture_size=512, save=False)
    tex, uv, owner = r.last_texture
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--mode", "validate_mesh", "--is_continue",
                        "--exp_root", str(tmp_path), "--mesh_simplify", "cells:16", "--mesh_texture", "views", "--texture_size", "512"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("mesh_texture views:")]) == 1, p.stdout
    names = ["00000000_textured.obj", "00000000_textured.obj.mtl", "00000000_textured_texture_kd.png", "00000000_texture.json"]
    assert sorted(os.listdir(d)) == sorted(list(before) + names)
    for n, data in before.items():
        assert open(os.path.join(d, n), "rb").read() == data
    st = json.load(open(os.path.join(d, "00000000_texture.json")))
    assert st["mode"] == "views" and st["size"] == 512 and st["faces"] == sf.shape[0] and st["verts"] == sv.shape[0]
    mine = r.last_texture_stats
    assert st["unseen_texels"] == mine["unseen_texels"] and st["mean_views"] == pytest.approx(mine["mean_views"])
    assert len(st["frames"]) == 3 and st["frames"] == mine["frames"] and st["psnr"] == mine["psnr"] and st["psnr_pixels"] > 0
    # the files give the image the in-memory atlas gives
    lv, lf, luv, ltex = load_textured_obj(os.path.join(d, names[0]))
    assert torch.equal(lv, sv.cpu()) and torch.equal(lf, sf.cpu()) and torch.equal(luv, uv.cpu()) and torch.equal(ltex, tex.cpu())
    ds = r.dataset
    zbuf = raster_depth(sv, sf, ds.R, ds.T, ds.K, ds.H, ds.W)
    a = render_textured(sv, sf, zbuf, ds.R, ds.T, ds.K, uv, tex, rgb=ds.rgb)[0]
    b = render_textured(lv.to(DEV), lf.to(DEV), zbuf, ds.R, ds.T, ds.K, luv.to(DEV), ltex.to(DEV), rgb=ds.rgb)[0]
    assert torch.equal(a, b) and bool((a != ds.rgb).any())
    r.close()


def test_visualize_mesh_untextured_is_unchanged_and_textured_uses_the_texture(tmp_path):
    from PIL import Image
    from dynhor_amd.mesh import write_ply
    from dynhor_amd.mesh_color import raster_depth, vertex_normals
    from dynhor_amd.mesh_texture import render_textured, write_textured_obj
    from dynhor_amd.mesh_vis import shade
    from dynhor_amd.runner import Runner
    r = Runner(conf=_conf("vis"), device="cuda:0", exp_root=str(tmp_path))
    sv, sf = r.validate_mesh(resolution=64, simplify="cells:16", texture="views", texture_size=512, save=False)
    tex, uv, _ = r.last_texture
    ds = r.dataset
    zbuf = raster_depth(sv, sf, ds.R, ds.T, ds.K, ds.H, ds.W)

    def jpeg(img):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=95)
        return buf.getvalue()

    # an untextured mesh: the files are those of dh_mesh_shade called directly
    ply = str(tmp_path / "plain.ply")
    write_ply(ply, sv, sf)
    res = r.visualize_mesh(mesh=ply)
    assert "textured" not in res
    direct = shade(sv, sf, zbuf, ds.R, ds.T, ds.K, rgb=ds.rgb, label=ds.label, alpha=0.6)
    stems = list(ds.stems) if ds.stems is not None else ["%04d" % k for k in range(ds.n_images)]
    for k in range(ds.n_images):
        assert open(os.path.join(r.last_vis_dir, stems[k] + ".jpg"), "rb").read() == jpeg(direct[0][k].cpu().numpy())
    assert [fr["tp"] for fr in res["frames"]] == direct[1][:, 0].tolist()
    # a textured one: drawn through dh_mesh_shade_tex, lit; the same counts
    obj = str(tmp_path / "tex.obj")
    write_textured_obj(obj, sv, sf, uv, tex)
    res2 = r.visualize_mesh(mesh=obj)
    assert res2["textured"] is True and [fr["tp"] for fr in res2["frames"]] == [fr["tp"] for fr in res["frames"]]
    lit = render_textured(sv, sf, zbuf, ds.R, ds.T, ds.K, uv, tex, normals=vertex_normals(sv, sf), rgb=ds.rgb, alpha=0.6, lit=True)[0]
    for k in range(ds.n_images):
        assert open(os.path.join(r.last_vis_dir, stems[k] + ".jpg"), "rb").read() == jpeg(lit[k].cpu().numpy())
    assert bool((lit != direct[0]).any())
    r.close()
