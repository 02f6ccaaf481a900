"""CPU: the face atlas' invariants, the textured OBJ writer and reader (V flip, Meshlab's dialect), the texture entry points'
declaration, export and host-side argument checks, the mesh_texture config block and CLI options, and what the fp64 restatements of
tests/mesh_texture_util.py promise on the GPU tests' own inputs (the share of ambiguous texels, the end-to-end PSNR)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_texture_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dh_texture_bake", "dh_mesh_shade_tex")
FACE_COUNTS = (1, 2, 3, 7, 8, 9, 5000)


# ------------------------------------------------------------------------------------------------ atlas
def _expected_owner(nf, size):
    """The layout of the issue, texel by texel in numpy: g = ceil(sqrt(ceil(nf / 2))) cells of c = size // g texels, face k in cell
    k // 2 (row-major), the cell split along its anti-diagonal; -1 outside the cells and in the unused half of an odd count."""
    g = math.ceil(math.sqrt(math.ceil(nf / 2)))
    while g * g < math.ceil(nf / 2):
        g += 1
    while g > 1 and (g - 1) * (g - 1) >= math.ceil(nf / 2):
        g -= 1
    c = size // g
    y, x = np.mgrid[0:size, 0:size]
    cell = (y // c) * g + x // c
    face = 2 * cell + ((x % c + y % c) >= c)
    return np.where((x < g * c) & (y < g * c) & (face < nf), face, -1), g, c


@pytest.mark.parametrize("nf", FACE_COUNTS)
def test_atlas_invariants(nf):
    from dynhor_amd.mesh_texture import MIN_CELL, atlas_min_size, face_atlas
    smallest = atlas_min_size(nf)
    for size in (smallest, smallest + 5):
        uv, owner, info = face_atlas(nf, size)
        assert uv.dtype == torch.float32 and tuple(uv.shape) == (nf, 3, 2)
        assert owner.dtype == torch.int32 and tuple(owner.shape) == (size, size)
        exp, g, c = _expected_owner(nf, size)
        assert (info["cells_per_side"], info["cell"]) == (g, c) and c >= MIN_CELL
        # (a) every texel has one owner, as laid out; -1 outside the cells and in the unused half
        np.testing.assert_array_equal(owner.numpy(), exp)
        assert bool((owner[g * c:, :] == -1).all()) and bool((owner[:, g * c:] == -1).all())
        counts = torch.bincount(owner[owner >= 0].long(), minlength=nf)
        assert int(counts.min()) >= c * (c - 1) // 2 and info["owned_texels"] == int(counts.sum())
        if nf % 2:
            cx, cy = ((nf - 1) // 2) % g, ((nf - 1) // 2) // g
            blk = owner[cy * c:(cy + 1) * c, cx * c:(cx + 1) * c]
            assert set(blk.unique().tolist()) == {-1, nf - 1}
        # (c) positive area, in the face's vertex order
        a, b, cc = uv[:, 0].double(), uv[:, 1].double(), uv[:, 2].double()
        area = (b[:, 0] - a[:, 0]) * (cc[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (cc[:, 0] - a[:, 0])
        assert float(area.min()) > 0
        # (b) every tap of a bilinear fetch at the corners, the edge midpoints and 1000 random interior points is the face's own
        gen = torch.Generator().manual_seed(nf)
        r = torch.rand(nf, 1000, 2, generator=gen, dtype=torch.float64)
        flip = r.sum(-1) > 1
        r = torch.where(flip[..., None], 1 - r, r)
        w = torch.cat([torch.stack([1 - r.sum(-1), r[..., 0], r[..., 1]], -1),
                       torch.tensor([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]],
                                    dtype=torch.float64).expand(nf, 6, 3)], 1)
        pts = (w[..., None] * uv.double()[:, None]).sum(-2)                   # [nf, 1006, 2]
        taps = U.bilinear_taps(pts[..., 0].reshape(-1), pts[..., 1].reshape(-1))
        assert int(taps.min()) >= 0 and int(taps.max()) < size
        got = owner[taps[..., 1], taps[..., 0]].view(nf, -1)
        assert bool((got == torch.arange(nf, dtype=torch.int32)[:, None]).all())
        # (d) a function of (nf, size) alone
        uv2, owner2, info2 = face_atlas(nf, size)
        assert torch.equal(uv, uv2) and torch.equal(owner, owner2) and info == info2
    with pytest.raises(ValueError) as e:
        face_atlas(nf, smallest - 1)
    msg = str(e.value)
    g1 = (smallest - 1) // MIN_CELL
    assert f"at most {2 * g1 * g1} faces" in msg and "--mesh_simplify" in msg and "--texture_size" in msg


# ------------------------------------------------------------------------------------------------ OBJ
def _two_faces():
    verts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0, 0.25], [1.0, 1.0, -0.125]])
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]])
    return verts, faces


@pytest.mark.parametrize("image", ["png", "jpg"])
def test_textured_obj_round_trip_and_v_flip(tmp_path, image):
    from PIL import Image
    from dynhor_amd.mesh_texture import load_textured_obj, write_textured_obj
    from dynhor_amd.metrics import load_mesh
    verts, faces = _two_faces()
    Sh, Sw = 8, 16
    tex = torch.zeros(Sh, Sw, 3, dtype=torch.uint8)
    tex[1, 3] = 255                                              # the marked texel: column 3, row 1 from the top
    uv = torch.tensor([[[3.5, 1.5], [12.0, 1.0], [1.0, 6.0]], [[15.0, 7.0], [4.0, 7.0], [15.0, 2.0]]])
    obj, mtl, img = write_textured_obj(str(tmp_path / "m.obj"), verts, faces, uv, tex, image=image)
    assert (obj, mtl, img) == (str(tmp_path / "m.obj"), str(tmp_path / "m.obj.mtl"), str(tmp_path / f"m_texture_kd.{image}"))
    text = open(obj).read().splitlines()
    assert "mtllib ./m.obj.mtl" in text and "usemtl material_0" in text
    assert [ln for ln in open(mtl).read().splitlines() if ln.startswith("map_Kd")] == [f"map_Kd m_texture_kd.{image}"]
    vts = [tuple(float(x) for x in ln.split()[1:]) for ln in text if ln.startswith("vt ")]
    fls = [ln for ln in text if ln.startswith("f ")]
    assert len(vts) == 6 and fls == ["f 1/1 2/2 3/3", "f 3/4 2/5 4/6"]
    # the first corner points at the marked texel's centre: v counts from the bottom of the image
    assert vts[0] == pytest.approx((3.5 / Sw, 1.0 - 1.5 / Sh), abs=1e-9)
    im = np.asarray(Image.open(img).convert("RGB"))
    assert im.shape == (Sh, Sw, 3)
    col, row_from_top = int(vts[0][0] * Sw), int((1.0 - vts[0][1]) * Sh)
    assert (col, row_from_top) == (3, 1) and im[row_from_top, col].min() > 128 and im[Sh - 1 - row_from_top, col].max() < 128
    lv, lf, luv, ltex = load_textured_obj(obj)
    assert torch.equal(lv, verts) and torch.equal(lf, faces) and torch.equal(luv, uv)
    assert ltex.dtype == torch.uint8 and tuple(ltex.shape) == (Sh, Sw, 3)
    if image == "png":
        assert torch.equal(ltex, tex)
    mv, mf = load_mesh(obj)                                      # the geometry reader is unchanged and reads the same mesh
    assert torch.equal(mv, verts) and torch.equal(mf, faces)
    with pytest.raises(ValueError):
        write_textured_obj(str(tmp_path / "m.ply"), verts, faces, uv, tex)
    with pytest.raises(ValueError):
        write_textured_obj(obj, verts, faces, uv, tex, image="bmp")
    with pytest.raises(ValueError):
        write_textured_obj(obj, verts, faces, uv[:1], tex)


def test_load_textured_obj_reads_the_meshlab_dialect(tmp_path):
    from PIL import Image
    from dynhor_amd.mesh_texture import load_textured_obj
    os.makedirs(tmp_path / "mat")
    tex = (np.arange(4 * 6 * 3) % 251).astype(np.uint8).reshape(4, 6, 3)
    Image.fromarray(tex).save(tmp_path / "mat" / "kd.png")
    (tmp_path / "mat" / "m.mtl").write_text("# Wavefront material file\nnewmtl material_0\nKa 0.2 0.2 0.2\nKd 1 1 1\nillum 2\n"
                                            "map_Kd kd.png\n")
    (tmp_path / "m.obj").write_text(
        "####\n# OBJ File Generated by Meshlab\n####\nmtllib ./mat/m.mtl\n"
        "vn 0 0 1\nv 0 0 0\nvn 0 0 1\nv 1 0 0\nvn 0 0 1\nv 1 1 0\nvn 0 0 1\nv 0 1 0\n"
        "usemtl material_0\n"
        "vt 0.0 0.0\nvt 1.0 0.0\nvt 1.0 1.0\nvt 0.0 1.0\n"
        "f 1/1/1 2/2/2 3/3/3 4/4/4\n"                            # a quad: fanned together with its vt
        "v 0.5 0.5 1  # apex\nvt 0.5 0.5\n"
        "f -5/-5/-4 -4/-4/-3 -1/-1/1\n")                         # relative indices
    v, f, uv, t = load_textured_obj(str(tmp_path / "m.obj"))
    assert tuple(v.shape) == (5, 3) and v[4].tolist() == [0.5, 0.5, 1.0]
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4]]
    assert torch.equal(t, torch.from_numpy(tex))
    Sh, Sw = 4, 6
    exp = [[[0, Sh], [Sw, Sh], [Sw, 0]], [[0, Sh], [Sw, 0], [0, 0]], [[0, Sh], [Sw, Sh], [Sw / 2, Sh / 2]]]
    assert uv.tolist() == exp
    # without an image the mesh still loads, without a texture; vt on some corners only is an error
    os.remove(tmp_path / "mat" / "kd.png")
    v2, f2, uv2, t2 = load_textured_obj(str(tmp_path / "m.obj"))
    assert torch.equal(v2, v) and torch.equal(f2, f) and uv2 is None and t2 is None
    (tmp_path / "plain.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert load_textured_obj(str(tmp_path / "plain.obj"))[2:] == (None, None)
    (tmp_path / "mixed.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2 3\n")
    with pytest.raises(ValueError):
        load_textured_obj(str(tmp_path / "mixed.obj"))


# ------------------------------------------------------------------------------------------------ entry points
def test_entry_points_declared_exported_and_bound(hiplib):
    from dynhor_amd import _lib
    header = open(os.path.join(ROOT, "include", "dynhor_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header, name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name


def _bake(hiplib, nv=4, nf=2, S=16, n_frames=3, H=8, W=8, eps=0.01, mc=0.1, sharpen=2, ptrs=False, acc=None):
    """dh_texture_bake with null pointers, or with dummy non-null addresses everywhere (nothing is launched: an argument is wrong)."""
    p = ctypes.c_void_p(4096) if ptrs else ctypes.c_void_p(0)
    a = p if acc is None else ctypes.c_void_p(acc)
    return hiplib.dh_texture_bake(p, p, nv, p, nf, p, p, S, p, p, p, p, p, p, n_frames, H, W, eps, mc, sharpen, a, p, None)


def _shade(hiplib, nv=4, nf=2, Sh=16, Sw=16, n_frames=2, H=8, W=8, alpha=0.5, lit=0, ptrs=False, rgb=False, usable=False, sums=False,
           out=None):
    p = ctypes.c_void_p(4096) if ptrs else ctypes.c_void_p(0)
    null = ctypes.c_void_p(0)
    o = p if out is None else ctypes.c_void_p(out)
    return hiplib.dh_mesh_shade_tex(p, p, nv, p, nf, p, p, Sh, Sw, p, p, p, p, n_frames, H, W, ctypes.c_void_p(1 << 20) if rgb else null,
                                    p if usable else null, alpha, lit, o, p if sums else null, None)


def test_entry_points_reject_bad_arguments_without_launching(hiplib):
    # empty inputs are no-ops
    assert _bake(hiplib, nf=0) == 0 and _bake(hiplib, S=0) == 0 and _bake(hiplib, n_frames=0) == 0
    assert _shade(hiplib, n_frames=0) == 0
    # null pointers, negative counts, empty images, bad thresholds
    assert _bake(hiplib) == -1
    for kw in ({"nv": -1}, {"nf": -1}, {"S": -1}, {"n_frames": -1}, {"H": 0}, {"W": 0}, {"eps": -0.01}, {"eps": float("nan")},
               {"mc": float("nan")}, {"sharpen": -1}, {"sharpen": 5}, {"acc": 4100}):
        assert _bake(hiplib, ptrs=True, **kw) == -1, kw
    assert _shade(hiplib) == -1
    for kw in ({"nv": -1}, {"nf": -1}, {"n_frames": -1}, {"H": 0}, {"W": 0}, {"alpha": -0.1}, {"alpha": 1.5}, {"alpha": float("nan")},
               {"lit": 2}, {"Sh": 0}, {"Sw": 0}, {"usable": True}, {"sums": True}, {"usable": True, "sums": True},
               {"rgb": True, "out": (1 << 20) + 3}):
        assert _shade(hiplib, ptrs=True, **kw) == -1, kw
    # owner is int32, the bake's grid is (S / 16)^2, pixel centres must be exact in fp32, the shade's grid is one-dimensional
    for kw in ({"nf": 1 << 31}, {"S": (1 << 15) + 1}, {"n_frames": 1 << 31}, {"W": (1 << 24) + 1}):
        assert _bake(hiplib, ptrs=True, **kw) == -2, kw
    for kw in ({"nf": 1 << 32}, {"n_frames": 1 << 31}, {"H": (1 << 24) + 1}, {"Sw": (1 << 24) + 1},
               {"n_frames": 1 << 22, "H": 1 << 10, "W": 1 << 10}):
        assert _shade(hiplib, ptrs=True, **kw) == -2, kw


def test_wrappers_reject_cpu_tensors_and_bad_modes():
    from dynhor_amd import _lib
    from dynhor_amd import mesh_texture as mt
    verts, faces = _two_faces()
    uv, owner, _ = mt.face_atlas(2, 16)
    ds = U.Frames(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.ones(1, 8, 8, dtype=torch.int8), torch.eye(3)[None],
                  torch.zeros(1, 3), torch.eye(3))
    with pytest.raises(_lib.DynhorHipError):
        mt.bake_texture(verts, faces, ds, size=16)
    with pytest.raises(_lib.DynhorHipError):
        mt.render_textured(verts, faces, torch.zeros(1, 8, 8, dtype=torch.int64), ds.R, ds.T, ds.K, uv, torch.zeros(16, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        mt.bake_texture(verts, faces, ds, mode="network")
    assert mt.bake_texture(verts, faces, ds, mode="none")[:3] == (None, None, None)
    assert mt.psnr_from_sums(0, 0) is None and mt.psnr_from_sums(0, 5) == float("inf")
    assert mt.psnr_from_sums(3 * 5, 5) == pytest.approx(10 * math.log10(255.0 ** 2))


# ------------------------------------------------------------------------------------------------ config and CLI
def test_runner_texture_config_defaults_and_checks():
    from dynhor_amd.runner import MESH_TEXTURE_DEFAULTS, Runner
    assert MESH_TEXTURE_DEFAULTS == {"mode": "none", "size": 1024, "erode_px": 1, "min_cos": 0.1, "depth_eps": 0.01, "sharpen": 2,
                                     "image": "png"}
    r = Runner.__new__(Runner)
    r.conf = {"mesh_texture": {"mode": "views", "size": 2048}}
    assert r._texture_conf() == dict(MESH_TEXTURE_DEFAULTS, mode="views", size=2048)
    assert r._texture_conf("views+network", 512)["mode"] == "views+network" and r._texture_conf(None, 512)["size"] == 512
    for bad in ({"mode": "network"}, {"size": 4}, {"size": 1.5}, {"sharpen": 5}, {"image": "bmp"}):
        r.conf = {"mesh_texture": bad}
        with pytest.raises(ValueError):
            r._texture_conf()
    r.conf = {}
    assert r._texture_conf()["mode"] == "none"


def test_cli_lists_mesh_texture():
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "{none,views,views+network}" in p.stdout.split("--mesh_texture", 1)[1]
    assert "--texture_size" in p.stdout


# ------------------------------------------------------------------------------------------------ the restatements' own promises
def test_restatement_excludes_few_texels_on_the_bake_scene():
    """tests/test_gpu_mesh_texture.py compares dh_texture_bake with bake_fp64 outside the texels bake_fp64 calls ambiguous; on that
    test's inputs, with the fp64 brute-force z-buffer in place of the GPU's, those are fewer than 2 % of the texels worked on, every
    branch of the rule is taken, and most texels see a view."""
    from dynhor_amd.mesh_color import vertex_normals
    from dynhor_amd.mesh_texture import face_atlas
    verts, faces, ds = U.bake_scene()
    assert faces.shape[0] % 2 == 1
    S = U.atlas_size_with_margin(faces.shape[0])
    assert (S * S) % 256 != 0
    uv, owner, info = face_atlas(faces.shape[0], S)
    assert info["cells_per_side"] * info["cell"] < S
    zbuf = U.raster_fp64(verts, faces, ds.R, ds.T, ds.K, ds.H, ds.W)
    usable = U.erode_object(ds.label, 1)
    acc, cnt, amb, worked = U.bake_fp64(verts, vertex_normals(verts, faces), faces, uv, owner, ds.rgb, usable, zbuf, ds.R, ds.T, ds.K)
    assert torch.equal(worked, owner >= 0)
    share = int(amb.sum()) / int(worked.sum())
    seen = int((cnt > 0).sum()) / int(worked.sum())
    print(f"bake scene: {faces.shape[0]} faces, S {S}, ambiguous {100 * share:.3f} %, seen {100 * seen:.1f} %, max views {int(cnt.max())}")
    assert share < 0.02
    assert seen > 0.6 and int(cnt.max()) >= 2
    # the camera inside the sphere: points behind it and points projecting outside the image
    idx, p, _ = U.texel_geometry64(verts, vertex_normals(verts, faces), faces, uv, owner)
    _, z, u, w = U.project64(p, ds.R[-1], ds.T[-1], ds.K)
    assert int((z <= 1e-3).sum()) > 100 and int(((z > 1e-3) & ((u < 0) | (u > ds.W - 1) | (w < 0) | (w > ds.H - 1))).sum()) > 100


def test_restatement_reaches_40_db_end_to_end():
    """The bound tests/test_gpu_mesh_texture.py::test_end_to_end_psnr derives, confirmed for the restatement alone (fp64 brute-force
    z-buffer): at least 40 dB, and a constant grey texture at least 10 dB below."""
    from dynhor_amd.mesh_texture import face_atlas
    verts, faces, ds = U.e2e_scene()
    uv, owner, _ = face_atlas(faces.shape[0], 512)
    zbuf = U.raster_fp64(verts, faces, ds.R, ds.T, ds.K, ds.H, ds.W)
    tex, img, mask = U.e2e_restatement(verts, faces, ds, uv, owner, zbuf)
    val, sse, count = U.psnr(img, ds.rgb, mask)
    from dynhor_amd.mesh_color import vertex_normals
    grey = torch.full_like(tex, 128)
    gimg, _ = U.shade_tex_fp64(verts, vertex_normals(verts, faces), faces, uv, grey, zbuf, ds.R, ds.T, ds.K, rgb=ds.rgb)
    gval = U.psnr(U.to_bytes(gimg), ds.rgb, mask)[0]
    print(f"end to end, fp64: {val:.2f} dB over {count} pixels (rms {math.sqrt(sse / (3 * count)):.3f} levels); grey {gval:.2f} dB")
    assert count > 5000
    assert val >= 40.0
    assert gval <= val - 10.0
