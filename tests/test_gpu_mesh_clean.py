"""Mesh cleaning on the GPU: label dilation against a numpy max filter, the silhouette votes against an fp64 restatement (and the
round trip through dh_gen_rays), connected components against a numpy union-find, the pipeline on the synthetic scene with a floater,
and Runner.validate_mesh / evaluate_mesh / the CLI with cleaning on."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. dilation
def _max_filter(label, r):
    nz = label != 0
    F, H, W = nz.shape
    pad = np.zeros((F, H + 2 * r, W + 2 * r), dtype=bool)
    pad[:, r:r + H, r:r + W] = nz
    out = np.zeros_like(nz)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[:, dy:dy + H, dx:dx + W]
    return out.astype(np.uint8)


@pytest.mark.parametrize("radius", [0, 1, 3])
def test_dilation_equals_max_filter(radius):
    from dynhor_amd.mesh_clean import dilate_labels
    rng = np.random.default_rng(radius)
    # sparse non-background pixels, some on every image edge, so that clipped windows are exercised
    lab = np.where(rng.random((3, 37, 53)) < 0.04, rng.choice([-1, 1], size=(3, 37, 53)), 0).astype(np.int8)
    lab[0, 0, 0] = lab[1, 36, 52] = lab[2, 0, 52] = lab[2, 36, 0] = -1
    lab[1, 18, 0] = lab[1, 0, 26] = 1
    keep = dilate_labels(torch.from_numpy(lab).to(DEV), radius)
    assert keep.dtype == torch.uint8 and keep.shape == lab.shape
    np.testing.assert_array_equal(keep.cpu().numpy(), _max_filter(lab, radius))


# ------------------------------------------------------------------------------------------------ 2. votes
def _votes_fp64(verts, keep, R, T, K, tol_px=1e-3, tol_z=1e-6):
    """(bg, seen, ambiguous) per vertex in fp64: ambiguous = frames where the pixel coordinate + 0.5 lies within tol_px of an integer
    (a rounding boundary or the image edge) or |z| < tol_z -- the only frames where fp32 may decide differently."""
    v = verts.double().cpu().numpy()
    kp = keep.cpu().numpy()
    Rn, Tn, Kn = R.double().cpu().numpy().reshape(-1, 3, 3), T.double().cpu().numpy().reshape(-1, 3), K.double().cpu().numpy()
    F, H, W = kp.shape
    bg = np.zeros(len(v), np.int64)
    seen = np.zeros(len(v), np.int64)
    amb = np.zeros(len(v), np.int64)
    for f in range(F):
        c = v @ Rn[f].T + Tn[f]
        z = c[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (c @ Kn[0]) / z + 0.5
            w = (c @ Kn[1]) / z + 0.5
            near = lambda a: np.abs(a - np.round(a)) < tol_px
            a = (np.abs(z) < tol_z) | ((z > 0) & (near(u) | near(w)))
            px, py = np.floor(u), np.floor(w)
            ins = (z > 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
        pxi, pyi = np.where(ins, px, 0).astype(np.int64), np.where(ins, py, 0).astype(np.int64)
        seen += ins
        bg += ins & (kp[f, pyi, pxi] == 0)
        amb += a
    return bg, seen, amb


def _pixel_points(ds, f, px, py, depth):
    """Points that project exactly onto the centres of pixels (px, py) of frame f, at camera depth `depth`."""
    pix = torch.stack([px.double(), py.double(), torch.ones_like(px, dtype=torch.float64)], -1)
    xc = pix @ torch.inverse(ds.K.double()).T * depth[:, None]
    return ((xc - ds.T[f].double()) @ ds.R[f].double()).float()          # R^T (x_cam - T)


def test_votes_match_fp64_restatement():
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.mesh_clean import dilate_labels, mask_votes
    ds = Dataset.from_synthetic(n_frames=6, H=48, W=64, seed=11, device=DEV, hand=True)
    keep = dilate_labels(ds.label, 0)
    g = torch.Generator(device="cpu").manual_seed(3)
    pts = [torch.rand(4000, 3, generator=g) * 1.6 - 0.8,                    # in and around the object, some off-image
           torch.rand(500, 3, generator=g) * 10.0 - 5.0]                    # far away: behind cameras, outside images
    lab0 = ds.label[0].cpu()
    for value in (-1, 0, 1):                                                # exactly on pixel centres of hand / background / object
        yx = (lab0 == value).nonzero()
        assert yx.shape[0] > 0, value
        sel = yx[torch.randperm(yx.shape[0], generator=g)[:300]]
        depth = 1.5 + torch.rand(sel.shape[0], generator=g, dtype=torch.float64)
        pts.append(_pixel_points(ds, 0, sel[:, 1].to(DEV), sel[:, 0].to(DEV), depth.to(DEV)).cpu())
    cam = -(ds.T[1].double() @ ds.R[1].double())                            # camera 1's centre; points just behind it
    fwd = ds.R[1, 2].double()
    pts.append((cam[None] - fwd[None] * torch.linspace(1e-3, 1.0, 200, dtype=torch.float64, device=DEV)[:, None]).float().cpu())
    verts = torch.cat(pts).to(DEV).contiguous()
    bg, seen = mask_votes(verts, keep, ds.R, ds.T, ds.K)
    assert bg.dtype == seen.dtype == torch.int32
    rbg, rseen, amb = _votes_fp64(verts, keep, ds.R, ds.T, ds.K)
    dbg = np.abs(bg.cpu().numpy() - rbg)
    dseen = np.abs(seen.cpu().numpy() - rseen)
    assert (dbg <= amb).all() and (dseen <= amb).all(), (int((dbg > amb).sum()), int((dseen > amb).sum()))
    assert int(amb.sum()) < 0.01 * verts.shape[0] * ds.n_images, int(amb.sum())      # the exemption stays rare
    # the kinds of vertex the test means to cover all occur
    assert (rseen == 0).any() and (rseen == ds.n_images).any() and (rbg > 0).any()
    # reproducible
    bg2, seen2 = mask_votes(verts, keep, ds.R, ds.T, ds.K)
    assert torch.equal(bg, bg2) and torch.equal(seen, seen2)


def test_hand_pixels_never_vote_background():
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.mesh_clean import dilate_labels, mask_votes
    ds = Dataset.from_synthetic(n_frames=2, H=48, W=64, seed=11, device=DEV, hand=True)
    keep = dilate_labels(ds.label, 0)
    yx = (ds.label[0] == -1).nonzero()
    assert yx.shape[0] > 0
    v = _pixel_points(ds, 0, yx[:, 1], yx[:, 0], torch.full((yx.shape[0],), 2.0, dtype=torch.float64, device=DEV))
    bg, seen = mask_votes(v, keep[:1].contiguous(), ds.R[:1].contiguous(), ds.T[:1].contiguous(), ds.K)
    assert (seen == 1).all() and (bg == 0).all()


def test_rays_round_trip_to_their_pixels():
    """Points o + t d on the rays of dh_gen_rays through pixel (px, py) are seen in that frame at exactly (px, py): the pixel index is
    read back bit by bit through single-frame keep maps that hold one bit of y * W + x each."""
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.mesh_clean import mask_votes
    ds = Dataset.from_synthetic(n_frames=3, H=48, W=64, seed=11, device=DEV, hand=True)
    H, W = ds.H, ds.W
    lin = torch.arange(H * W, device=DEV)
    for f in range(ds.n_images):
        g = torch.Generator(device=DEV).manual_seed(f)
        px = torch.randint(0, W, (2000,), device=DEV, generator=g)
        py = torch.randint(0, H, (2000,), device=DEV, generator=g)
        rays = ds.gen_rays_at_pixels(f, px, py)
        t = 1.5 + torch.rand(2000, 1, device=DEV, generator=g)
        v = (rays[:, :3] + t * rays[:, 3:6]).contiguous()
        got = torch.zeros(2000, dtype=torch.int64, device=DEV)
        Rf, Tf = ds.R[f:f + 1].contiguous(), ds.T[f:f + 1].contiguous()
        for b in range(int(math.ceil(math.log2(H * W)))):
            keep = ((lin >> b) & 1).to(torch.uint8).view(1, H, W)
            bg, seen = mask_votes(v, keep, Rf, Tf, ds.K)
            assert (seen == 1).all()
            got |= (1 - bg.long()) << b
        assert torch.equal(got, py * W + px), int((got != py * W + px).sum())


# ------------------------------------------------------------------------------------------------ 3. components
def _components_ref(nv, faces):
    par = np.arange(nv)

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x

    for a, b, c in faces:
        for p, q in ((a, b), (a, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                par[max(rp, rq)] = min(rp, rq)
    return np.array([find(x) for x in range(nv)], dtype=np.int64)


def _random_mesh(seed, nv=6000, groups=400):
    rng = np.random.default_rng(seed)
    grp = rng.integers(0, groups, nv)
    faces = []
    for gi in range(groups):
        members = np.nonzero(grp == gi)[0]
        if len(members) < 2 or gi % 7 == 0:                    # every 7th group: isolated vertices only
            continue
        for _ in range(len(members)):
            faces.append(rng.choice(members, 3, replace=len(members) < 3))
    faces = np.array(faces, dtype=np.int64)
    faces = np.concatenate([faces, faces[:50], np.stack([faces[50:80, 0], faces[50:80, 0], faces[50:80, 1]], 1)])   # duplicates, degenerate
    return faces[rng.permutation(len(faces))]


@pytest.mark.parametrize("seed", [0, 1])
def test_components_match_union_find(seed):
    from dynhor_amd.mesh_clean import vertex_components
    nv = 6000
    faces = _random_mesh(seed, nv)
    ref = _components_ref(nv, faces)
    lab = vertex_components(nv, torch.from_numpy(faces).to(DEV))
    assert lab.dtype == torch.int32
    np.testing.assert_array_equal(lab.cpu().numpy(), ref)
    assert 100 < len(np.unique(ref)) < nv
    assert torch.equal(lab, vertex_components(nv, torch.from_numpy(faces).to(DEV)))   # two launches, the same bits


def test_components_without_faces():
    from dynhor_amd.mesh_clean import vertex_components
    lab = vertex_components(1000, torch.zeros(0, 3, dtype=torch.int64, device=DEV))
    assert torch.equal(lab.cpu(), torch.arange(1000, dtype=torch.int32))


def test_components_of_a_million_vertex_path():
    from dynhor_amd.mesh_clean import vertex_components
    n = 1_000_000
    i = torch.arange(n - 1, device=DEV)
    path = torch.stack([i, i + 1, i + 1], 1)
    lab = vertex_components(n, path)
    assert int(lab.max()) == 0 and int(lab.min()) == 0
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(DEV)      # the same path through shuffled indices
    shuffled = perm[path]
    lab = vertex_components(n, shuffled)
    assert int(lab.max()) == 0
    assert torch.equal(lab, vertex_components(n, shuffled))


def test_keep_components_picks_largest_area_and_compacts():
    from dynhor_amd.mesh_clean import keep_components
    tri = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    # component A (vertices 0..2, area 0.5), an isolated vertex 3, component B (4..6, area 2), component C (7..9, area 0.5 x 1.44)
    verts = torch.cat([tri, torch.tensor([[5.0, 5, 5]]), tri * 2 + 3, tri * 1.2 - 3]).to(DEV)
    faces = torch.tensor([[0, 1, 2], [4, 5, 6], [7, 8, 9]], device=DEV)
    v, f = keep_components(verts, faces)
    assert torch.equal(v, verts[4:7]) and f.tolist() == [[0, 1, 2]]
    v, f = keep_components(verts, faces, min_area_frac=0.3)
    assert torch.equal(v, verts[[4, 5, 6, 7, 8, 9]]) and f.tolist() == [[0, 1, 2], [3, 4, 5]]
    # a tie goes to the smaller label
    v, f = keep_components(torch.cat([tri, tri + 4]).to(DEV), torch.tensor([[3, 4, 5], [0, 1, 2]], device=DEV))
    assert torch.equal(v, tri.to(DEV)) and f.tolist() == [[0, 1, 2]]


# ------------------------------------------------------------------------------------------------ 4. synthetic scene with a floater
FLOATER_C, FLOATER_R = (0.05, 0.0, 0.45), 0.04


def _mesh_of(sdf, N=512, chunk=1 << 22):
    from dynhor_amd.mesh import marching_cubes
    ax = torch.linspace(-0.55, 0.55, N, device=DEV)
    u = torch.empty(N * N * N, device=DEV)
    for s in range(0, N * N * N, chunk):
        i = torch.arange(s, min(s + chunk, N * N * N), device=DEV)
        p = torch.stack([ax[i // (N * N)], ax[(i // N) % N], ax[i % N]], dim=-1)
        u[s:s + i.shape[0]] = -sdf(p)
    return marching_cubes(u.view(N, N, N), 0.0, [-0.55] * 3, [0.55] * 3)


@pytest.fixture(scope="module")
def scene():
    from dynhor_amd.dataset import Dataset
    from dynhor_amd.scene import scene_sdf
    ds = Dataset.from_synthetic(device=DEV, hand=True)                       # 64 frames of 512 x 512
    c = torch.tensor(FLOATER_C, device=DEV)
    obj = _mesh_of(scene_sdf)
    both = _mesh_of(lambda p: torch.minimum(scene_sdf(p), torch.linalg.norm(p - c, dim=-1) - FLOATER_R))
    return ds, obj, both


def test_floater_projects_to_background(scene):
    ds, _, _ = scene
    c = torch.tensor(FLOATER_C, device=DEV)
    x = ds.R @ c + ds.T                                                         # [F,3]
    uv = (x @ ds.K.T)[:, :2] / x[:, 2:3]
    px, py = uv[:, 0].round().long(), uv[:, 1].round().long()
    ok = (x[:, 2] > 0) & (px >= 0) & (px < ds.W) & (py >= 0) & (py < ds.H)
    lab = ds.label[torch.arange(ds.n_images, device=DEV)[ok], py[ok], px[ok]]
    assert int((lab == 0).sum()) >= 1


def test_default_dilation_culls_no_object_vertex(scene):
    from dynhor_amd.mesh_clean import cull_by_masks, dilate_labels
    from dynhor_amd.runner import MESH_CLEAN_DEFAULTS
    ds, (ov, of), _ = scene
    culled = {}
    for r in range(4):
        v, _ = cull_by_masks(ov, of, dilate_labels(ds.label, r), ds.R, ds.T, ds.K)
        culled[r] = ov.shape[0] - v.shape[0]
    print(f"object vertices culled by dilation radius (of {ov.shape[0]}): {culled}")
    assert culled[MESH_CLEAN_DEFAULTS["dilate_px"]] == 0
    smallest_safe = min(r for r in culled if all(culled[q] == 0 for q in culled if q >= r))
    assert smallest_safe < MESH_CLEAN_DEFAULTS["dilate_px"], culled           # the default keeps a margin


@pytest.mark.parametrize("mode", ["mask", "largest", "mask+largest"])
def test_clean_removes_the_floater_exactly(scene, mode):
    from dynhor_amd.mesh_clean import clean_mesh
    from dynhor_amd.runner import MESH_CLEAN_DEFAULTS
    ds, (ov, of), (bv, bf) = scene
    assert bv.shape[0] > ov.shape[0] + 100
    v, f, st = clean_mesh(bv, bf, ds, mode, dilate_px=MESH_CLEAN_DEFAULTS["dilate_px"], min_bg_votes=1)
    assert torch.equal(v, ov) and torch.equal(f, of), (mode, st)
    assert st["removed_verts"] == bv.shape[0] - ov.shape[0] and st["removed_faces"] == bf.shape[0] - of.shape[0]
    assert st["components"] == (2 if mode == "largest" else 1), st          # the floater is its own component until culled


def test_clean_accuracy_equals_object_alone(scene):
    from dynhor_amd.mesh_clean import clean_mesh
    from dynhor_amd.metrics import mesh_metrics
    from dynhor_amd.scene import scene_sdf
    ds, (ov, of), (bv, bf) = scene
    v, f, _ = clean_mesh(bv, bf, ds, "mask+largest")
    gt_v, gt_f = _mesh_of(scene_sdf, N=256)
    a = mesh_metrics(v, f, gt_v, gt_f, n_samples=200_000, device=DEV)
    b = mesh_metrics(ov, of, gt_v, gt_f, n_samples=200_000, device=DEV)
    raw = mesh_metrics(bv, bf, gt_v, gt_f, n_samples=200_000, device=DEV)
    assert a["accuracy"] == b["accuracy"] and a["chamfer_l1"] == b["chamfer_l1"]
    assert raw["accuracy"] > a["accuracy"]


# ------------------------------------------------------------------------------------------------ 5. Runner and CLI
def _conf(name):
    return {"seq_name": "mclean", "exp_name": name,
            "data_info": {"synthetic": {"n_frames": 3, "H": 64, "W": 64, "seed": 5}},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100},
            # geometric initialisation is a rough sphere larger than the object: a wide dilation keeps part of it
            "mesh_clean": {"dilate_px": 16},
            "eval": {"n_samples": 50_000, "gt_resolution": 128}}


def test_runner_evaluate_and_validate_with_cleaning(tmp_path):
    from dynhor_amd.metrics import load_mesh
    from dynhor_amd.runner import Runner
    r = Runner(conf=_conf("runner"), device="cuda:0", exp_root=str(tmp_path))
    plain = r.evaluate_mesh(resolution=64, save=False)
    assert not any(k.startswith("clean") for k in plain)
    e = r.evaluate_mesh(resolution=64, clean="mask+largest", save=True)
    keys = ("clean", "clean_removed_verts", "clean_removed_faces", "clean_components")
    assert e["clean"] == "mask+largest" and all(isinstance(e[k], int) and e[k] >= 0 for k in keys[1:]), e
    assert e["clean_components"] >= 1 and math.isfinite(e["chamfer_l1"])
    assert e["n_pred_faces"] == plain["n_pred_faces"] - e["clean_removed_faces"]
    saved = json.load(open(os.path.join(r.base_exp_dir, "meshes", "{:0>8d}_eval.json".format(r.iter_step))))
    assert all(saved[k] == e[k] for k in keys)

    d = os.path.join(r.base_exp_dir, "meshes")
    raw_v, raw_f = r.validate_mesh(resolution=64)
    raw_bytes = open(os.path.join(d, "00000000.ply"), "rb").read()
    assert not os.path.exists(os.path.join(d, "00000000_clean.ply"))
    cv, cf = r.validate_mesh(resolution=64, clean="mask")
    assert open(os.path.join(d, "00000000.ply"), "rb").read() == raw_bytes
    lv, lf = load_mesh(os.path.join(d, "00000000_clean.ply"))
    assert torch.equal(lv, cv.cpu()) and torch.equal(lf, cf.cpu())
    assert cf.shape[0] == raw_f.shape[0] - r.last_clean_stats["removed_faces"]
    r.close()
    blob = b"".join(open(os.path.join(r.base_exp_dir, "board", fn), "rb").read() for fn in os.listdir(os.path.join(r.base_exp_dir, "board")))
    assert b"eval/clean_removed_verts" in blob


def test_cli_evaluate_mesh_with_cleaning(tmp_path):
    from dynhor_amd.runner import Runner
    conf = _conf("cli")
    r = Runner(conf=conf, device="cuda:0", exp_root=str(tmp_path))
    r.train(2)
    r.save_checkpoint()
    import yaml
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--mode", "evaluate_mesh", "--is_continue",
                        "--exp_root", str(tmp_path), "--mesh_resolution", "64", "--mesh_clean", "mask+largest"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["clean"] == "mask+largest" and out["iter"] == 2 and "clean_removed_verts" in out, out
