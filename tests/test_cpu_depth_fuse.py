"""Depth fusion without a GPU (dynhor_amd/depth_fuse.py, csrc/tsdf.hip): the fixture of the kernel's GPU test priced in float32 against
fp64 (tests/depth_fuse_util.py), the dented sphere fused in fp64 against its hull, the frame whose depth is off found by its residual,
the settings, the CLI, the entry point's argument rules through ctypes and the plain-torch parts on CPU tensors.

Observed (fp64 restatement, 64^3 over [-0.7, 0.7]^3, trunc 4 cells, prior_weight 255): dent median of the fused crossings 0.0123
(95th percentile 0.0166) against the hull's 0.1135 (0.2121): 9.2 x; no fused crossing outside the dent further than 0.0132 from the
surface (cell 0.0222).  Frame 3 scaled by 1.03: residual median 0.0249 against at most 0.0043 for the others.  Kernel fixture: 16,007
points x 6 frames, 0.38 % of the pairs ambiguous, max |q32 - q64| = 1."""
import ctypes
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import depth_fuse_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the kernel's fixture
def test_float32_restatement_agrees_with_fp64_on_the_kernel_fixture():
    fx = U.kernel_fixture()
    r = U.fixture_references(fx)
    v64, v32, amb = r["v64"], r["v32"], r["amb"]
    share = float(amb.mean())
    print(f"{fx['pts'].shape[0]} points x {amb.shape[0]} frames: {100 * share:.3f} % of the pairs ambiguous; max |q32 - q64| = {r['dq']}; "
          f"{100 * v64['ok'].mean():.1f} % of the pairs contribute")
    assert share <= 0.01                                             # a condition on the fixture
    assert np.array_equal(v64["ok"][~amb], v32["ok"][~amb]) and np.array_equal(v64["wt"][~amb], v32["wt"][~amb])
    assert 1 <= r["dq"] <= 4                                         # rounding of d / trunc 65536 at |d| <= trunc = 0.05, z about 1.8
    assert int(np.abs(v64["q"]).max()) == U.Q_ONE and int(v64["q"].min()) >= -U.Q_ONE
    # every kind of pair is present: hidden, far in front (q = 65536), inside the band, weights 1 and 255, no weight, no depth
    ok = v64["ok"]
    assert int((ok & (v64["q"] == U.Q_ONE)).sum()) > 500 and int((ok & (np.abs(v64["q"]) < U.Q_ONE)).sum()) > 3000
    assert int((ok & (v64["wt"] == 1)).sum()) > 100 and int((ok & (v64["wt"] == 255)).sum()) > 100
    with np.errstate(invalid="ignore"):
        assert int((~ok & (v64["d"] < -fx["trunc"])).sum()) > 1000 and int((~ok & ~np.isfinite(v64["zd"]) & (v64["wt"] > 0)).sum()) > 1000
    num, den, obs = U.state(v64)
    assert int(obs.max()) >= 3 and int((obs == 0).sum()) > 1000 and int(np.abs(num).max()) <= 255 * U.Q_ONE * 6


# ------------------------------------------------------------------------------------------------------------ the scene in fp64
@functools.lru_cache(maxsize=None)
def _scene():
    sc = U.scene_inputs()
    pts = U.grid_points(U.SCENE_LO, U.SCENE_HI, U.SCENE_N)
    h = U.scene_hull_field(sc, pts)
    fld, trunc, cell = U.scene_fusion(sc, h)
    return sc, h, fld, trunc, cell


def test_fused_dent_is_five_times_closer_than_the_hull():
    sc, h, fld, trunc, cell = _scene()
    N = U.SCENE_N
    fused = U.dent_stats(U.crossings(fld, U.SCENE_LO, U.SCENE_HI))
    hull = U.dent_stats(U.crossings(h.reshape(N, N, N), U.SCENE_LO, U.SCENE_HI))
    print(f"dent: fused median {fused[0]:.4f}, p95 {fused[1]:.4f} over {fused[2]} crossings; hull median {hull[0]:.4f}, p95 {hull[1]:.4f} "
          f"over {hull[2]}; ratio {hull[0] / fused[0]:.1f}; outside the dent the fused crossings are within {fused[3]:.4f} (cell {cell:.4f})")
    assert fused[2] > 100 and hull[2] > 100
    assert hull[0] >= 5.0 * fused[0]
    assert fused[3] <= cell                                          # the hull prior leaves no back face
    assert int(((fld > 0) & (h.reshape(N, N, N) <= 0)).sum()) > 0    # carved cells


def test_scaled_depth_map_is_the_worst_residual():
    sc, h, fld, trunc, cell = _scene()
    depth = sc["depth"].copy()
    depth[U.BAD_FRAME] *= np.float32(U.BAD_SCALE)
    bad = U.scene_fusion(sc, h, depth=depth)[0]
    med, cnt, worst = U.residuals(bad, U.SCENE_LO, U.SCENE_HI, trunc, depth, sc["weight"], sc["R"], sc["T"], sc["K"])
    med0, _, _ = U.residuals(fld, U.SCENE_LO, U.SCENE_HI, trunc, sc["depth"], sc["weight"], sc["R"], sc["T"], sc["K"])
    print(f"frame {U.BAD_FRAME} x {U.BAD_SCALE}: medians {[round(m, 4) for m in med]}, worst {worst}; unscaled {[round(m, 4) for m in med0]}")
    assert worst[0] == U.BAD_FRAME and len(worst) == 5 and min(cnt) > 1000
    assert med[U.BAD_FRAME] >= 3.0 * sorted(med)[-2]
    assert max(med0) < 0.5 * cell


# ------------------------------------------------------------------------------------------------------------ settings and CLI
def test_defaults_and_check_settings():
    from dynhor_amd import depth_fuse as df
    assert df.DEPTH_FUSE_DEFAULTS == {"resolution": 128, "trunc_cells": 4, "prior_weight": 255, "weight": "cos", "floor_weight": 64,
                                      "frame_chunk": 16, "point_chunk": 1 << 22}
    df.check_settings(dict(df.DEPTH_FUSE_DEFAULTS))
    df.check_settings(dict(df.DEPTH_FUSE_DEFAULTS, resolution=512, trunc_cells=2.5, prior_weight=510, weight="uniform", floor_weight=1))
    bad = {"resolution": (513, 1, 64.0, True), "trunc_cells": (0, -1, float("nan"), "4"), "prior_weight": (0, -255, float("inf"), None),
           "weight": ("sin", None, 1), "floor_weight": (0, 256, 1.5), "frame_chunk": (0, 1.5), "point_chunk": (0, -4)}
    for k, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=k):
                df.check_settings(dict(df.DEPTH_FUSE_DEFAULTS, **{k: v}))
    with pytest.raises(ValueError, match="unknown.*truncation"):
        df.check_settings(dict(df.DEPTH_FUSE_DEFAULTS, truncation=3))
    with pytest.raises(ValueError, match="missing.*prior_weight"):
        df.check_settings({k: v for k, v in df.DEPTH_FUSE_DEFAULTS.items() if k != "prior_weight"})


def test_merge_settings_and_the_yaml_block():
    from dynhor_amd import depth_fuse as df
    from dynhor_amd.runner import DEFAULT_CONF
    assert "depth_fuse" not in DEFAULT_CONF                                          # the block is optional
    c = df.merge_settings({"resolution": 96, "prior_weight": 510}, resolution=None, trunc_cells=3)
    assert c == dict(df.DEPTH_FUSE_DEFAULTS, resolution=96, prior_weight=510, trunc_cells=3)
    with pytest.raises(ValueError, match=r"unknown.*'res'.*in the config"):
        df.merge_settings({"res": 96})
    with pytest.raises(ValueError, match=r"unknown.*'trunc'"):
        df.merge_settings(None, trunc=3)
    with pytest.raises(ValueError, match="prior_weight"):
        df.merge_settings({"prior_weight": 0})


def test_mode_is_listed_and_documented():
    from dynhor_amd import run
    assert "fuse_depth" in run.MODES
    assert "--mode fuse_depth" in run.__doc__
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    for flag in ("--mvs_dir", "--fuse_resolution", "--fuse_trunc_cells"):
        assert flag in p.stdout, flag
    args = run.build_parser().parse_args(["--config_path", "x.yaml", "--mode", "fuse_depth", "--mvs_dir", "d", "--fuse_resolution", "96",
                                          "--fuse_trunc_cells", "3"])
    assert (args.mode, args.mvs_dir, args.fuse_resolution, args.fuse_trunc_cells) == ("fuse_depth", "d", 96, 3.0)


# ------------------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_declared_exported_and_bound():
    from dynhor_amd import _lib
    header = open(os.path.join(ROOT, "include", "dynhor_hip.h")).read()
    assert "int dh_tsdf_integrate(" in header
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dh_tsdf_integrate")
    assert "dh_tsdf_integrate" in _lib.SIGNATURES


def test_argument_validation_without_gpu(hiplib):
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)      # some: non-null, never dereferenced: only refused calls and no-ops get it

    def call(n=5, n_frames=3, H=8, W=8, trunc=0.05, ptrs=None):
        p = [some] * 9 if ptrs is None else ptrs                # pts, depth, weight, R, T, K, num, den, obs
        return hiplib.dh_tsdf_integrate(p[0], n, p[1], p[2], p[3], p[4], p[5], n_frames, H, W, trunc, p[6], p[7], p[8], null)

    assert call(n=0) == 0 and call(n_frames=0) == 0
    assert call(n=0, ptrs=[null] * 9) == 0 and call(n_frames=0, ptrs=[null] * 9) == 0
    for k in range(9):
        assert call(ptrs=[null if j == k else some for j in range(9)]) == -1, k
    for trunc in (0.0, -0.05, float("nan"), float("inf")):
        assert call(trunc=trunc) == -1, trunc
        assert call(n=0, trunc=trunc) == -1, trunc
    assert call(H=0) == -1 and call(W=0) == -1 and call(H=-3) == -1
    assert call(n=-1) == -1 and call(n_frames=-1) == -1
    assert call(H=(1 << 24) + 1) == -2 and call(n_frames=1 << 31) == -2


def test_wrappers_refuse_cpu_tensors_and_noncontiguous_state():
    from dynhor_amd import _lib, depth_fuse as df
    with pytest.raises(_lib.DynhorHipError):
        df.integrate(torch.zeros(3, 3), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8), torch.eye(3)[None], torch.zeros(1, 3),
                     torch.eye(3), 0.05, torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="den is updated in place and must be contiguous"):
        df.integrate(torch.zeros(3, 3), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8), torch.eye(3)[None], torch.zeros(1, 3),
                     torch.eye(3), 0.05, torch.zeros(3, dtype=torch.int64), torch.zeros(3, 2, dtype=torch.int32)[:, 0],
                     torch.zeros(3, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------ plain torch, on the CPU
def test_weights_from_normals_on_cpu_tensors():
    from dynhor_amd import depth_fuse as df
    K = torch.tensor([[100.0, 0.0, 2.0], [0.0, 100.0, 1.5], [0.0, 0.0, 1.0]])
    Kinv = torch.inverse(K.double()).float()
    H, W = 4, 5
    n = torch.zeros(H, W, 3)
    n[..., 2] = -1.0                                                 # facing the camera
    n[0, 0] = torch.tensor([0.0, 0.0, 1.0])                          # facing away: cos < 0 -> the least weight 1
    n[1, 1] = torch.tensor([-math_sqrt_half(), 0.0, -math_sqrt_half()])
    ok = torch.ones(H, W, dtype=torch.bool)
    ok[3, 4] = False
    w = df.weights_from_normals(n, ok, Kinv)
    assert w.dtype == torch.uint8 and tuple(w.shape) == (H, W)
    assert int(w[0, 0]) == 1 and int(w[3, 4]) == 64 and int(w[1, 2]) == 255
    e = np.array([(1 - 2.0) / 100, (1 - 1.5) / 100, 1.0])
    want = int(np.floor(255 * max(0.0, -(np.array([-math_sqrt_half(), 0, -math_sqrt_half()]) @ e) / np.linalg.norm(e)) + 0.5))
    assert int(w[1, 1]) == want and 170 < want < 190
    assert int(df.weights_from_normals(n, ok, Kinv, floor_weight=7)[3, 4]) == 7
    sc = U.scene_inputs()                                            # and against the restatement's weights of the scene
    got = df.weights_from_normals(torch.from_numpy(sc["normal"]).float(), torch.from_numpy(np.isfinite(sc["depth"])),
                                  torch.from_numpy(np.linalg.inv(sc["K"])).float())
    got = torch.where(torch.from_numpy(np.isfinite(sc["depth"])), got, torch.zeros_like(got)).numpy().astype(np.int64)
    assert int(np.abs(got - sc["weight"].astype(np.int64)).max()) <= 1          # float32 against fp64 at a rounding boundary


def math_sqrt_half():
    return float(np.sqrt(0.5))


def test_loader_handles_inf_depth_and_128_normals(tmp_path):
    from PIL import Image
    from dynhor_amd import depth_fuse as df, mvs
    H, W = 6, 7
    z = np.full((H, W), np.inf, dtype=np.float32)
    z[2:4, 1:5] = 1.5
    z[0, 0] = np.nan
    n = torch.zeros(H, W, 3)
    n[..., 2] = -1.0
    okn = torch.zeros(H, W, dtype=torch.bool)
    okn[2:4, 1:4] = True
    os.makedirs(tmp_path / "depth")
    os.makedirs(tmp_path / "monocular_normal")
    np.save(tmp_path / "depth" / "a.npy", z)
    Image.fromarray(mvs.encode_normals(n, okn).numpy()).save(tmp_path / "monocular_normal" / "a.png")
    np.save(tmp_path / "depth" / "c.npy", z)                                      # a depth map without a normal map
    depth, enc, present = df.read_maps(str(tmp_path), ["a", "b", "c"], H, W)
    assert present == [True, False, True] and depth.dtype == torch.float32 and enc.dtype == torch.uint8
    assert bool(torch.isinf(depth[1]).all()) and bool((enc[1] == 128).all()) and bool((enc[2] == 128).all())
    assert float(depth[0, 0, 0]) == float("inf") and int(torch.isfinite(depth[0]).sum()) == 8
    nrm, ok = df.decode_normals(enc)
    assert torch.equal(ok[0], okn) and not bool(ok[1].any())
    assert float((nrm[0][okn] - n[okn]).abs().max()) < 1e-2
    Kinv = torch.inverse(torch.tensor([[50.0, 0, 3.0], [0, 50.0, 2.5], [0, 0, 1.0]]).double()).float()
    w = df.map_weights(depth, enc, Kinv, "cos", 64)
    assert bool((w[1] == 0).all()) and int(w[0, 2, 1]) >= 250 and int(w[0, 2, 4]) == 64 and int(w[0, 0, 0]) == 0 and int(w[0, 5, 6]) == 0
    assert bool((w[2][torch.isfinite(depth[2])] == 64).all())
    u = df.map_weights(depth, enc, Kinv, "uniform")
    assert torch.equal(u > 0, torch.isfinite(depth)) and int(u.max()) == 255
    np.save(tmp_path / "depth" / "b.npy", np.zeros((H + 1, W), dtype=np.float32))
    with pytest.raises(ValueError, match=r"b\.npy.*shape"):
        df.read_maps(str(tmp_path), ["a", "b"], H, W)


def test_frame_residuals_on_cpu_tensors_agree_with_the_restatement():
    from dynhor_amd import depth_fuse as df
    sc, h, fld, trunc, cell = _scene()
    depth = sc["depth"].copy()
    depth[U.BAD_FRAME] *= np.float32(U.BAD_SCALE)
    bad = U.scene_fusion(sc, h, depth=depth)[0]
    med, cnt, worst = U.residuals(bad, U.SCENE_LO, U.SCENE_HI, trunc, depth, sc["weight"], sc["R"], sc["T"], sc["K"])
    got = df.frame_residuals(torch.from_numpy(bad).float(), U.SCENE_LO, U.SCENE_HI, trunc, torch.from_numpy(depth),
                             torch.from_numpy(sc["weight"]), torch.from_numpy(sc["R"]), torch.from_numpy(sc["T"]), torch.from_numpy(sc["K"]))
    assert got["worst"][0] == worst[0] == U.BAD_FRAME and len(got["worst"]) == 5       # the scene's symmetric frames tie behind it
    assert max(abs(a - b) for a, b in zip(got["count"], cnt)) <= 2                      # |field| < 1 and the box's edge, in float32
    assert max(abs(a - b) for a, b in zip(got["median"], med)) < 1e-4                   # float32 samples; the lower of two middle values
    none = df.frame_residuals(torch.from_numpy(bad).float(), U.SCENE_LO, U.SCENE_HI, trunc, torch.full((2, 4, 4), float("inf")),
                              torch.ones(2, 4, 4, dtype=torch.uint8), torch.from_numpy(sc["R"][:2]), torch.from_numpy(sc["T"][:2]),
                              torch.from_numpy(sc["K"]), names=["a", "b"])
    assert none == {"median": [None, None], "count": [0, 0], "worst": ["a", "b"]}


def test_runner_names_mvs_depth_when_there_are_no_maps(tmp_path):
    from dynhor_amd.runner import Runner
    me = SimpleNamespace(world=1, conf={}, last_mvs_dir=None, base_exp_dir=str(tmp_path), _visual_hull_conf=lambda **kw: {})
    with pytest.raises(ValueError, match="--mode mvs_depth"):
        Runner.fuse_depth(me)
    with pytest.raises(ValueError, match="--mode mvs_depth"):
        Runner.fuse_depth(me, mvs_dir=str(tmp_path / "nothing"))
    with pytest.raises(ValueError, match="unknown.*blur"):
        Runner.fuse_depth(me, blur=2)
