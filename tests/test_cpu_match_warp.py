"""CPU: the affine-warped matcher without a GPU -- the restatement's warped patch on known cases (tests/match_warp_util.py), the
finite-difference affine restatement against its own half step, the settings, the CLI and the argument validation of
dh_match_search_warp."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import match_util as M
from tests import match_warp_util as WU
from tests import mesh_texture_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement's warped patch
def _images(seed=5):
    g = np.random.default_rng(seed)
    gray = g.integers(0, 256, (2, 21, 30), dtype=np.uint8)
    valid = np.ones_like(gray)
    valid[0, 12, 17] = 0
    return gray, valid


def test_identity_warp_is_the_plain_patch():
    gray, valid = _images()
    for px, py, P in ((10, 10, 4), (0, 0, 2), (29, 20, 3), (17, 12, 1), (-3, 40, 2)):
        vals, ok = WU.warp_patch(gray, valid, 0, px, py, WU.IDENTITY, P)
        want, want_ok = M._patch(gray, valid, 0, px, py, P)
        assert np.array_equal(ok, want_ok) and np.array_equal(vals, want), (px, py, P)


def test_warped_patch_on_known_cases():
    gray, valid = _images()
    g = gray[0].astype(np.int64)
    # a quarter turn: cell (c, r) reads (px - r, py + c)
    vals, ok = WU.warp_patch(gray, valid, 0, 10, 8, (0, -65536, 65536, 0), 2)
    assert ok.all()
    for r in range(-2, 3):
        for c in range(-2, 3):
            assert vals[r + 2, c + 2] == g[8 + c, 10 - r]
    # half a pixel to the right at scale 1: fx = 128, fy = 0: two taps, the lower row is not needed -- also on the last row
    for py in (8, 20):
        vals, ok = WU.warp_patch(gray, valid, 0, 10, py, (65536, 0, 0, 65536), 0)
        assert ok.all() and vals[0, 0] == g[py, 10]
    a = (65536 + 32768, 0, 0, 65536)                          # cell c = 1 lands on x = px + 1.5
    vals, ok = WU.warp_patch(gray, valid, 0, 10, 20, a, 1)
    assert ok[0].all() and ok[1].all() and not ok[2].any()    # row r = 1 leaves the image; r = 0 on the last row needs no row below
    assert vals[1, 2] == (128 * 256 * (g[20, 11] + g[20, 12]) + 32768) >> 16
    # fx = 255: weights 1 and 255; fx exactly 0 after a fractional part below 1 / 256: one tap
    vals, ok = WU.warp_patch(gray, valid, 0, 10, 8, (65536 + 255 * 256, 0, 0, 65536 + 255), 1)
    assert ok.all() and vals[1, 2] == (256 * (1 * g[8, 11] + 255 * g[8, 12]) + 32768) >> 16
    assert vals[2, 1] == g[9, 10]                             # Y = 9 + 255 / 65536: fy = 0, one tap
    assert vals[0, 1] == (256 * (1 * g[6, 10] + 255 * g[7, 10]) + 32768) >> 16            # Y = 7 - 255 / 65536: floor 6, fy = 255
    # negative coordinates: the floor is arithmetic
    vals, ok = WU.warp_patch(gray, valid, 0, 0, 0, (32768, 0, 0, 65536), 1)
    assert ok.tolist() == [[False] * 3, [False, True, True], [False, True, True]]        # x = -0.5 needs the tap x = -1
    # a tap on an invalid pixel makes its cells invalid, a tap of weight 0 on it does not
    vals, ok = WU.warp_patch(gray, valid, 0, 16, 12, (65536, 0, 0, 65536), 1)
    assert ok.sum() == 8 and not ok[1, 2]
    vals, ok = WU.warp_patch(gray, valid, 0, 16, 12, (32768, 0, 0, 65536), 1)
    assert not ok[1, 2] and ok[1, 1] and ok[1, 0]             # c = 1 reads x = 16.5: the taps 16 and 17
    # the largest weighted sum fits: all taps 255 gives 255
    full = np.full((1, 9, 9), 255, np.uint8)
    vals, ok = WU.warp_patch(full, np.ones_like(full), 0, 4, 4, (40000, 9000, -9000, 40000), 2)
    assert ok.all() and (vals == 255).all()


def test_search_restatement_with_the_identity_equals_match_util():
    gray, valid = _images()
    g = np.random.default_rng(1)
    q = np.array([(0, 1, int(g.integers(0, 30)), int(g.integers(0, 21)), int(g.integers(0, 30)), int(g.integers(0, 21))) for _ in range(40)])
    want = M.search_ref(gray, valid, q, 2, 3, 1, 1)
    got = WU.search_warp_ref(gray, valid, np.concatenate([q, np.tile(WU.IDENTITY, (40, 1))], 1), 2, 3, 1, 1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    assert (want[0][:, 2] == 0).sum() >= 5 and (want[0][:, 2] == 1).sum() >= 5


# ------------------------------------------------------------------------------------------------ the affine restatement
@functools.lru_cache(maxsize=None)
def three_camera_restatement():
    """The N = 20 sphere before the three cameras of the mesh-guide test, brute-force fp64 z-buffer: (fi, fj, p, keep of the guide,
    X, n, J at FD_STEP, bound of J, bound of J^-1)."""
    H, W = 96, 128
    R, T, K = WU.three_cameras(H, W)
    verts, faces = TU.sphere_mesh((0.0, 0.0, 0.0), TU.SPHERE_R, N=20)
    zbuf = TU.raster_fp64(verts, faces, R, T, K, H, W)
    fi, fj, p = WU.three_camera_queries(H, W)
    _, keep, _ = M.mesh_guesses_ref(fi, fj, p, zbuf, verts, faces, R, T, K)
    keep = keep.numpy()
    has, X, n = WU.surface_points(fi.numpy(), p.numpy(), zbuf, verts, faces, R, T, K)
    assert has[keep].all()
    a, b = fi.numpy()[keep], fj.numpy()[keep]
    J, bj, bi = WU.fd_bound(a, b, X[keep], n[keep], R, T, K)
    return a, b, p.numpy()[keep], X[keep], n[keep], J, bj, bi, (R, T, K)


def test_finite_difference_affines_agree_with_their_half_step_within_the_rounding_cap():
    """The bound the GPU test gives mesh_affines is 4 x |J(h) - J(h / 2)| of the restatement itself; the quantised integers are compared
    only where A 65536 is further than that from a rounding boundary: at most 0.5 % of the kept queries may be left out."""
    a, b, p, X, n, J, bj, bi, cams = three_camera_restatement()
    keep, sv, det = WU.affine_verdict(J)
    amb = WU.near_rounding(J, bj) | WU.near_rounding(np.linalg.inv(J), bi)
    print(f"fd affines: {len(J)} queries, step {WU.FD_STEP:g}, bound J median {np.median(bj):.3e} largest {bj.max():.3e}, bound J^-1 median "
          f"{np.median(bi):.3e} largest {bi.max():.3e}, {int(keep.sum())} within warp_max, near a rounding boundary {int(amb.sum())} "
          f"({100 * amb.mean():.3f} %; of those within warp_max {100 * amb[keep].mean():.3f} %), singular values {sv.min():.3f} .. "
          f"{sv.max():.3f}")
    assert len(J) > 1000 and np.isfinite(J).all() and (det > 0).all()
    assert amb.mean() <= 0.005 and amb[keep].mean() <= 0.005
    assert 0 < keep.sum() < len(J)                           # the three views hold queries on both sides of warp_max
    # the step is one at which the difference is truncation (c h^2: a quarter at half the step), not rounding noise
    half = WU.fd_bound(a, b, X, n, cams[0], cams[1], cams[2], WU.FD_STEP / 2)[1]
    assert 3.5 <= np.median(bj) / np.median(half) <= 4.5, np.median(bj) / np.median(half)
    # the analytic derivative of a pinhole camera, written out for one query, agrees with the differences
    R, T, K = (WU._np(t) for t in cams)
    k = len(J) // 2
    D = []
    for f in (a[k], b[k]):
        c = R[f] @ X[k] + T[f]
        u, w = c @ K[0] / c[2], c @ K[1] / c[2]
        D.append(np.stack([K[0] - u * np.array([0, 0, 1.0]), K[1] - w * np.array([0, 0, 1.0])]) @ R[f] / c[2])
    B = np.concatenate([D[0], n[k][None]], 0)
    assert np.abs(D[1] @ np.linalg.inv(B)[:, :2] - J[k]).max() <= bj[k]


# ------------------------------------------------------------------------------------------------ settings, CLI, arguments
def test_settings_and_cli_know_the_warp():
    from dynhor_amd.match import DEFAULTS, GUIDES, check_settings
    from dynhor_amd.run import build_parser
    from dynhor_amd.runner import DEFAULT_CONF, _merge
    assert DEFAULTS["warp"] == "none" and DEFAULTS["warp_max"] == 3.0 and GUIDES == ("none", "mesh")
    assert DEFAULT_CONF["match"] == DEFAULTS
    s = check_settings({})
    assert s["warp"] == "none" and s["warp_max"] == 3.0
    s = check_settings({"guide": "mesh", "warp": "affine", "warp_max": 2})
    assert s["warp"] == "affine" and s["warp_max"] == 2.0 and s["range"] == 12
    assert check_settings({"guide": "mesh", "warp_max": 1})["warp_max"] == 1.0
    for bad in ({"warp": "affine"}, {"warp": "affine", "guide": "none"}, {"guide": "mesh", "warp": "homography"}, {"warp_max": 0.99},
                {"guide": "mesh", "warp": "affine", "warp_max": 0.5}, {"warp_max": 8.5}, {"warp_max": float("nan")}):
        with pytest.raises(ValueError):
            check_settings(bad)
    assert _merge(DEFAULT_CONF, {"match": {"warp": "affine", "guide": "mesh"}})["match"]["warp"] == "affine"
    base = ["--config_path", "x.yaml", "--mode", "match_frames"]
    assert build_parser().parse_args(base).match_warp is None
    assert build_parser().parse_args(base + ["--match_warp", "affine"]).match_warp == "affine"
    assert build_parser().parse_args(base + ["--match_warp", "none"]).match_warp == "none"
    for word in ("homography", "mesh", ""):
        with pytest.raises(SystemExit):
            build_parser().parse_args(base + ["--match_warp", word])


def test_entry_point_validates_its_arguments(hiplib):
    from dynhor_amd import _lib
    L = hiplib
    header = open(os.path.join(ROOT, "include", "dynhor_hip.h")).read()
    assert "dh_match_search_warp(" in header and "dh_match_search_warp" in _lib.SIGNATURES
    assert _lib.SIGNATURES["dh_match_search_warp"] == _lib.SIGNATURES["dh_match_search"]
    null, some, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4098)

    def call(gray=some, valid=some, F=2, H=8, W=8, q=some, n=5, P=4, R=8, excl=2, min_va=1, oi=some, of=some):
        return L.dh_match_search_warp(gray, valid, F, H, W, q, n, P, R, excl, min_va, oi, of, null)
    assert call(n=0, gray=null, valid=null, q=null, oi=null, of=null) == 0                            # n == 0: a no-op
    assert call(gray=null) == -1 and call(valid=null) == -1 and call(q=null) == -1 and call(oi=null) == -1 and call(of=null) == -1
    assert call(of=odd) == -1 and call(oi=odd) == -1 and call(q=odd) == -1
    assert call(n=-1) == -1 and call(F=-1) == -1 and call(H=0) == -1 and call(W=0) == -1
    assert call(P=0) == -1 and call(P=8) == -1 and call(R=-1) == -1 and call(R=33) == -1 and call(excl=-1) == -1
    assert call(min_va=0) == -1 and call(min_va=-5) == -1
    assert call(n=1 << 31) == -2 and call(F=1 << 31) == -2 and call(H=(1 << 24) + 1) == -2


def test_wrappers_refuse_cpu_tensors():
    from dynhor_amd import _lib, match
    g, v = torch.zeros(1, 4, 4, dtype=torch.uint8), torch.ones(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(_lib.DynhorHipError):
        match.search_warp(g, v, torch.zeros(1, 10, dtype=torch.int32))
    q = torch.zeros(1, 6, dtype=torch.int32)
    a = torch.tensor([WU.IDENTITY], dtype=torch.int32)
    with pytest.raises(_lib.DynhorHipError):
        match.match_pairs(g, v, q, affine_fwd=a, affine_bwd=a)
    with pytest.raises(ValueError):
        match.match_pairs(g, v, q, affine_fwd=a)
