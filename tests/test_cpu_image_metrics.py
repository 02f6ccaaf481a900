"""CPU: the taps of the SSIM window, the numpy restatement of dh_ssim (tests/image_metrics_util.py) against an independent float SSIM
and on cases with known answers, the held-out frames of the frame permutation, the image_eval settings and CLI, and dh_ssim's argument
checks (no launch: there is no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch

from dynhor_amd import image_metrics as im
from dynhor_amd import schedules
from tests import image_metrics_util as U

TAPS = im.gaussian_taps_q16(1.5, 5)
HALF = im.weight_threshold(0.5)


def _textured(H, W, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(x / 3.0)[..., None] * np.cos(y / 4.0)[..., None] + rng.normal(0, 12, (H, W, 3))
    return np.clip(np.round(base), 0, 255).astype(np.uint8)[None]


# ------------------------------------------------------------------------------------------------ taps
def test_taps_sum_symmetry_and_known_values():
    assert TAPS[:6] == [67, 498, 2359, 7167, 13960, 17434]
    for sigma, r in ((1.5, 5), (0.5, 1), (3.0, 16), (10.0, 16), (0.3, 4), (1.5, 0)):
        t = im.gaussian_taps_q16(sigma, r)
        assert len(t) == 2 * r + 1 and sum(t) == 65536 and min(t) >= 0
        assert t == t[::-1]
        assert all(isinstance(v, int) for v in t)
    assert im.gaussian_taps_q16(1.5, 0) == [65536]
    for bad in ((0.0, 5), (-1.0, 5), (float("nan"), 5), (1.5, -1), (1.5, 17)):
        with pytest.raises(ValueError):
            im.gaussian_taps_q16(*bad)
    assert im.weight_threshold(0.5) == 1 << 31 and im.weight_threshold(1.0) == 1 << 32 and im.weight_threshold(1e-12) == 1
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            im.weight_threshold(bad)


def test_psnr_from_sums():
    assert im.psnr_from_sums(0.0, 0) is None and im.psnr_from_sums(0.0, 10) == float("inf")
    assert im.psnr_from_sums(3.0 * 10 * 65025.0, 10) == 0.0
    assert abs(im.psnr_from_sums(3.0 * 10, 10) - 20 * np.log10(255.0)) < 1e-12


# ------------------------------------------------------------------------------------------------ the restatement
def test_interior_equals_a_plain_float_ssim_exactly():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (2, 23, 29, 3), dtype=np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
    ref = U.ssim_ref(a, b, None, TAPS, HALF)
    plain = U.ssim_plain(a, b, TAPS)
    assert plain.shape == (2, 13, 19)
    assert np.array_equal(ref["s"][:, 5:-5, 5:-5], plain)          # everything is dyadic and below 2^53
    assert ref["counted"][:, 5:-5, 5:-5].all()
    # the corners of a full image see (sum of the taps from the centre on)^2 / 2^32 = 0.40 of the weight
    corner = sum(TAPS[5:]) ** 2
    assert ref["wt"][0, 0, 0] == corner and 0.39 < corner / 2 ** 32 < 0.41
    for f in range(2):
        c = ref["counted"][f]
        assert not c[0, 0] and not c[0, -1] and not c[-1, 0] and not c[-1, -1]
        assert int((~c).sum()) == 4


def test_identical_images_score_exactly_one():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (1, 40, 37, 3), dtype=np.uint8)
    usable = (rng.random((1, 40, 37)) < 0.7).astype(np.uint8)
    for us in (None, usable):
        ref = U.ssim_ref(a, a, us, TAPS, 1)
        assert ref["counted"].any() and np.all(ref["s"][ref["counted"]] == 1.0)
        assert ref["out"][0, 2] == 0 and ref["out"][0, 3] == 0 and ref["out"][0, 0] == ref["out"][0, 1]


def test_disc_mask_is_counted_whole_at_half_weight():
    m = U.disc_mask(48, 48, 24, 24, 15)[None]
    assert int(m.sum()) == 697
    a = _textured(48, 48)
    ref = U.ssim_ref(a, a, m, TAPS, HALF)
    assert ref["out"][0, 4] == 697 and ref["out"][0, 1] == 697
    assert not ref["counted"][m == 0].any() and np.all(ref["map"][m == 0] == 0)
    one = np.zeros((1, 9, 9), np.uint8)
    one[0, 4, 4] = 1                                            # a one-pixel island holds (17434 / 65536)^2 = 0.07 of its window
    assert U.ssim_ref(a[:, :9, :9], a[:, :9, :9], one, TAPS, HALF)["out"][0, 1] == 0
    assert U.ssim_ref(a[:, :9, :9], a[:, :9, :9], one, TAPS, 1)["out"][0, 1] == 1


def test_radius_zero_is_the_per_pixel_luminance_term():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (1, 6, 7, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (1, 6, 7, 3), dtype=np.uint8)
    ref = U.ssim_ref(a, b, None, [65536], 1 << 32)
    x, y = a.astype(np.float64), b.astype(np.float64)
    want = ((2 * x * y + U.C1) / (x * x + y * y + U.C1)).sum(-1) / 3.0
    assert ref["counted"].all() and np.allclose(ref["s"], want, rtol=0, atol=1e-15)


def test_ssim_falls_with_noise_and_with_blur():
    a = _textured(40, 40, seed=4)
    rng = np.random.default_rng(5)
    n = rng.normal(0, 1, a.shape)
    scores = []
    for amp in (0, 4, 10, 25, 60):
        b = np.clip(np.round(a + amp * n), 0, 255).astype(np.uint8)
        r = U.ssim_ref(a, b, None, TAPS, HALF)
        scores.append(r["out"][0, 0] / r["out"][0, 1])
    assert scores[0] == 1.0 and all(p > q for p, q in zip(scores, scores[1:])), scores
    blurred, cur = [], a.astype(np.float64)
    for _ in range(4):
        blurred.append(np.clip(np.round(cur), 0, 255).astype(np.uint8))
        p = np.pad(cur, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
        cur = sum(p[:, dy:dy + 40, dx:dx + 40] for dy in range(3) for dx in range(3)) / 9.0
    scores = []
    for b in blurred:
        r = U.ssim_ref(a, b, None, TAPS, HALF)
        scores.append(r["out"][0, 0] / r["out"][0, 1])
    assert scores[0] == 1.0 and all(p > q for p, q in zip(scores, scores[1:])), scores


def test_checkerboard_against_its_negative_is_negative():
    y, x = np.mgrid[0:24, 0:24]
    a = (((x + y) & 1) * 255).astype(np.uint8)[None, ..., None].repeat(3, -1)
    r = U.ssim_ref(a, 255 - a, None, TAPS, HALF)
    assert r["s"][r["counted"]].max() < 0


def test_all_255_reaches_the_largest_row_sum_below_2_32():
    a = np.full((1, 20, 20, 3), 255, np.uint8)
    r = U.ssim_ref(a, a, None, TAPS, HALF)
    assert r["max_row"] == 65025 * 65536 and r["max_row"] < 1 << 32
    assert np.all(r["s"][r["counted"]] == 1.0)
    a = np.full((1, 3, 40, 3), 255, np.uint8)                   # wide enough to hold a whole row of the largest window
    r16 = U.ssim_ref(a, a, None, im.gaussian_taps_q16(4.0, 16), 1)
    assert r16["max_row"] == 65025 * 65536


# ------------------------------------------------------------------------------------------------ holdout
def test_holdout_parsing():
    assert schedules.split_holdout("none", 6) == ([0, 1, 2, 3, 4, 5], [])
    assert schedules.split_holdout(None, 3) == ([0, 1, 2], [])
    assert schedules.split_holdout("every:4", 10) == ([1, 2, 3, 5, 6, 7, 9], [0, 4, 8])
    assert schedules.split_holdout("every:4:3", 10)[1] == [3, 7]
    assert schedules.split_holdout(["0002", "0000"], 4) == ([1, 3], [0, 2])
    assert schedules.split_holdout("b,c", 3, stems=["a", "b", "c"]) == ([0], [1, 2])
    assert schedules.select_frames("all", 3) == [0, 1, 2]
    for bad in ("every:0", "every:4:4", "every:x", "every:2:0:1", "every:", ["nope"], "0009", 7):
        with pytest.raises(ValueError, match="train.holdout"):
            schedules.split_holdout(bad, 8)
    for bad in ("every:1", "all", ["0000", "0001"]):
        with pytest.raises(ValueError, match="train.holdout"):
            schedules.split_holdout(bad, 2)


def test_no_holdout_is_exactly_the_plain_permutation():
    n, seed = 7, 4321
    plain = schedules.FramePermutation(n, seed)
    none = schedules.FramePermutation(n, seed, frames=None)
    for slot in range(3 * n):
        assert plain.frame(slot) == none.frame(slot)
    a, b = plain.state_dict(), none.state_dict()
    assert set(a) == set(b) == {"gen", "perm", "epoch"}
    assert torch.equal(a["gen"], b["gen"]) and torch.equal(a["perm"], b["perm"]) and a["epoch"] == b["epoch"] == 2


def test_holdout_never_draws_a_held_out_frame():
    n = 10
    train, held = schedules.split_holdout("every:4", n)
    p = schedules.FramePermutation(n, 4321, frames=train)
    for epoch in range(3):
        drawn = [p.frame(epoch * len(train) + k) for k in range(len(train))]
        assert sorted(drawn) == train and not set(drawn) & set(held)
    q = schedules.FramePermutation(n, 99, frames=train)
    q.load_state_dict(p.state_dict())
    assert q.frame(3 * len(train)) == p.frame(3 * len(train))
    with pytest.raises(ValueError, match="train.holdout"):
        schedules.FramePermutation(n, 4321).load_state_dict(p.state_dict())
    with pytest.raises(ValueError):
        schedules.FramePermutation(n, 1, frames=[])
    with pytest.raises(ValueError):
        schedules.FramePermutation(n, 1, frames=[n])


# ------------------------------------------------------------------------------------------------ config and CLI
def test_image_eval_defaults_and_cli():
    import argparse
    from dynhor_amd.run import MODES, build_parser, mode_arg
    from dynhor_amd.runner import DEFAULT_CONF, IMAGE_EVAL_DEFAULTS, Runner
    assert IMAGE_EVAL_DEFAULTS == {"frames": "auto", "sigma": 1.5, "radius": 5, "min_weight": 0.5, "erode_px": 0, "maps": False}
    assert DEFAULT_CONF["train"]["holdout"] == "none"
    assert "evaluate_views" in MODES and mode_arg("evaluate_views") == "evaluate_views"
    with pytest.raises(argparse.ArgumentTypeError):
        mode_arg("evaluate_view")
    ap = build_parser()
    a = ap.parse_args(["--config_path", "x.yaml", "--mode", "evaluate_views", "--eval_frames", "every:2:1", "--eval_maps"])
    assert a.eval_frames == "every:2:1" and a.eval_maps is True
    a = ap.parse_args(["--config_path", "x.yaml", "--mode", "evaluate_views"])
    assert a.eval_frames is None and a.eval_maps is None
    stub = Runner.__new__(Runner)                         # the settings need no device
    stub.conf = {"image_eval": {"radius": 3, "sigam": 2.0}}
    with pytest.raises(ValueError, match="sigam"):
        stub._image_eval_conf()
    stub.conf = {"image_eval": {"radius": 3}}
    assert stub._image_eval_conf(frames="all", maps=True) == dict(IMAGE_EVAL_DEFAULTS, radius=3, frames="all", maps=True)
    stub.conf = {"image_eval": {"erode_px": -1}}
    with pytest.raises(ValueError, match="erode_px"):
        stub._image_eval_conf()


def test_ssim_frames_names_what_is_wrong():
    a = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(im._lib.DynhorHipError, match="a must be a device tensor"):
        im.ssim_frames(a, a)


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_ssim_argument_checks_without_gpu(hiplib):
    OK, BAD, UNSUP = 0, -1, -2
    assert hiplib.dh_ssim_sums() == 6 == im.SUMS
    assert hiplib.dh_ssim_workspace(1, 1, 1) == 6 * 8
    assert hiplib.dh_ssim_workspace(3, 1080, 1920) == 3 * 68 * 60 * 6 * 8
    assert hiplib.dh_ssim_workspace(2, 17, 33) == 2 * 2 * 2 * 6 * 8           # the tiles depend on H and W alone
    assert hiplib.dh_ssim_workspace(-1, 4, 4) == BAD and hiplib.dh_ssim_workspace(1, 0, 4) == BAD
    assert hiplib.dh_ssim_workspace(65536, 4, 4) == UNSUP and hiplib.dh_ssim_workspace(1, (1 << 24) + 1, 4) == UNSUP
    null = ctypes.c_void_p(0)
    p = ctypes.c_void_p(0x1000)                                               # never dereferenced: every call below ends in the checks
    taps = (ctypes.c_int32 * 11)(*TAPS)
    notaps = ctypes.POINTER(ctypes.c_int32)()

    def call(a=p, b=p, usable=null, n=1, H=8, W=8, t=taps, r=5, w_min=HALF, smap=null, out=p, ws=p):
        return hiplib.dh_ssim(a, b, usable, n, H, W, t, r, w_min, smap, out, ws, null)

    assert call(a=null, b=null, out=null, ws=null, t=notaps, n=0) == OK        # n_frames == 0: no-op
    assert call(a=null) == BAD and call(b=null) == BAD and call(t=notaps) == BAD and call(out=null) == BAD and call(ws=null) == BAD
    assert call(ws=ctypes.c_void_p(0x1008)) == BAD                             # misaligned
    assert call(n=-1) == BAD and call(r=-1) == BAD and call(H=0) == BAD and call(W=0) == BAD
    assert call(w_min=0) == BAD and call(w_min=(1 << 32) + 1) == BAD
    neg = list(TAPS)
    neg[0], neg[5] = -1, neg[5] + 68
    assert sum(neg) == 65536 and call(t=(ctypes.c_int32 * 11)(*neg)) == BAD
    short = list(TAPS)
    short[5] -= 1
    assert call(t=(ctypes.c_int32 * 11)(*short)) == BAD
    assert call(t=taps, r=4) == BAD                                            # the first nine taps do not sum to 65536
    big = (ctypes.c_int32 * 35)(*([0] * 17 + [65536] + [0] * 17))
    assert call(t=big, r=17) == UNSUP and call(n=65536) == UNSUP
    assert call(H=(1 << 24) + 1) == UNSUP and call(W=(1 << 24) + 1) == UNSUP
