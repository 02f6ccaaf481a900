"""CPU: the visual hull's settings, entry point and CLI; the code of the carving kernel (no scratch in any instantiation); and the
rule itself, restated in fp64 numpy (tests/visual_hull_util.py), shown to do what it is for on the synthetic scene: the hull contains
the object, exceeds it by little, and a frame with a shifted pose is the frame that carves alone."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import visual_hull_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ settings
def test_defaults_and_check_settings():
    from dynhor_amd import visual_hull as vh
    assert vh.VISUAL_HULL_DEFAULTS == {"resolution": 128, "bound": "auto", "coarse_resolution": 48, "band_px": 16, "min_carve_votes": 1,
                                       "min_seen": 0.5, "outside_value": 1.0, "frame_chunk": 16, "point_chunk": 1 << 22}
    vh.check_settings(dict(vh.VISUAL_HULL_DEFAULTS))
    vh.check_settings(dict(vh.VISUAL_HULL_DEFAULTS, resolution=512, bound=0.6, min_carve_votes=8, min_seen=0))
    bad = {"resolution": (513, 1, 64.0, True), "bound": ("box", 0, -1.0, float("nan")), "coarse_resolution": (1, 1000),
           "band_px": (0, 0.5, "wide", 5000), "min_carve_votes": (0, 9, 1.5, True), "min_seen": (-0.1, 1.5, None),
           "outside_value": (0, -1.0, float("inf")), "frame_chunk": (0, 2.5), "point_chunk": (0, -4)}
    assert set(bad) == set(vh.VISUAL_HULL_DEFAULTS)
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=key):
                vh.check_settings(dict(vh.VISUAL_HULL_DEFAULTS, **{key: v}))
    with pytest.raises(ValueError, match="resolutoin"):
        vh.check_settings(dict(vh.VISUAL_HULL_DEFAULTS, resolutoin=64))
    with pytest.raises(ValueError, match="band_px"):
        vh.check_settings({k: v for k, v in vh.VISUAL_HULL_DEFAULTS.items() if k != "band_px"})


def test_yaml_block_merges_under_the_overrides():
    from dynhor_amd import visual_hull as vh
    from dynhor_amd.runner import DEFAULT_CONF, Runner
    assert "visual_hull" not in DEFAULT_CONF                                         # the block is optional
    me = SimpleNamespace(conf={"visual_hull": {"resolution": 96, "min_carve_votes": 2}})
    c = Runner._visual_hull_conf(me, resolution=None, band_px=8)
    assert c == dict(vh.VISUAL_HULL_DEFAULTS, resolution=96, min_carve_votes=2, band_px=8)
    assert Runner._visual_hull_conf(me, resolution=64)["resolution"] == 64
    assert Runner._visual_hull_conf(SimpleNamespace(conf={})) == vh.VISUAL_HULL_DEFAULTS
    with pytest.raises(ValueError, match="votes"):
        Runner._visual_hull_conf(SimpleNamespace(conf={"visual_hull": {"votes": 2}}))
    with pytest.raises(ValueError, match="min_seen"):
        Runner._visual_hull_conf(me, min_seen=2.0)
    with pytest.raises(ValueError, match="grid"):
        Runner._visual_hull_conf(me, grid=64)


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_point_declared_exported_and_bound():
    from dynhor_amd import _lib
    header = open(os.path.join(ROOT, "include", "dynhor_hip.h")).read()
    assert "int dh_hull_accumulate(" in header
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dh_hull_accumulate")
    assert "dh_hull_accumulate" in _lib.SIGNATURES


def test_argument_validation_without_gpu(hiplib):
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)

    def call(n=5, n_frames=3, H=8, W=8, frame0=0, m=2, ptrs=None):
        p = [some] * 8 if ptrs is None else ptrs             # pts, sd, R, T, K, topk, arg, seen
        return hiplib.dh_hull_accumulate(p[0], n, p[1], p[2], p[3], p[4], n_frames, H, W, frame0, m, p[5], p[6], p[7], null)

    assert call(n=0, ptrs=[null] * 8) == 0 and call(n_frames=0, ptrs=[null] * 8) == 0        # no-ops
    for k in range(8):                                                                        # every pointer is required
        assert call(ptrs=[null if j == k else some for j in range(8)]) == -1, k
    assert call(n=-1) == -1 and call(n_frames=-1) == -1 and call(frame0=-1) == -1
    assert call(H=1) == -1 and call(W=1) == -1 and call(H=0) == -1
    assert call(m=0) == -1 and call(m=9) == -1
    assert call(H=(1 << 24) + 1) == -2 and call(W=(1 << 24) + 1) == -2
    assert call(n=(1 << 31) * 256) == -2
    assert call(n_frames=1 << 31) == -2 and call(n_frames=10, frame0=(1 << 31) - 5) == -2
    assert call(n=0, m=9, ptrs=[null] * 8) == -1                                              # a bad m is refused before the no-op


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from dynhor_amd import _lib, visual_hull as vh
    with pytest.raises(_lib.DynhorHipError):
        vh.signed_label_distance(torch.zeros(1, 4, 4, dtype=torch.int8), 4)
    with pytest.raises(_lib.DynhorHipError):
        vh.hull_accumulate(torch.zeros(3, 3), torch.zeros(1, 4, 4), torch.eye(3)[None], torch.zeros(1, 3), torch.eye(3), 0,
                           torch.zeros(3, 2), torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(_lib.DynhorHipError):
        vh.hull_field(torch.zeros(3, 3), SimpleNamespace(n_images=1))


# ------------------------------------------------------------------------------------------------------------ the CLI
def test_mode_is_listed_and_documented():
    from dynhor_amd import run
    assert "visual_hull" in run.MODES
    assert "--mode visual_hull" in run.__doc__
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "visual_hull" in p.stdout.split("--mode", 1)[1].split("--is_continue", 1)[0]
    for flag in ("--hull_resolution", "--hull_votes"):
        assert flag in p.stdout, flag
    args = run.build_parser().parse_args(["--config_path", "x.yaml", "--mode", "visual_hull", "--hull_resolution", "96", "--hull_votes", "2"])
    assert (args.mode, args.hull_resolution, args.hull_votes) == ("visual_hull", 96, 2)


# ------------------------------------------------------------------------------------------------------------ the kernel's code
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_kernel_listing_keeps_the_top_values_in_registers(tmp_path):
    from tests.test_cpu_isa_inflight import LISTING
    out = tmp_path / "visual_hull.s"
    subprocess.run(LISTING + [os.path.join(ROOT, "dynhor_amd", "csrc", "visual_hull.hip"), "-o", str(out)], check=True, timeout=600,
                   stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels = re.findall(r"^(_ZN2dh\w*hull_accumulate_kernelILi(\d)E\w*):.*?; ScratchSize: (\d+)", text, flags=re.S | re.M)
    assert sorted(int(m) for _, m, _ in kernels) == list(range(1, 9)), kernels             # one instantiation per m = 1 .. 8
    assert all(int(scratch) == 0 for _, _, scratch in kernels), kernels
    assert not [ln for ln in text.split("\n") if ln.strip().startswith("scratch_")]


# ------------------------------------------------------------------------------------------------------------ the rule
@functools.lru_cache(maxsize=None)
def _sequence(n_frames):
    from dynhor_amd.scene import make_sequence
    seq = make_sequence(n_frames=n_frames, H=96, W=96, seed=11, hand=True)
    return seq, U.signed_label_distance(seq["label"], 16)


def _scene_sdf(p):
    from dynhor_amd.scene import scene_sdf
    return scene_sdf(torch.from_numpy(np.asarray(p, dtype=np.float64))).numpy()


def _foot(seq):
    """One pixel's footprint in object units at the far side of the sampled box, in the farthest frame."""
    return (float(seq["T"].norm(dim=1).max()) + 0.6) / float(seq["K"][0, 0])


def test_restatement_hull_contains_the_object_and_exceeds_it_by_little():
    seq, sd = _sequence(24)
    pts = np.random.default_rng(5).uniform(-0.6, 0.6, size=(60000, 3))
    foot = _foot(seq)
    assert abs(foot - 0.0268) < 2e-4, foot
    topk, arg, seen = U.hull_state(pts, None, seq["R"], seq["T"], seq["K"], m=2, sd=sd)
    sdf = _scene_sdf(pts)
    deep = sdf <= -1.5 * foot
    ratios = {}
    for k in (1, 2):
        h = U.field_from_state(topk, seen, 24, min_carve_votes=k)
        ratios[k] = float((h <= 0).sum()) / float((sdf <= 0).sum())
        print(f"k = {k}: {int(deep.sum())} points at least 1.5 foot = {1.5 * foot:.4f} inside the object, worst h {h[deep].max():.4f}; "
              f"hull / object volume {ratios[k]:.4f}")
        assert int(deep.sum()) > 2000 and bool((h[deep] <= 0).all())
        assert 1.0 <= ratios[k] <= 1.1
    assert ratios[2] >= ratios[1]
    # a hand pixel is solid: no point of the object is carved by a frame whose hand hides it (above), and arg names a real frame
    assert int(arg.min()) >= 0 and int(arg.max()) < 24


def test_restatement_shifted_frame_is_the_sole_carver():
    """One frame's T moved by (0.06, 0, 0), about 3 px: the prototype gave that frame 4.4 % of the k = 2 hull as its sole-carved
    share against 0.8 % for the runner-up, and 0.8 % for the largest share without the shift."""
    seq, sd = _sequence(16)
    bad = 5
    pts = U.grid_points([-0.6] * 3, [0.6] * 3, 64).astype(np.float64)
    share0, hull0 = U.sole_carved_share(*U.hull_state(pts, None, seq["R"], seq["T"], seq["K"], m=2, sd=sd), 16)
    T = seq["T"].clone()
    T[bad] += torch.tensor([0.06, 0.0, 0.0])
    share1, hull1 = U.sole_carved_share(*U.hull_state(pts, None, seq["R"], T, seq["K"], m=2, sd=sd), 16)
    order = np.argsort(-share1, kind="stable")
    print(f"sole-carved share: shifted frame {bad} {100 * share1[bad]:.2f} %, runner-up (frame {order[1]}) {100 * share1[order[1]]:.2f} %; "
          f"without the shift the largest is {100 * share0.max():.2f} % (frame {int(share0.argmax())}); k = 2 hull {hull0} / {hull1} cells")
    assert order[0] == bad
    assert share1[bad] >= 3.0 * share1[order[1]]
    assert share1[bad] >= 3.0 * share0.max()
