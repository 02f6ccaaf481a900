"""Mesh evaluation on the GPU: dh_nearest_sqdist against an fp64 brute force, its reproducibility and slab split, the metrics on
analytic shapes, Runner.evaluate_mesh end to end (NeuS and hash families, file and analytic ground truth) and the CLI mode."""
import ctypes
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from tests.mesh_eval_util import icosphere

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _fma32(a, b, c):
    """fp32 fma(a, b, c), correctly rounded, from fp64: the product of two fp32 numbers is exact in fp64, the sum is formed
    rounded to odd (TwoSum error term), and rounding that to fp32 is then a single correct rounding (53 >= 24 + 2)."""
    p = a.double() * b.double()
    cd = c.double()
    s = p + cd
    bb = s - p
    err = (p - (s - bb)) + (cd - bb)
    even = (s.view(torch.int64) & 1) == 0
    toward = torch.where(err > 0, torch.full_like(s, math.inf), torch.full_like(s, -math.inf))
    s = torch.where((err != 0) & even, torch.nextafter(s, toward), s)
    return s.float()


def _direct_form(q, r):
    """The kernel's arithmetic, one pair per row: fma(dz, dz, fma(dy, dy, dx * dx)), dx = q.x - r.x in fp32."""
    d = q - r
    return _fma32(d[:, 2], d[:, 2], _fma32(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))


def _brute_min_fp64(q, ref, chunk=256):
    """min_j |q_i - r_j| in fp64, every pair (the direct form, chunked over the queries).  torch.cdist(compute_mode=
    "donot_use_mm_for_euclid_dist") computes the same, but returned zeros for some rows of a 2048 x 37,000 fp64 call on this
    platform, so the reference is written out."""
    q64, r64 = q.double(), ref.double()
    out = []
    for s in range(0, q.shape[0], chunk):
        out.append(((q64[s:s + chunk, None, :] - r64[None, :, :]) ** 2).sum(dim=-1).min(dim=1).values.sqrt())
    return torch.cat(out)


def _raw_launch(q, ref, ws, stream=None):
    """dh_nearest_sqdist straight through the C ABI (ws None = the one-slab sweep)."""
    from dynhor_amd import _lib
    d2 = torch.empty(q.shape[0], device=DEV)
    idx = torch.empty(q.shape[0], dtype=torch.int32, device=DEV)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    _lib.check(_lib.lib().dh_nearest_sqdist(_lib.ptr(q), q.shape[0], _lib.ptr(ref), ref.shape[0], _lib.ptr(d2), _lib.ptr(idx),
                                            _lib.ptr(ws) if ws is not None else None, st))
    return d2, idx


def _clouds(nq, nr, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = (torch.rand(nq, 3, device=DEV, generator=g) - 0.5) * 1.2
    ref = (torch.rand(nr, 3, device=DEV, generator=g) - 0.5) * 1.2
    return q, ref


@pytest.mark.parametrize("nq,nr", [(1, 1), (63, 1000), (100_000, 37_000), (37, 200_000)])
def test_kernel_matches_fp64_brute_force(nq, nr):
    from dynhor_amd import _lib
    from dynhor_amd.metrics import nearest_sqdist
    q, ref = _clouds(nq, nr, seed=nq * 7 + nr)
    coinc, dup = [], []
    if nr >= 1000 and nq >= 20:
        # a reference duplicated far down the list (another slab in the split path) and queries sitting exactly on references
        k1, k2 = 5, nr - 3
        ref[k2] = ref[k1]
        q[3] = ref[k2]; dup.append((3, k1))
        for j, k in ((7, nr // 2), (11, nr - 1), (13, 0)):
            q[j] = ref[k]; coinc.append(j)
    if nq == 37:
        assert _lib.lib().dh_nearest_sqdist_workspace(nq, nr) > 0, "this size must take the slab path"
    d2, idx = nearest_sqdist(q, ref, return_index=True)
    assert d2.shape == (nq,) and idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < nr
    dmin = _brute_min_fp64(q, ref)
    d_at = (q.double() - ref.double()[idx]).norm(dim=1)
    assert bool((d_at <= dmin * (1 + 1e-6)).all()), float(((d_at - dmin) / dmin.clamp(min=1e-30)).max())
    exact = _direct_form(q, ref[idx])
    assert torch.equal(d2, exact), "d2 must be the fp32 direct form at the returned index, bit for bit"
    for j in coinc:
        assert float(d2[j]) == 0.0
    for j, k in dup:
        assert float(d2[j]) == 0.0 and int(idx[j]) == k, "duplicated references: the smallest index wins"
    d2_only = nearest_sqdist(q, ref)
    assert torch.equal(d2_only, d2)


@pytest.mark.parametrize("nq,nr", [(37, 200_000), (5000, 300_000)])
def test_reproducible_across_launches_streams_and_slab_split(nq, nr):
    from dynhor_amd import _lib
    q, ref = _clouds(nq, nr, seed=99)
    ref[nr // 3] = ref[nr - 2]                   # a tie across slabs
    q[0] = ref[nr - 2]
    nbytes = _lib.lib().dh_nearest_sqdist_workspace(nq, nr)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    a = _raw_launch(q, ref, ws)
    b = _raw_launch(q, ref, ws)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = _raw_launch(q, ref, ws, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    one = _raw_launch(q, ref, None)
    for other in (b, c, one):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
    assert int(a[1][0]) == nr // 3 and float(a[0][0]) == 0.0


def test_cpu_tensors_raise():
    from dynhor_amd import _lib
    from dynhor_amd.metrics import nearest_sqdist
    with pytest.raises(_lib.DynhorHipError):
        nearest_sqdist(torch.zeros(4, 3), torch.zeros(5, 3))


def test_metrics_on_icospheres(tmp_path):
    from dynhor_amd.mesh import write_ply
    from dynhor_amd.metrics import load_mesh, mesh_metrics
    for r in (0.5, 0.45):
        v, f = icosphere(r, 5)
        write_ply(str(tmp_path / f"s{r}.ply"), v, f)
    a_v, a_f = load_mesh(str(tmp_path / "s0.5.ply"))
    b_v, b_f = load_mesh(str(tmp_path / "s0.45.ply"))
    n = 200_000
    spacing = math.sqrt(math.pi / n)             # mean distance between neighbouring samples on the r = 0.5 sphere
    same = mesh_metrics(a_v, a_f, a_v, a_f, n_samples=n, device=DEV)
    off = mesh_metrics(b_v, b_f, a_v, a_f, n_samples=n, device=DEV)
    assert same["chamfer_l1"] < spacing, same
    assert abs(off["chamfer_l1"] - 0.05) < spacing, off
    assert same["fscore@0.02"] == 1.0 and off["fscore@0.02"] == 0.0
    assert same["normal_consistency"] > 0.99 and off["normal_consistency"] > 0.99
    assert same["n_samples"] == n and same["n_pred_faces"] == same["n_gt_faces"] == a_f.shape[0] and "gt_scale" not in same
    # the same seed gives the same numbers; the ground truth in other units comes back with its scale
    assert mesh_metrics(a_v, a_f, a_v, a_f, n_samples=n, device=DEV) == same
    big = mesh_metrics(a_v, a_f, a_v * 8 + 3, a_f, n_samples=n, device=DEV, gt_normalize="reference")
    assert abs(big["gt_scale"] - 8.0) < 1e-3 and big["chamfer_l1"] < spacing


def _synthetic_conf(name, **model):
    return {"seq_name": "meval", "exp_name": name,
            "data_info": {"synthetic": {"n_frames": 3, "H": 64, "W": 64, "seed": 5}},
            "train": {"batch_size": 256, "report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "end_iter": 100},
            **({"model": model} if model else {})}


def test_evaluate_mesh_end_to_end(tmp_path):
    """Geometric initialisation puts the zero level set near the r = 0.5 sphere: the metrics against an r = 0.5 icosphere must
    match the analytic distance of the reconstruction's own samples to that sphere (mean | |p| - 0.5 |: the nearest point of a
    sphere is radial), and the numbers land in the JSON and the board."""
    from dynhor_amd.mesh import write_ply
    from dynhor_amd.metrics import sample_surface
    from dynhor_amd.runner import Runner
    v, f = icosphere(0.5, 5)
    sphere = str(tmp_path / "sphere.ply")
    write_ply(sphere, v, f)
    r = Runner(conf=_synthetic_conf("neus"), device="cuda:0", exp_root=str(tmp_path))
    n, res = 200_000, 128
    m = r.evaluate_mesh(gt_mesh=sphere, resolution=res, n_samples=n, save=False)
    keys = {"accuracy", "completeness", "chamfer_l1", "chamfer_l2", "normal_consistency", "n_samples", "n_pred_faces", "n_gt_faces"}
    keys |= {f"{k}@{t:g}" for k in ("precision", "recall", "fscore") for t in (0.005, 0.01, 0.02)}
    assert keys <= set(m) and all(math.isfinite(m[k]) for k in keys)
    pv, pf = r.validate_mesh(resolution=res, save=False)
    p, _ = sample_surface(pv, pf, n, torch.Generator(device=DEV).manual_seed(0))
    analytic = float((p.norm(dim=1) - 0.5).abs().double().mean())
    print(f"geometric init vs r=0.5 sphere: {json.dumps(m)}; analytic accuracy {analytic:.5f}")
    assert abs(m["accuracy"] - analytic) < 0.005, (m["accuracy"], analytic)
    # bounds much looser than a near-perfect sphere would allow (chamfer_l1 < 0.01, fscore@0.02 > 0.95): the 8 x 256 network's geometric
    # initialisation is only a rough sphere (level-set radius 0.32 - 0.73, as tests/test_gpu_fullsize_and_runner.py notes).  Measured on
    # MI355X at this seed and resolution: chamfer_l1 0.0815, fscore@0.02 0.147, accuracy 0.08238 against 0.08228 analytic
    assert m["chamfer_l1"] < 0.15 and m["fscore@0.02"] > 0.05, m

    e = r.evaluate_mesh(resolution=96, gt_resolution=192, n_samples=100_000)
    assert e["gt"] == "scene_sdf@192" and all(math.isfinite(e[k]) for k in keys), e
    path = os.path.join(r.base_exp_dir, "meshes", "{:0>8d}_eval.json".format(r.iter_step))
    assert json.load(open(path))["chamfer_l1"] == e["chamfer_l1"]
    r.close()
    board = os.path.join(r.base_exp_dir, "board")
    assert any(fn.startswith("events") for fn in os.listdir(board))
    blob = b"".join(open(os.path.join(board, fn), "rb").read() for fn in os.listdir(board))
    assert b"eval/chamfer_l1" in blob and b"eval/fscore@0.01" in blob


def test_evaluate_mesh_hash_family(tmp_path):
    from dynhor_amd.runner import Runner
    r = Runner(conf=_synthetic_conf("hash", family="hash"), device="cuda:0", exp_root=str(tmp_path))
    m = r.evaluate_mesh(resolution=96, gt_resolution=128, n_samples=50_000, save=False)
    assert all(math.isfinite(v) for k, v in m.items() if k not in ("gt",)), m


def test_evaluate_mesh_without_ground_truth_raises(tmp_path):
    from dynhor_amd.runner import Runner
    r = Runner(conf=_synthetic_conf("nogt"), device="cuda:0", exp_root=str(tmp_path))
    r.dataset.synthetic = False                  # as for a sequence read from disk
    with pytest.raises(ValueError, match="ground truth"):
        r.evaluate_mesh(resolution=32, n_samples=1000)


def test_cli_evaluate_mesh(tmp_path):
    """python -m dynhor_amd.run --mode evaluate_mesh on a saved synthetic checkpoint, in a fresh child process."""
    from dynhor_amd.runner import Runner
    conf = _synthetic_conf("cli")
    conf["eval"] = {"n_samples": 50_000, "gt_resolution": 128}
    r = Runner(conf=conf, device="cuda:0", exp_root=str(tmp_path))
    r.train(2)
    r.save_checkpoint()
    import yaml
    cfg = str(tmp_path / "cli.yaml")
    with open(cfg, "w") as fh:
        yaml.safe_dump(conf, fh)
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "dynhor_amd.run", "--config_path", cfg, "--mode", "evaluate_mesh", "--is_continue",
                        "--exp_root", str(tmp_path), "--mesh_resolution", "64"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["iter"] == 2 and out["resolution"] == 64 and out["n_samples"] == 50_000 and out["gt"] == "scene_sdf@128"
    for k in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "fscore@0.01", "normal_consistency"):
        assert math.isfinite(out[k]), out
