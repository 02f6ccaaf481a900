"""Record tests/golden/train_step.json: what six training iterations of the Runner leave behind, bit for bit, in both model families
and on both samplers of the hash family (A-E, G, H), and what the network stages give outside the training step (F: vertex colours,
colours at hit points, three steps of the SDF warm start).  tests/test_gpu_train_step_replay.py replays the file.

    python tests/golden/make_golden_train_step.py [--out path]

It needs an MI355X and calls only entry points that outlive a reorganisation of the training path: Runner and train_iteration,
mesh_color.network_vertex_colors, surface_render.network_at_hits and sdf_init.fit_step.  Run it at the commit BEFORE a change that
must not move a bit, twice, and keep the file only when both runs wrote the same bytes; a difference in the test is a finding to
explain, never a reason to run this again.

Every case A-E, G, H builds a Runner on the synthetic scene (6 frames of 64 x 64, the default seeds, no report, checkpoint or validation)
and records the stats [8] of each of 6 iterations, the side statistics the step leaves (last_prior_stats, last_corr_stats), the
SHA-256 of store.flat at the end and, where the poses move, of dataset.R and dataset.T.
  A  NeuS, batch 77 (77 x 128 points: ragged against a pair workgroup), normal_weight 0.05
  B  NeuS, the full loss stack without pose refinement: correspondences (corr_weight 0.1, a quarter of the batch of 128, a vote at
     iteration 3), the depth prior from iteration 2 on, the masked normal prior
  C  NeuS with pose refinement from iteration 1 on, the normal term and the depth prior.  (Pose refinement TOGETHER with the
     correspondence term sums the partner poses' gradients with float atomics: not reproducible, so not recorded.)
  D  hash family, hierarchical sampler, batch 77
  E  hash family, occupancy-grid sampler (grid 32^3, refreshed every 2 iterations), batch 128, the depth and masked normal priors
  G  hash family, hierarchical sampler, batch 77, pose refinement from iteration 1 on, the normal term, no correspondences
  H  hash family, occupancy-grid sampler as in E, batch 128, pose refinement from iteration 1 on, the normal term, no correspondences
     (G and H: the point and direction adjoints of the hash-grid kernels, which D and E do not run)
json keeps a Python float exactly, so the replay compares without a tolerance."""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

ITERS = 6
NET_CHUNK = 128                     # case F: 300 points go in chunks of 128, 128 and 44
SYNTHETIC = {"n_frames": 6, "H": 64, "W": 64, "seed": 11}
QUIET = {"report_freq": 10 ** 9, "save_freq": 10 ** 9, "val_freq": 0, "warm_up_end": 2, "end_iter": 2000}
HASH_OCCGRID = {"sampler": "occgrid", "march_samples_per_ray": 256, "grid_res": 32, "grid_update_every": 2}
PRIORS = {"depth_weight": 0.5, "normal_weight": 0.05, "normal_skip_missing": True}
HASH_REFINE = {"refine_poses": True, "pose_start_iter": 1, "normal_weight": 0.05}
CASES = {
    "A_neus_ragged": dict(family="neus", train={"batch_size": 77, "normal_weight": 0.05}),
    "B_neus_full_loss_stack": dict(family="neus", synthetic={"correspondences": 256, "depth": True},
                                   train=dict(PRIORS, batch_size=128, corr_weight=0.1, corr_fraction=0.25, corr_vote_freq=3,
                                              depth_start_iter=2)),
    "C_neus_refine_poses": dict(family="neus", synthetic={"depth": True},
                                train={"batch_size": 128, "refine_poses": True, "pose_start_iter": 1, "normal_weight": 0.05,
                                       "depth_weight": 0.5}),
    "D_hash_hierarchical": dict(family="hash", train={"batch_size": 77}),
    "E_hash_occgrid": dict(family="hash", hash_renderer=HASH_OCCGRID, synthetic={"depth": True}, train=dict(PRIORS, batch_size=128)),
}
# recorded after F, so that A-F run in the order in which they were first recorded
HASH_POSE_CASES = {
    "G_hash_hierarchical_refine_poses": dict(family="hash", train=dict(HASH_REFINE, batch_size=77)),
    "H_hash_occgrid_refine_poses": dict(family="hash", hash_renderer=HASH_OCCGRID, train=dict(HASH_REFINE, batch_size=128)),
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _runner(root, name, family, train=None, synthetic=None, hash_renderer=None, device="cuda:0"):
    from dynhor_amd.runner import Runner
    conf = {"seq_name": "train_step", "exp_name": name, "data_info": {"synthetic": dict(SYNTHETIC, **(synthetic or {}))},
            "train": dict(QUIET, **(train or {})), "model": {"family": family}}
    if hash_renderer:
        conf["model"]["hash_renderer"] = hash_renderer
    return Runner(conf=conf, device=device, exp_root=root)


def _train_case(root, name, spec, device):
    r = _runner(root, name, device=device, **spec)
    rec = {"stats": [], "prior_stats": [], "corr_stats": []}
    for _ in range(ITERS):
        rec["stats"].append(r.train_iteration().tolist())
        for key, attr in (("prior_stats", "last_prior_stats"), ("corr_stats", "last_corr_stats")):
            side = getattr(r.renderer, attr, None)
            rec[key].append(None if side is None else side.tolist())
    rec["flat_sha256"] = sha(r.store.flat)
    if r.pose_refiner is not None:
        rec["R_sha256"], rec["T_sha256"] = sha(r.dataset.R), sha(r.dataset.T)
    return rec


def _points(n, seed, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, 3, generator=g)
    x = x / x.norm(dim=1, keepdim=True) * torch.rand(n, 1, generator=g) ** (1 / 3) * 0.9
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    return x.to(device).contiguous(), d.to(device).contiguous()


def _network_case(root, family, device):
    """Case F on the freshly built models of a Runner of this family."""
    import dynhor_amd.renderer
    from dynhor_amd import mesh_color, sdf_init, surface_render
    ren = _runner(root, "F_" + family, family, train={"batch_size": 64}, device=device).renderer
    mods = [m for m in (dynhor_amd.renderer, mesh_color, surface_render) if hasattr(m, "NET_CHUNK")]
    kept = [m.NET_CHUNK for m in mods]
    for m in mods:
        m.NET_CHUNK = NET_CHUNK
    try:
        pts, dirs = _points(300, 5, device)
        rec = {"vertex_colors_with_normals": sha(mesh_color.network_vertex_colors(ren, pts, dirs)),
               "vertex_colors_without_normals": sha(mesh_color.network_vertex_colors(ren, pts))}
        normals, colors = surface_render.network_at_hits(ren, pts, dirs)
        rec["at_hits_normals"], rec["at_hits_colors"] = sha(normals), sha(colors)
    finally:
        for m, v in zip(mods, kept):
            m.NET_CHUNK = v
    pts, _ = _points(256, 6, device)
    target = (pts.norm(dim=1) - 0.4).contiguous()
    rec["fit_loss"], rec["fit_sdf_sha256"] = [], []
    for _ in range(3):
        loss, s = sdf_init.fit_step(ren, pts, target, 1e-3, 0.1, 8)
        rec["fit_loss"].append(float(loss))
        rec["fit_sdf_sha256"].append(sha(s.sdf))
    rec["flat_sha256"] = sha(ren.store.flat)
    return rec


def run_cases(device="cuda:0"):
    """{case: its record} of the cases A-E, of F for both families, and of G and H."""
    out = {}
    with tempfile.TemporaryDirectory() as root:
        for name, spec in CASES.items():
            out[name] = _train_case(root, name, spec, device)
        for family in ("neus", "hash"):
            out["F_network_stages_" + family] = _network_case(root, family, device)
        for name, spec in HASH_POSE_CASES.items():
            out[name] = _train_case(root, name, spec, device)
    return json.loads(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "train_step.json"))
    args = ap.parse_args()
    out = run_cases()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases -> {args.out}: " + ", ".join(f"{k} (keys {sorted(v)})" for k, v in out.items()))


if __name__ == "__main__":
    main()
