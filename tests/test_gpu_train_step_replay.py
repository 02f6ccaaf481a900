"""The training step of both model families and the network stages outside it against tests/golden/train_step.json (recorded twice,
byte for byte the same, by tests/golden/make_golden_train_step.py on an MI355X before the network-stage state and the loss stage were
made one; cases G and H, the hash family's pose refinement, recorded in the same way before the hash-grid kernels' shared helpers): six
Runner iterations of NeuS (ragged batch; the full loss stack; pose refinement), of the hash family on both samplers without and with
pose refinement, and vertex colours, hit-point colours and SDF warm-start steps of both families must give the recorded numbers bit for
bit."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "train_step.json")) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def replay():
    spec = importlib.util.spec_from_file_location("make_golden_train_step", os.path.join(HERE, "golden", "make_golden_train_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.run_cases()


def test_the_recording_covers_the_cases():
    assert sorted(RECORDED) == ["A_neus_ragged", "B_neus_full_loss_stack", "C_neus_refine_poses", "D_hash_hierarchical", "E_hash_occgrid",
                                "F_network_stages_hash", "F_network_stages_neus", "G_hash_hierarchical_refine_poses",
                                "H_hash_occgrid_refine_poses"]
    for name, rec in RECORDED.items():
        if name[0] == "F":
            assert len(rec["fit_loss"]) == len(rec["fit_sdf_sha256"]) == 3 and len(set(rec["fit_sdf_sha256"])) == 3, name
            assert rec["vertex_colors_with_normals"] != rec["vertex_colors_without_normals"], name
            continue
        assert len(rec["stats"]) == 6 and all(len(s) == 8 for s in rec["stats"]) and len(rec["flat_sha256"]) == 64, name
        assert all((p is not None) == (name[0] in "BCE") for p in rec["prior_stats"]), name
        assert all((c is not None) == (name[0] == "B") for c in rec["corr_stats"]), name
        assert ("R_sha256" in rec) == ("T_sha256" in rec) == (name[0] in "CGH"), name
    depth_rays = [p[1] for p in RECORDED["B_neus_full_loss_stack"]["prior_stats"]]
    assert depth_rays[:2] == [0.0, 0.0] and all(n > 0 for n in depth_rays[2:])          # the depth term comes on inside the run


@pytest.mark.parametrize("case", sorted(RECORDED))
def test_training_path_matches_the_recording_bit_for_bit(case, replay):
    want, got = RECORDED[case], replay[case]
    assert sorted(want) == sorted(got), f"{case}: the record's keys differ from the recording"
    text = lambda r: json.dumps(r, sort_keys=True)                  # as text: a NaN compares equal to itself
    for key in sorted(want):
        if isinstance(want[key], list):
            assert len(want[key]) == len(got[key]), (case, key)
            wrong = {k: (w, g) for k, (w, g) in enumerate(zip(want[key], got[key])) if text(w) != text(g)}
            assert not wrong, f"{case}: {key} differs at iterations {sorted(wrong)}: {wrong}"
        else:
            assert text(want[key]) == text(got[key]), f"{case}: {key} differs: {want[key]} != {got[key]}"
