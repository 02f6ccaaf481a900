"""pose_sil.refine_poses with its optional terms against tests/golden/pose_refine.json (recorded twice, byte for byte the same, by
tests/golden/make_golden_pose_refine.py on an MI355X before the terms took over the code that reads their own rows): the silhouette
alone, with the photometric term, with the correspondence term and a fixed frame, and with both terms on a subset of the frames must
give the recorded poses, curve, IoUs, settings and residuals bit for bit."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "pose_refine.json")) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def replay():
    spec = importlib.util.spec_from_file_location("make_golden_pose_refine", os.path.join(HERE, "golden", "make_golden_pose_refine.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.run_cases()


def test_the_recording_covers_the_four_cases():
    assert sorted(RECORDED) == ["A_silhouette", "B_photo", "C_corr_fixed_frame", "D_all_terms_subset"]
    for name, rec in RECORDED.items():
        assert len(rec["curve"]) == 6 and {"R", "T", "iou_before", "iou_after", "settings"} <= set(rec), name
        assert ("photo" in rec["settings"]) == (name[0] in "BD") == ("photo_pairs" in rec) == ("loss_photo" in rec["curve"][0]), name
        assert ("corr" in rec["settings"]) == (name[0] in "CD") == ("corr_worst" in rec) == ("loss_corr" in rec["curve"][0]), name
    assert [c["blur_sigma"] for c in RECORDED["B_photo"]["curve"]] == [1.0] * 3 + [0.0] * 3      # the level changes inside the run


@pytest.mark.parametrize("case", sorted(RECORDED))
def test_refine_poses_matches_the_recording_bit_for_bit(case, replay):
    want, got = RECORDED[case], replay[case]
    assert sorted(want) == sorted(got), f"{case}: the result's keys differ from the recording"
    text = lambda r: json.dumps(r, sort_keys=True)                  # as text: a NaN compares equal to itself
    for key in sorted(want):
        if key == "curve":
            assert len(want[key]) == len(got[key]), case
            for k, (w, g) in enumerate(zip(want[key], got[key])):
                assert sorted(w) == sorted(g), (case, k, sorted(w), sorted(g))
                wrong = {x: (w[x], g[x]) for x in w if text(w[x]) != text(g[x])}
                assert not wrong, f"{case}: curve entry {k} differs: {wrong}"
        else:
            assert text(want[key]) == text(got[key]), f"{case}: {key} differs: {want[key]} != {got[key]}"
