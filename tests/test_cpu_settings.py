"""The settings blocks of the Runner and of the feature modules against tests/golden/runner_settings.json (recorded by
tests/golden/make_golden_runner_settings.py before the settings code was gathered in dynhor_amd/settings.py): every case must give the
recorded dict, or the recorded exception type and message, to the letter.  Then dynhor_amd.settings on its own: the layering of merge,
its two unknown-key wordings, the predicates and the two helpers that raise.  No GPU."""
import importlib.util
import json
import math
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "runner_settings.json")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_runner_settings", os.path.join(HERE, "golden", "make_golden_runner_settings.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def replay():
    return _recorder().run_cases()


with open(GOLDEN) as _f:
    RECORDED = json.load(_f)


@pytest.mark.parametrize("block", sorted(RECORDED))
def test_block_matches_the_recording(block, replay):
    want, got = RECORDED[block], replay[block]
    assert sorted(want) == sorted(got), f"{block}: the case list differs from the recording"
    text = lambda r: json.dumps(r, sort_keys=True)                  # as text: a NaN in a merged dict compares equal to itself
    wrong = {k: (want[k], got[k]) for k in want if text(want[k]) != text(got[k])}
    assert not wrong, f"{block}: {len(wrong)} of {len(want)} cases differ, the first: {next(iter(wrong.items()))}"


def test_the_recording_covers_every_block():
    assert set(RECORDED) == {"mesh_clean", "mesh_color", "mesh_texture", "mesh_extract", "mesh_simplify", "mesh_vis", "surface_render",
                             "image_eval", "sdf_init", "visual_hull", "depth_fuse", "mvs", "match", "pose_sil", "pose_photo", "pose_corr",
                             "pose_init", "eval"}
    for block, cases in RECORDED.items():
        assert {"empty", "partial", "none_overrides", "unknown_config"} <= set(cases), block
        assert any(k.startswith("override:") for k in cases), block
        kinds = {next(iter(r)) for r in cases.values()}
        assert kinds <= {"ok", "error", "select_mesh"} and "error" in kinds, (block, kinds)


def test_merge_layers_defaults_block_and_overrides():
    from dynhor_amd.settings import merge
    D = {"a": 1, "b": 2, "c": 3}
    assert merge("x", D, None) == D and merge("x", D, {}) == D and merge("x", D, None, None) == D
    assert merge("x", D, {"a": 10, "b": 20}, {"b": 200, "c": None}) == {"a": 10, "b": 200, "c": 3}     # None is no override
    assert merge("x", D, {"a": None}) == {"a": None, "b": 2, "c": 3}                                   # the block's null is a value
    assert list(merge("x", D, {"b": 0})) == list(D)                                                    # the defaults' order
    out = merge("x", D, {"a": 5})
    out["a"] = 6
    assert D["a"] == 1                                                                                 # a copy
    assert merge("x", D, {"z": 1}, {"y": 2}) == {"a": 1, "b": 2, "c": 3, "z": 1, "y": 2}               # nothing is checked unless asked


def test_merge_unknown_key_wordings():
    from dynhor_amd.settings import merge
    D = {"a": 1, "b": 2}
    with pytest.raises(ValueError) as e:
        merge("x", D, None, {"z": 1}, check_overrides=True)
    assert str(e.value) == "x: unknown setting(s) ['z']; known: ['a', 'b']"
    with pytest.raises(ValueError) as e:
        merge("x", D, {"z": 1, "y": 2}, check_block=True)
    assert str(e.value) == "x: unknown setting(s) ['y', 'z'] in the config; known: ['a', 'b']"
    with pytest.raises(ValueError) as e:
        merge("x", D, None, {"z": None}, who="mode_fn", check_overrides=True)                          # named even when it is None
    assert str(e.value) == "mode_fn: unknown x setting(s) ['z']; known: ['a', 'b']"
    with pytest.raises(ValueError) as e:
        merge("x", D, {"z": 1}, who="mode_fn", check_block=True)
    assert str(e.value) == "mode_fn: unknown x setting(s) ['z'] in the config; known: ['a', 'b']"
    with pytest.raises(ValueError) as e:
        merge("x", D, {"z": 1}, check_block="keys")
    assert str(e.value) == "x: unknown keys ['z']; known: ['a', 'b']"
    with pytest.raises(ValueError, match=r"\['y'\]; known"):                                            # the overrides are looked at first
        merge("x", D, {"z": 1}, {"y": 1}, check_block=True, check_overrides=True)
    assert merge("x", D, {"z": 1}, {"a": 3}, check_overrides=True) == {"a": 3, "b": 2, "z": 1}         # each side on its own


def test_predicates():
    from dynhor_amd.settings import is_int, is_num
    assert is_int(0) and is_int(-3) and is_int(1 << 40)
    assert not any(is_int(v) for v in (True, False, 1.0, "1", None, float("nan")))
    assert is_num(0) and is_num(-2.5) and is_num(1e300)
    assert not any(is_num(v) for v in (True, False, "1", None, float("nan"), float("inf"), -math.inf))


def test_raising_helpers():
    from dynhor_amd.settings import int_in, one_of
    assert int_in("blk", "key", 1, 1, 4) is None and int_in("blk", "key", 4, 1, 4) is None
    for v in (0, 5, True, 2.0, "2", float("nan")):
        with pytest.raises(ValueError) as e:
            int_in("blk", "key", v, 1, 4)
        assert str(e.value) == f"blk key must be an integer in [1, 4], got {v!r}"
    assert one_of("blk", "mode", "a", ("a", "b")) is None
    with pytest.raises(ValueError) as e:
        one_of("blk", "mode", "c", ("a", "b"))
    assert str(e.value) == "blk mode must be one of ('a', 'b'), got 'c'"
