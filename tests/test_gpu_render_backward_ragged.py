"""GPU: whole-renderer parameter gradients at point counts that are no multiple of the 64-point tile.

tests/test_gpu_render_backward.py runs 2048, 16640 and 3072 points: whole tiles, and more tiles than the weight-gradient kernel has
workgroups.  Here the last tile is partial and there are fewer tiles than workgroups (30, 130, 280 and 2046 points: 1, 3, 5 and 32
tiles), at that test's tolerances (relative L2 of every parameter gradient <= 2e-4 against the fp64 oracle, or within 10 x torch
fp32's own error).  Before each case the same renderer renders and differentiates a larger batch, so the reused uninitialised
workspace holds that launch's tiles: pad rows and regions a small launch does not rewrite are stale numbers, not zeros.

(33, 50, 12) up-samples in 2 steps of 6 (the per-ray kernels need an even count per step); the others in the usual 4."""
import pytest

from dynhor_amd import _lib
from tests.test_gpu_render_backward import check_parameter_gradients

pytestmark = pytest.mark.gpu

CASES = {(3, 10, 0): (0.3, 0.05, False, 4), (5, 26, 0): (1.0, 0.0, True, 4), (7, 32, 8): (0.0, 0.05, False, 4),
         (33, 50, 12): (0.5, 0.05, True, 2)}


def _run(B, ns, ni, arithmetic):
    car, normal_w, bg, steps = CASES[(B, ns, ni)]
    check_parameter_gradients(B, ns, ni, car, normal_w, bg, arithmetic=arithmetic, stale_batch=2 * B + 3, up_sample_steps=steps)


@pytest.mark.parametrize("B,ns,ni", list(CASES))
def test_ragged_parameter_gradients_match_oracle_autograd(B, ns, ni):
    _run(B, ns, ni, None)


@pytest.mark.parametrize("arithmetic", ["fp32_mfma", "split_bf16"])
@pytest.mark.parametrize("B,ns,ni", [(3, 10, 0), (33, 50, 12)])
def test_ragged_parameter_gradients_in_the_other_arithmetics(B, ns, ni, arithmetic):
    _run(B, ns, ni, _lib.ARITH_NAMES[arithmetic])
