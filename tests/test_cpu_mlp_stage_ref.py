"""CPU anchors of tests/mlp_stage_util.py, before tests/test_gpu_mlp_stages.py relies on it.

  * the fp64 restatements of the three stages equal oracle/neus_oracle.py (SDFNetwork forward / autograd, RenderingNetwork) to 1e-12 of
    each output's largest element, on 130 points;
  * the acceptance criterion rejects planted faults in an otherwise exact output (the fp64 reference rounded to fp32), so "subtly
    wrong" is defined before a GPU is involved.

torch's Softplus takes a shortcut the kernels and the restatement of the input gradient do not: for beta z > 20 it returns z and its
autograd returns EXACTLY 1, where sigma'(z) = 1 - exp(-beta h) is 1 - 2.1e-9.  The adjoint anchor therefore differentiates the
oracle's SDFNetwork with that shortcut moved out of reach (nn.Softplus(beta=100, threshold=600): the same function, evaluated in full)
and feeds the restatement the activations of that very network; against the unmodified oracle the same quantities agree to
exp(-20) = 2.1e-9 per layer, asserted at 8 layers' worth."""
import math

import pytest
import torch

from oracle import neus_oracle as O
from tests import mlp_stage_util as S
from tests.dw_util import TM
from tests.ray_kernels_util import CANARY_BITS, F32, F64
from tests.util import flat_from_oracle, randomized_models

NPTS = 130
TOL = 1e-12


def _close(got, ref, tol=TOL):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, (err, scale)


@pytest.fixture(scope="module")
def nets():
    sdf, col, var = randomized_models(seed=11, device="cpu", jitter=0.05)
    flat = flat_from_oracle(sdf, var, col)
    g = torch.Generator().manual_seed(3)
    pts = ((torch.rand(NPTS, 3, generator=g) * 2 - 1) * 1.2)
    pts[0] = 0.0
    pts[1, 0], pts[2, 1], pts[3, 2] = 1.2, -1.2, 0.0
    return sdf.double(), col.double(), flat, pts


def _oracle_sdf_trace(net, pts64):
    """(z_0..z_7, act_0..7, y) of the oracle's forward, read with hooks on its own linears and activation"""
    zs, hooks = [], []
    for l in range(9):
        hooks.append(getattr(net, f"lin{l}").register_forward_hook(lambda m, i, o: zs.append(o)))
    try:
        y = net(pts64)
    finally:
        for h in hooks:
            h.remove()
    assert len(zs) == 9
    return zs[:8], [net.activation(z) for z in zs[:8]], y


def test_sdf_forward_equals_the_oracle(nets):
    sdf, _, flat, pts = nets
    W = S.Weights(flat, F64)
    ref = S.sdf_forward_ref(W, pts)
    with torch.no_grad():
        _, acts, y = _oracle_sdf_trace(sdf, pts.double())
    _close(ref["sdf"], y[:, 0])
    _close(ref["feat"], y[:, 1:])
    _close(ref["eaux"], O.embed(pts.double(), 6))
    for l in range(8):
        assert ref["act"][l].shape[1] == (217 if l == 3 else 256)
        _close(ref["act"][l], acts[l])
    # pad rows are the origin's rows
    pad = S.sdf_forward_ref(W, pts, pad_rows=3)
    assert torch.equal(pad["sdf"][:NPTS], ref["sdf"]) and torch.equal(pad["act"][7][NPTS], pad["act"][7][0])      # (pts[0] is the origin)


def test_input_gradient_equals_the_oracles_autograd(nets):
    sdf, _, flat, pts = nets
    W = S.Weights(flat, F64)
    full = torch.nn.Softplus(beta=100, threshold=600)
    for lifted, tol in ((True, TOL), (False, 8 * math.exp(-20.0))):
        keep = sdf.activation
        if lifted:
            sdf.activation = full
        try:
            x = pts.double().clone().requires_grad_(True)
            zs, acts, y = _oracle_sdf_trace(sdf, x)
            grads = torch.autograd.grad(y[:, 0].sum(), zs + [x])
            normals = sdf.gradient(pts.double().clone()).squeeze(1).detach()
        finally:
            sdf.activation = keep
        a_ref, n_ref = grads[:8], grads[8]
        _close(normals, n_ref, TOL)
        got = S.sdf_gradient_ref(W, pts, [h.detach() for h in acts])
        for l in range(8):
            _close(got["a"][l], a_ref[l], tol)
        _close(got["normals"], n_ref, tol)
        # ge = d sdf / d embedding: the oracle has no such leaf; n = J_e^T ge is what pins it, and gesave is judged against it
        assert got["ge"].shape == (NPTS, 39)


def test_colour_forward_equals_the_oracle(nets):
    _, col, flat, pts = nets
    W = S.Weights(flat, F64)
    g = torch.Generator().manual_seed(5)
    for n_per_ray in (1, 4, 64, 200):
        nrays = (NPTS + n_per_ray - 1) // n_per_ray
        dirs = torch.nn.functional.normalize(torch.randn(nrays, 3, generator=g), dim=-1)
        normals = torch.randn(NPTS, 3, generator=g)
        feat = torch.randn(NPTS, 256, generator=g)
        got = S.color_forward_ref(W, pts, dirs, n_per_ray, normals, feat)
        d = dirs[torch.arange(NPTS) // n_per_ray].double()
        outs, hooks = [], []
        for l in range(4):
            hooks.append(getattr(col, f"lin{l}").register_forward_hook(lambda m, i, o: outs.append(torch.relu(o))))
        try:
            with torch.no_grad():
                c = col(pts.double(), normals.double(), d, feat.double())
        finally:
            for h in hooks:
                h.remove()
        _close(got["color"], c)
        _close(got["caux"], torch.cat([pts.double(), O.embed(d, 4), normals.double()], -1))
        for l in range(4):
            _close(got["cact"][l], outs[l])
    pad = S.color_forward_ref(W, pts, dirs, n_per_ray, normals, torch.cat([feat, feat[:2]]), pad_rows=2)
    assert bool((pad["caux"][NPTS:] == 0).all()) and pad["color"].shape == (NPTS, 3) and pad["cact"][0].shape[0] == NPTS + 2


# ------------------------------------------------------------------------------------------------ planted faults
RAGGED = TM + 37          # two tiles, the second ragged


@pytest.fixture(scope="module")
def exact(nets):
    """Every saved region of the three stages at a ragged size in row form, whole tiles: (fp64 reference, fp32 restatement, the "exact"
    output = the fp64 reference rounded to fp32 with the pad columns the code leaves)."""
    _, _, flat, pts = nets
    pts = pts[:RAGGED]
    pad = 2 * TM - RAGGED
    g = torch.Generator().manual_seed(9)
    dirs = torch.nn.functional.normalize(torch.randn((RAGGED + 3) // 4, 3, generator=g), dim=-1)
    # each stage's inputs are fp32 values, as a kernel is given them: the previous stage's fp64 result rounded once
    W64 = S.Weights(flat, F64)
    act_in = [h.float() for h in S.sdf_forward_ref(W64, pts, pad_rows=pad)["act"]]
    feat_in = S.sdf_forward_ref(W64, pts, pad_rows=pad)["feat"].float()
    normals_in = S.sdf_gradient_ref(W64, pts, act_in)["normals"].float()
    out = {}
    for dt in (F64, F32):
        W = S.Weights(flat, dt)
        f = S.sdf_forward_ref(W, pts, pad_rows=pad)
        gr = S.sdf_gradient_ref(W, pts, act_in)
        c = S.color_forward_ref(W, pts, dirs, 4, normals_in, feat_in, pad_rows=pad)
        out[dt] = {"act": f["act"], "feat": f["feat"], "eaux": f["eaux"], "asave": gr["a"], "cact": c["cact"], "caux": c["caux"]}

    def tile_rows(name, l, x):
        w = 64 if name in ("eaux", "caux") else 256
        full = torch.zeros(x.shape[0], w)
        full[:, : x.shape[1]] = x.float()
        if name == "act" and l == 3:
            full[:, 217:] = S.SOFTPLUS0
        return full
    regions = [("act", l) for l in range(8)] + [("asave", l) for l in range(8)] + [("cact", l) for l in range(4)] + \
              [("feat", 0), ("eaux", 0), ("caux", 0)]
    pick = lambda d, n, l: d[n][l] if n in ("act", "asave", "cact") else d[n]
    return {(n, l): (pick(out[F64], n, l), pick(out[F32], n, l), tile_rows(n, l, pick(out[F64], n, l))) for n, l in regions}


def _misses(exact, got_of):
    led = S.StageLedger()
    for (n, l), (r64, r32, ex) in exact.items():
        S.judge_tile_rows(led, n, l, "planted", got_of.get((n, l), ex), r64, r32, npts=RAGGED)
    return led.failures


def test_the_exact_output_passes(exact):
    assert _misses(exact, {}) == []


def _one_element_off(exact, key, rel):
    got = exact[key][2].clone()
    w = S.valid_width(*key)
    tile = got[TM:, :w]                                   # the ragged tile
    got[TM + 5, w // 2] += rel * tile.abs().max().item()
    return _misses(exact, {key: got})


# What the criterion can resolve on an output is 4 x the fp32 restatement's own error there.  Measured on this fixture as a fraction of
# a fault of 2^-18 of the ragged tile's maximum: eaux, caux 0.13, a_7 0.17 (one product), act[0..7] 0.47 .. 0.69, cact[0..3] 0.63 .. 0.86,
# a_0..a_6 0.59 .. 0.91, feat 1.01 (the end of nine fp32 layers: 2^-20 of its maximum, times the margin of 4).  The 2^-18 fault is
# planted where that fraction is below 0.7, so that another BLAS's summation order does not decide the test; a fault of 2^-17 is
# rejected in every region.
@pytest.mark.parametrize("region", ["act0", "act1", "act3", "act7", "asave5", "asave7", "cact1", "cact2", "eaux0", "caux0"])
def test_one_element_off_by_2e_minus_18_of_its_tiles_maximum_is_rejected(exact, region):
    assert len(_one_element_off(exact, (region[:-1], int(region[-1])), 2.0 ** -18)) == 1


def test_one_element_off_by_2e_minus_17_is_rejected_in_every_region(exact):
    for key in exact:
        assert len(_one_element_off(exact, key, 2.0 ** -17)) == 1, key


def test_structural_faults_are_rejected(exact):
    a3 = exact[("act", 3)][2]
    # two rows of the last ragged tile exchanged
    got = a3.clone()
    got[[TM + 3, TM + 20]] = got[[TM + 20, TM + 3]]
    assert _misses(exact, {("act", 3): got})
    # layer l and l + 1 of a saved region exchanged
    for name, l in (("act", 5), ("asave", 1), ("cact", 2)):
        assert len(_misses(exact, {(name, l): exact[(name, l + 1)][2], (name, l + 1): exact[(name, l)][2]})) >= 2
    # column 216 and column 217 of act[3] exchanged
    got = a3.clone()
    got[:, [216, 217]] = got[:, [217, 216]]
    assert len(_misses(exact, {("act", 3): got})) == 2    # the valid columns and the pad columns
    # a pad row holding the canary
    for key in (("act", 0), ("feat", 0), ("caux", 0), ("asave", 6)):
        got = exact[key][2].clone()
        got.view(torch.int32)[2 * TM - 1] = CANARY_BITS
        assert _misses(exact, {key: got})
    # caux pad rows must be zero, not the extras of a point at the origin
    got = exact[("caux", 0)][2].clone()
    got[RAGGED:, 9:12] = 1.0
    assert _misses(exact, {("caux", 0): got})


def test_class_words_one_binade_off_are_rejected():
    for m in (1.0, 1.5, 1.9999999, 3.1e-3, 47.0):
        bits = S.float_bits(m)
        assert S.class_word_ok(bits, m) and S.class_word_ok(bits, m, exact=m)
        assert not S.class_word_ok(S.float_bits(2 * m), m)          # one binade too high: a class pushed towards fp16 subnormals
        assert not S.class_word_ok(S.float_bits(0.5 * m), m)        # one binade too low: a piece overflows, inf x 0 = NaN in a pad row
        assert not S.class_word_ok(bits - 1, m)                     # below the maximum at all
        assert not S.class_word_ok(bits + 1, m, exact=m)
    # ABSMAX_CAUX: floored at 1
    assert S.class_word_ok(S.float_bits(1.0), 0.83, exact=1.0) and not S.class_word_ok(S.float_bits(0.83), 0.83, exact=1.0)
    assert not S.class_word_ok(0, 0.5) and not S.class_word_ok(CANARY_BITS, 0.5)
