"""GPU: the tail of the weight-gradient stage (csrc/dw.hip) -- the tile-partial reduction that rides behind the GEMM kernel's jobs
(dw_tpart_tail) and the one-pass slab reduction + weight-norm fold (reduce_fold_kernel) -- at 64, 65 and 64 * 33 points: one tile
(most of the 256 workgroups own no tile and still write zero slabs), a second tile for one point, an odd tile count that neither
the job groups' workgroup counts nor the 64-way tile-partial split divide.

tests/test_gpu_dw_stage.py pins WHAT the stage computes (integer operands: every order of summation gives the same bits).  Here the
operands are floats, so the ORDER shows, and the order is part of the contract (gradients are bitwise
reproducible and a change of kernel form does not move them):
  (a) the reduced block equals, bit for bit, the eight-partial sum of the split-K slabs the GEMM kernel left in the workspace: slab g
      of a job group goes to partial g % 8 in increasing g, then ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)) -- restated in
      torch with elementwise fp32 additions (IEEE: the same bits).  All of it: the rows and columns no parameter folds included.
  (b) tred[s][slot] equals, bit for bit, the fp32 sum of its split's tiles in tile order; once more at 200 tiles, where a split has
      three or four tiles (at 33 it has one or none).
  (c) two launches on the same inputs give a bitwise identical flat gradient.
  (d) at 65 points with test_gpu_dw_stage's integer operands, the flat gradient against dw_util.fold_reference in fp64, bounded by
      that file's K_FOLD x the error of the same reference evaluated in fp32.
"""
import pytest
import torch

from tests import dw_util as U
from tests.test_gpu_dw_stage import ARITHS, DEV, K_FOLD, Stage

pytestmark = pytest.mark.gpu

NPTS = [64, 65, 64 * 33]
FORMS = ["fp32_mfma", "split_f16"]


@pytest.fixture(scope="module")
def stage(hiplib):
    return Stage(hiplib)


def _carve(stage, npts):
    lay = U.Layout(npts)
    assert lay.total_floats == stage._lib.workspace_floats(npts)[2]
    return lay, stage.big[:lay.total_floats]


def _write_floats(lay, ws, seed):
    """O(1) tame operands, heavy-tailed ones scaled 2^U(-12, 0) per tile, random tile partials; the scale words of SPLIT_F16"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    nt = lay.ntiles
    ws[:lay.tred].zero_()
    for name in U.OPERAND_REGIONS:
        layers, per = U.REGION_SHAPE[name]
        for l in range(layers):
            x = torch.randn(nt, per, generator=g, device=DEV)
            if name in U.HEAVY:
                x = x * torch.exp2(-12.0 * torch.rand(nt, 1, generator=g, device=DEV))
            lay.tiles(ws, name, l).copy_(x.reshape(-1))
    ws[lay.tpart: lay.tpart + lay.size["tpart"]] = torch.randn(lay.size["tpart"], generator=g, device=DEV)
    ws[lay.gesave:].zero_()
    U.write_scale_words(lay, ws)


def _eight_partial_sum(blocks):
    """[G, n] fp32 slabs of one job group -> [n]: the fixed order of the slab reduction"""
    G, n = blocks.shape
    s = torch.zeros(8, n, device=blocks.device)
    for g0 in range(0, G, 8):
        k = min(8, G - g0)
        s[:k] = s[:k] + blocks[g0: g0 + k]
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))


def _check_red(lay, ws, what):
    slabs = ws[lay.slabs: lay.slabs + U.DW_G * U.GSTRIDE].view(U.DW_G, U.GSTRIDE)
    red = ws[lay.red: lay.red + U.GSTRIDE]
    for job in range(15):
        a, b = U.JOB_OFF[job], U.JOB_OFF[job] + U.JOB_FLOATS[job]
        # the job group's workgroups are the ones that wrote this job's part of their split block (the rest is still the NaN fill)
        wrote = ~torch.isnan(slabs[:, a]).cpu()
        idx = wrote.nonzero().reshape(-1)
        assert len(idx) >= 1 and int(idx[-1]) - int(idx[0]) + 1 == len(idx), f"job {job}, {what}: writers {idx.tolist()}"
        want = _eight_partial_sum(slabs[int(idx[0]): int(idx[-1]) + 1, a:b])
        got = red[a:b]
        assert bool(torch.isfinite(got).all()), f"job {job}, {what}: the reduced slab is not complete"
        bad = got.view(torch.int32) != want.view(torch.int32)
        assert not bool(bad.any()), f"job {job}, {what}: {int(bad.sum())} of {bad.numel()} reduced words differ from the eight-partial sum, first at {int(bad.nonzero()[0])}"


def _check_tred(lay, ws, what):
    nt = lay.ntiles
    tp = ws[lay.tpart: lay.tpart + lay.size["tpart"]].view(nt, U.N_TILE_PART, 256)
    want = torch.zeros(U.DW_NS, U.N_TILE_PART, 256, device=DEV)
    for s in range(U.DW_NS):
        for t in range(nt * s // U.DW_NS, nt * (s + 1) // U.DW_NS):
            want[s] = want[s] + tp[t]
    got = ws[lay.tred: lay.tred + lay.size["tred"]].view(U.DW_NS, U.N_TILE_PART, 256)
    bad = got.view(torch.int32) != want.view(torch.int32)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} tred words differ from the in-order sum, first (split, slot, col) {tuple(int(v) for v in bad.nonzero()[0])}"


@pytest.mark.parametrize("npts", NPTS)
@pytest.mark.parametrize("arith", FORMS)
def test_reduction_orders_are_the_fixed_ones_and_two_launches_agree_bitwise(stage, arith, npts):
    lay, ws = _carve(stage, npts)
    _write_floats(lay, ws, seed=900 + npts)
    what = f"arithmetic {arith}, npts {npts}"
    stage.run(ARITHS[arith], lay, ws, what)
    _check_red(lay, ws, what)                                                 # (a)
    _check_tred(lay, ws, what)                                                # (b)
    first = stage.grad.clone()
    nan = torch.isnan(first)
    assert bool(nan[stage.var]) and int(nan.sum()) == 1, f"{what}: {int(nan.sum())} NaN slots in the flat gradient"
    stage.run(ARITHS[arith], lay, ws, what + ", second launch")               # (c)
    assert torch.equal(first.view(torch.int32), stage.grad.view(torch.int32)), f"{what}: two launches differ"


def test_tile_partials_are_added_in_tile_order_when_a_split_has_several_tiles(stage):
    lay, ws = _carve(stage, 64 * 200)
    ws[:lay.tred].zero_()
    g = torch.Generator(device=DEV).manual_seed(31)
    ws[lay.tpart: lay.tpart + lay.size["tpart"]] = torch.randn(lay.size["tpart"], generator=g, device=DEV)
    ws[lay.gesave:].zero_()
    stage.run(ARITHS["fp32_mfma"], lay, ws, "200 tiles")
    _check_tred(lay, ws, "200 tiles")


@pytest.mark.parametrize("arith", FORMS)
def test_fold_at_a_ragged_second_tile_matches_the_fp64_reference(stage, arith):
    lay, ws = _carve(stage, 65)
    assert lay.ntiles == 2
    g = torch.Generator(device=DEV).manual_seed(4321)
    ws[:lay.tred] = torch.randint(-8, 9, (lay.tred,), generator=g, device=DEV).float()
    ws[lay.gesave:].zero_()
    U.write_scale_words(lay, ws)
    rows = {}
    for name in U.OPERAND_REGIONS:
        for l in range(U.REGION_SHAPE[name][0]):
            t = lay.tiles(ws, name, l)
            rows[(name, l)] = U.native_to_rows(t) if U.region_width(name) == 256 else U.aux_native_to_rows(t)
    jobs = [U.job_product(j, rows).cpu() for j in range(15)]
    tsum = ws[lay.tpart: lay.tpart + lay.size["tpart"]].view(2, U.N_TILE_PART, 256).double().sum(0).cpu()
    flat = stage.flat.cpu()
    ref64 = U.fold_reference(jobs, tsum, flat)
    ref32 = U.fold_reference(jobs, tsum, flat, dtype=torch.float32).double()
    what = f"arithmetic {arith}, npts 65"
    stage.run(ARITHS[arith], lay, ws, what)
    for job in range(15):
        got = stage.job_matrix(lay, ws, job).double().cpu()
        assert bool((got == jobs[job]).all()), f"job {job}, {what}: the reduced slab differs from the integer product"
    got = stage.grad.double().cpu()
    fails = []
    for name, off, shape in U.param_tensors():
        n = int(torch.tensor(shape).prod())
        r = ref64[off: off + n]
        scale = float(r.abs().max())
        assert scale > 0, name
        err = float((got[off: off + n] - r).abs().max()) / scale
        yard = float((ref32[off: off + n] - r).abs().max()) / scale
        print(f"{name:20s} {what}: max error / max {err:.3e}, fp32 reference {yard:.3e}")
        if not err <= K_FOLD * yard:
            fails.append(f"{name}, {what}: error {err:.3e} against {K_FOLD} x {yard:.3e} (fold_reference in fp32)")
    assert not fails, "\n".join(fails)
